// hip_sgm_core.h — OpenCV-free core of the MatcherHIPSGM plugin.
//
// Holds the matcher parameters with the reference's setter semantics
// (src/stereoMatcher/matcherOpenCVSGBM.cpp:53-110) and runs the match through the C-ABI
// (include/sgm_hip.h). MatcherHIPSGM (matcherHIPSGM.{h,cpp}) is a thin cv::Mat shell
// around it, so everything with behaviour is compiled and tested without OpenCV/ROS.
#ifndef HIP_SGM_CORE_H
#define HIP_SGM_CORE_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sgm_hip.h"

namespace sgm_hip {

// SGM_HIP_OCV_COMPAT (melodic | noetic | scalar | <bits>), else `fallback`
int ocv_compat_from_env(int fallback);
// SGM_HIP_CENSUS_PATHS (4 | 8, any integer is passed on), else `fallback`
int census_paths_from_env(int fallback);
// SGM_HIP_CENSUS_WINDOW (<tx>x<ty>[/<step>] | cfg; each number 1 to 6 digits, passed on as it is).
// Returns the window; *follow_cfg: setWindowSize drives it (cfg). Unset, blank or unparsable (with
// a note on stderr): the 9x7 default and no following.
sgm_census_window census_window_from_env(bool* follow_cfg);
// SGM_HIP_FILL (off | background | median[:gap[:min]]; gap and min: 1 to 6 digits, defaults 16 and
// 2, passed on as they are); unset, blank or unparsable (with a note on stderr): off
sgm_fill_params fill_from_env();
// SGM_HIP_FILL_WHEN (always | interp): true for interp; anything else (with a note) is always
bool fill_when_interp_from_env();
// SGM_HIP_PYRAMID (0 | 1 | scale): the pyramid level; *follow_scale: setDownsampleScale drives it
// (scale). Unset, blank or unparsable (with a note on stderr): level 0 and no following.
int pyramid_from_env(bool* follow_scale);

class MatcherCore {
public:
    // mode < 0: SGM_HIP_MODE env var, default SGM_MODE_OCV_SGBM5 (the reference's SGBM
    // path never sets a mode, generate_disparity.cpp:241-261 -> cv::StereoSGBM::MODE_SGBM).
    // SGM_MODE_OCV_BM (3) starts from cv::StereoBM::create(64, 9) like MatcherOpenCVBlock.
    explicit MatcherCore(int device = 0, int mode = -1);
    ~MatcherCore();
    MatcherCore(const MatcherCore&) = delete;
    MatcherCore& operator=(const MatcherCore&) = delete;

    // --- setters, reference semantics ------------------------------------------------
    void setDisparityRange(int disparity_range, int image_width);  // <=0 -> ((W/8)+15)&-16
    void setWindowSize(int window_size);
    void setMinDisparity(int min_disparity);
    void setUniquenessRatio(int ratio);
    void setSpeckleFilterWindow(int window);
    void setSpeckleFilterRange(int range);
    void setDisp12MaxDiff(int diff);
    void setPreFilterCap(int cap);
    void setP1(float p1);   // OpenCV's setP1(int) truncates the reference's float
    void setP2(float p2);
    void setInterpolation(bool enable);
    void setMode(int mode);
    void setOcvCompat(int bits);   // SGM_OCV_* (default: SGM_HIP_OCV_COMPAT env, else melodic)
    // SGM_MODE_CENSUS8 only: 8 or 4 aggregation paths (sgm_set_census_paths; default: the
    // SGM_HIP_CENSUS_PATHS env var, else 8). Forward and backward matches both use it.
    void setCensusPaths(int paths);
    // SGM_MODE_CENSUS8 only: the census window (sgm_set_census_window; default: the
    // SGM_HIP_CENSUS_WINDOW env var, else 9x7 step 1). Stored as given: an invalid window fails at
    // match time. With SGM_HIP_CENSUS_WINDOW=cfg (or setCensusWindowFollowsSize(true)) setWindowSize
    // also sets it, through sgm_census_window_from_size; otherwise setWindowSize leaves it alone (the
    // node's default slider value is 15 and existing census users keep their results). Forward and
    // backward matches and imageCb all use it.
    void setCensusWindow(int taps_x, int taps_y, int step = 1);
    void setCensusWindowFollowsSize(bool follow);
    // The hole filter after every match (sgm_set_fill_params; default: the SGM_HIP_FILL env var,
    // else off). Stored as given: bad values fail at match time. With SGM_HIP_FILL_WHEN=interp the
    // interp flag drives it instead: setInterpolation(true) returns the forward disparity filled
    // (mode background when none is configured) in place of Q3's right-view image, in forwardMatch
    // and in imageCb, and setInterpolation(false) returns it unfilled.
    void setHoleFilling(int mode, int max_gap = 16, int min_neighbours = 2);
    void setFillWhenInterp(bool interp);
    // The pyramid level of every match (sgm_set_pyramid_params with the default radius; default:
    // the SGM_HIP_PYRAMID env var, else 0). Stored as given: a level other than 0 or 1 fails at
    // match time. Level 1 matches at half resolution on the device and refines at full resolution;
    // forward and backward matches and imageCb all use it. With SGM_HIP_PYRAMID=scale (or
    // setPyramidFollowsScale(true)) setDownsampleScale(s) drives it: s <= 0.5 selects level 1, any
    // other scale level 0; otherwise setDownsampleScale changes nothing (the node calls it with 1
    // on every frame). No CPU resize ever happens.
    void setPyramidLevel(int level);
    void setPyramidFollowsScale(bool follow);
    void setDownsampleScale(double scale);
    sgm_fill_params effectiveFill() const;
    bool q3() const { return interpolate_ && !fill_when_interp_; }
    // cv::StereoBM only (SGM_MODE_OCV_BM); stored but unused in the other modes, where the
    // reference's matchers ignore them too (matcherOpenCVSGBM.h:31-34)
    void setTextureThreshold(int threshold);
    void setPreFilterSize(int size);

    // --- matching -------------------------------------------------------------------
    // u8 mono rectified pair -> CV_32FC1-layout disparity in 1/16 px (x16 fixed point,
    // invalid = (minD-1)*16). Returns 0, or -1 after printing to stderr (the reference's
    // catch(cv::Exception&) behaviour, matcherOpenCVSGBM.cpp:37-43).
    int forwardMatch(const uint8_t* left, const uint8_t* right, int width, int height, size_t stride,
                     float* out, size_t out_stride);
    // right-view match (cv::ximgproc::createRightMatcher semantics) into `out`: float32, or
    // int16 (backwardMatch16: the CV_16S disparity_rl of matcherOpenCVSGBM.cpp:46-51).
    int backwardMatch(const uint8_t* left, const uint8_t* right, int width, int height, size_t stride,
                      float* out, size_t out_stride);
    int backwardMatch16(const uint8_t* left, const uint8_t* right, int width, int height, size_t stride,
                        int16_t* out, size_t out_stride);

    // --- the node's frame -------------------------------------------------------------
    // processDisparity's window (generate_disparity.cpp:447-450): min_disp = (float)(T*f/depth_max),
    // max_disp = (float)(T*f/depth_min), +inf when depth_min == 0 (Q8).
    static void disparityWindow(double f, double T, double depth_min, double depth_max, float* min_disp,
                                float* max_disp);
    // imageCb's compute (generate_disparity.cpp:635-713) in one sgm_node_frame call: raw u8 pair
    // (channels 1: 8UC1, 3: 8UC3; strides in bytes) + both CameraInfos -> rectified images (either
    // may be null), the DisparityImage float image (stride in floats) and, with q5 (sgm_depth_points'
    // five Q terms), the depth image. The grey set of colour frames follows the compat bits (3.x:
    // SGM_GRAY_Y14, else SGM_GRAY_Y15). With interpolation on, the right matcher's parameters run on
    // (right, left) with the camera infos and the rectified outputs swapped (Q3). Returns 0, or -1
    // after printing to stderr like forwardMatch.
    int imageCb(const uint8_t* raw_left, const uint8_t* raw_right, int width, int height, int channels,
                size_t raw_stride, const sgm_camera_info& info_left, const sgm_camera_info& info_right, double f,
                double T, double depth_min, double depth_max, uint8_t* rect_left, uint8_t* rect_right,
                size_t rect_stride, float* disparity, size_t disparity_stride, float* depth = nullptr,
                size_t depth_stride = 0, const double* q5 = nullptr);
    // how often the frame calls (re)built the rectification maps (sgm_node_frame_map_builds)
    int mapBuilds() const;

    // Keep the forwardMatch output buffer page-locked between frames (sgm_host_register) so the
    // copy-out overlaps the match; the caller must call releaseOutput() before that buffer is
    // freed or reallocated (MatcherHIPSGM: before disparity_lr.create() changes its size/type).
    void keepOutputRegistered(bool enable);
    void releaseOutput();

    const sgm_params& params() const { return params_; }
    const sgm_bm_params& bmParams() const { return bm_; }
    bool interpolation() const { return interpolate_; }
    int disparityRange() const { return params_.num_disparities; }
    int censusPaths() const { return census_paths_; }
    const sgm_census_window& censusWindow() const { return census_window_; }
    bool censusWindowFollowsSize() const { return census_window_cfg_; }
    const sgm_fill_params& holeFilling() const { return fill_; }
    int pyramidLevel() const { return pyramid_level_; }
    bool pyramidFollowsScale() const { return pyramid_scale_; }
    const std::string& lastError() const { return err_; }
    // SGBM modes: cv::ximgproc::createRightMatcher of a StereoSGBM. BM mode: of a StereoBM —
    // minD' = -(minD + D) + 1, same D and window, uniqueness 0, no speckle filter, and (through
    // rightMatcherBmParams) texture threshold 0. The BM rule is restated from ximgproc and not
    // verified against it.
    static sgm_params rightMatcherParams(const sgm_params& p);
    static sgm_bm_params rightMatcherBmParams(const sgm_bm_params& b);

private:
    int run(const sgm_params& p, const sgm_bm_params& bm, const uint8_t* a, const uint8_t* b, int w, int h,
            size_t stride, float* outf, int16_t* out16, size_t out_stride);
    int device_;
    sgm_handle* handle_ = nullptr;   // opened lazily at the first match
    sgm_params params_{};
    sgm_bm_params bm_{};
    int census_paths_ = 8;
    sgm_census_window census_window_{9, 7, 1};
    bool census_window_cfg_ = false;   // setWindowSize drives census_window_
    sgm_fill_params fill_{};
    bool fill_when_interp_ = false;
    int pyramid_level_ = 0;
    bool pyramid_scale_ = false;       // setDownsampleScale drives pyramid_level_
    bool interpolate_ = false;
    bool keep_reg_ = false;
    void* reg_ptr_ = nullptr;        // the registered output range
    size_t reg_bytes_ = 0;
    std::string err_;
};

}  // namespace sgm_hip
#endif
