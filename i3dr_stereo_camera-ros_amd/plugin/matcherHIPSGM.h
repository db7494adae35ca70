// matcherHIPSGM.h — drop-in AbstractStereoMatcher subclass for the reference ROS package.
// Copy into include/stereoMatcher/ of i3dr_stereo_camera-ros; it
// mirrors matcherOpenCVSGBM.h:6-39 and delegates compute to libsgm_hip.so.
#ifndef MATCHERHIPSGM_H
#define MATCHERHIPSGM_H

#include "stereoMatcher/abstractStereoMatcher.h"
#include "hip_sgm_core.h"

class MatcherHIPSGM : public AbstractStereoMatcher
{
public:
  // mode: an SGM_MODE_* of sgm_hip.h; -1 reads SGM_HIP_MODE (default SGM_MODE_OCV_SGBM5).
  // The census mode's path set (8 or 4) comes from SGM_HIP_CENSUS_PATHS (hip_sgm_core.h setCensusPaths),
  // its census window from SGM_HIP_CENSUS_WINDOW (setCensusWindow below).
  // SGM_MODE_OCV_BM (3) makes this the drop-in for MatcherOpenCVBlock (cv::StereoBM).
  explicit MatcherHIPSGM(std::string &param_file, cv::Size _image_size, int mode = -1)
      : AbstractStereoMatcher(param_file, _image_size), core_(0, mode)
  {
    init();
  }

  int forwardMatch(void);
  int backwardMatch(void);

  // imageCb's compute in one device call (MatcherCore::imageCb, sgm_node_frame): raw CV_8UC1 /
  // CV_8UC3 pair + both CameraInfos -> the rectified images the node publishes and the
  // DisparityImage float image (CV_32FC1, MISSING_Z outside [T*f/depth_max, T*f/depth_min]).
  // depth (may be null) with q5 = {Q(2,3), Q(0,3), Q(1,3), Q(3,2), Q(3,3)}: the depth image.
  int imageCb(const cv::Mat &raw_left, const cv::Mat &raw_right, const sgm_camera_info &info_left,
              const sgm_camera_info &info_right, double f, double T, double depth_min, double depth_max,
              cv::Mat &rect_left, cv::Mat &rect_right, cv::Mat &disparity, cv::Mat *depth = nullptr,
              const double *q5 = nullptr);

  void setMinDisparity(int min_disparity);
  void setDisparityRange(int disparity_range);
  void setWindowSize(int window_size);
  void setUniquenessRatio(int ratio);
  void setSpeckleFilterWindow(int window);
  void setSpeckleFilterRange(int range);
  void setP1(float p1);
  void setP2(float p2);
  void setDisp12MaxDiff(int diff);
  void setInterpolation(bool enable);
  void setPreFilterCap(int cap);
  // The hole filter after every match (SGM_FILL_*; default: env SGM_HIP_FILL, else off). With env
  // SGM_HIP_FILL_WHEN=interp, setInterpolation drives it in place of the Q3 right-view result
  // (hip_sgm_core.h setHoleFilling).
  void setHoleFilling(int mode, int max_gap = 16, int min_neighbours = 2);
  // The census mode's window (default: env SGM_HIP_CENSUS_WINDOW, else 9x7 step 1). With
  // SGM_HIP_CENSUS_WINDOW=cfg, setWindowSize (the node's correlation_window_size slider) drives it
  // through sgm_census_window_from_size (hip_sgm_core.h setCensusWindow).
  void setCensusWindow(int taps_x, int taps_y, int step = 1);
  // The pyramid level (default: env SGM_HIP_PYRAMID, else 0): 1 matches at half resolution on the
  // device and refines at full resolution (hip_sgm_core.h setPyramidLevel). With
  // SGM_HIP_PYRAMID=scale, setDownsampleScale(s) drives it (s <= 0.5: level 1, else 0); without, the
  // node's per-frame setDownsampleScale(1) changes nothing. The base class's scale stays 1 either
  // way: setImages never resizes on the CPU.
  void setPyramidLevel(int level);
  void setDownsampleScale(double scale);

  // cv::StereoBM parameters: used in BM mode, ignored by the SGM modes (matcherOpenCVSGBM.h:31-34)
  void setTextureThreshold(int threshold);
  void setPreFilterSize(int size);
  // Not used (no-op)
  void setOcclusionDetection(bool enable){};

private:
  sgm_hip::MatcherCore core_;
  void init(void);
};

#endif // MATCHERHIPSGM_H
