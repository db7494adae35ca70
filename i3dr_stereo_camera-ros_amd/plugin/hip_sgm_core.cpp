// hip_sgm_core.cpp — see hip_sgm_core.h.
#include "hip_sgm_core.h"

#include <cctype>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

namespace sgm_hip {

// SGM_HIP_OCV_COMPAT = melodic | noetic | scalar | <bits>: the OpenCV build the OCV modes
// reproduce (include/sgm_hip.h SGM_OCV_*); unset: sgm_default_params' melodic default.
// Case and surrounding blanks are ignored; an unparseable value warns on stderr and keeps
// the fallback (the Python mirror's ocv_compat_from_env does the same).
int ocv_compat_from_env(int fallback)
{
    const char* e = std::getenv("SGM_HIP_OCV_COMPAT");
    if (!e) return fallback;
    std::string v(e);
    while (!v.empty() && std::isspace((unsigned char)v.back())) v.pop_back();
    size_t b = 0;
    while (b < v.size() && std::isspace((unsigned char)v[b])) b++;
    v = v.substr(b);
    if (v.empty()) return fallback;
    for (char& c : v) c = (char)std::tolower((unsigned char)c);
    if (v == "melodic") return SGM_OCV_COMPAT_MELODIC;
    if (v == "noetic") return SGM_OCV_COMPAT_NOETIC;
    if (v == "scalar") return SGM_OCV_COMPAT_SCALAR;
    char* end = nullptr;
    const long bits = std::strtol(v.c_str(), &end, 0);
    if (end == v.c_str() || *end) {
        std::cerr << "SGM_HIP_OCV_COMPAT=\"" << e << "\" is not melodic | noetic | scalar | <bits>: using "
                  << fallback << std::endl;
        return fallback;
    }
    return (int)bits & (SGM_OCV_COL0_LEGACY | SGM_OCV_SIMD_SAT | SGM_OCV_LANE_TIE);
}

// SGM_HIP_CENSUS_PATHS = 4 | 8: the census mode's path set (sgm_set_census_paths); unset or
// blank: `fallback`. Surrounding blanks are ignored; any integer is passed on (a value other
// than 4 or 8 fails at match time, like every parameter), an unparseable value warns on stderr
// and keeps the fallback (the Python mirror's census_paths_from_env does the same).
int census_paths_from_env(int fallback)
{
    const char* e = std::getenv("SGM_HIP_CENSUS_PATHS");
    if (!e) return fallback;
    std::string v(e);
    while (!v.empty() && std::isspace((unsigned char)v.back())) v.pop_back();
    size_t b = 0;
    while (b < v.size() && std::isspace((unsigned char)v[b])) b++;
    v = v.substr(b);
    if (v.empty()) return fallback;
    char* end = nullptr;
    const long n = std::strtol(v.c_str(), &end, 10);
    if (end == v.c_str() || *end || n < -1000000 || n > 1000000) {
        std::cerr << "SGM_HIP_CENSUS_PATHS=\"" << e << "\" is not 4 or 8: using " << fallback << std::endl;
        return fallback;
    }
    return (int)n;
}

static std::string trimmed_lower(const char* e)
{
    std::string v(e);
    while (!v.empty() && std::isspace((unsigned char)v.back())) v.pop_back();
    size_t b = 0;
    while (b < v.size() && std::isspace((unsigned char)v[b])) b++;
    v = v.substr(b);
    for (char& c : v) c = (char)std::tolower((unsigned char)c);
    return v;
}

// SGM_HIP_CENSUS_WINDOW = <tx>x<ty>[/<step>] | cfg: the census mode's window
// (sgm_set_census_window). Case and surrounding blanks are ignored. "7x7" or "9x7/2": that window,
// each number 1 to 6 decimal digits, passed on as it is (one that is not among the 24 valid windows
// fails at match time); the text splits at the first '/' and then at the first 'x'. "cfg":
// *follow_cfg, setWindowSize drives the window. Unset or blank: the 9x7 default. An unparsable
// value gives the default and a note on stderr (the Python mirror's census_window_from_env does the
// same).
sgm_census_window census_window_from_env(bool* follow_cfg)
{
    sgm_census_window def;
    sgm_default_census_window(&def);
    if (follow_cfg) *follow_cfg = false;
    const char* e = std::getenv("SGM_HIP_CENSUS_WINDOW");
    if (!e) return def;
    const std::string v = trimmed_lower(e);
    if (v.empty()) return def;
    if (v == "cfg") {
        if (follow_cfg) *follow_cfg = true;
        return def;
    }
    const size_t slash = v.find('/');
    const std::string size = v.substr(0, slash);
    const size_t x = size.find('x');
    bool ok = x != std::string::npos;
    std::vector<std::string> nums;
    if (ok) {
        nums.push_back(size.substr(0, x));
        nums.push_back(size.substr(x + 1));
        if (slash != std::string::npos) nums.push_back(v.substr(slash + 1));
    }
    for (const std::string& n : nums) {
        ok = ok && !n.empty() && n.size() <= 6;
        for (char c : n) ok = ok && c >= '0' && c <= '9';
    }
    if (!ok) {
        std::cerr << "SGM_HIP_CENSUS_WINDOW=\"" << e << "\" is not <tx>x<ty>[/<step>] | cfg: using 9x7" << std::endl;
        return def;
    }
    return sgm_census_window{std::atoi(nums[0].c_str()), std::atoi(nums[1].c_str()),
                             nums.size() > 2 ? std::atoi(nums[2].c_str()) : 1};
}

// SGM_HIP_FILL = off | background | median[:gap[:min]]: the hole filter of the adapter
// (sgm_set_fill_params). Case and surrounding blanks are ignored; gap and min are 1 to 6 decimal
// digits (defaults 16 and 2) and are passed on as they are (a value out of range fails at match
// time). Unset or blank: off. An unparsable value gives off and a note on stderr (the Python
// mirror's fill_from_env does the same).
sgm_fill_params fill_from_env()
{
    sgm_fill_params off;
    sgm_default_fill_params(&off);
    const char* e = std::getenv("SGM_HIP_FILL");
    if (!e) return off;
    const std::string v = trimmed_lower(e);
    if (v.empty()) return off;
    std::vector<std::string> parts(1);
    for (char c : v) {
        if (c == ':') parts.emplace_back();
        else parts.back() += c;
    }
    sgm_fill_params f = off;
    bool ok = parts.size() <= 3;
    if (parts[0] == "off") f.mode = SGM_FILL_OFF;
    else if (parts[0] == "background") f.mode = SGM_FILL_BACKGROUND;
    else if (parts[0] == "median") f.mode = SGM_FILL_MEDIAN;
    else ok = false;
    for (size_t i = 1; ok && i < parts.size(); i++) {
        const std::string& n = parts[i];
        ok = !n.empty() && n.size() <= 6;
        for (char c : n) ok = ok && c >= '0' && c <= '9';
        if (ok) (i == 1 ? f.max_gap : f.min_neighbours) = std::atoi(n.c_str());
    }
    if (!ok) {
        std::cerr << "SGM_HIP_FILL=\"" << e << "\" is not off | background | median[:gap[:min]]: hole filling off"
                  << std::endl;
        return off;
    }
    return f;
}

bool fill_when_interp_from_env()
{
    const char* e = std::getenv("SGM_HIP_FILL_WHEN");
    if (!e) return false;
    const std::string v = trimmed_lower(e);
    if (v.empty() || v == "always") return false;
    if (v == "interp") return true;
    std::cerr << "SGM_HIP_FILL_WHEN=\"" << e << "\" is not always | interp: using always" << std::endl;
    return false;
}

// SGM_HIP_PYRAMID = 0 | 1 | scale: the pyramid level of the adapter (sgm_set_pyramid_params). Case
// and surrounding blanks are ignored. "scale": *follow_scale, setDownsampleScale drives the level.
// Unset or blank: level 0. Another value gives level 0 and a note on stderr (the Python mirror's
// pyramid_from_env does the same).
int pyramid_from_env(bool* follow_scale)
{
    if (follow_scale) *follow_scale = false;
    const char* e = std::getenv("SGM_HIP_PYRAMID");
    if (!e) return 0;
    const std::string v = trimmed_lower(e);
    if (v.empty() || v == "0") return 0;
    if (v == "1") return 1;
    if (v == "scale") {
        if (follow_scale) *follow_scale = true;
        return 0;
    }
    std::cerr << "SGM_HIP_PYRAMID=\"" << e << "\" is not 0 | 1 | scale: pyramid level 0" << std::endl;
    return 0;
}

MatcherCore::MatcherCore(int device, int mode) : device_(device)
{
    pyramid_level_ = pyramid_from_env(&pyramid_scale_);
    census_paths_ = census_paths_from_env(8);
    census_window_ = census_window_from_env(&census_window_cfg_);
    fill_ = fill_from_env();
    fill_when_interp_ = fill_when_interp_from_env();
    if (mode < 0) {
        const char* env = std::getenv("SGM_HIP_MODE");
        mode = env ? std::atoi(env) : SGM_MODE_OCV_SGBM5;
    }
    sgm_default_params(&params_, mode);
    sgm_default_bm_params(&bm_);
    if (mode == SGM_MODE_OCV_BM) {
        // cv::StereoBM::create(64, 9): minDisparity 0, preFilterCap 31 / size 9, texture 10,
        // uniqueness 15, no speckle filter, disp12MaxDiff -1
        params_.min_disparity = 0;
        params_.num_disparities = 64;
        params_.block_size = 9;
        params_.prefilter_cap = 31;
        params_.uniqueness_ratio = 15;
        params_.speckle_window_size = params_.speckle_range = 0;
        params_.disp12_max_diff = -1;
        bm_.texture_threshold = 10;
        bm_.prefilter_size = 9;
        return;
    }
    params_.ocv_compat = ocv_compat_from_env(params_.ocv_compat);
    // cv::StereoSGBM::create(64, 9, 5) (matcherOpenCVSGBM.cpp:14): overwritten by the setters
    params_.min_disparity = 64;
    params_.num_disparities = 9;
    params_.block_size = 5;
    params_.p1 = params_.p2 = params_.uniqueness_ratio = params_.disp12_max_diff = 0;
    params_.prefilter_cap = params_.speckle_window_size = params_.speckle_range = 0;
}

MatcherCore::~MatcherCore()
{
    releaseOutput();
    sgm_destroy(handle_);
}

void MatcherCore::keepOutputRegistered(bool enable)
{
    keep_reg_ = enable;
    if (!enable) releaseOutput();
}

void MatcherCore::releaseOutput()
{
    if (reg_ptr_ && handle_) (void)sgm_host_unregister(handle_, reg_ptr_);
    reg_ptr_ = nullptr;
    reg_bytes_ = 0;
}

void MatcherCore::setDisparityRange(int r, int image_width)
{
    r = r > 0 ? r : ((image_width / 8) + 15) & -16;
    params_.num_disparities = r;
}
void MatcherCore::setWindowSize(int w)
{
    params_.block_size = w;
    if (census_window_cfg_) (void)sgm_census_window_from_size(w, &census_window_);   // the one slider table
}
void MatcherCore::setMinDisparity(int d) { params_.min_disparity = d; }
void MatcherCore::setUniquenessRatio(int r) { params_.uniqueness_ratio = r; }
void MatcherCore::setSpeckleFilterWindow(int w) { params_.speckle_window_size = w; }
void MatcherCore::setSpeckleFilterRange(int r) { params_.speckle_range = r; }
void MatcherCore::setDisp12MaxDiff(int d) { params_.disp12_max_diff = d; }
void MatcherCore::setPreFilterCap(int c) { params_.prefilter_cap = c; }
void MatcherCore::setP1(float p1) { params_.p1 = (int)p1; }
void MatcherCore::setP2(float p2) { params_.p2 = (int)p2; }
void MatcherCore::setInterpolation(bool e) { interpolate_ = e; }
void MatcherCore::setMode(int m) { params_.mode = m; }
void MatcherCore::setOcvCompat(int bits) { params_.ocv_compat = bits; }
void MatcherCore::setCensusPaths(int paths) { census_paths_ = paths; }
void MatcherCore::setCensusWindow(int taps_x, int taps_y, int step) { census_window_ = sgm_census_window{taps_x, taps_y, step}; }
void MatcherCore::setCensusWindowFollowsSize(bool follow) { census_window_cfg_ = follow; }
void MatcherCore::setHoleFilling(int mode, int max_gap, int min_neighbours) { fill_ = sgm_fill_params{mode, max_gap, min_neighbours}; }
void MatcherCore::setFillWhenInterp(bool interp) { fill_when_interp_ = interp; }
void MatcherCore::setPyramidLevel(int level) { pyramid_level_ = level; }
void MatcherCore::setPyramidFollowsScale(bool follow) { pyramid_scale_ = follow; }
void MatcherCore::setDownsampleScale(double scale)
{
    if (pyramid_scale_) pyramid_level_ = scale <= 0.5 ? 1 : 0;
}
sgm_fill_params MatcherCore::effectiveFill() const
{
    sgm_fill_params f = fill_;
    if (!fill_when_interp_) return f;
    if (!interpolate_) f.mode = SGM_FILL_OFF;
    else if (f.mode == SGM_FILL_OFF) f.mode = SGM_FILL_BACKGROUND;
    return f;
}
void MatcherCore::setTextureThreshold(int t) { bm_.texture_threshold = t; }
void MatcherCore::setPreFilterSize(int s) { bm_.prefilter_size = s; }

sgm_params MatcherCore::rightMatcherParams(const sgm_params& p)
{
    sgm_params r = p;
    r.min_disparity = -(p.min_disparity + p.num_disparities) + 1;
    r.uniqueness_ratio = 0;
    if (p.mode == SGM_MODE_OCV_BM) {
        r.speckle_window_size = r.speckle_range = 0;
        return r;
    }
    r.disp12_max_diff = 1000000;
    r.speckle_window_size = 0;
    return r;
}

sgm_bm_params MatcherCore::rightMatcherBmParams(const sgm_bm_params& b)
{
    sgm_bm_params r = b;
    r.texture_threshold = 0;
    return r;
}

// One host-buffer match: float32 output (the CV_32FC1 of matcherOpenCVSGBM.cpp:34, converted
// on the device by sgm_match_f32) or int16 (CV_16S, the right matcher's disparity_rl).
int MatcherCore::run(const sgm_params& p, const sgm_bm_params& bm, const uint8_t* a, const uint8_t* b, int w, int h,
                     size_t stride, float* outf, int16_t* out16, size_t out_stride)
{
    int rc = SGM_OK;
    if (!handle_) rc = sgm_create(&handle_, device_);
    if (rc == SGM_OK) rc = sgm_set_params(handle_, &p);
    if (rc == SGM_OK) rc = sgm_set_bm_params(handle_, &bm);
    if (rc == SGM_OK) rc = sgm_set_census_paths(handle_, census_paths_);
    if (rc == SGM_OK) rc = sgm_set_census_window(handle_, &census_window_);
    const sgm_fill_params fill = effectiveFill();
    if (rc == SGM_OK) rc = sgm_set_fill_params(handle_, &fill);
    sgm_pyramid_params pyr;
    sgm_default_pyramid_params(&pyr);
    pyr.level = pyramid_level_;
    if (rc == SGM_OK) rc = sgm_set_pyramid_params(handle_, &pyr);
    if (rc == SGM_OK && keep_reg_ && outf) {
        const size_t bytes = out_stride * sizeof(float) * (size_t)(h - 1) + (size_t)w * sizeof(float);
        if (reg_ptr_ != (void*)outf || reg_bytes_ != bytes) {
            releaseOutput();
            // not fatal: an unregistered output takes one synchronous copy
            if (sgm_host_register(handle_, outf, bytes) == SGM_OK) { reg_ptr_ = outf; reg_bytes_ = bytes; }
        }
    }
    if (rc == SGM_OK)
        rc = outf ? sgm_match_f32(handle_, a, b, w, h, stride, outf, out_stride)
                  : sgm_match(handle_, a, b, w, h, stride, out16, out_stride);
    if (rc != SGM_OK) {
        err_ = handle_ ? sgm_last_error(handle_) : "no HIP device";
        // matcherOpenCVBlock.cpp:40 / matcherOpenCVSGBM.cpp:40 style
        std::cerr << (p.mode == SGM_MODE_OCV_BM ? "Error in HIP StereoBM parameters" : "Error in HIP SGM parameters") << std::endl
                  << err_ << " (status " << rc << ")" << std::endl;
        return -1;
    }
    return 0;
}

void MatcherCore::disparityWindow(double f, double T, double depth_min, double depth_max, float* min_disp,
                                  float* max_disp)
{
    *min_disp = (float)(T * f / depth_max);
    *max_disp = depth_min != 0 ? (float)(T * f / depth_min) : std::numeric_limits<float>::infinity();   // Q8
}

int MatcherCore::mapBuilds() const { return sgm_node_frame_map_builds(handle_); }

int MatcherCore::imageCb(const uint8_t* raw_left, const uint8_t* raw_right, int w, int h, int channels,
                         size_t raw_stride, const sgm_camera_info& info_left, const sgm_camera_info& info_right,
                         double f, double T, double depth_min, double depth_max, uint8_t* rect_left,
                         uint8_t* rect_right, size_t rect_stride, float* disparity, size_t disparity_stride,
                         float* depth, size_t depth_stride, const double* q5)
{
    const bool q3 = this->q3();      // interp on and not taken over by the hole filter
    const sgm_params p = q3 ? rightMatcherParams(params_) : params_;
    const sgm_bm_params bm = q3 ? rightMatcherBmParams(bm_) : bm_;
    const sgm_fill_params fill = effectiveFill();
    sgm_node_frame_io io{};
    io.struct_size = sizeof io;
    io.raw_left = q3 ? raw_right : raw_left;       // Q3: the right matcher on (right, left)
    io.raw_right = q3 ? raw_left : raw_right;
    io.raw_stride = raw_stride;
    io.width = w;
    io.height = h;
    disparityWindow(f, T, depth_min, depth_max, &io.min_disparity, &io.max_disparity);
    io.rect_left = q3 ? rect_right : rect_left;
    io.rect_right = q3 ? rect_left : rect_right;
    io.rect_stride = rect_stride;
    io.disparity = disparity;
    io.disparity_stride = disparity_stride;
    io.depth = depth;
    io.depth_stride = depth_stride;
    io.q5 = q5;
    io.depth_min = depth_min;
    io.depth_max = depth_max;
    int rc = SGM_OK;
    if (!handle_) rc = sgm_create(&handle_, device_);
    if (rc == SGM_OK) rc = sgm_set_params(handle_, &p);
    if (rc == SGM_OK) rc = sgm_set_bm_params(handle_, &bm);
    if (rc == SGM_OK) rc = sgm_set_census_paths(handle_, census_paths_);
    if (rc == SGM_OK) rc = sgm_set_census_window(handle_, &census_window_);
    if (rc == SGM_OK) rc = sgm_set_fill_params(handle_, &fill);
    sgm_pyramid_params pyr;
    sgm_default_pyramid_params(&pyr);
    pyr.level = pyramid_level_;
    if (rc == SGM_OK) rc = sgm_set_pyramid_params(handle_, &pyr);
    // colour frames: the grey set of the OpenCV release the compat bits name (COL0_LEGACY marks 3.x)
    if (rc == SGM_OK)
        rc = sgm_set_raw_format(handle_, channels, (p.ocv_compat & SGM_OCV_COL0_LEGACY) ? SGM_GRAY_Y14 : SGM_GRAY_Y15);
    if (rc == SGM_OK && keep_reg_ && disparity && h > 0) {
        const size_t bytes = disparity_stride * sizeof(float) * (size_t)(h - 1) + (size_t)w * sizeof(float);
        if (reg_ptr_ != (void*)disparity || reg_bytes_ != bytes) {
            releaseOutput();
            // not fatal: an unregistered output takes one synchronous copy
            if (sgm_host_register(handle_, disparity, bytes) == SGM_OK) { reg_ptr_ = disparity; reg_bytes_ = bytes; }
        }
    }
    if (rc == SGM_OK)
        rc = sgm_node_frame(handle_, q3 ? &info_right : &info_left, q3 ? &info_left : &info_right, &io);
    if (rc != SGM_OK) {
        err_ = handle_ ? sgm_last_error(handle_) : "no HIP device";
        std::cerr << (p.mode == SGM_MODE_OCV_BM ? "Error in HIP StereoBM parameters" : "Error in HIP SGM parameters") << std::endl
                  << err_ << " (status " << rc << ")" << std::endl
                  << "Failed to compute stereo match" << std::endl;
        return -1;
    }
    return 0;
}

int MatcherCore::forwardMatch(const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, float* out,
                              size_t out_stride)
{
    if (q3())  // Q3: WLS output discarded, right-view disparity returned
        return backwardMatch(left, right, w, h, stride, out, out_stride);
    return run(params_, bm_, left, right, w, h, stride, out, nullptr, out_stride);
}

int MatcherCore::backwardMatch(const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, float* out,
                               size_t out_stride)
{
    return run(rightMatcherParams(params_), rightMatcherBmParams(bm_), right, left, w, h, stride, out, nullptr,
               out_stride);
}

int MatcherCore::backwardMatch16(const uint8_t* left, const uint8_t* right, int w, int h, size_t stride, int16_t* out,
                                 size_t out_stride)
{
    return run(rightMatcherParams(params_), rightMatcherBmParams(bm_), right, left, w, h, stride, nullptr, out,
               out_stride);
}

}  // namespace sgm_hip
