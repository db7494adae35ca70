/*
 * sgm_hip.h — C-ABI of the MI355X-native Semi-Global Matching engine (libsgm_hip.so).
 *
 * This is the drop-in boundary for the reference's stereo-matcher plugin surface.
 * It replaces the work that `MatcherOpenCVSGBM::forwardMatch` delegates to
 * `cv::StereoSGBM::compute` (reference: src/stereoMatcher/matcherOpenCVSGBM.cpp:17-44,
 * call at :21) and is called from the plugin adapter `MatcherHIPSGM`
 * (i3dr_stereo_camera-ros_amd/plugin/matcherHIPSGM.{h,cpp}), a subclass of the
 * reference's `AbstractStereoMatcher` (include/stereoMatcher/abstractStereoMatcher.h:12-92).
 *
 * Plain C types only: pointers, sizes, ints. No torch / OpenCV / HIP types in signatures
 * (streams are passed as `void*` = hipStream_t).
 *
 * Output contract (identical to the reference's SGBM path, abstractStereoMatcher.cpp:44-53,
 * generate_disparity.cpp:403-436): int16 disparity in 1/16-pixel fixed point
 * (OpenCV DISP_SCALE = 16); invalid pixels = (min_disparity - 1) * 16; columns outside
 * [max(maxD,0), W + min(minD,0)) are invalid.
 *
 * Error convention (reference: matcherOpenCVSGBM.cpp:37-43 returns -1 on cv::Exception;
 * generate_disparity.cpp:355-365 logs and publishes nothing): every call returns an int
 * status, 0 = OK, < 0 = error class below; `sgm_last_error()` gives the text. The adapter
 * maps any non-zero status to -1, exactly like the OpenCV wrapper.
 */
#ifndef SGM_HIP_H
#define SGM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ABI version ------------------------------------------------------------------- */
/* Bumped whenever a struct or signature of this header changes. Round 3 grew sgm_params
 * from 14 to 15 ints (ocv_compat, version 3); round 4 added sgm_match_tiled_device
 * (version 4); version 5 adds SGM_MODE_OCV_BM with the sgm_bm_params entry points. A caller
 * compiled against an older header must check sgm_abi_version() == SGM_ABI_VERSION before
 * passing an sgm_params (a 14-int struct would be read one int past its end).
 * sgm_set_census_paths / sgm_get_census_paths were added under version 5: they change no
 * existing struct or signature (sgm_params stays 15 ints), so the version did not move; a
 * caller that needs them checks for the symbols. The colour entry points (sgm_bgr2gray,
 * sgm_remap_cubic_c3, sgm_set_raw_format, sgm_get_raw_format) came the same way, and so did
 * sgm_node_frame / sgm_node_frame_map_builds with their two structs, and the census window
 * entry points (sgm_*_census_window*) with sgm_census_window, and the pyramid entry points
 * (sgm_*_pyramid_params, sgm_pyramid_plan, sgm_debug_pyr_*) with sgm_pyramid_params.           */
#define SGM_ABI_VERSION 5
int  sgm_abi_version(void);

/* ---- status codes ------------------------------------------------------------------ */
#define SGM_OK                0
#define SGM_ERR_ARG          -1   /* null pointer, bad size / stride                      */
#define SGM_ERR_PARAM        -2   /* invalid matcher parameters (e.g. D % 16 != 0)       */
#define SGM_ERR_DEVICE       -3   /* no HIP device / HIP runtime failure                  */
#define SGM_ERR_ALLOC        -4   /* device / host allocation failure                     */
#define SGM_ERR_UNSUPPORTED  -5   /* parameter combination this build does not implement */

/* ---- matching modes ---------------------------------------------------------------- */
/* OpenCV-compatible modes: Birchfield-Tomasi cost on the Sobel-prefiltered + raw image,
 * SAD block aggregation, int16 path costs. Bit-exact with the CPU oracle's restatement of
 * cv::StereoSGBM (oracle/sgm_oracle.c).                                                   */
#define SGM_MODE_OCV_SGBM5    0   /* cv::StereoSGBM::MODE_SGBM: 5 directions (reference default, Q1) */
#define SGM_MODE_OCV_HH8      1   /* cv::StereoSGBM::MODE_HH: 8 directions (cfg `fullDP`)             */
/* North-star mode: 9x7 census, Hamming cost, 8 directions, u8 path costs, u16 sums.       */
#define SGM_MODE_CENSUS8      2
/* cv::StereoBM, the generate_disparity node's default algorithm (generate_disparity.cpp:98):
 * XSOBEL pre-filter, SAD block matching, winner-takes-all with texture / uniqueness tests and
 * the StereoBM sub-pixel formula, optional speckle filter; no path aggregation, no median.
 * A restatement of OpenCV's scalar findStereoCorrespondenceBM (BM section),
 * unverified against a real OpenCV. Uses sgm_params' min_disparity, num_disparities,
 * block_size, prefilter_cap, uniqueness_ratio, speckle_*, disp12_max_diff (must be < 0: off)
 * plus sgm_bm_params; p1, p2, subpixel, lr_check, median and ocv_compat are ignored. Nothing
 * is repaired in this mode: invalid values are SGM_ERR_PARAM at match time.                */
#define SGM_MODE_OCV_BM       3

/* OpenCV build variants of the OCV modes (`sgm_params.ocv_compat`, a bitfield). The reference
 * pins OpenCV only through its ROS distro — melodic (OpenCV 3.2.0, the reference's Dockerfile:1,
 * amd64) and noetic (OpenCV 4.2.0; CI matrix .github/workflows/ros-build.yml:14-21) — and
 * computeDisparitySGBM differs between those releases and between its scalar and SIMD (SSE2 /
 * universal-intrinsic, every x86-64 build) branches. Bits:
 *   COL0_LEGACY  3.x cost loop: C' column 0 is never updated for rows y > 0
 *   SIMD_SAT     saturating int16 box sums, path recurrence and S (SIMD branches)
 *   LANE_TIE     3.x SSE2 MODE_SGBM WTA: among equal minimal sums the lowest lane (d mod 8) wins
 * The three agree with the scalar restatement except on column 0 (COL0, every frame), on int16
 * overflow (SIMD_SAT) and on exact cross-lane ties (LANE_TIE). Census mode ignores the field. */
#define SGM_OCV_COL0_LEGACY   1
#define SGM_OCV_SIMD_SAT      2
#define SGM_OCV_LANE_TIE      4
#define SGM_OCV_COMPAT_SCALAR   0                      /* the scalar 4.x restatement            */
#define SGM_OCV_COMPAT_NOETIC   SGM_OCV_SIMD_SAT      /* noetic x86-64: OpenCV 4.2, SIMD        */
#define SGM_OCV_COMPAT_MELODIC  (SGM_OCV_COL0_LEGACY | SGM_OCV_SIMD_SAT | SGM_OCV_LANE_TIE)
                                                       /* melodic x86-64 (the Docker image): 3.2, SSE2;
                                                        * the default of sgm_default_params      */

/* Parameter block. Field names follow the reference's setters
 * (abstractStereoMatcher.h:27-48) and cfg/i3DR_Disparity.cfg:21-39.                      */
typedef struct sgm_params {
    int mode;                 /* SGM_MODE_*                                               */
    int min_disparity;        /* setMinDisparity                  (cfg min_disparity)     */
    int num_disparities;      /* setDisparityRange, multiple of 16 (cfg disparity_range)  */
    int block_size;           /* setWindowSize: OCV SAD window (cfg correlation_window_size); census: ignored (its window: sgm_set_census_window) */
    int p1;                   /* setP1 (float in the reference API, truncated like OpenCV's int setter) */
    int p2;                   /* setP2                                                    */
    int uniqueness_ratio;     /* setUniquenessRatio (percent)                             */
    int disp12_max_diff;      /* setDisp12MaxDiff (<=0 -> 1, as OpenCV SGBM)              */
    int prefilter_cap;        /* setPreFilterCap (OCV modes)                              */
    int speckle_window_size;  /* setSpeckleFilterWindow (0 = speckle filter off)          */
    int speckle_range;        /* setSpeckleFilterRange (max diff in pixels; x16 internally; BM mode: unscaled) */
    int subpixel;             /* census: parabolic 1/16 interpolation on/off (OCV: always on) */
    int lr_check;             /* census: left-right (disp2) check on/off (OCV: always on)     */
    int median;               /* census: 3x3 median post-filter on/off (OCV: always on)       */
    int ocv_compat;           /* OCV modes: SGM_OCV_* bits of the OpenCV build to reproduce   */
} sgm_params;

/* The two cv::StereoBM parameters sgm_params has no field for (sgm_params stays 15 ints).
 * prefilter_size is validated (odd, 5..255) but otherwise unused: the pre-filter type is
 * always PREFILTER_XSOBEL, which the reference never changes.                              */
typedef struct sgm_bm_params {
    int texture_threshold;    /* setTextureThreshold (cfg texture_threshold), >= 0           */
    int prefilter_size;       /* setPreFilterSize    (cfg prefilter_size)                    */
} sgm_bm_params;

typedef struct sgm_handle sgm_handle;

/* ---- device / handle management ------------------------------------------------------ */
/* Number of visible HIP devices (0 if none / runtime unavailable). Never throws.           */
int  sgm_device_count(void);

/* Create a matcher handle bound to `device` (reference ctor: abstractStereoMatcher.h:15,
 * subclasses call init(), matcherOpenCVSGBM.h:10-14). Cheap: no device allocation happens
 * until the first match (the reference constructs every matcher lazily on the first frame,
 * generate_disparity.cpp:268-278). Returns SGM_ERR_DEVICE if `device` is not visible.     */
int  sgm_create(sgm_handle** out, int device);
void sgm_destroy(sgm_handle* h);

/* Page-lock and map a caller's host buffer (hipHostRegister, mapped) for as long as it stays
 * registered: a registered output of sgm_match / sgm_match_f32 is copied back by DMA without the
 * runtime's pageable staging, or — sgm_match_f32 in the census mode without median / speckles —
 * written by the WTA kernel itself as the rows finish. The caller must unregister a buffer
 * before freeing it (unregistering waits for the handle's last call; on failure the buffer stays
 * registered and mapped). sgm_destroy unregisters every buffer still registered through the
 * handle: HIP registrations are process-wide, so a caller that keeps using a buffer page-locked
 * after destroying the handle registers it again. The MatcherHIPSGM adapter registers its
 * persistent disparity_lr, matcherOpenCVSGBM.cpp:34's output Mat.                              */
int  sgm_host_register(sgm_handle* h, void* ptr, size_t bytes);
int  sgm_host_unregister(sgm_handle* h, void* ptr);

/* Defaults: census mode = north-star config (P1 10, P2 120, uniq 5, subpixel+LR on);
 * OCV modes = the generate_disparity node defaults (generate_disparity.cpp:100-112) and
 * ocv_compat = SGM_OCV_COMPAT_MELODIC (the OpenCV the reference's Dockerfile:1 ships).     */
void sgm_default_params(sgm_params* p, int mode);
/* SGM_MODE_OCV_BM defaults: sgm_default_params gives the node's values (min_disparity 9,
 * num_disparities 64, block_size 15, uniqueness 15, prefilter_cap 31, speckles 100 / 4,
 * disp12_max_diff -1); the BM-only pair defaults to texture_threshold 10, prefilter_size 9. */
void sgm_default_bm_params(sgm_bm_params* p);
/* The BM-only parameters of a handle (used by SGM_MODE_OCV_BM matches only).                */
int  sgm_set_bm_params(sgm_handle* h, const sgm_bm_params* p);
int  sgm_get_bm_params(const sgm_handle* h, sgm_bm_params* p);

/* Census mode: the number of aggregation paths, per handle. 8 (the default): all eight
 * directions. 4: only the axis directions (down, up, left-to-right, right-to-left; directions
 * 0, 1, 6, 7 of sgm_debug_census_path), S being the u16 sum of those four u8 volumes; each
 * volume comes from the same recurrence (P1, P2 clamp at 193, path starts) and the WTA,
 * uniqueness, sub-pixel, LR check, median and speckle steps run unchanged on that S. Four paths
 * write and read 3 volumes per pipelined frame where eight take 7 and need half the volume
 * workspace; they trade quality for speed (the diagonals no longer smooth slanted structure).
 * Like every setter this stores any value: one other than 4 or 8 is SGM_ERR_PARAM at match
 * time in the census mode. The OCV and BM modes ignore it. Honoured by sgm_match,
 * sgm_match_f32, sgm_match_device, sgm_match_device_batch[_rect], sgm_match_batch,
 * sgm_match_tiled and sgm_match_tiled_device (sub-handles inherit it);
 * sgm_match_tiled_exact runs with 8 paths only (SGM_ERR_UNSUPPORTED with 4: its seam exchange
 * carries three directions per sweep family; left for later). With 4 paths the profiling
 * stages are named paths4 / paths3+up_wta.. in place of paths8 / paths7+up_wta.. and
 * sgm_stage_bytes follows the set (paths4: 4 bytes per cell).                               */
int  sgm_set_census_paths(sgm_handle* h, int paths);
int  sgm_get_census_paths(const sgm_handle* h, int* paths);

/* Census mode: the census window, per handle: what setWindowSize means for the census matcher
 * (the I3DR matcher resizes its census window the same way). Specified by this project;
 * tests/census_window_reference.py is the executable statement. A window is
 * (taps_x, taps_y, step) with taps_x in {3, 5, 7, 9}, taps_y in {3, 5, 7}, step in {1, 2}; the
 * default {9, 7, 1} is the 9x7 window.
 *   - tap (j, i), j in [-(taps_y-1)/2, (taps_y-1)/2], i in [-(taps_x-1)/2, (taps_x-1)/2], compares
 *     I(clamp(y + step*j), clamp(x + step*i)) < I(y, x) (replicate clamping, as the 9x7 census);
 *   - its bit is the one the offset (dy = j, dx = i) has in the 9x7 code: raster order over
 *     dy = -3..3, dx = -4..4, centre skipped, LSB first; bits of taps outside the window are 0.
 * So a code stays a uint64_t of at most 62 bits and the Hamming cost stays <= 62; a dense
 * (step 1) window's code equals code_9x7 & mask(taps_x, taps_y); {9, 7, 2} spans 17 x 13 pixels;
 * and everything after the codes (path recurrence with its P2 <= 193 clamp, WTA, uniqueness,
 * sub-pixel, LR check, median, speckles, hole filling, 4 or 8 paths) is unchanged.
 * Like every setter sgm_set_census_window stores any value: an invalid window is SGM_ERR_PARAM
 * at match time in the census mode; the OCV and BM modes ignore it. Honoured by sgm_match,
 * sgm_match_f32, sgm_match_device, sgm_match_device_batch[_rect], sgm_match_batch,
 * sgm_node_frame, sgm_match_tiled, sgm_match_tiled_device and sgm_match_tiled_exact (whose band
 * images carry 3 * step halo rows), with colour and raw frames wherever the default window takes
 * them; sub-handles inherit it; sgm_debug_census and sgm_debug_census_path use it too.
 * With the default window nothing changes (same launches, stage names and workspace). With any
 * other the census is a launch of its own on 8UC1 planes (profiling stage `census_win`,
 * sgm_stage_bytes 1 B/px read and 8 B/px written per image) and the pipelined batch's fused
 * launches carry no census (their stage names lose the `+census`); colour and / or raw frames
 * first go through the pre-pass of the OCV modes into per-handle grey planes (stage `gray`, or
 * `rectify`, which also writes the requested rectified images: bit-identical to the default
 * window's). Added under ABI version 5 (no existing struct or signature changed): callers check
 * for the symbols.                                                                             */
typedef struct sgm_census_window { int taps_x, taps_y, step; } sgm_census_window;
/* {9, 7, 1} */
void sgm_default_census_window(sgm_census_window* w);
int  sgm_set_census_window(sgm_handle* h, const sgm_census_window* w);
int  sgm_get_census_window(const sgm_handle* h, sgm_census_window* w);
/* Validate a window without a handle (0 = a census match would accept it). Host-only.          */
int  sgm_check_census_window(const sgm_census_window* w);
/* The window of a correlation_window_size slider value (cfg/i3DR_Disparity.cfg), the one table
 * the adapters use: w|1 <= 3: {3,3,1}; 5: {5,5,1}; 7: {7,7,1}; 9: {9,7,1}; 11, 13: {7,7,2};
 * >= 15: {9,7,2} (even values count as the next odd one). Host-only.                           */
int  sgm_census_window_from_size(int w, sgm_census_window* out);

/* ---- hole filling ------------------------------------------------------------------------- */
/* The post filter behind the node's `interp` knob (cfg/i3DR_Disparity.cfg:39, "will smooth
 * holes"): a bounded 8-direction nearest-valid interpolation of the final int16 disparity, run
 * after median and speckle filter (profiling stage `fill`, last of the post filters;
 * sgm_stage_bytes: 2 B/px read + 2 B/px written). Specified by this project (the I3DR matcher's
 * interpolator is closed, and the OpenCV matchers' WLS result never reaches the node's output,
 * SURVEY Q3); tests/fill_reference.py is the executable statement. Off by default.
 *   - invalid = (min_disparity - 1) * 16. A hole is a pixel of the fill rectangle that equals
 *     invalid; every other pixel is copied.
 *   - each of the 8 directions (left, right, up, down and the four diagonals, one pixel on both
 *     axes per step) contributes at most one candidate: the pixel at the smallest k in
 *     1..max_gap steps that lies inside the image and is not invalid. Candidates may lie outside
 *     the rectangle and are always read from the input, never from a filled pixel, so the result
 *     does not depend on any processing order.
 *   - with n candidates sorted v_0 <= .. <= v_{n-1}: n < min_neighbours leaves the pixel
 *     invalid; SGM_FILL_BACKGROUND takes v_1 (v_0 when n == 1): the second-lowest value prefers
 *     the background and tolerates one outlier; SGM_FILL_MEDIAN takes the lower median
 *     v_{(n-1)/2}. SGM_FILL_OFF is a plain copy.
 *   - inside a match the rectangle is the region where the mode can produce a disparity:
 *     columns [max(maxD, 0), W + min(minD, 0)) and all rows for the SGBM, HH and census modes;
 *     columns [X0, X1) of sgm_debug_bm_sad and rows [w/2, H - w/2) for BM. A frame without a
 *     disparity window stays all invalid.
 * Like every setter sgm_set_fill_params stores any value; with a mode other than SGM_FILL_OFF,
 * a mode that is not BACKGROUND or MEDIAN, max_gap outside 1..255 or min_neighbours outside 1..8
 * is SGM_ERR_PARAM at match time. Honoured by sgm_match, sgm_match_f32, sgm_match_device,
 * sgm_match_device_batch[_rect], sgm_match_batch, sgm_node_frame (disparity and depth) and
 * sgm_match_tiled_exact (its post filters run on the assembled frame); sub-handles inherit it.
 * sgm_match_tiled and sgm_match_tiled_device return SGM_ERR_UNSUPPORTED while it is on: filling
 * band by band would differ at the seams. While it is on, the two "the WTA writes the float rows
 * itself" shortcuts (sgm_match_f32, sgm_node_frame) are not taken. Added under ABI version 5
 * (no existing struct or signature changed): callers check for the symbols.                   */
#define SGM_FILL_OFF         0
#define SGM_FILL_BACKGROUND  1
#define SGM_FILL_MEDIAN      2
typedef struct sgm_fill_params {
    int mode;                 /* SGM_FILL_*                                                    */
    int max_gap;              /* G: the farthest step a candidate may lie away, 1..255         */
    int min_neighbours;       /* N: candidates a hole needs to be filled, 1..8                 */
} sgm_fill_params;
/* {SGM_FILL_OFF, 16, 2} */
void sgm_default_fill_params(sgm_fill_params* p);
int  sgm_set_fill_params(sgm_handle* h, const sgm_fill_params* p);
int  sgm_get_fill_params(const sgm_handle* h, sgm_fill_params* p);
/* Validate fill parameters without a handle (0 = a match would accept them). Host-only.       */
int  sgm_check_fill_params(const sgm_fill_params* p);
/* The filter alone on device buffers, asynchronous on `stream` (NULL = the handle's stream) like
 * sgm_disparity_to_msg: d_src -> d_dst (width x height int16, strides in elements), holes of
 * [x0, x1) x [y0, y1) (0 <= x0 <= x1 <= width, 0 <= y0 <= y1 <= height) filled under `params`
 * (validated as above; the handle's own fill parameters are not used). d_dst == d_src is
 * SGM_ERR_ARG. It uses the handle's workspace, so it is ordered with the handle's other calls. */
int  sgm_fill_holes(sgm_handle* h, const int16_t* d_src, size_t src_stride, int width, int height, int invalid,
                    const sgm_fill_params* params, int x0, int y0, int x1, int y1, int16_t* d_dst,
                    size_t dst_stride, void* stream);

/* ---- half-resolution pyramid level --------------------------------------------------------- */
/* Coarse-to-fine matching with one coarse level, per handle: the pair is halved, the handle's mode
 * matches the coarse pair over half the disparity range, and a refinement kernel brings the result
 * back to full resolution on census codes of the full-resolution images. A quarter of the pixels
 * times half the disparities is about an eighth of the matching work, and the census mode reaches
 * num_disparities up to 1024 (its 512 cap applies to the coarse range). Specified by this project
 * (the I3DR matcher the census mode stands in for is a closed coarse-to-fine matcher);
 * tests/pyramid_reference.py is the executable statement. Level 0 (the default) is a plain match:
 * same launches, stage names, workspace and results. Level 1, for a W x H frame with
 * m = min_disparity and D = num_disparities:
 *   1. coarse geometry: Wc = (W + 1) >> 1, Hc = (H + 1) >> 1, mc = m >> 1 (arithmetic shift),
 *      Dc = 16 * ceil((((m + D - 1) >> 1) - mc + 1) / 16).
 *   2. down: Ic(xc, yc) = (I(x0,y0) + I(x1,y0) + I(x0,y1) + I(x1,y1) + 2) >> 2 with x0 = 2 xc,
 *      x1 = min(2 xc + 1, W - 1), likewise for y, on both 8UC1 images (profiling stage `pyr_down`).
 *      Colour and raw frames first go through the pre-pass of the OCV modes into full-resolution
 *      grey planes (stage `gray`, or `rectify`, which writes the requested rectified images
 *      unchanged), in every mode.
 *   3. coarse match: exactly a level-0 match of (Lc, Rc) in the handle's mode with (mc, Dc) and
 *      every other setting unchanged, hole filling off. Median and speckle filters therefore run
 *      at coarse resolution with unscaled values: a coarse pixel covers four, so a speckle window
 *      of n coarse pixels removes regions of up to 4 n full-resolution pixels. Its stages are
 *      profiled under their usual names with the bytes of the coarse geometry.
 *   4. refine (stage `pyr_refine`): KL, KR are the 24-bit 5x5 census codes of the full-resolution
 *      grey images (raster over dy = -2..2, dx = -2..2, centre skipped, LSB first; bit =
 *      I(clamp(y + dy), clamp(x + dx)) < I(y, x)), and h(x, y, d) the sum over j, i in {-1, 0, 1} of
 *      popcount(KL(cx(x + i), cy(y + j)) ^ KR(cx(x + i - d), cy(y + j))), cx / cy clamping to the
 *      image. Per pixel, c = C(x >> 1, y >> 1): c == (mc - 1) * 16 gives (m - 1) * 16 (invalid);
 *      else d0 = (2 c + 8) >> 4 and the candidates d0 + k, k = 0, -1, +1, .. up to +-radius in that
 *      order, of which those inside [m, m + D - 1] count; the smallest h wins under a strict <
 *      (none inside: invalid). With sub-pixel on (the census mode's `subpixel`; always in the OCV
 *      and BM modes) and m < d* < m + D - 1: cm = h(d* - 1), cp = h(d* + 1), c0 = h(d*),
 *      den = cm + cp - 2 c0, and if cm >= c0, cp >= c0 and den > 0 the offset is
 *      ((cm - cp) * 16 + den) / (2 den) in C division. out = 16 d* + offset. Columns outside
 *      [max(m + D, 0), W + min(m, 0)) are invalid.
 *   5. hole filling, if on, runs last on the full-resolution image: those columns and all rows;
 *      BM: rows [2 (w / 2), min(H, 2 (Hc - w / 2))).
 * Like every setter sgm_set_pyramid_params stores any value: a level other than 0 or 1, or at
 * level 1 a radius outside 1..2, is SGM_ERR_PARAM at match time. At level 1 the full-resolution
 * parameters are checked as at level 0, except that the mode's range cap applies to Dc
 * (num_disparities <= 2048 stays for every mode), and every error of the coarse match (BM window
 * >= min(Wc, Hc), census Dc > 512, ..) is returned with a text naming the coarse geometry; all
 * errors are decided before any output byte is written. Honoured by sgm_match, sgm_match_f32,
 * sgm_match_device, sgm_match_device_batch[_rect] (a batch equals n single calls; its coarse frames
 * go through the level-0 batch in groups of at most 8) and sgm_node_frame, with mono, colour and
 * raw frames. The two "the WTA writes the float rows itself" shortcuts are not taken at level 1.
 * sgm_match_batch and the three sgm_match_tiled* calls return SGM_ERR_UNSUPPORTED at level 1 and
 * write nothing; the sgm_debug_* stage entry points run at level 0 whatever the level (they
 * still validate the pair like every parameter). sgm_stage_bytes: pyr_down
 * 2 B/px read, 0.5 B/px of coarse images and 8 B/px of code planes written; pyr_refine 8 B/px of
 * codes and 0.5 B/px of coarse disparity read, 2 B/px written. Added under ABI version 5 (no
 * existing struct or signature changed): callers check for the symbols.                          */
typedef struct sgm_pyramid_params {
    int level;                /* 0: off; 1: match at half resolution, refine at full resolution   */
    int radius;               /* level 1: full-resolution disparities searched each side, 1..2    */
} sgm_pyramid_params;
/* {0, 2} */
void sgm_default_pyramid_params(sgm_pyramid_params* p);
int  sgm_set_pyramid_params(sgm_handle* h, const sgm_pyramid_params* p);
int  sgm_get_pyramid_params(const sgm_handle* h, sgm_pyramid_params* p);
/* Validate pyramid parameters without a handle (0 = a match would accept them). Host-only.       */
int  sgm_check_pyramid_params(const sgm_pyramid_params* p);
/* The geometry a match of a width x height frame runs its matcher at (host-only, no handle):
 * out = {Wc, Hc, mc, Dc, invalid_c, invalid}; at level 0 that is {width, height, m, D, invalid,
 * invalid}. Returns 0, or the error a match would return (bm may be NULL: the BM defaults).      */
int  sgm_pyramid_plan(const sgm_params* p, const sgm_bm_params* bm, const sgm_pyramid_params* pyr, int width,
                      int height, int out[6]);

/* ---- colour frames ---------------------------------------------------------------------- */
/* The node accepts colour cameras: imageCb rectifies whatever encoding arrives
 * (generate_disparity.cpp:651-652, :674-675) and processDisparity converts both rectified images
 * with cv::cvtColor(COLOR_BGR2GRAY) before the matcher (:406-416). The two coefficient sets of
 * that conversion for 8UC3 -> 8UC1, over the bytes of a pixel in MEMORY order c0, c1, c2:
 *   SGM_GRAY_Y14  (c0*1868 + c1*9617 + c2*4899 + 2^13) >> 14   OpenCV 3.2 (melodic)
 *   SGM_GRAY_Y15  (c0*3735 + c1*19235 + c2*9798 + 2^14) >> 15  OpenCV 4.x (noetic)
 * Both are restatements: Y14 is what the Python mirror's bgr2gray() always did, Y15 is recalled
 * from OpenCV 4's colour code, and neither is verified against a real OpenCV (like every other
 * OpenCV restatement here). The node applies COLOR_BGR2GRAY whatever the message encoding, so an
 * RGB8 frame gets the R and B weights swapped; this API reproduces that: there is no channel-
 * order flag, callers pass the bytes as the node would see them.                            */
#define SGM_GRAY_Y14 0
#define SGM_GRAY_Y15 1

/* The raw format of the frames the match entry points take, per handle: channels 1 (8UC1, the
 * default) or 3 (interleaved 8UC3), and the grey set used with 3 channels (default
 * SGM_GRAY_Y14). Like every setter this stores any value: channels other than 1 or 3, or an
 * unknown grey set, are SGM_ERR_PARAM at match time. With channels = 3:
 *  - sgm_match, sgm_match_f32, sgm_match_device, sgm_match_device_batch and
 *    sgm_match_device_batch_rect take 8UC3 frames; their `stride` is in bytes (>= 3 * width).
 *  - under sgm_set_rectification the frames are raw colour, and the rectified outputs of
 *    sgm_match_device_batch_rect are rectified 8UC3 (rect_stride in bytes, >= 3 * width): what
 *    the node publishes and what sgm_depth_points(channels = 3) colours the cloud with.
 *  - the order is the node's: the colour image is remapped first, then converted; a grey image
 *    is never remapped. The census mode does both inside its census tiles (no grey image
 *    exists in memory); the OCV and BM modes produce both grey images in per-handle planes
 *    first and run their pipelines unchanged on those: a conversion alone for rectified frames
 *    (profiling stage `gray`), or, under sgm_set_rectification, the pre-pass that remaps the
 *    colour pixel and then converts it (stage `rectify`, which replaces `gray`).
 *  - sgm_match_batch, sgm_match_tiled, sgm_match_tiled_device and sgm_match_tiled_exact return
 *    SGM_ERR_UNSUPPORTED (their sub-handles do not carry the format yet).
 * sgm_stage_bytes of the census stages then counts 3 B/px read per image, plus 3 B/px per
 * rectified image written.                                                                  */
int  sgm_set_raw_format(sgm_handle* h, int channels, int gray_set);
int  sgm_get_raw_format(const sgm_handle* h, int* channels, int* gray_set);

/* Store parameters. Like the reference's setters this never fails on values; invalid
 * combinations surface at match time (matcherOpenCVSGBM.cpp:37-43 behaviour).            */
int  sgm_set_params(sgm_handle* h, const sgm_params* p);
int  sgm_get_params(const sgm_handle* h, sgm_params* p);

/* Validate parameters for a W-wide image without matching (0 = would run).                */
int  sgm_check_params(const sgm_params* p, int width, int height);
/* The same for SGM_MODE_OCV_BM with explicit BM parameters (sgm_check_params validates that
 * mode with sgm_default_bm_params).                                                        */
int  sgm_check_bm_params(const sgm_params* p, const sgm_bm_params* bm, int width, int height);

/* ---- matching -------------------------------------------------------------------------- */
/* Host buffers in, host buffer out; synchronous. L/R: W x H u8 mono (stride bytes), or 8UC3
 * after sgm_set_raw_format(h, 3, ..); disp: W x H int16 (out_stride in elements). Replaces
 * cv::StereoSGBM::compute (matcherOpenCVSGBM.cpp:21).                                      */
int  sgm_match(sgm_handle* h, const uint8_t* left, const uint8_t* right,
               int width, int height, size_t stride,
               int16_t* disp, size_t out_stride);

/* sgm_match with the CV_32FC1 output of the reference's matcher contract
 * (matcherOpenCVSGBM.cpp:34 `disparity_lr.convertTo(disparity_lr, CV_32FC1)`, still x16 fixed
 * point): the int16 -> float conversion runs on the device, so the caller's buffer is filled by
 * the D2H itself (out_stride in floats). Host buffers; synchronous.                        */
int  sgm_match_f32(sgm_handle* h, const uint8_t* left, const uint8_t* right,
                   int width, int height, size_t stride, float* disp, size_t out_stride);

/* Device buffers in/out (already resident in HBM), asynchronous on `stream` (hipStream_t,
 * NULL = the handle's own stream). The handle's device must own the buffers. Calls on one
 * handle share its workspace, so each call is ordered after the previous one whatever the
 * streams (an event recorded at the end of every call is waited on at the start of the next);
 * use one handle per concurrent stream to overlap matches.                                  */
int  sgm_match_device(sgm_handle* h, const uint8_t* d_left, const uint8_t* d_right,
                      int width, int height, size_t stride,
                      int16_t* d_disp, size_t out_stride, void* stream);

/* Frame batch, sharded frame i -> devices[i % n_dev] (SURVEY §8e "frame batch"). Each
 * device gets a driver thread, a packer and an unpacker thread, a compute stream and two
 * high-priority copy streams: its frames stream through pinned host rings (user rows ->
 * pinned -> H2D -> pipelined census batch / per-frame OCV pipeline -> D2H -> user rows), so
 * host copies, PCIe and kernels overlap. Host buffers with one row stride per side (stride,
 * out_stride in elements); synchronous; no cross-device traffic. n_dev <= 0 or
 * devices == NULL: all visible devices; a device may be listed more than once (one handle
 * per entry). Results equal sgm_match per frame.                                            */
int  sgm_match_batch(sgm_handle* h, const uint8_t* const* lefts, const uint8_t* const* rights,
                     int n_frames, int width, int height, size_t stride,
                     int16_t* const* disps, size_t out_stride,
                     const int* devices, int n_dev);

/* One large frame split into n_bands row bands (band b -> devices[b % n_dev]), SURVEY §8(e)
 * "single huge frame" in overlap mode: each band is matched on its rows extended by `halo`
 * rows above and below, and only its own rows are kept. No path state crosses bands, so
 * pixels near band seams can differ from the full-frame result (the tests report the
 * disagreement); n_bands = 1 is exactly sgm_match. Host buffers; synchronous. With hole
 * filling on (sgm_set_fill_params) this call and sgm_match_tiled_device return
 * SGM_ERR_UNSUPPORTED: a band filled alone would differ from the frame at its seams.     */
int  sgm_match_tiled(sgm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                     size_t stride, int16_t* disp, size_t out_stride, int n_bands, int halo,
                     const int* devices, int n_dev);

/* Overlap mode on device buffers (C5 with the frame already in HBM of h's device): band b's
 * rows + halo are copied to devices[b % n_dev] (hipMemcpyPeerAsync over xGMI when the device
 * differs), matched there with sgm_match_device on that device's sub-handle, and the band's
 * own rows are copied back into d_disp. One host thread + stream per device. Work queued on
 * `stream` (may be NULL) before the call is complete before the band copies start;
 * synchronous: d_disp is complete on return. Same results as sgm_match_tiled.             */
int  sgm_match_tiled_device(sgm_handle* h, const uint8_t* d_left, const uint8_t* d_right, int width, int height,
                            size_t stride, int16_t* d_disp, size_t out_stride, int n_bands, int halo,
                            const int* devices, int n_dev, void* stream);

/* The same band split in exact mode (SURVEY §8(e) "exact mode", census mode only): band b
 * continues the path lines of its neighbours. Its downward sweeps start from the last
 * volume row of band b-1 and its upward sweeps from the first row of band b+1. Those
 * boundary rows (3 directions x width1 x D u8 per seam) move device to device with
 * hipMemcpyPeerAsync (xGMI). The top-down and bottom-up chains run concurrently; the WTA of a
 * band uses only its own rows, and median/speckle filters run on the assembled frame on h's
 * device. The result is bit-identical to sgm_match for any band count. Host buffers;
 * synchronous. Replaces nothing in the reference (no reference tile mode exists); the
 * per-frame contract is that of cv::StereoSGBM::compute (matcherOpenCVSGBM.cpp:21).       */
int  sgm_match_tiled_exact(sgm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                           size_t stride, int16_t* disp, size_t out_stride, int n_bands,
                           const int* devices, int n_dev);

/* Frame batch on device buffers (host arrays of n_frames device pointers), asynchronous on
 * `stream`. Census mode pipelines the frames: the path aggregation of frame i+1 and the
 * WTA of frame i run in ONE launch (VALU-bound and HBM-bound work side by side), with two
 * workspace volume sets. Results are identical to n_frames sgm_match_device calls.     */
int  sgm_match_device_batch(sgm_handle* h, const uint8_t* const* d_lefts, const uint8_t* const* d_rights,
                            int n_frames, int width, int height, size_t stride,
                            int16_t* const* d_disps, size_t out_stride, void* stream);

/* Synchronise the handle's stream (after sgm_match_device with stream == NULL).          */
int  sgm_synchronize(sgm_handle* h);

const char* sgm_last_error(const sgm_handle* h);

/* ---- profiling: per-stage device time (hipEvents on the handle's stream) ---------------- */
#define SGM_MAX_STAGES 16
/* enable != 0: (re)start recording a hipEvent around every kernel launch ("stage") of
 * every match; records since the last enable are kept (no host sync per match).          */
int  sgm_set_profiling(sgm_handle* h, int enable);
/* Synchronises on the last record and fills up to `max` per-stage AVERAGE times (ms per
 * launch) — stages are identified by name, in first-launch order; returns their number. */
int  sgm_get_stage_times(sgm_handle* h, float* ms, int max);
/* Number of frames matched while profiling.                                               */
int  sgm_profiled_matches(const sgm_handle* h);
const char* sgm_stage_name(const sgm_handle* h, int i);
/* Algorithmic HBM bytes per launch of stage i.                         */
double sgm_stage_bytes(const sgm_handle* h, int i);
/* Number of launches of stage i recorded since profiling was enabled.                    */
int  sgm_stage_launches(const sgm_handle* h, int i);

/* ---- after the matcher: DisparityImage packing and disparity -> depth / point cloud ----- */
/* The node's processDisparity tail (generate_disparity.cpp:426-452) on device buffers:
 * out = disp * (1/16) as float, then MISSING_Z (10000) where out < min_disparity and where
 * out > max_disparity (min/max = T*f/depth_max and T*f/depth_min, as float, :447-450).
 * Asynchronous on `stream` (NULL = the handle's stream).                                   */
int  sgm_disparity_to_msg(sgm_handle* h, const int16_t* d_disp, size_t disp_stride, int width, int height,
                          float min_disparity, float max_disparity, float* d_out, size_t out_stride,
                          void* stream);

/* Q of disparity_to_depth.cpp calc_q (:62-84) from the left camera matrix K (3x3) and the
 * rectified projections P_right, P_left (3x4), all row-major doubles. Host-only.          */
void sgm_calc_q(const double K_left[9], const double P_right[12], const double P_left[12], double Q[16]);

/* One point of the cloud: pcl::PointXYZRGB's x, y, z and its packed rgba (b | g<<8 | r<<16 |
 * 255<<24).                                                                                 */
typedef struct sgm_point_xyzrgb { float x, y, z; uint32_t rgba; } sgm_point_xyzrgb;

/* disparity_to_depth.cpp:127-205 on device buffers, asynchronous on `stream`:
 *   d_disp     DisparityImage float image (pixels; 0 and MISSING_Z are skipped)
 *   d_color    MONO8 (channels 1) / BGR8 (channels 3) image, or NULL with channels 0 (black)
 *   q          {Q(2,3), Q(0,3), Q(1,3), Q(3,2), Q(3,3)} (cast to float, as the node does)
 *   depth_min/max  the node's depth window (z kept when depth_min <= z <= depth_max)
 *   d_depth    (may be NULL) W x H float depth, 0 where no point
 *   d_points   (may be NULL) the first max_points points in raster order (pcl push_back order)
 *   d_num_points (device int, may be NULL) receives the total number of points.
 * The per-row counts live in one buffer of the handle whatever `stream` is: calls on one handle
 * must be ordered by the caller (the same stream, or an event between them).                */
int  sgm_depth_points(sgm_handle* h, const float* d_disp, size_t disp_stride, int width, int height,
                      const uint8_t* d_color, size_t color_stride, int channels, const double q[5],
                      double depth_min, double depth_max, float* d_depth, size_t depth_stride,
                      sgm_point_xyzrgb* d_points, int max_points, int* d_num_points, void* stream);

/* ---- rectification: the node's rectify(), generate_disparity.cpp:370-386
 * and rectify.cpp:111-127 — cv::initUndistortRectifyMap(K, D, R, P, size, CV_32FC1) then
 * cv::remap(INTER_CUBIC, BORDER_CONSTANT 0) — with the map computed once per calibration. */

/* Float rectification maps (map_x, map_y: W x H, row stride map_stride floats) on the device
 * from the CameraInfo matrices (row-major doubles): K 3x3, D (n_dist = 0, 4, 5, 8 or 12:
 * k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]]; the node passes 5), R 3x3 (NULL = identity),
 * P 3x4 (its left 3x3 is the new camera matrix). Asynchronous on `stream`.
 * SGM_ERR_UNSUPPORTED for other n_dist (the tilted-sensor model); SGM_ERR_ARG if P*R is
 * singular.                                                                                */
int  sgm_rectify_map(sgm_handle* h, const double K[9], const double* D, int n_dist, const double R[9],
                     const double P[12], int width, int height, float* d_map_x, float* d_map_y,
                     size_t map_stride, void* stream);
/* One remapped u8 image: dst(x, y) = bicubic(src at (map_x, map_y)), OpenCV's fixed-point
 * INTER_CUBIC (1/32 px positions, 15-bit weights), source pixels outside src_w x src_h read
 * 0. dst is width x height like the maps. Asynchronous on `stream`.                        */
int  sgm_remap_cubic(sgm_handle* h, const uint8_t* d_src, size_t src_stride, int src_w, int src_h,
                     const float* d_map_x, const float* d_map_y, size_t map_stride, int width, int height,
                     uint8_t* d_dst, size_t dst_stride, void* stream);
/* The same for an interleaved 8UC3 image (src_stride, dst_stride in bytes; src and dst are
 * 8UC3): one map look-up and one weight row per pixel shared by the three channels, each
 * channel equal to sgm_remap_cubic of its plane (OpenCV's remapBicubic treats channels
 * independently); taps outside the source read 0 in every channel.                          */
int  sgm_remap_cubic_c3(sgm_handle* h, const uint8_t* d_src, size_t src_stride, int src_w, int src_h,
                        const float* d_map_x, const float* d_map_y, size_t map_stride, int width, int height,
                        uint8_t* d_dst, size_t dst_stride, void* stream);
/* cv::cvtColor(COLOR_BGR2GRAY) on device buffers: src 8UC3 (src_stride in bytes), dst 8UC1
 * (dst_stride in bytes), gray_set = SGM_GRAY_Y14 / SGM_GRAY_Y15 (another value: SGM_ERR_PARAM).
 * Asynchronous on `stream`.                                                                 */
int  sgm_bgr2gray(sgm_handle* h, const uint8_t* d_src, size_t src_stride, int width, int height,
                  uint8_t* d_dst, size_t dst_stride, int gray_set, void* stream);
/* Rectification ahead of the matcher, as the node's imageCb does it (generate_disparity.cpp:
 * 651-652): after this call the device matches (sgm_match_device, sgm_match_device_batch,
 * sgm_match_device_batch_rect) take RAW images of src_width x src_height (their stride
 * argument = the raw stride) and rectify them through the maps (W x H = the match geometry,
 * e.g. from sgm_rectify_map; left x/y, right x/y), in every mode:
 *  - SGM_MODE_CENSUS8 remaps inside its census tiles (no rectified image exists in memory
 *    unless one is requested);
 *  - SGM_MODE_OCV_SGBM5, SGM_MODE_OCV_HH8 and SGM_MODE_OCV_BM run one pre-pass launch per
 *    frame pair (profiling stage `rectify`) that remaps both images into per-handle grey
 *    planes, then their unchanged pipelines on those. sgm_stage_bytes of that stage: 16 B/px
 *    of maps and 2 * channels B/px of source read, 2 B/px of grey and channels B/px per
 *    requested rectified image written.
 * The maps must stay valid while set. All four maps NULL switches it off. A frame without a
 * disparity window (width <= the disparity span) is SGM_ERR_UNSUPPORTED while it is on, as are
 * sgm_match / sgm_match_f32 (host buffers) and sgm_match_tiled_device.                       */
int  sgm_set_rectification(sgm_handle* h, const float* d_map_xl, const float* d_map_yl, const float* d_map_xr,
                           const float* d_map_yr, size_t map_stride, int src_width, int src_height);
/* sgm_match_device_batch that also returns the rectified images (d_rect_lefts /
 * d_rect_rights: arrays of n device pointers, W x H u8 with row stride rect_stride; either
 * array may be NULL, and an image that is not requested is not written). Rectified outputs
 * need sgm_set_rectification; with it, every mode fills them: the raw frames of an OCV or BM
 * batch are rectified frame by frame on the lane that matches them. With 3 channels
 * (sgm_set_raw_format) they are 8UC3 and rect_stride is in bytes (>= 3 * width).             */
int  sgm_match_device_batch_rect(sgm_handle* h, const uint8_t* const* d_raw_lefts, const uint8_t* const* d_raw_rights,
                                 int n_frames, int width, int height, size_t raw_stride,
                                 uint8_t* const* d_rect_lefts, uint8_t* const* d_rect_rights, size_t rect_stride,
                                 int16_t* const* d_disps, size_t out_stride, void* stream);
/* The 32 x 32 x 16 int16 INTER_CUBIC weight table (entry fy*32 + fx, tap row*4 + col) the
 * remap uses. Host-only.                                                                   */
void sgm_cubic_table(int16_t tab[16384]);

/* ---- the node's frame in one host call ---------------------------------------------------- */
/* One camera's CameraInfo, row-major doubles: K 3x3, D with n_dist = 0, 4, 5, 8 or 12 elements
 * (as sgm_rectify_map), R 3x3 (has_R == 0: identity, R is not read), P 3x4.                  */
typedef struct sgm_camera_info {
    double K[9]; double D[12]; int n_dist;
    int has_R; double R[9];
    double P[12];
} sgm_camera_info;

/* The buffers of one frame; every image pointer is a HOST pointer. */
typedef struct sgm_node_frame_io {
    size_t struct_size;                       /* sizeof(sgm_node_frame_io), checked              */
    const uint8_t* raw_left; const uint8_t* raw_right; size_t raw_stride;   /* bytes             */
    int width, height;                        /* the node rectifies at the input size            */
    float min_disparity, max_disparity;       /* as sgm_disparity_to_msg                         */
    uint8_t* rect_left; uint8_t* rect_right; size_t rect_stride;  /* bytes; either may be NULL   */
    float* disparity; size_t disparity_stride;                    /* floats; required            */
    float* depth; size_t depth_stride; const double* q5;          /* optional; q5 as sgm_depth_points */
    double depth_min, depth_max;
} sgm_node_frame_io;

/* The whole compute of the node's imageCb (generate_disparity.cpp:635-713) on host buffers,
 * synchronous: both raw images (8UC1, or 8UC3 after sgm_set_raw_format) are uploaded, rectified
 * through maps built from the two CameraInfos (rectify(), :370-386), matched in the handle's
 * mode (sgm_set_params, sgm_set_bm_params, sgm_set_census_paths), and the outputs come back:
 *   rect_left / rect_right  the rectified images the node publishes: sgm_remap_cubic /
 *                           sgm_remap_cubic_c3 through sgm_rectify_map of that camera
 *   disparity               the DisparityImage float image: sgm_disparity_to_msg of what
 *                           sgm_match_device_batch_rect gives for the raw pair
 *   depth                   the depth image of sgm_depth_points on `disparity` (d_points NULL)
 * each bit for bit what those calls give. The four float maps are cached on the handle and
 * rebuilt only when the size or any byte of K, D[0..n_dist), n_dist, has_R, R or P of either
 * camera changes (sgm_node_frame_map_builds counts the builds); sgm_destroy frees them. The
 * rectified images are copied back on a second stream beside the match. An output inside an
 * sgm_host_register range goes through its mapping; in the census mode without median and
 * speckle filter the final WTA launch then writes the `disparity` rows itself (no pass after the
 * matcher; with `depth` it also fills a device int16 image, which one depth pass reads).
 * Otherwise one launch after the matcher (profiling stage `msg`; sgm_stage_bytes: 2 B/px read,
 * 4 B/px per float image written) reads the int16 disparity once and writes both float images.
 * The caller's sgm_set_rectification state is left exactly as found, also on failure, and the
 * call is ordered with the handle's other calls like every match.
 * Errors: SGM_ERR_ARG for a null handle, io or required pointer, a struct_size other than
 * sizeof(sgm_node_frame_io), a stride smaller than a row, depth without q5; sgm_rectify_map's
 * SGM_ERR_UNSUPPORTED (n_dist) and SGM_ERR_ARG (singular P * R); then the matcher's parameter
 * errors as at any match (a frame without a disparity window: SGM_ERR_UNSUPPORTED). All of them
 * are decided before any output byte is written. Added under ABI version 5 (no existing struct
 * or signature changed): callers check for the symbol.                                        */
int  sgm_node_frame(sgm_handle* h, const sgm_camera_info* left, const sgm_camera_info* right,
                    const sgm_node_frame_io* io);
/* How often sgm_node_frame (re)built the handle's cached maps (0 for a null handle).          */
int  sgm_node_frame_map_builds(const sgm_handle* h);

/* ---- stage entry points (parity tests compare each stage with the CPU oracle) ----------- */
/* Census codes of one image under the handle's window, 9x7 by default (host buffers; out:
 * W x H uint64, row-major). An invalid window is SGM_ERR_PARAM in the census mode; in the
 * OCV and BM modes, which ignore the window, it gives the 9x7 codes.                       */
int  sgm_debug_census(sgm_handle* h, const uint8_t* img, int width, int height,
                      size_t stride, uint64_t* out);
/* Census mode: u8 path-cost volume of direction `dir` (0..7; see DESIGN.md for the order),
 * layout [H][width1][D]. Runs census + that direction only (a direction, not a path set:
 * sgm_set_census_paths does not change it), with the handle's census window.               */
int  sgm_debug_census_path(sgm_handle* h, const uint8_t* left, const uint8_t* right,
                           int width, int height, size_t stride, int dir, uint8_t* vol);
/* OCV modes: int16 aggregated matching cost C' = SAD + P2 used by the path recurrence,
 * layout [H][width1][D].                                                                  */
int  sgm_debug_ocv_cost(sgm_handle* h, const uint8_t* left, const uint8_t* right,
                        int width, int height, size_t stride, int16_t* cost);
/* BM mode: the XSOBEL pre-filtered image (host u8 in, W x H u8 out, row-major).             */
int  sgm_debug_bm_prefilter(sgm_handle* h, const uint8_t* img, int width, int height, size_t stride,
                            uint8_t* out);
/* BM mode, small frames: the int32 SAD volume of the fused kernel, layout [H][X1 - X0][D]
 * with X0 = max(D - 1 + minD, 0), X1 = min(W, W + minD), and the int32 texture plane
 * [H][X1 - X0]. The last index is e = D - 1 - (d - minD): e = 0 is the LARGEST disparity
 * minD + D - 1, the order OpenCV's inner loop scans. Rows outside [w/2, H - w/2) are 0.
 * Either output may be NULL. SGM_ERR_UNSUPPORTED above 2^27 volume cells.                  */
int  sgm_debug_bm_sad(sgm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                      size_t stride, int32_t* sad, int32_t* texture);
/* BM mode: the tiling of the fused SAD + WTA kernel that a match of a width x height frame
 * takes on a device of n_cu compute units (host-only, no handle, no device). The environment
 * override of a match applies: SGM_BM_VGLOBAL=1 (column sums in the workspace). out[] in this
 * order:
 *    0 TX       output columns of a workgroup's strip     6 vglobal  1: column sums in HBM
 *    1 nsx      strips (grid x)                           7 wide     1: u32 column sums, 0: u16
 *    2 nsy      bands (grid y)                            8 nk       64-disparity chunks per lane
 *    3 RB       output rows of a band                     9 Dp       padded disparities, 64 * nk
 *    4 waves    waves of a workgroup (8 or 16)           10 width1   computed columns X1 - X0
 *    5 lds      dynamic LDS bytes of a workgroup         11 rows     computed rows H - 2 * (w / 2)
 * Returns 0, or the parameter error a match would return (SGM_ERR_ARG for a null pointer or a
 * mode other than SGM_MODE_OCV_BM). A frame without a computed column (width1 0) is planned as
 * one of a single column, as make_layout does. Added under ABI version 5 (no existing struct
 * or signature changed): callers check for the symbol.                                      */
int  sgm_debug_bm_plan(const sgm_params* p, const sgm_bm_params* bm, int width, int height, int n_cu,
                       int out[12]);
/* Census mode: the path work list one launch would dispatch (host-only, no device): every
 * 16-line block of the directions in dir_mask (bit d) of `group` frames, plus the up+WTA
 * blocks (code 8) of `up_group` frames, as dir << 24 | frame << 22 | block, longest first,
 * dealt in a snake over rounds of n_slots. Returns the entry count (out may be NULL), or
 * < 0 on an error (cap too small: SGM_ERR_ARG).                                           */
int  sgm_debug_path_items(const sgm_params* p, int width, int height, unsigned dir_mask, int n_slots,
                          int group, int up_group, uint32_t* out, int cap);
/* 3x3 median (replicate border) and speckle filter on a host int16 image, in place.       */
int  sgm_debug_median3(sgm_handle* h, int16_t* disp, int width, int height);
int  sgm_debug_speckle(sgm_handle* h, int16_t* disp, int width, int height,
                       int new_val, int max_size, int max_diff);
/* The post filters launched as a match launches them, on host buffers (synchronous): `disp` is the
 * raw W x H image; `out` has row stride width + out_pad, is uploaded first (so the pad columns keep
 * whatever the caller put there) and returned whole. median != 0 with max_size <= 0 runs the 3x3
 * median alone; max_size > 0 runs the speckle filter, with the median fused into its tile kernel
 * when median != 0; neither copies the image. Added under ABI version 5: callers check for the
 * symbol.                                                                                     */
int  sgm_debug_post(sgm_handle* h, const int16_t* disp, int width, int height, int out_pad, int median,
                    int new_val, int max_size, int max_diff, int16_t* out);
/* sgm_fill_holes on a host int16 image, in place; synchronous.                             */
int  sgm_debug_fill(sgm_handle* h, int16_t* disp, int width, int height, int invalid,
                    const sgm_fill_params* params, int x0, int y0, int x1, int y1);
/* The two pyramid kernels on host buffers (synchronous; the handle's pyramid parameters are not
 * used). sgm_debug_pyr_down: both 8UC1 images halved into ((W + 1) / 2) x ((H + 1) / 2) row-major
 * images. sgm_debug_pyr_refine: step 4 of the level-1 specification on the full-resolution pair and
 * a coarse int16 image of that size: m, D the full-resolution range, mc the coarse minimum (its
 * invalid value is (mc - 1) * 16), radius 1..2 (else SGM_ERR_PARAM); out: W x H int16.           */
int  sgm_debug_pyr_down(sgm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                        size_t stride, uint8_t* out_left, uint8_t* out_right);
int  sgm_debug_pyr_refine(sgm_handle* h, const uint8_t* left, const uint8_t* right, int width, int height,
                          size_t stride, const int16_t* coarse, int m, int D, int mc, int radius, int subpixel,
                          int16_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SGM_HIP_H */
