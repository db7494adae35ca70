// sgm_host.h — what the host sources of libsgm_hip.so share (internal, never installed).
//
// The sources and what each may use from the others (everything below is declared here):
//   sgm_plan.cpp      decides without touching the device: geometry, workspace layouts, knobs
//   sgm_pipeline.cpp  the handle's resources, the frame pipelines and batch schedulers (uses plan)
//   sgm_api.cpp       create / destroy / set / get, the match and standalone kernel entry points
//   sgm_pyramid.cpp   pyramid level 1 around the level-0 entry points of sgm_api.cpp (uses pipeline)
//   sgm_node.cpp      sgm_node_frame: the node's imageCb on host buffers (uses pipeline, pyramid)
//   sgm_batch_io.cpp  per-device sub-handles and the host streaming ring of sgm_match_batch
//   sgm_tiled.cpp     the two multi-device tile modes (uses open_subs / run_on_subs of batch_io)
//   sgm_debug.cpp     profiling and the sgm_debug_* stage entry points
#pragma once

#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "sgm_device.h"
#include "sgm_hip.h"
#include "sgm_launch.h"

namespace sgm {

constexpr size_t kAlign = 256;
constexpr size_t kTrashBytes = 4096;   // >= 64 lanes x 32 disparities (census_sgm.hip trash stores)
inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

constexpr sgm_bm_params kBmDefaults = {10, 9};   // texture_threshold, prefilter_size
constexpr sgm_fill_params kFillDefaults = {SGM_FILL_OFF, 16, 2};   // mode, max_gap, min_neighbours
constexpr sgm_census_window kCensusWindowDefault = {9, 7, 1};     // taps_x, taps_y, step
constexpr sgm_pyramid_params kPyramidDefaults = {0, 2};           // level, radius
constexpr int kPyrGroup = 8;           // frames of a level-1 batch whose planes exist at once

// What a handle matches with: the setters write it, every sub-handle family receives it whole.
struct MatchConfig {
    sgm_params params{};
    sgm_bm_params bm = kBmDefaults;   // SGM_MODE_OCV_BM only
    int census_paths = 8;             // SGM_MODE_CENSUS8 only: 8, or 4 (sgm_set_census_paths)
    int raw_ch = 1;                   // sgm_set_raw_format: channels of the frames (1, or 3 = 8UC3)
    int gray_set = SGM_GRAY_Y14;      // ... and the COLOR_BGR2GRAY coefficient set used with 3
    sgm_fill_params fill = kFillDefaults;   // sgm_set_fill_params: the hole-filling post filter
    sgm_census_window cwin = kCensusWindowDefault;   // SGM_MODE_CENSUS8 only (sgm_set_census_window)
    sgm_pyramid_params pyr = kPyramidDefaults;       // sgm_set_pyramid_params: level 1 = coarse match + refinement
};
inline bool pyramid_on(const MatchConfig& c) { return c.pyr.level != 0; }
inline bool fill_on(const MatchConfig& c) { return c.fill.mode != SGM_FILL_OFF; }
// the census runs as its own launch on 8UC1 planes (census_win.hip): the census mode with a
// window other than the default
inline bool census_win_on(const MatchConfig& c)
{
    return c.params.mode == SGM_MODE_CENSUS8 && !census_window_default(c.cwin);
}
// ... and its frames are colour and / or raw, so a pre-pass fills the grey planes first
inline bool census_win_prepass(const MatchConfig& c, bool rect_on) { return census_win_on(c) && (rect_on || c.raw_ch == 3); }

struct Workspace {
    void* base = nullptr;
    size_t size = 0;
};

}  // namespace sgm

struct sgm_handle {
    int device = 0;
    sgm::MatchConfig cfg;
    hipStream_t stream = nullptr;
    std::string err;
    std::mutex mu;
    sgm::Workspace ws;
    uint8_t* pin = nullptr;      // pinned host staging
    size_t pin_size = 0;
    // profiling: one hipEvent before every launch and one after the last launch of a
    // match; launch k runs from event `start` to the next recorded event
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;   // grows on demand, reused after a re-enable
    size_t ev_used = 0;
    struct LaunchRec { int stage; size_t ev0, ev1; };
    std::vector<LaunchRec> launches;
    int prof_frames = 0;
    int nstages = 0;                   // distinct stage names seen (first-launch order)
    const char* stage_name[SGM_MAX_STAGES] = {};
    double stage_bytes[SGM_MAX_STAGES] = {};
    std::vector<sgm_handle*> sub;  // per-device handles for sgm_match_batch
    int n_cu = 0;                  // compute units of the device (path work-list dealing)
    int* aux = nullptr;            // per-row counts / offsets of sgm_depth_points
    size_t aux_n = 0;
    uint32_t* items_pin = nullptr; // pinned host copy of the uploaded path work list
    int items_cap = 0;
    std::string items_key[2];      // geometry + workspace each device copy (single / group) belongs to
    std::string layout_sig;        // the workspace carve-up of the last prepared call (prepare)
    int16_t* cubic_tab = nullptr;  // device INTER_CUBIC weight table (sgm_remap_cubic), built once
    bool rect_on = false;          // sgm_set_rectification: device-match inputs are raw (rectified in the census
                                   // tiles, or by the k_rectify_pair pre-pass of the OCV / BM modes)
    sgm::RectifyIn rect{};
    // exact tile mode (sgm_match_tiled_exact): one handle per row band, each with a second
    // stream for its upward sweeps and four events (census, down, up, gather)
    std::vector<sgm_handle*> bands;
    // OCV-mode frame batches: frames dealt over a few same-device handles, each with its own
    // stream and workspace, so the small launches of one frame overlap another's
    std::vector<sgm_handle*> par;
    hipEvent_t par_ev = nullptr;   // recorded on the handle's stream, then each lane's done
    hipStream_t stream2 = nullptr;
    hipEvent_t bev[4] = {};
    // cross-call ordering: every call that uses the workspace records `done` on the stream it
    // ran on, and the next call (whatever its stream) waits on it first
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    // host-buffer frame streaming (sgm_match_batch): device + pinned rings, copy streams
    void* io_dev = nullptr;
    size_t io_dev_size = 0;
    uint8_t* io_pin = nullptr;
    size_t io_pin_size = 0;
    hipStream_t up = nullptr, down = nullptr;
    std::vector<hipEvent_t> io_ev;
    // host buffers page-locked and mapped by sgm_host_register (host range -> device address)
    struct HostReg { char* host; size_t bytes; char* dev; };
    std::vector<HostReg> regs;
    // host-buffer matches: the right image's copy runs on `cpy` beside the left image's census
    hipStream_t cpy = nullptr;
    hipEvent_t cpy_ev = nullptr;
    // sgm_node_frame: the cached rectification maps (four W x H float planes: left x / y, right
    // x / y) with the bytes of the size and calibrations they were built from, the device images of
    // a frame (raw, rectified, int16, DisparityImage, depth) and the event that follows the launch
    // writing the rectified images
    float* node_maps = nullptr;
    size_t node_maps_px = 0;
    std::vector<unsigned char> node_key;
    int node_builds = 0;
    char* node_buf = nullptr;
    size_t node_buf_size = 0;
    hipEvent_t node_ev = nullptr;
    // pyramid level 1: the planes of a group of frames (grey, coarse images, code planes, coarse
    // disparity, the image in front of the hole filter) and the host entry points' staging
    char* pyr_buf = nullptr;
    size_t pyr_buf_size = 0;
};

namespace sgm {

inline int fail(sgm_handle* h, int code, const std::string& msg)
{
    if (h) h->err = msg;
    return code;
}

inline int hip_fail(sgm_handle* h, hipError_t e, const char* where)
{
    return fail(h, SGM_ERR_DEVICE, std::string(where) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr, where)                                   \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return hip_fail(h, e_, where);   \
    } while (0)

// Workspace carve-up for one geometry. Offsets are 256-B aligned.
struct Layout {
    // census: set 0 serves single matches; a pipelined batch uses code sets 0 .. 3*group-1
    // (the census of group k+1 runs beside the up+WTA sweeps of group k-1), volume sets
    // 0 .. 2*group-1 and one up+WTA result image per frame of a group
    size_t cL[3 * sgm::kMaxGroup] = {}, cR[3 * sgm::kMaxGroup] = {}, vols[2 * sgm::kMaxGroup] = {};
    size_t res[sgm::kMaxGroup] = {};
    size_t vol_bytes = 0;
    int np = 8;                                            // census path set: slices per volume set
    int group = 1;                                         // frames per pipelined launch
    bool up_wta = false;                                   // pipelined batch: up+WTA scheme
    size_t items[2] = {}; int n_items[2] = {};             // path work lists: one frame / a group
    size_t planes = 0, bufA = 0, bufB = 0, ovols = 0, ovf = 0;  // ocv
    size_t ores = 0;                                       // ocv: per-pixel results of k_ocv_vwta
    size_t bmL = 0, bmR = 0, bmV = 0;                      // bm: pre-filtered images, HBM column sums
    size_t grayL = 0, grayR = 0;                           // ocv / bm with colour or raw frames: the grey planes
                                                           // (census with a non-default window: a pair per group frame)
    sgm::BmPlan bm{};                                      // bm: tiling of the fused kernel
    size_t tmp = 0, lab = 0, cnt = 0;                      // post
    size_t inL = 0, inR = 0, out = 0, outf = 0;            // host-API staging (int16 / float out)
    // hole filling on (behind everything else, so the layout without it is unchanged): the frame
    // before the fill (one image per frame of a group, row stride W) and the kernel's three planes
    bool fill = false;
    size_t fsrc = 0, fpl = 0;
    size_t total = 0;
};

// Where the post filters of a frame leave their result (and the producer writes without a
// median): the caller's image, or with hole filling this frame's image in front of the fill.
inline int16_t* post_image(const Layout& l, const Geom& g, char* ws, size_t frame, int16_t* dOut)
{
    return l.fill ? (int16_t*)(ws + l.fsrc) + frame * (size_t)g.W * g.H : dOut;
}
inline size_t post_stride(const Layout& l, const Geom& g, size_t out_stride) { return l.fill ? (size_t)g.W : out_stride; }

// sgm_pipeline.cpp: the profiling events and stage table of a handle
long record_event(sgm_handle* h);
int stage_index(sgm_handle* h, const char* name, double bytes);

// Stage bookkeeping of one match call: begin() before every launch, end() after the last.
struct StageRec {
    sgm_handle* h;
    long open = -1;      // index into h->launches of the launch waiting for its end event
    void close(long ev)
    {
        if (open >= 0 && ev >= 0) h->launches[open].ev1 = (size_t)ev;
        open = -1;
    }
    void begin(const char* name, double bytes)
    {
        const int st = stage_index(h, name, bytes);
        if (!h->profiling) return;
        const long ev = record_event(h);
        close(ev);
        if (st < 0 || ev < 0) return;
        h->launches.push_back({st, (size_t)ev, (size_t)ev});
        open = (long)h->launches.size() - 1;
    }
    void end()
    {
        if (h->profiling && open >= 0) close(record_event(h));
    }
};

// Callbacks of a frame batch whose inputs arrive and outputs leave while it runs (the
// host-buffer streaming of sgm_match_batch). Frames [f0, f0 + n):
//   inputs       before the first launch that reads their input images;
//   outputs_free before the first launch that writes their disparities;
//   outputs_done after the last launch that writes them.
// Each returns a status (non-zero aborts the batch).
struct FrameHooks {
    virtual int inputs(int f0, int n) = 0;
    virtual int outputs_free(int f0, int n) = 0;
    virtual int outputs_done(int f0, int n) = 0;
    virtual ~FrameHooks() = default;
};

// OCV / BM modes on raw frames (sgm_set_rectification): where one frame's rectified images go
// (null: not wanted; stride in bytes). Passing one to run_pipeline makes its inputs raw frames.
struct RectOut {
    uint8_t* L = nullptr;
    uint8_t* R = nullptr;
    size_t stride = 0;
};

// sgm_node_frame's hooks into the census frame pipeline (one frame). rows: the final standalone
// WTA launch writes the DisparityImage rows itself (a mapped host buffer, stride in floats, window
// and optional int16 copy in win) and the int16 output is not written; rect_ev: recorded on the
// stream after the launch that writes the rectified images.
struct NodeOut {
    float* rows = nullptr;
    size_t stride = 0;
    MsgWin win{};
    hipEvent_t rect_ev = nullptr;
};

// sgm_plan.cpp
int make_geom(const sgm_params& p, int W, int H, Geom& g, std::string& err, const sgm_bm_params* bm = nullptr);
bool use_median(const sgm_params& p);
bool use_speckle(const sgm_params& p);
int speckle_scale(int mode);
Layout make_layout(const MatchConfig& c, const Geom& g, bool host_io, int group = 0, int n_cu = 0, bool rect = false);
Layout make_post_layout(const sgm_params& p, const Geom& g, bool fill = false);
int fill_params_status(const sgm_fill_params& f, std::string& err);
int census_window_status(const sgm_census_window& w, std::string& err);
int batch_group(int n);
bool ocv_vwta_on(const Geom& g, int fullDP);
int ocv_batch_lanes(int n);

// sgm_pipeline.cpp
int ensure_stream(sgm_handle* h);
int order_after_last(sgm_handle* h, hipStream_t st);
int mark_done(sgm_handle* h, hipStream_t st);
int ensure_ws(sgm_handle* h, size_t bytes);
int ensure_pin(sgm_handle* h, size_t bytes);
int ensure_cubic_table(sgm_handle* h);
int path_items(sgm_handle* h, const Layout& l, const Geom& g, unsigned dir_mask, int group, hipStream_t st,
               const uint32_t** dev, int up_group = 0);
int run_post(sgm_handle* h, const Layout& l, const Geom& g, int16_t* dOut, size_t out_stride, StageRec& rec,
             size_t tmp_off = 0);
int run_pipeline(sgm_handle* h, const Layout& l, const Geom& g, const uint8_t* dL, const uint8_t* dR, size_t stride,
                 int16_t* dOut, size_t out_stride, const std::function<hipEvent_t()>& copy_r = nullptr,
                 float* outf = nullptr, size_t outf_stride = 0, const RectOut* raw = nullptr,
                 hipEvent_t rect_ev = nullptr);
int run_batch_census(sgm_handle* h, const Layout& l, const Geom& g, const uint8_t* const* dLs,
                     const uint8_t* const* dRs, int n, size_t stride, int16_t* const* outs, size_t out_stride,
                     uint8_t* const* rectLs = nullptr, uint8_t* const* rectRs = nullptr, size_t rect_stride = 0,
                     FrameHooks* hooks = nullptr, const NodeOut* node = nullptr);
int run_batch_ocv(sgm_handle* h, const Layout& l0, const Geom& g0, int W, int H, const uint8_t* const* dLs,
                  const uint8_t* const* dRs, int n, size_t stride, int16_t* const* outs, size_t out_stride,
                  uint8_t* const* rectLs = nullptr, uint8_t* const* rectRs = nullptr, size_t rect_stride = 0);
int raw_format_status(sgm_handle* h, const MatchConfig& c);
int refuse_fill(sgm_handle* h, const char* what);
int refuse_colour(sgm_handle* h, const char* what);
size_t raw_bpp(const sgm_handle* h);
int prepare(sgm_handle* h, const MatchConfig& c, int W, int H, bool host_io, Geom& g, Layout& l, int group = 0,
            bool rect = false);
int match_host(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, void* out,
               size_t out_stride, bool f32);

int config_status(sgm_handle* h, const MatchConfig& c);

// sgm_api.cpp: sgm_match_device_batch_rect with h->mu already held and the buffers checked
int device_batch_locked(sgm_handle* h, const uint8_t* const* dLs, const uint8_t* const* dRs, int n, int W, int H,
                        size_t stride, uint8_t* const* rectLs, uint8_t* const* rectRs, size_t rect_stride,
                        int16_t* const* outs, size_t out_stride, void* stream);

// sgm_pyramid.cpp: level 1 (h->mu held by the caller, buffers checked)
struct PyrPlan { int Wc, Hc, mc, Dc, invalid_c, invalid; };
int pyramid_status(const sgm_pyramid_params& p, std::string& err);
int pyramid_plan(const MatchConfig& c, int W, int H, PyrPlan& pl, MatchConfig& coarse, std::string& err);
int refuse_pyramid(sgm_handle* h, const char* what);
int pyr_device_batch(sgm_handle* h, const uint8_t* const* dLs, const uint8_t* const* dRs, int n, int W, int H,
                     size_t stride, uint8_t* const* rectLs, uint8_t* const* rectRs, size_t rect_stride,
                     int16_t* const* outs, size_t out_stride, void* stream, bool host_io = false,
                     hipEvent_t rect_ev = nullptr);
int pyr_match_host(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, void* out,
                   size_t out_stride, bool f32);

// sgm_api.cpp: sgm_fill_holes with h->mu already held
int fill_holes_locked(sgm_handle* h, const int16_t* d_src, size_t src_stride, int W, int H, int invalid,
                      const sgm_fill_params* params, int x0, int y0, int x1, int y1, int16_t* d_dst,
                      size_t dst_stride, void* stream);

// sgm_batch_io.cpp
int open_subs(sgm_handle* h, const int* devices, int n_dev, std::vector<int>& devs);

// Runs job(t, sub-handle) on one host thread per device; first error wins.
template <typename F>
int run_on_subs(sgm_handle* h, const std::vector<int>& devs, F job)
{
    std::vector<int> rcs(devs.size(), SGM_OK);
    std::vector<std::thread> th;
    for (size_t t = 0; t < devs.size(); t++) th.emplace_back([&, t]() { rcs[t] = job((int)t, h->sub[t]); });
    for (auto& t : th) t.join();
    for (size_t t = 0; t < devs.size(); t++)
        if (rcs[t]) return fail(h, rcs[t], std::string("device ") + std::to_string(devs[t]) + ": " + h->sub[t]->err);
    return SGM_OK;
}

}  // namespace sgm
