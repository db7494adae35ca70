// sgm_node.cpp — sgm_node_frame: the node's imageCb compute (generate_disparity.cpp:635-713) on
// host buffers in one call. match_host (sgm_pipeline.cpp) is the template: 2-D copies between the
// caller's rows and device images, the right image on the copy stream, outputs inside an
// sgm_host_register range through their mapping. The stages are the existing ones (the census
// frame pipeline with rectification in its tiles, or run_pipeline with the k_rectify_pair
// pre-pass); what this file adds is the map cache, the frame's device images, the copies of the
// rectified images beside the match and the frame tail (depth.hip k_msg_tail, or the WTA launch
// writing the DisparityImage rows itself).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "sgm_host.h"

using namespace sgm;

namespace {

// The bytes a camera's maps depend on: D only up to n_dist, no struct padding.
void append_camera(std::vector<unsigned char>& key, const sgm_camera_info& c)
{
    auto put = [&](const void* p, size_t n) { key.insert(key.end(), (const unsigned char*)p, (const unsigned char*)p + n); };
    put(c.K, sizeof c.K);
    put(&c.n_dist, sizeof c.n_dist);
    put(c.D, sizeof(double) * (size_t)std::min(std::max(c.n_dist, 0), 12));
    put(&c.has_R, sizeof c.has_R);
    put(c.R, sizeof c.R);
    put(c.P, sizeof c.P);
}

// sgm_rectify_map's checks of one camera; ir receives inverse(P[:, :3] * R)
int check_camera(sgm_handle* h, const sgm_camera_info& c, double ir[9])
{
    if (c.n_dist != 0 && c.n_dist != 4 && c.n_dist != 5 && c.n_dist != 8 && c.n_dist != 12)
        return fail(h, SGM_ERR_UNSUPPORTED, "distortion vector must have 0, 4, 5, 8 or 12 elements");
    if (!sgm::rectify_inverse(c.P, c.has_R ? c.R : nullptr, ir)) return fail(h, SGM_ERR_ARG, "singular P[:, :3] * R");
    return SGM_OK;
}

// Device address of a host range that lies inside an sgm_host_register mapping (null: none)
char* mapped(const sgm_handle* h, const void* p, size_t bytes)
{
    for (const auto& r : h->regs)
        if (r.dev && (const char*)p >= r.host && (const char*)p + bytes <= r.host + r.bytes)
            return r.dev + ((const char*)p - r.host);
    return nullptr;
}

// the caller's sgm_set_rectification state, put back however the call ends
struct RectRestore {
    sgm_handle* h;
    sgm::RectifyIn rect;
    bool on;
    explicit RectRestore(sgm_handle* hh) : h(hh), rect(hh->rect), on(hh->rect_on) {}
    ~RectRestore() { h->rect = rect; h->rect_on = on; }
};

int node_frame(sgm_handle* h, const sgm_camera_info& cl, const sgm_camera_info& cr, const sgm_node_frame_io& io)
{
    const int W = io.width, H = io.height;
    const size_t bpp = raw_bpp(h), row = (size_t)W * bpp, WH = (size_t)W * H;
    const bool want_rect = io.rect_left || io.rect_right;
    if (!io.raw_left || !io.raw_right || !io.disparity || W <= 0 || H <= 0 || io.raw_stride < row ||
        (want_rect && io.rect_stride < row) || io.disparity_stride < (size_t)W ||
        (io.depth && (io.depth_stride < (size_t)W || !io.q5)))
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    // the rectified images' validity first, then the matcher's parameters; nothing is written before
    double ir[2][9];
    int rc = check_camera(h, cl, ir[0]);
    if (rc || (rc = check_camera(h, cr, ir[1]))) return rc;
    Geom g;
    Layout l;
    const sgm_params& p = h->cfg.params;
    const bool census = p.mode == SGM_MODE_CENSUS8;
    // pyramid level 1: the level-1 batch of one raw frame does the matching (its own checks, first)
    const bool pyr = pyramid_on(h->cfg);
    if (pyr) {
        PyrPlan pl;
        MatchConfig coarse;
        if ((rc = pyramid_plan(h->cfg, W, H, pl, coarse, h->err)) || (rc = config_status(h, h->cfg))) return rc;
        if (W + std::min(p.min_disparity, 0) - std::max(p.min_disparity + p.num_disparities, 0) <= 0)
            return fail(h, SGM_ERR_UNSUPPORTED, "fused rectification needs a non-empty disparity window");
        if ((rc = ensure_stream(h))) return rc;
    } else {
        if ((rc = make_geom(h->cfg.params, W, H, g, h->err, &h->cfg.bm))) return rc;
        if (g.width1 <= 0) return fail(h, SGM_ERR_UNSUPPORTED, "fused rectification needs a non-empty disparity window");
        // the pre-pass into the grey planes: the OCV / BM modes, and the census with a non-default window
        if ((rc = prepare(h, h->cfg, W, H, false, g, l, census ? batch_group(1) : 0, !census || census_win_on(h->cfg))))
            return rc;
    }
    if ((rc = ensure_cubic_table(h))) return rc;
    hipStream_t st = h->stream;
    if (!h->cpy) HIP_TRY(hipStreamCreateWithFlags(&h->cpy, hipStreamNonBlocking), "hipStreamCreate");
    if (!h->cpy_ev) HIP_TRY(hipEventCreateWithFlags(&h->cpy_ev, hipEventDisableTiming), "hipEventCreate");
    if (!h->node_ev) HIP_TRY(hipEventCreateWithFlags(&h->node_ev, hipEventDisableTiming), "hipEventCreate");
    if ((rc = order_after_last(h, st))) return rc;

    // the frame's device images: raw L / R, rectified L / R, int16, DisparityImage, depth
    const size_t img = align_up((size_t)H * row), need = 4 * img + align_up(WH * 2) + 2 * align_up(WH * 4);
    if (h->node_buf_size < need) {
        HIP_TRY(hipStreamSynchronize(st), "sync");
        if (h->node_buf) (void)hipFree(h->node_buf);
        h->node_buf = nullptr;
        h->node_buf_size = 0;
        if (hipMalloc((void**)&h->node_buf, need) != hipSuccess) {
            h->node_buf = nullptr;
            return fail(h, SGM_ERR_ALLOC, "hipMalloc node frame images");
        }
        h->node_buf_size = need;
    }
    uint8_t* dRawL = (uint8_t*)h->node_buf;
    uint8_t* dRawR = dRawL + img;
    uint8_t* dRectL = dRawR + img;
    uint8_t* dRectR = dRectL + img;
    int16_t* d16 = (int16_t*)(dRectR + img);
    float* dMsg = (float*)((char*)d16 + align_up(WH * 2));
    float* dDepth = (float*)((char*)dMsg + align_up(WH * 4));

    // the map cache: rebuilt when the size or a byte of either calibration changed
    std::vector<unsigned char> key;
    key.insert(key.end(), (const unsigned char*)&W, (const unsigned char*)&W + sizeof W);
    key.insert(key.end(), (const unsigned char*)&H, (const unsigned char*)&H + sizeof H);
    append_camera(key, cl);
    append_camera(key, cr);
    if (!h->node_maps || key != h->node_key) {
        h->node_key.clear();
        if (h->node_maps_px < WH) {
            HIP_TRY(hipStreamSynchronize(st), "sync");     // a previous frame may still read the old maps
            if (h->node_maps) (void)hipFree(h->node_maps);
            h->node_maps = nullptr;
            h->node_maps_px = 0;
            if (hipMalloc((void**)&h->node_maps, 4 * WH * sizeof(float)) != hipSuccess) {
                h->node_maps = nullptr;
                return fail(h, SGM_ERR_ALLOC, "hipMalloc rectification maps");
            }
            h->node_maps_px = WH;
        }
        const sgm_camera_info* cams[2] = {&cl, &cr};
        for (int i = 0; i < 2; i++) {
            double d12[12] = {};
            for (int k = 0; k < cams[i]->n_dist; k++) d12[k] = cams[i]->D[k];
            HIP_TRY(sgm::launch_rectify_map(cams[i]->K, d12, ir[i], W, H, h->node_maps + (2 * i) * WH,
                                            h->node_maps + (2 * i + 1) * WH, W, st), "rectify_map");
        }
        h->node_key = key;
        h->node_builds++;
    }

    // uploads: the left image on the stream, the right one on the copy stream
    HIP_TRY(hipEventRecord(h->cpy_ev, st), "hipEventRecord");          // the images are free
    HIP_TRY(hipStreamWaitEvent(h->cpy, h->cpy_ev, 0), "hipStreamWaitEvent");
    HIP_TRY(hipMemcpy2DAsync(dRawL, row, io.raw_left, io.raw_stride, row, H, hipMemcpyHostToDevice, st), "H2D L");
    HIP_TRY(hipMemcpy2DAsync(dRawR, row, io.raw_right, io.raw_stride, row, H, hipMemcpyHostToDevice, h->cpy), "H2D R");
    HIP_TRY(hipEventRecord(h->cpy_ev, h->cpy), "hipEventRecord");
    HIP_TRY(hipStreamWaitEvent(st, h->cpy_ev, 0), "hipStreamWaitEvent");

    // outputs inside a registered range go through their mapping
    char* mDisp = mapped(h, io.disparity, io.disparity_stride * 4 * (size_t)(H - 1) + (size_t)W * 4);
    char* mDepth = io.depth ? mapped(h, io.depth, io.depth_stride * 4 * (size_t)(H - 1) + (size_t)W * 4) : nullptr;
    const bool wta_rows = !pyr && census && !use_median(p) && !use_speckle(p) && !l.fill && mDisp;
    const float qf[5] = {io.q5 ? (float)io.q5[0] : 0.f, io.q5 ? (float)io.q5[1] : 0.f, io.q5 ? (float)io.q5[2] : 0.f,
                         io.q5 ? (float)io.q5[3] : 0.f, io.q5 ? (float)io.q5[4] : 0.f};

    {
        RectRestore keep(h);
        const float* m = h->node_maps;
        h->rect = sgm::RectifyIn{{m, m + WH, m + 2 * WH, m + 3 * WH}, (size_t)W, W, H, h->cubic_tab};
        h->rect_on = true;
        uint8_t* rl = io.rect_left ? dRectL : nullptr;
        uint8_t* rr = io.rect_right ? dRectR : nullptr;
        if (pyr) {
            const uint8_t* l1[1] = {dRawL};
            const uint8_t* r1[1] = {dRawR};
            int16_t* o1[1] = {d16};
            uint8_t* rl1[1] = {rl};
            uint8_t* rr1[1] = {rr};
            rc = pyr_device_batch(h, l1, r1, 1, W, H, row, rl ? rl1 : nullptr, rr ? rr1 : nullptr, row, o1, W, nullptr,
                                  false, want_rect ? h->node_ev : nullptr);
        } else if (census) {
            NodeOut no;
            no.rect_ev = want_rect ? h->node_ev : nullptr;
            if (wta_rows) {
                no.rows = (float*)mDisp;
                no.stride = io.disparity_stride;
                no.win = MsgWin{io.min_disparity, io.max_disparity, io.depth ? d16 : nullptr};
            }
            const uint8_t* l1[1] = {dRawL};
            const uint8_t* r1[1] = {dRawR};
            int16_t* o1[1] = {d16};
            uint8_t* rl1[1] = {rl};
            uint8_t* rr1[1] = {rr};
            rc = run_batch_census(h, l, g, l1, r1, 1, row, o1, W, rl ? rl1 : nullptr, rr ? rr1 : nullptr, row, nullptr,
                                  &no);
        } else {
            const RectOut ro{rl, rr, row};
            rc = run_pipeline(h, l, g, dRawL, dRawR, row, d16, W, nullptr, nullptr, 0, &ro,
                              want_rect ? h->node_ev : nullptr);
        }
        if (rc) return rc;
    }

    // the frame tail: one pass over the int16 image writes the DisparityImage rows and the depth
    // rows (after WTA-written rows: the depth alone, from the int16 copy on the device)
    float* msg_dst = wta_rows ? nullptr : mDisp ? (float*)mDisp : dMsg;
    const size_t msg_stride = mDisp ? io.disparity_stride : (size_t)W;
    float* depth_dst = !io.depth ? nullptr : mDepth ? (float*)mDepth : dDepth;
    const size_t depth_stride = mDepth ? io.depth_stride : (size_t)W;
    if (msg_dst || depth_dst) {
        StageRec rec{h};
        rec.begin("msg", (2 + (msg_dst ? 4 : 0) + (depth_dst ? 4 : 0)) * (double)WH);
        HIP_TRY(sgm::launch_msg_tail(d16, W, W, H, io.min_disparity, io.max_disparity, msg_dst, msg_stride, qf,
                                     io.depth_min, io.depth_max, depth_dst, depth_stride, st), "msg");
        rec.end();
    }
    // the rectified images leave on the copy stream once the launch that wrote them is done
    if (want_rect) {
        HIP_TRY(hipStreamWaitEvent(h->cpy, h->node_ev, 0), "hipStreamWaitEvent");
        if (io.rect_left)
            HIP_TRY(hipMemcpy2DAsync(io.rect_left, io.rect_stride, dRectL, row, row, H, hipMemcpyDeviceToHost, h->cpy),
                    "D2H rect L");
        if (io.rect_right)
            HIP_TRY(hipMemcpy2DAsync(io.rect_right, io.rect_stride, dRectR, row, row, H, hipMemcpyDeviceToHost, h->cpy),
                    "D2H rect R");
    }
    if (msg_dst == dMsg)
        HIP_TRY(hipMemcpy2DAsync(io.disparity, io.disparity_stride * 4, dMsg, (size_t)W * 4, (size_t)W * 4, H,
                                 hipMemcpyDeviceToHost, st), "D2H disparity");
    if (depth_dst == dDepth && io.depth)
        HIP_TRY(hipMemcpy2DAsync(io.depth, io.depth_stride * 4, dDepth, (size_t)W * 4, (size_t)W * 4, H,
                                 hipMemcpyDeviceToHost, st), "D2H depth");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    HIP_TRY(hipStreamSynchronize(h->cpy), "sync");
    return mark_done(h, st);
}

}  // namespace

extern "C" {

int sgm_node_frame(sgm_handle* h, const sgm_camera_info* left, const sgm_camera_info* right,
                   const sgm_node_frame_io* io)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!left || !right || !io) return fail(h, SGM_ERR_ARG, "null camera info or io");
    if (io->struct_size != sizeof(sgm_node_frame_io))
        return fail(h, SGM_ERR_ARG, "sgm_node_frame_io.struct_size is not this library's sizeof(sgm_node_frame_io)");
    return node_frame(h, *left, *right, *io);
}

int sgm_node_frame_map_builds(const sgm_handle* h) { return h ? h->node_builds : 0; }

}  // extern "C"
