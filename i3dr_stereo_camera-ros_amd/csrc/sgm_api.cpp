// sgm_api.cpp — C-ABI of libsgm_hip.so (include/sgm_hip.h).
//
// The handle owns one HIP stream and one device workspace on its device. Geometry-
// dependent buffers are (re)allocated lazily at the first match and whenever W, H, D or
// the mode change — mirroring the reference, which constructs its matchers lazily at the
// first frame (generate_disparity.cpp:342-346) and never frees them.
// A per-handle mutex serialises set_params against match (the reference's only locking
// matcher does the same: I3DRSGM.cpp:152, :635).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>

#include "sgm_host.h"

using namespace sgm;

// ==================================================================================== C-ABI
extern "C" {

int sgm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void sgm_default_params(sgm_params* p, int mode)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->mode = mode;
    if (mode == SGM_MODE_CENSUS8) {
        p->min_disparity = 0; p->num_disparities = 128; p->p1 = 10; p->p2 = 120;
        p->uniqueness_ratio = 5; p->disp12_max_diff = 1; p->subpixel = 1; p->lr_check = 1; p->median = 0;
    } else {
        // generate_disparity.cpp:100-112 node defaults
        p->min_disparity = 9; p->num_disparities = 64; p->block_size = 15; p->p1 = 200; p->p2 = 400;
        p->uniqueness_ratio = 15; p->disp12_max_diff = 0; p->prefilter_cap = 31; p->speckle_window_size = 100;
        p->speckle_range = 4; p->subpixel = 1; p->lr_check = 1; p->median = 1;
        p->ocv_compat = SGM_OCV_COMPAT_MELODIC;   // the reference's Dockerfile:1 (melodic, OpenCV 3.2 SSE2)
        if (mode == SGM_MODE_OCV_BM) {            // cv::StereoBM: disp12MaxDiff -1 = off, nothing SGBM-only
            p->disp12_max_diff = -1; p->p1 = p->p2 = 0; p->median = 0; p->lr_check = 0; p->ocv_compat = 0;
        }
    }
}

void sgm_default_bm_params(sgm_bm_params* p)
{
    if (p) *p = kBmDefaults;
}

int sgm_set_bm_params(sgm_handle* h, const sgm_bm_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->cfg.bm = *p;
    return SGM_OK;
}

int sgm_get_bm_params(const sgm_handle* h, sgm_bm_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    *p = h->cfg.bm;
    return SGM_OK;
}

int sgm_set_census_paths(sgm_handle* h, int paths)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->cfg.census_paths = paths;      // checked at match time (prepare), like every parameter
    return SGM_OK;
}

int sgm_get_census_paths(const sgm_handle* h, int* paths)
{
    if (!h || !paths) return SGM_ERR_ARG;
    *paths = h->cfg.census_paths;
    return SGM_OK;
}

void sgm_default_census_window(sgm_census_window* w)
{
    if (w) *w = kCensusWindowDefault;
}

int sgm_set_census_window(sgm_handle* h, const sgm_census_window* w)
{
    if (!h || !w) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->cfg.cwin = *w;                 // checked at match time (prepare), like every parameter
    return SGM_OK;
}

int sgm_get_census_window(const sgm_handle* h, sgm_census_window* w)
{
    if (!h || !w) return SGM_ERR_ARG;
    *w = h->cfg.cwin;
    return SGM_OK;
}

int sgm_check_census_window(const sgm_census_window* w)
{
    if (!w) return SGM_ERR_ARG;
    std::string err;
    return census_window_status(*w, err);
}

// the one table from the node's correlation_window_size slider to a census window
int sgm_census_window_from_size(int w, sgm_census_window* out)
{
    if (!out) return SGM_ERR_ARG;
    const int s = w | 1;              // even values count as the next odd one
    if (s <= 3) *out = {3, 3, 1};
    else if (s == 5) *out = {5, 5, 1};
    else if (s == 7) *out = {7, 7, 1};
    else if (s == 9) *out = {9, 7, 1};
    else if (s <= 13) *out = {7, 7, 2};
    else *out = {9, 7, 2};
    return SGM_OK;
}

void sgm_default_fill_params(sgm_fill_params* p)
{
    if (p) *p = kFillDefaults;
}

int sgm_set_fill_params(sgm_handle* h, const sgm_fill_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->cfg.fill = *p;                 // checked at match time (prepare), like every parameter
    return SGM_OK;
}

int sgm_get_fill_params(const sgm_handle* h, sgm_fill_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    *p = h->cfg.fill;
    return SGM_OK;
}

int sgm_check_fill_params(const sgm_fill_params* p)
{
    if (!p) return SGM_ERR_ARG;
    std::string err;
    return fill_params_status(*p, err);
}

int sgm_fill_holes(sgm_handle* h, const int16_t* d_src, size_t src_stride, int W, int H, int invalid,
                   const sgm_fill_params* params, int x0, int y0, int x1, int y1, int16_t* d_dst, size_t dst_stride,
                   void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    return fill_holes_locked(h, d_src, src_stride, W, H, invalid, params, x0, y0, x1, y1, d_dst, dst_stride, stream);
}

}  // extern "C"

// sgm_fill_holes with h->mu held by the caller. The workspace only ever grows, so a caller that
// sized it for more than the kernel's planes (sgm_debug_fill) keeps its pointers.
int sgm::fill_holes_locked(sgm_handle* h, const int16_t* d_src, size_t src_stride, int W, int H, int invalid,
                           const sgm_fill_params* params, int x0, int y0, int x1, int y1, int16_t* d_dst,
                           size_t dst_stride, void* stream)
{
    if (!d_src || !d_dst || !params || d_src == d_dst || W <= 0 || H <= 0 || W > 32767 || H > 32767 ||
        src_stride < (size_t)W || dst_stride < (size_t)W || x0 < 0 || x0 > x1 || x1 > W || y0 < 0 || y0 > y1 || y1 > H ||
        invalid < -32768 || invalid > 32767)
        return fail(h, SGM_ERR_ARG, "bad buffers, sizes or rectangle");
    int rc = fill_params_status(*params, h->err);
    if (rc || (rc = ensure_stream(h))) return rc;
    // the kernel's three planes live in the workspace: ordered with the handle's other calls, and
    // an uploaded path work list does not survive
    if ((rc = ensure_ws(h, sgm::fill_plane_bytes(W, H)))) return rc;
    h->items_key[0].clear();
    h->items_key[1].clear();
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = order_after_last(h, st))) return rc;
    HIP_TRY(sgm::launch_fill_holes(d_src, src_stride, d_dst, dst_stride, W, H, invalid, params->mode, params->max_gap,
                                   params->min_neighbours, x0, y0, x1, y1, h->ws.base, st), "fill");
    return mark_done(h, st);
}

extern "C" {

int sgm_set_raw_format(sgm_handle* h, int channels, int gray_set)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->cfg.raw_ch = channels;         // checked at match time (prepare), like every parameter
    h->cfg.gray_set = gray_set;
    return SGM_OK;
}

int sgm_get_raw_format(const sgm_handle* h, int* channels, int* gray_set)
{
    if (!h || !channels || !gray_set) return SGM_ERR_ARG;
    *channels = h->cfg.raw_ch;
    *gray_set = h->cfg.gray_set;
    return SGM_OK;
}

int sgm_check_bm_params(const sgm_params* p, const sgm_bm_params* bm, int width, int height)
{
    if (!p || !bm) return SGM_ERR_ARG;
    Geom g;
    std::string err;
    return make_geom(*p, width, height, g, err, bm);
}

int sgm_create(sgm_handle** out, int device)
{
    if (!out) return SGM_ERR_ARG;
    *out = nullptr;
    const int n = sgm_device_count();
    if (device < 0 || device >= n) return SGM_ERR_DEVICE;
    sgm_handle* h = new (std::nothrow) sgm_handle();
    if (!h) return SGM_ERR_ALLOC;
    h->device = device;
    sgm_default_params(&h->cfg.params, SGM_MODE_CENSUS8);
    *out = h;
    return SGM_OK;
}

void sgm_destroy(sgm_handle* h)
{
    if (!h) return;
    for (sgm_handle* s : h->sub) sgm_destroy(s);
    for (sgm_handle* s : h->bands) sgm_destroy(s);
    for (sgm_handle* s : h->par) sgm_destroy(s);
    if (hipSetDevice(h->device) == hipSuccess) {
        if (h->par_ev) (void)hipEventDestroy(h->par_ev);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        if (h->stream2) (void)hipStreamSynchronize(h->stream2);
        if (h->done_stream) (void)hipEventSynchronize(h->done);   // the last call on a caller's stream
        for (hipEvent_t e : h->bev) if (e) (void)hipEventDestroy(e);
        if (h->stream2) (void)hipStreamDestroy(h->stream2);
        if (h->ws.base) (void)hipFree(h->ws.base);
        if (h->pin) (void)hipHostFree(h->pin);
        if (h->items_pin) (void)hipHostFree(h->items_pin);
        if (h->aux) (void)hipFree(h->aux);
        if (h->cubic_tab) (void)hipFree(h->cubic_tab);
        for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
        if (h->up) { (void)hipStreamSynchronize(h->up); (void)hipStreamDestroy(h->up); }
        if (h->down) { (void)hipStreamSynchronize(h->down); (void)hipStreamDestroy(h->down); }
        for (hipEvent_t e : h->io_ev) (void)hipEventDestroy(e);
        if (h->io_dev) (void)hipFree(h->io_dev);
        if (h->io_pin) (void)hipHostFree(h->io_pin);
        if (h->cpy) { (void)hipStreamSynchronize(h->cpy); (void)hipStreamDestroy(h->cpy); }
        if (h->cpy_ev) (void)hipEventDestroy(h->cpy_ev);
        if (h->node_ev) (void)hipEventDestroy(h->node_ev);
        if (h->node_maps) (void)hipFree(h->node_maps);
        if (h->node_buf) (void)hipFree(h->node_buf);
        if (h->pyr_buf) (void)hipFree(h->pyr_buf);
        for (const auto& r : h->regs) (void)hipHostUnregister(r.host);
        if (h->done) (void)hipEventDestroy(h->done);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

int sgm_set_params(sgm_handle* h, const sgm_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->cfg.params = *p;
    return SGM_OK;
}

int sgm_get_params(const sgm_handle* h, sgm_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    *p = h->cfg.params;
    return SGM_OK;
}

int sgm_abi_version(void) { return SGM_ABI_VERSION; }

int sgm_host_register(sgm_handle* h, void* ptr, size_t bytes)
{
    if (!h) return SGM_ERR_ARG;
    if (!ptr || !bytes) return fail(h, SGM_ERR_ARG, "null or empty host range");
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    // a failed registration is not fatal to the caller (it falls back to pageable copies), so
    // HIP's last error is cleared here: the next launcher's hipGetLastError must not report it
    hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return hip_fail(h, e, "hipHostRegister");
    }
    void* dev = nullptr;
    if ((e = hipHostGetDevicePointer(&dev, ptr, 0)) != hipSuccess) dev = nullptr;   // registered, not mapped
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(h->mu);
    h->regs.push_back({(char*)ptr, bytes, (char*)dev});
    return SGM_OK;
}

int sgm_host_unregister(sgm_handle* h, void* ptr)
{
    if (!h) return SGM_ERR_ARG;
    if (!ptr) return fail(h, SGM_ERR_ARG, "null host pointer");
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->done_stream) HIP_TRY(hipEventSynchronize(h->done), "hipEventSynchronize");   // no kernel still writes it
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) {                 // still registered: the handle keeps its mapping
        (void)hipGetLastError();
        return hip_fail(h, e, "hipHostUnregister");
    }
    for (size_t i = 0; i < h->regs.size(); i++)
        if (h->regs[i].host == (char*)ptr) { h->regs.erase(h->regs.begin() + i); break; }
    return SGM_OK;
}

int sgm_check_params(const sgm_params* p, int width, int height)
{
    if (!p) return SGM_ERR_ARG;
    Geom g;
    std::string err;
    return make_geom(*p, width, height, g, err);
}

const char* sgm_last_error(const sgm_handle* h) { return h ? h->err.c_str() : "null handle"; }

int sgm_match_device(sgm_handle* h, const uint8_t* dL, const uint8_t* dR, int W, int H, size_t stride, int16_t* dOut,
                     size_t out_stride, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    // raw inputs: rectified in the census tiles or by the OCV / BM pre-pass; pyramid level 1: a batch of one
    if (h->rect_on || pyramid_on(h->cfg)) {
        const uint8_t* l1[1] = {dL};
        const uint8_t* r1[1] = {dR};
        int16_t* o1[1] = {dOut};
        return sgm_match_device_batch_rect(h, l1, r1, 1, W, H, stride, nullptr, nullptr, 0, o1, out_stride, stream);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    if (!dL || !dR || !dOut || W <= 0 || stride < (size_t)W * raw_bpp(h) || out_stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers");
    Geom g;
    Layout l;
    int rc = prepare(h, h->cfg, W, H, false, g, l);
    if (rc) return rc;
    hipStream_t own = h->stream;
    if (stream) h->stream = (hipStream_t)stream;
    rc = order_after_last(h, h->stream);
    if (!rc) rc = run_pipeline(h, l, g, dL, dR, stride, dOut, out_stride);
    if (!rc) rc = mark_done(h, h->stream);
    h->stream = own;
    return rc;
}

int sgm_match_device_batch_rect(sgm_handle* h, const uint8_t* const* dLs, const uint8_t* const* dRs, int n, int W,
                                int H, size_t stride, uint8_t* const* rectLs, uint8_t* const* rectRs,
                                size_t rect_stride, int16_t* const* outs, size_t out_stride, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t bpp = raw_bpp(h);     // strides of colour frames are in bytes
    const size_t in_w = (h->rect_on ? (size_t)h->rect.src_w : (size_t)std::max(W, 0)) * bpp;
    if (n < 0 || (n > 0 && (!dLs || !dRs || !outs)) || stride < in_w || out_stride < (size_t)std::max(W, 0))
        return fail(h, SGM_ERR_ARG, "bad buffers");
    if ((rectLs || rectRs) && (!h->rect_on || rect_stride < (size_t)std::max(W, 0) * bpp))
        return fail(h, SGM_ERR_ARG, "rectified outputs need sgm_set_rectification and rect_stride >= a row's bytes");
    for (int i = 0; i < n; i++)
        if (!dLs[i] || !dRs[i] || !outs[i]) return fail(h, SGM_ERR_ARG, "null frame pointer");
    if (n == 0) return SGM_OK;
    return device_batch_locked(h, dLs, dRs, n, W, H, stride, rectLs, rectRs, rect_stride, outs, out_stride, stream);
}

}  // extern "C"

int sgm::device_batch_locked(sgm_handle* h, const uint8_t* const* dLs, const uint8_t* const* dRs, int n, int W, int H,
                             size_t stride, uint8_t* const* rectLs, uint8_t* const* rectRs, size_t rect_stride,
                             int16_t* const* outs, size_t out_stride, void* stream)
{
    if (pyramid_on(h->cfg))
        return pyr_device_batch(h, dLs, dRs, n, W, H, stride, rectLs, rectRs, rect_stride, outs, out_stride, stream);
    Geom g;
    Layout l;
    int rc = make_geom(h->cfg.params, W, H, g, h->err, &h->cfg.bm);
    if (rc) return rc;
    if (h->rect_on && g.width1 <= 0)
        return fail(h, SGM_ERR_UNSUPPORTED, "fused rectification needs a non-empty disparity window");
    // raw frames: the census mode rectifies inside its tiles, the OCV / BM modes in a pre-pass
    // of each frame (k_rectify_pair) into the handle's grey planes
    // (the census mode with a non-default window does the same ahead of its census launch: the
    // planes are planned with the same flag, and run_batch_census runs the pre-pass itself)
    const bool prepass = h->rect_on && (h->cfg.params.mode != SGM_MODE_CENSUS8 || census_win_on(h->cfg));
    const bool pipelined = h->cfg.params.mode == SGM_MODE_CENSUS8 && (n >= 2 || h->rect_on) && g.width1 > 0;
    rc = prepare(h, h->cfg, W, H, false, g, l, pipelined ? batch_group(n) : 0, prepass);
    if (rc) return rc;
    hipStream_t own = h->stream;
    if (stream) h->stream = (hipStream_t)stream;
    rc = order_after_last(h, h->stream);
    if (rc) {
    } else if (pipelined) {
        rc = run_batch_census(h, l, g, dLs, dRs, n, stride, outs, out_stride, rectLs, rectRs, rect_stride);
    } else if (h->cfg.params.mode != SGM_MODE_CENSUS8 && ocv_batch_lanes(n) > 1 && !h->profiling) {
        rc = run_batch_ocv(h, l, g, W, H, dLs, dRs, n, stride, outs, out_stride, rectLs, rectRs, rect_stride);
    } else {
        for (int i = 0; i < n && rc == 0; i++) {
            const RectOut ro{rectLs ? rectLs[i] : nullptr, rectRs ? rectRs[i] : nullptr, rect_stride};
            rc = run_pipeline(h, l, g, dLs[i], dRs[i], stride, outs[i], out_stride, nullptr, nullptr, 0,
                              prepass ? &ro : nullptr);
        }
    }
    if (!rc) rc = mark_done(h, h->stream);
    h->stream = own;
    return rc;
}

extern "C" {

int sgm_match_device_batch(sgm_handle* h, const uint8_t* const* dLs, const uint8_t* const* dRs, int n, int W, int H,
                           size_t stride, int16_t* const* outs, size_t out_stride, void* stream)
{
    return sgm_match_device_batch_rect(h, dLs, dRs, n, W, H, stride, nullptr, nullptr, 0, outs, out_stride, stream);
}

int sgm_set_rectification(sgm_handle* h, const float* d_map_xl, const float* d_map_yl, const float* d_map_xr,
                          const float* d_map_yr, size_t map_stride, int src_w, int src_h)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!d_map_xl && !d_map_yl && !d_map_xr && !d_map_yr) { h->rect_on = false; return SGM_OK; }
    if (!d_map_xl || !d_map_yl || !d_map_xr || !d_map_yr || src_w <= 0 || src_h <= 0 || map_stride == 0)
        return fail(h, SGM_ERR_ARG, "rectification needs four maps and the raw image size");
    int rc = ensure_stream(h);
    if (rc) return rc;
    if ((rc = ensure_cubic_table(h))) return rc;
    h->rect = sgm::RectifyIn{{d_map_xl, d_map_yl, d_map_xr, d_map_yr}, map_stride, src_w, src_h, h->cubic_tab};
    h->rect_on = true;
    return SGM_OK;
}

int sgm_disparity_to_msg(sgm_handle* h, const int16_t* d_disp, size_t disp_stride, int W, int H, float min_disparity,
                         float max_disparity, float* d_out, size_t out_stride, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!d_disp || !d_out || W <= 0 || H <= 0 || disp_stride < (size_t)W || out_stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    int rc = ensure_stream(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIP_TRY(sgm::launch_disp_to_msg(d_disp, disp_stride, W, H, min_disparity, max_disparity, d_out, out_stride, st),
            "disp_to_msg");
    return SGM_OK;
}

int sgm_rectify_map(sgm_handle* h, const double K[9], const double* dist, int n_dist, const double R[9],
                    const double P[12], int W, int H, float* d_map_x, float* d_map_y, size_t map_stride, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!K || !P || !d_map_x || !d_map_y || W <= 0 || H <= 0 || map_stride < (size_t)W || (n_dist > 0 && !dist))
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    if (n_dist != 0 && n_dist != 4 && n_dist != 5 && n_dist != 8 && n_dist != 12)
        return fail(h, SGM_ERR_UNSUPPORTED, "distortion vector must have 0, 4, 5, 8 or 12 elements");
    double d12[12] = {};
    for (int i = 0; i < n_dist; i++) d12[i] = dist[i];
    double ir[9];
    if (!sgm::rectify_inverse(P, R, ir)) return fail(h, SGM_ERR_ARG, "singular P[:, :3] * R");
    int rc = ensure_stream(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIP_TRY(sgm::launch_rectify_map(K, d12, ir, W, H, d_map_x, d_map_y, map_stride, st), "rectify_map");
    return SGM_OK;
}

void sgm_cubic_table(int16_t* tab) { if (tab) sgm::cubic_table(tab); }

int sgm_remap_cubic(sgm_handle* h, const uint8_t* d_src, size_t src_stride, int src_w, int src_h, const float* d_map_x,
                    const float* d_map_y, size_t map_stride, int W, int H, uint8_t* d_dst, size_t dst_stride,
                    void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!d_src || !d_map_x || !d_map_y || !d_dst || W <= 0 || H <= 0 || src_w <= 0 || src_h <= 0 ||
        src_stride < (size_t)src_w || map_stride < (size_t)W || dst_stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    int rc = ensure_stream(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = ensure_cubic_table(h))) return rc;
    HIP_TRY(sgm::launch_remap_cubic(d_src, src_stride, src_w, src_h, d_map_x, d_map_y, map_stride, W, H,
                                    h->cubic_tab, d_dst, dst_stride, st), "remap_cubic");
    return SGM_OK;
}

int sgm_remap_cubic_c3(sgm_handle* h, const uint8_t* d_src, size_t src_stride, int src_w, int src_h,
                       const float* d_map_x, const float* d_map_y, size_t map_stride, int W, int H, uint8_t* d_dst,
                       size_t dst_stride, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!d_src || !d_map_x || !d_map_y || !d_dst || W <= 0 || H <= 0 || src_w <= 0 || src_h <= 0 ||
        src_stride < (size_t)src_w * 3 || map_stride < (size_t)W || dst_stride < (size_t)W * 3)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    int rc = ensure_stream(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = ensure_cubic_table(h))) return rc;
    HIP_TRY(sgm::launch_remap_cubic_c3(d_src, src_stride, src_w, src_h, d_map_x, d_map_y, map_stride, W, H,
                                       h->cubic_tab, d_dst, dst_stride, st), "remap_cubic_c3");
    return SGM_OK;
}

int sgm_bgr2gray(sgm_handle* h, const uint8_t* d_src, size_t src_stride, int W, int H, uint8_t* d_dst,
                 size_t dst_stride, int gray_set, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!d_src || !d_dst || W <= 0 || H <= 0 || src_stride < (size_t)W * 3 || dst_stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    if (gray_set != SGM_GRAY_Y14 && gray_set != SGM_GRAY_Y15)
        return fail(h, SGM_ERR_PARAM, "unknown grey set " + std::to_string(gray_set));
    int rc = ensure_stream(h);
    if (rc) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    HIP_TRY(sgm::launch_bgr2gray(d_src, nullptr, src_stride, W, H, d_dst, nullptr, dst_stride, gray_set, st), "bgr2gray");
    return SGM_OK;
}

void sgm_calc_q(const double K[9], const double Pr[12], const double Pl[12], double Q[16])
{
    // disparity_to_depth.cpp:62-84
    const double cx = Pl[2], cxr = Pr[2], cy = Pl[4 + 2], fx = K[0];
    const double p14 = Pr[3];
    const double T = -p14 / fx;
    const double q33 = -(cx - cxr) / T;
    for (int i = 0; i < 16; i++) Q[i] = 0.0;
    Q[0] = 1.0;  Q[3] = -cx;
    Q[5] = 1.0;  Q[7] = -cy;
    Q[11] = fx;
    Q[14] = 1.0 / T;
    Q[15] = q33;
}

int sgm_depth_points(sgm_handle* h, const float* d_disp, size_t disp_stride, int W, int H, const uint8_t* d_color,
                     size_t color_stride, int channels, const double q[5], double depth_min, double depth_max,
                     float* d_depth, size_t depth_stride, sgm_point_xyzrgb* d_points, int max_points,
                     int* d_num_points, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!d_disp || !q || W <= 0 || H <= 0 || disp_stride < (size_t)W || (d_depth && depth_stride < (size_t)W) ||
        (channels != 0 && channels != 1 && channels != 3) || (channels && !d_color) ||
        (channels && color_stride < (size_t)W * channels) || (d_points && max_points < 0))
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    int rc = ensure_stream(h);
    if (rc) return rc;
    if (h->aux_n < (size_t)(2 * H + 1)) {
        if (h->aux) (void)hipFree(h->aux);
        h->aux = nullptr;
        h->aux_n = 0;
        HIP_TRY(hipMalloc(&h->aux, sizeof(int) * (2 * (size_t)H + 1)), "hipMalloc aux");
        h->aux_n = 2 * (size_t)H + 1;
    }
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const float qf[5] = {(float)q[0], (float)q[1], (float)q[2], (float)q[3], (float)q[4]};   // :134-138
    int* row_count = h->aux;
    int* row_off = h->aux + H;
    HIP_TRY(sgm::launch_depth_points(d_disp, disp_stride, W, H, qf, depth_min, depth_max, d_color, color_stride,
                                     channels, d_depth, depth_stride, (float4*)d_points, d_points ? max_points : 0,
                                     row_count, row_off, st), "depth_points");
    if (d_num_points)
        HIP_TRY(hipMemcpyAsync(d_num_points, row_off + H, sizeof(int), hipMemcpyDeviceToDevice, st), "count");
    return SGM_OK;
}

int sgm_synchronize(sgm_handle* h)
{
    if (!h) return SGM_ERR_ARG;
    if (!h->stream) return SGM_OK;
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    HIP_TRY(hipStreamSynchronize(h->stream), "hipStreamSynchronize");
    return SGM_OK;
}

int sgm_match(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, int16_t* disp,
              size_t out_stride)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->rect_on) return fail(h, SGM_ERR_UNSUPPORTED, "fused rectification applies to device-buffer matches");
    if (!L || !R || !disp || W <= 0 || H <= 0 || stride < (size_t)W * raw_bpp(h) || out_stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    if (pyramid_on(h->cfg)) return pyr_match_host(h, L, R, W, H, stride, disp, out_stride, false);
    return match_host(h, L, R, W, H, stride, disp, out_stride, false);
}

int sgm_match_f32(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, float* disp,
                  size_t out_stride)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->rect_on) return fail(h, SGM_ERR_UNSUPPORTED, "fused rectification applies to device-buffer matches");
    if (!L || !R || !disp || W <= 0 || H <= 0 || stride < (size_t)W * raw_bpp(h) || out_stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    if (pyramid_on(h->cfg)) return pyr_match_host(h, L, R, W, H, stride, disp, out_stride, true);
    return match_host(h, L, R, W, H, stride, disp, out_stride, true);
}

}  // extern "C"
