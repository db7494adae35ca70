// sgm_debug.cpp — profiling (per-stage timings of a handle) and the sgm_debug_* entry points that
// run one stage alone for the tests.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sgm_host.h"

using namespace sgm;

extern "C" {

int sgm_set_profiling(sgm_handle* h, int enable)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->profiling = enable != 0;
    h->ev_used = 0;
    h->launches.clear();
    h->prof_frames = 0;
    h->nstages = 0;
    return SGM_OK;
}

int sgm_profiled_matches(const sgm_handle* h) { return h ? h->prof_frames : 0; }

int sgm_get_stage_times(sgm_handle* h, float* ms, int max)
{
    if (!h || !ms) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->launches.empty()) return 0;
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    HIP_TRY(hipEventSynchronize(h->ev_pool[h->ev_used - 1]), "hipEventSynchronize");
    const int n = std::min(h->nstages, max);
    std::vector<double> acc(h->nstages, 0.0);
    std::vector<int> cnt(h->nstages, 0);
    for (const auto& r : h->launches) {
        if (r.ev1 == r.ev0) continue;           // never closed
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, h->ev_pool[r.ev0], h->ev_pool[r.ev1]), "hipEventElapsedTime");
        acc[r.stage] += t;
        cnt[r.stage]++;
    }
    for (int i = 0; i < n; i++) ms[i] = (float)(acc[i] / std::max(cnt[i], 1));
    return n;
}

const char* sgm_stage_name(const sgm_handle* h, int i)
{
    if (!h || i < 0 || i >= h->nstages) return "";
    return h->stage_name[i];
}

double sgm_stage_bytes(const sgm_handle* h, int i)
{
    if (!h || i < 0 || i >= h->nstages) return 0.0;
    return h->stage_bytes[i];
}

int sgm_stage_launches(const sgm_handle* h, int i)
{
    if (!h || i < 0 || i >= h->nstages) return 0;
    int c = 0;
    for (const auto& r : h->launches) c += (r.stage == i && r.ev1 != r.ev0) ? 1 : 0;
    return c;
}

// ------------------------------------------------------------------ stage entry points
int sgm_debug_census(sgm_handle* h, const uint8_t* img, int W, int H, size_t stride, uint64_t* out)
{
    if (!h || !img || !out || W <= 0 || H <= 0 || stride < (size_t)W) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    // the handle's window; an invalid one is an error in the census mode only: the OCV and BM modes
    // ignore the stored window, so there the call keeps giving the 9x7 codes
    sgm_census_window cw = h->cfg.cwin;
    int rc = SGM_OK;
    if (!census_window_ok(cw)) {
        if (h->cfg.params.mode == SGM_MODE_CENSUS8) return census_window_status(cw, h->err);
        cw = kCensusWindowDefault;
    }
    if ((rc = ensure_stream(h)) || (rc = order_after_last(h, h->stream))) return rc;
    const size_t WH = (size_t)W * H;
    if ((rc = ensure_ws(h, align_up(WH) + WH * 8))) return rc;
    char* ws = (char*)h->ws.base;
    HIP_TRY(hipMemcpy2DAsync(ws, W, img, stride, W, H, hipMemcpyHostToDevice, h->stream), "H2D");
    HIP_TRY(sgm::launch_census_planes(cw, (const uint8_t*)ws, nullptr, W, W, H, (uint64_t*)(ws + align_up(WH)),
                                      nullptr, h->stream), "census");
    HIP_TRY(hipMemcpyAsync(out, ws + align_up(WH), WH * 8, hipMemcpyDeviceToHost, h->stream), "D2H");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SGM_OK;
}

int sgm_debug_census_path(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, int dir,
                          uint8_t* vol)
{
    if (!h || !L || !R || !vol || dir < 0 || dir > 7) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cfg.params.mode != SGM_MODE_CENSUS8) return fail(h, SGM_ERR_PARAM, "census mode required");
    Geom g;
    Layout l;
    // one direction, not a path set: always the eight-slice layout (slice = direction)
    MatchConfig c = h->cfg;
    c.census_paths = 8;
    int rc = prepare(h, c, W, H, true, g, l);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    if (g.width1 <= 0) return SGM_OK;
    char* ws = (char*)h->ws.base;
    HIP_TRY(hipMemcpy2DAsync(ws + l.inL, W, L, stride, W, H, hipMemcpyHostToDevice, h->stream), "H2D");
    HIP_TRY(hipMemcpy2DAsync(ws + l.inR, W, R, stride, W, H, hipMemcpyHostToDevice, h->stream), "H2D");
    uint64_t* cL = (uint64_t*)(ws + l.cL[0]);
    uint64_t* cR = (uint64_t*)(ws + l.cR[0]);
    uint8_t* vols = (uint8_t*)(ws + l.vols[0]);
    HIP_TRY(sgm::launch_census_planes(c.cwin, (const uint8_t*)(ws + l.inL), (const uint8_t*)(ws + l.inR), W, W, H, cL, cR,
                                      h->stream), "census");
    const uint32_t* items;
    const int n_items = path_items(h, l, g, 1u << dir, 1, h->stream, &items);
    if (n_items < 0) return n_items;
    sgm::PathFrames pf{};
    pf.cL[0] = cL; pf.cR[0] = cR; pf.vols[0] = vols; pf.n = 1;
    HIP_TRY(sgm::launch_census_paths(pf, l.vol_bytes, g, items, n_items, h->stream), "paths");
    const size_t cells = (size_t)g.width1 * g.H * g.D;
    HIP_TRY(hipMemcpyAsync(vol, vols + (size_t)dir * l.vol_bytes, cells, hipMemcpyDeviceToHost, h->stream), "D2H");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    // the device order is interleaved inside G-byte chunks (sgm_device.h pair_d): back to [D]
    const int G = sgm::census_vol_group(g.D);
    uint8_t t[16];
    for (size_t c = 0; c + G <= cells; c += G) {
        for (int b = 0; b < G; b++) t[sgm::vol_byte_d(G, b)] = vol[c + b];
        memcpy(vol + c, t, G);
    }
    return SGM_OK;
}

int sgm_debug_ocv_cost(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, int16_t* cost)
{
    if (!h || !L || !R || !cost) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cfg.params.mode == SGM_MODE_CENSUS8 || h->cfg.params.mode == SGM_MODE_OCV_BM)
        return fail(h, SGM_ERR_PARAM, "OCV mode required");
    Geom g;
    Layout l;
    int rc = prepare(h, h->cfg, W, H, true, g, l);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    if (g.width1 <= 0) return SGM_OK;
    char* ws = (char*)h->ws.base;
    HIP_TRY(hipMemcpy2DAsync(ws + l.inL, W, L, stride, W, H, hipMemcpyHostToDevice, h->stream), "H2D");
    HIP_TRY(hipMemcpy2DAsync(ws + l.inR, W, R, stride, W, H, hipMemcpyHostToDevice, h->stream), "H2D");
    int16_t* A = (int16_t*)(ws + l.bufA);
    int16_t* B = (int16_t*)(ws + l.bufB);
    int flag = 0;
    if (g.wide == 2) {
        g.ovf = (int*)(ws + l.ovf);
        HIP_TRY(hipMemsetAsync(g.ovf, 0, sizeof(int), h->stream), "hipMemsetAsync");
    }
    HIP_TRY(sgm::launch_ocv_cost((const uint8_t*)(ws + l.inL), (const uint8_t*)(ws + l.inR), W, g,
                                 h->cfg.params.mode == SGM_MODE_OCV_HH8, (uint8_t*)(ws + l.planes), A, B, h->stream),
            "ocv_cost");
    if (g.wide == 2) HIP_TRY(hipMemcpyAsync(&flag, g.ovf, sizeof(int), hipMemcpyDeviceToHost, h->stream), "D2H flag");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    // C' of every frame kind ends in bufA (SIMD_SAT frames in the overflow regime: the exact
    // saturating cost, written over the plain one)
    (void)flag;
    const size_t cells = (size_t)g.width1 * g.H * g.D;
    HIP_TRY(hipMemcpyAsync(cost, A, cells * 2, hipMemcpyDeviceToHost, h->stream), "D2H");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SGM_OK;
}

int sgm_debug_bm_prefilter(sgm_handle* h, const uint8_t* img, int W, int H, size_t stride, uint8_t* out)
{
    if (!h || !img || !out || stride < (size_t)std::max(W, 0)) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cfg.params.mode != SGM_MODE_OCV_BM) return fail(h, SGM_ERR_PARAM, "BM mode required");
    Geom g;
    Layout l;
    int rc = prepare(h, h->cfg, W, H, true, g, l);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    char* ws = (char*)h->ws.base;
    HIP_TRY(hipMemcpy2DAsync(ws + l.inL, W, img, stride, W, H, hipMemcpyHostToDevice, h->stream), "H2D");
    HIP_TRY(sgm::launch_bm_prefilter((const uint8_t*)(ws + l.inL), nullptr, W, W, H, g.ftzero, (uint8_t*)(ws + l.bmL),
                                     nullptr, h->stream),
            "bm_prefilter");
    HIP_TRY(hipMemcpyAsync(out, ws + l.bmL, (size_t)W * H, hipMemcpyDeviceToHost, h->stream), "D2H");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SGM_OK;
}

int sgm_debug_bm_sad(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, int32_t* sad,
                     int32_t* texture)
{
    if (!h || !L || !R || stride < (size_t)std::max(W, 0)) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->cfg.params.mode != SGM_MODE_OCV_BM) return fail(h, SGM_ERR_PARAM, "BM mode required");
    Geom g;
    Layout l;
    int rc = prepare(h, h->cfg, W, H, true, g, l);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    if (g.width1 <= 0) return SGM_OK;
    const size_t pix = (size_t)g.width1 * H, cells = pix * g.D;
    if (cells > ((size_t)1 << 27)) return fail(h, SGM_ERR_UNSUPPORTED, "sgm_debug_bm_sad is for small frames");
    // the debug planes sit behind the match workspace
    const size_t vol_off = align_up(l.total), tex_off = vol_off + align_up(cells * 4);
    if ((rc = ensure_ws(h, tex_off + align_up(pix * 4)))) return rc;
    char* ws = (char*)h->ws.base;
    hipStream_t st = h->stream;
    HIP_TRY(hipMemcpy2DAsync(ws + l.inL, W, L, stride, W, H, hipMemcpyHostToDevice, st), "H2D");
    HIP_TRY(hipMemcpy2DAsync(ws + l.inR, W, R, stride, W, H, hipMemcpyHostToDevice, st), "H2D");
    HIP_TRY(hipMemsetAsync(ws + vol_off, 0, tex_off + align_up(pix * 4) - vol_off, st), "hipMemsetAsync");
    uint8_t* PL = (uint8_t*)(ws + l.bmL);
    uint8_t* PR = (uint8_t*)(ws + l.bmR);
    HIP_TRY(sgm::launch_bm_prefilter((const uint8_t*)(ws + l.inL), (const uint8_t*)(ws + l.inR), W, W, H, g.ftzero, PL,
                                     PR, st),
            "bm_prefilter");
    HIP_TRY(sgm::launch_bm_match(PL, PR, g, l.bm, (int16_t*)(ws + l.out), W, ws + l.bmV, (int*)(ws + vol_off),
                                 (int*)(ws + tex_off), st),
            "bm_match");
    if (sad) HIP_TRY(hipMemcpyAsync(sad, ws + vol_off, cells * 4, hipMemcpyDeviceToHost, st), "D2H");
    if (texture) HIP_TRY(hipMemcpyAsync(texture, ws + tex_off, pix * 4, hipMemcpyDeviceToHost, st), "D2H");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    return mark_done(h, st);
}

static int debug_post(sgm_handle* h, int16_t* disp, int W, int H, int which, int nv, int ms, int md)
{
    if (!h || !disp || W <= 0 || H <= 0) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = ensure_stream(h);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    const size_t WH = (size_t)W * H;
    if ((rc = ensure_ws(h, align_up(WH * 2) * 2 + align_up(WH * 4) * 2))) return rc;
    char* ws = (char*)h->ws.base;
    int16_t* a = (int16_t*)ws;
    int16_t* b = (int16_t*)(ws + align_up(WH * 2));
    int* lab = (int*)(ws + 2 * align_up(WH * 2));
    int* cnt = (int*)(ws + 2 * align_up(WH * 2) + align_up(WH * 4));
    HIP_TRY(hipMemcpyAsync(a, disp, WH * 2, hipMemcpyHostToDevice, h->stream), "H2D");
    if (which == 0) {
        HIP_TRY(sgm::launch_median3(a, W, b, W, W, H, h->stream), "median3");
        HIP_TRY(hipMemcpyAsync(disp, b, WH * 2, hipMemcpyDeviceToHost, h->stream), "D2H");
    } else {
        HIP_TRY(sgm::launch_speckle(nullptr, 0, a, W, W, H, nv, ms, md, lab, cnt, h->stream), "speckle");
        HIP_TRY(hipMemcpyAsync(disp, a, WH * 2, hipMemcpyDeviceToHost, h->stream), "D2H");
    }
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SGM_OK;
}

int sgm_debug_median3(sgm_handle* h, int16_t* disp, int W, int H) { return debug_post(h, disp, W, H, 0, 0, 0, 0); }

// The post filters launched the way run_post launches them: the raw image at stride W, the result in
// an image of row stride W + out_pad. `out` comes in holding the caller's canary and goes back whole.
int sgm_debug_post(sgm_handle* h, const int16_t* disp, int W, int H, int out_pad, int median, int new_val, int max_size,
                   int max_diff, int16_t* out)
{
    if (!h || !disp || !out || W <= 0 || H <= 0 || out_pad < 0) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = ensure_stream(h);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    const size_t WH = (size_t)W * H, stride = (size_t)W + out_pad, OH = stride * H;
    const size_t o_dst = align_up(WH * 2), o_lab = o_dst + align_up(OH * 2), o_cnt = o_lab + align_up(WH * 4);
    if ((rc = ensure_ws(h, o_cnt + align_up(WH * 4)))) return rc;
    char* ws = (char*)h->ws.base;
    int16_t* raw = (int16_t*)ws;
    int16_t* dst = (int16_t*)(ws + o_dst);
    const bool med = median != 0, spk = max_size > 0;           // use_speckle's rule
    HIP_TRY(hipMemcpyAsync(dst, out, OH * 2, hipMemcpyHostToDevice, h->stream), "H2D");
    if (med)
        HIP_TRY(hipMemcpyAsync(raw, disp, WH * 2, hipMemcpyHostToDevice, h->stream), "H2D");
    else      // without a median the matcher writes straight into the destination
        HIP_TRY(hipMemcpy2DAsync(dst, stride * 2, disp, (size_t)W * 2, (size_t)W * 2, H, hipMemcpyHostToDevice,
                                 h->stream), "H2D");
    if (med && !spk) HIP_TRY(sgm::launch_median3(raw, W, dst, stride, W, H, h->stream), "median3");
    if (spk)
        HIP_TRY(sgm::launch_speckle(med ? raw : nullptr, W, dst, stride, W, H, new_val, max_size, max_diff,
                                    (int*)(ws + o_lab), (int*)(ws + o_cnt), h->stream), "speckle");
    HIP_TRY(hipMemcpyAsync(out, dst, OH * 2, hipMemcpyDeviceToHost, h->stream), "D2H");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SGM_OK;
}

int sgm_debug_fill(sgm_handle* h, int16_t* disp, int W, int H, int invalid, const sgm_fill_params* params, int x0,
                   int y0, int x1, int y1)
{
    if (!h || !disp || !params || W <= 0 || H <= 0) return SGM_ERR_ARG;
    const size_t WH = (size_t)W * H, img = align_up(WH * 2);
    std::lock_guard<std::mutex> lk(h->mu);        // held to the end: the workspace stays as carved here
    int rc = ensure_stream(h);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    // the two images behind the planes that the filter takes from the workspace's start
    if ((rc = ensure_ws(h, sgm::fill_plane_bytes(W, H) + 2 * img))) return rc;
    int16_t* a = (int16_t*)((char*)h->ws.base + sgm::fill_plane_bytes(W, H));
    int16_t* b = (int16_t*)((char*)a + img);
    HIP_TRY(hipMemcpyAsync(a, disp, WH * 2, hipMemcpyHostToDevice, h->stream), "H2D");
    if ((rc = fill_holes_locked(h, a, W, W, H, invalid, params, x0, y0, x1, y1, b, W, nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(disp, b, WH * 2, hipMemcpyDeviceToHost, h->stream), "D2H");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SGM_OK;
}

int sgm_debug_path_items(const sgm_params* p, int width, int height, unsigned dir_mask, int n_slots, int group,
                         int up_group, uint32_t* out, int cap)
{
    if (!p || p->mode != SGM_MODE_CENSUS8) return SGM_ERR_ARG;
    Geom g;
    std::string err;
    const int rc = make_geom(*p, width, height, g, err);
    if (rc) return rc;
    if (g.width1 <= 0) return 0;
    const int n = sgm::census_path_items(g, dir_mask & 0xFFu, n_slots, group, nullptr, 0, up_group);
    if (!out) return n;
    if (n > cap) return SGM_ERR_ARG;
    return sgm::census_path_items(g, dir_mask & 0xFFu, n_slots, group, out, cap, up_group);
}

int sgm_debug_bm_plan(const sgm_params* p, const sgm_bm_params* bm, int width, int height, int n_cu, int out[12])
{
    if (!p || !bm || !out || p->mode != SGM_MODE_OCV_BM) return SGM_ERR_ARG;
    Geom g;
    std::string err;
    const int rc = make_geom(*p, width, height, g, err, bm);
    if (rc) return rc;
    const sgm::BmPlan pl = sgm::bm_plan(g, n_cu);
    const int v[12] = {pl.TX, pl.nsx, pl.nsy, pl.RB, pl.waves, (int)pl.lds, pl.vglobal, pl.wide, pl.nk, pl.Dp,
                       g.width1, std::max(g.H - 2 * g.SW2, 0)};
    std::copy(v, v + 12, out);
    return SGM_OK;
}

int sgm_debug_speckle(sgm_handle* h, int16_t* disp, int W, int H, int new_val, int max_size, int max_diff)
{
    return debug_post(h, disp, W, H, 1, new_val, max_size, max_diff);
}

}  // extern "C"
