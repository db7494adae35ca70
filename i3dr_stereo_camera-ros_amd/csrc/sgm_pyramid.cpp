// sgm_pyramid.cpp — the half-resolution pyramid level (sgm_set_pyramid_params): its plan and
// validation, the level-1 layer around the unchanged level-0 entry points, and the two stage entry
// points of the parity tests.
//
// A level-1 call halves each pair (pyramid.hip k_pyr_down, which also writes the full-resolution
// code planes), runs the coarse frames through device_batch_locked under a coarse copy of the
// handle's configuration (level 0, mc / Dc, hole filling off, mono rectified frames), refines each
// frame (k_pyr_refine) and fills its holes. The planes live in a buffer of their own (the
// workspace belongs to the coarse match) for at most kPyrGroup frames at a time.
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "sgm_host.h"

using namespace sgm;

namespace sgm {

int pyramid_status(const sgm_pyramid_params& p, std::string& err)
{
    if (p.level != 0 && p.level != 1) {
        err = "pyramid level must be 0 or 1 (sgm_set_pyramid_params), got " + std::to_string(p.level);
        return SGM_ERR_PARAM;
    }
    if (p.level == 1 && (p.radius < 1 || p.radius > 2)) {
        err = "pyramid radius must be within 1..2 (sgm_set_pyramid_params), got " + std::to_string(p.radius);
        return SGM_ERR_PARAM;
    }
    return SGM_OK;
}

// The coarse geometry and configuration of a level-1 match of a W x H frame under c, with the
// parameter errors a match returns: the full-resolution parameters as at level 0, except that the
// mode's range cap applies to Dc, then those of the coarse match.
int pyramid_plan(const MatchConfig& c, int W, int H, PyrPlan& pl, MatchConfig& coarse, std::string& err)
{
    int rc = pyramid_status(c.pyr, err);
    if (rc) return rc;
    const sgm_params& p = c.params;
    Geom g;
    sgm_params full = p;
    if (p.num_disparities > 2048 && p.num_disparities % 16 == 0) {
        err = "numDisparities > 2048 is not supported";
        return SGM_ERR_UNSUPPORTED;
    }
    // the census mode's own cap is checked on the coarse range below
    if (p.mode == SGM_MODE_CENSUS8 && p.num_disparities > 512 && p.num_disparities % 16 == 0) full.num_disparities = 512;
    if ((rc = make_geom(full, W, H, g, err, &c.bm))) return rc;
    const int m = p.min_disparity, D = p.num_disparities;
    pl.Wc = (W + 1) >> 1;
    pl.Hc = (H + 1) >> 1;
    pl.mc = m >> 1;
    pl.Dc = 16 * ((((m + D - 1) >> 1) - pl.mc + 1 + 15) / 16);
    pl.invalid_c = (pl.mc - 1) * 16;
    pl.invalid = (m - 1) * 16;
    coarse = c;
    coarse.params.min_disparity = pl.mc;
    coarse.params.num_disparities = pl.Dc;
    coarse.fill.mode = SGM_FILL_OFF;
    coarse.raw_ch = 1;
    coarse.pyr.level = 0;
    std::string cerr;
    if ((rc = make_geom(coarse.params, pl.Wc, pl.Hc, g, cerr, &coarse.bm))) {
        err = "pyramid level 1, coarse match (" + std::to_string(pl.Wc) + " x " + std::to_string(pl.Hc) +
              ", min_disparity " + std::to_string(pl.mc) + ", num_disparities " + std::to_string(pl.Dc) + "): " + cerr;
        return rc;
    }
    return SGM_OK;
}

int refuse_pyramid(sgm_handle* h, const char* what)
{
    const int rc = pyramid_status(h->cfg.pyr, h->err);
    if (rc) return rc;
    if (pyramid_on(h->cfg))
        return fail(h, SGM_ERR_UNSUPPORTED, std::string(what) + " matches at level 0 only (sgm_set_pyramid_params: level 1)");
    return SGM_OK;
}

namespace {

// The carve-up of the pyramid buffer: the host entry points' staging, the hole filter's planes,
// then the planes of nf frames.
struct PyrLayout {
    size_t inL = 0, inR = 0, out = 0, outf = 0, fpl = 0;
    size_t frames = 0, frame_bytes = 0;
    size_t gL = 0, gR = 0, Lc = 0, Rc = 0, KL = 0, KR = 0, C = 0, pre = 0;   // inside a frame
    size_t total = 0;
};

PyrLayout pyr_layout(int W, int H, int nf, size_t in_row, bool host_io, bool prepass, bool fill)
{
    PyrLayout l;
    const size_t WH = (size_t)W * H, WHc = (size_t)((W + 1) >> 1) * ((H + 1) >> 1);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    if (host_io) {
        l.inL = take(in_row * H); l.inR = take(in_row * H); l.out = take(WH * 2); l.outf = take(WH * 4);
    }
    if (fill) l.fpl = take(fill_plane_bytes(W, H));
    l.frames = o;
    o = 0;
    if (prepass) { l.gL = take(WH); l.gR = take(WH); }
    l.Lc = take(WHc); l.Rc = take(WHc);
    l.KL = take(WH * 4); l.KR = take(WH * 4);
    l.C = take(WHc * 2);
    if (fill) l.pre = take(WH * 2);
    l.frame_bytes = o;
    l.total = l.frames + (size_t)nf * l.frame_bytes;
    return l;
}

int ensure_pyr_buf(sgm_handle* h, size_t bytes)
{
    if (h->pyr_buf_size >= bytes) return SGM_OK;
    if (h->pyr_buf) {
        (void)hipStreamSynchronize(h->stream);
        if (h->done_stream) (void)hipEventSynchronize(h->done);
        (void)hipFree(h->pyr_buf);
        h->pyr_buf = nullptr;
        h->pyr_buf_size = 0;
    }
    if (hipMalloc((void**)&h->pyr_buf, bytes) != hipSuccess) {
        h->pyr_buf = nullptr;
        (void)hipGetLastError();
        return fail(h, SGM_ERR_ALLOC, "hipMalloc pyramid planes");
    }
    h->pyr_buf_size = bytes;
    return SGM_OK;
}

// the handle's configuration and rectification state, put back however the call ends
struct ConfigRestore {
    sgm_handle* h;
    MatchConfig cfg;
    sgm::RectifyIn rect;
    bool on;
    explicit ConfigRestore(sgm_handle* hh) : h(hh), cfg(hh->cfg), rect(hh->rect), on(hh->rect_on) {}
    ~ConfigRestore() { h->cfg = cfg; h->rect = rect; h->rect_on = on; }
};

}  // namespace

int pyr_device_batch(sgm_handle* h, const uint8_t* const* dLs, const uint8_t* const* dRs, int n, int W, int H,
                     size_t stride, uint8_t* const* rectLs, uint8_t* const* rectRs, size_t rect_stride,
                     int16_t* const* outs, size_t out_stride, void* stream, bool host_io, hipEvent_t rect_ev)
{
    PyrPlan pl;
    MatchConfig coarse;
    int rc = pyramid_plan(h->cfg, W, H, pl, coarse, h->err);
    if (rc || (rc = config_status(h, h->cfg))) return rc;
    const sgm_params& p = h->cfg.params;
    const int m = p.min_disparity, D = p.num_disparities;
    if (h->rect_on && W + std::min(m, 0) - std::max(m + D, 0) <= 0)
        return fail(h, SGM_ERR_UNSUPPORTED, "fused rectification needs a non-empty disparity window");
    if ((rc = ensure_stream(h))) return rc;
    const int ch = h->cfg.raw_ch == 3 ? 3 : 1;
    const bool prepass = h->rect_on || ch == 3;
    const bool fill = fill_on(h->cfg);
    const bool bm = p.mode == SGM_MODE_OCV_BM;
    const int subpix = p.mode == SGM_MODE_CENSUS8 ? p.subpixel != 0 : 1;
    const int nf = std::min(n, kPyrGroup);
    const PyrLayout l = pyr_layout(W, H, nf, (size_t)W * ch, host_io, prepass, fill);
    if ((rc = ensure_pyr_buf(h, l.total))) return rc;
    const double WH = (double)W * H;
    hipStream_t own = h->stream;
    struct StreamRestore { sgm_handle* h; hipStream_t own; ~StreamRestore() { h->stream = own; } } keep_stream{h, own};
    if (stream) h->stream = (hipStream_t)stream;
    hipStream_t st = h->stream;
    if ((rc = order_after_last(h, st))) return rc;
    auto frame = [&](int f) { return h->pyr_buf + l.frames + (size_t)f * l.frame_bytes; };
    for (int f0 = 0; f0 < n; f0 += nf) {
        const int ng = std::min(nf, n - f0);
        std::vector<const uint8_t*> cL(ng), cR(ng);
        std::vector<int16_t*> cO(ng);
        {
            StageRec rec{h};
            for (int f = 0; f < ng; f++) {
                char* fb = frame(f);
                const uint8_t* L = dLs[f0 + f];
                const uint8_t* R = dRs[f0 + f];
                size_t s = stride;
                if (prepass) {
                    uint8_t* GL = (uint8_t*)(fb + l.gL);
                    uint8_t* GR = (uint8_t*)(fb + l.gR);
                    if (h->rect_on) {
                        uint8_t* rl = rectLs ? rectLs[f0 + f] : nullptr;
                        uint8_t* rr = rectRs ? rectRs[f0 + f] : nullptr;
                        rec.begin("rectify", (16 + 2 * ch + 2 + ch * ((rl ? 1 : 0) + (rr ? 1 : 0))) * WH);
                        HIP_TRY(sgm::launch_rectify_pair(h->rect, L, R, stride, ch, h->cfg.gray_set, W, H, GL, GR, rl, rr,
                                                         rect_stride, st), "rectify");
                        if (rect_ev) HIP_TRY(hipEventRecord(rect_ev, st), "hipEventRecord");
                    } else {
                        rec.begin("gray", 6 * WH + 2 * WH);
                        HIP_TRY(sgm::launch_bgr2gray(L, R, stride, W, H, GL, GR, W, h->cfg.gray_set, st), "gray");
                    }
                    L = GL; R = GR; s = (size_t)W;
                }
                rec.begin("pyr_down", 10.5 * WH);
                HIP_TRY(sgm::launch_pyr_down(L, R, s, W, H, (uint8_t*)(fb + l.Lc), (uint8_t*)(fb + l.Rc),
                                             (uint32_t*)(fb + l.KL), (uint32_t*)(fb + l.KR), st), "pyr_down");
                cL[f] = (const uint8_t*)(fb + l.Lc);
                cR[f] = (const uint8_t*)(fb + l.Rc);
                cO[f] = (int16_t*)(fb + l.C);
            }
            rec.end();
        }
        {   // the coarse frames: a level-0 batch of mono rectified frames under the coarse configuration
            ConfigRestore keep(h);
            h->cfg = coarse;
            h->rect_on = false;
            rc = device_batch_locked(h, cL.data(), cR.data(), ng, pl.Wc, pl.Hc, (size_t)pl.Wc, nullptr, nullptr, 0,
                                     cO.data(), (size_t)pl.Wc, st);
            h->stream = st;
        }
        if (rc) {
            h->err = "pyramid level 1, coarse match: " + h->err;
            return rc;
        }
        StageRec rec{h};
        for (int f = 0; f < ng; f++) {
            char* fb = frame(f);
            int16_t* dst = fill ? (int16_t*)(fb + l.pre) : outs[f0 + f];
            const size_t dstride = fill ? (size_t)W : out_stride;
            rec.begin("pyr_refine", 10.5 * WH);
            HIP_TRY(sgm::launch_pyr_refine((const uint32_t*)(fb + l.KL), (const uint32_t*)(fb + l.KR),
                                           (const int16_t*)(fb + l.C), (size_t)pl.Wc, W, H, m, D, pl.mc,
                                           h->cfg.pyr.radius, subpix, dst, dstride, st), "pyr_refine");
            if (fill) {
                // the rectangle: the full-resolution columns; BM: the rows its coarse match computes, doubled
                const sgm_fill_params& fp = h->cfg.fill;
                const int x0 = std::max(m + D, 0), x1 = std::max(W + std::min(m, 0), x0);
                const int w2 = p.block_size / 2;
                const int y0 = bm ? std::min(2 * w2, H) : 0, y1 = bm ? std::max(std::min(H, 2 * (pl.Hc - w2)), y0) : H;
                rec.begin("fill", 4 * WH);
                HIP_TRY(sgm::launch_fill_holes(dst, dstride, outs[f0 + f], out_stride, W, H, pl.invalid, fp.mode,
                                               fp.max_gap, fp.min_neighbours, x1 > x0 ? x0 : 0, y0, x1 > x0 ? x1 : 0, y1,
                                               h->pyr_buf + l.fpl, st), "fill");
            }
        }
        rec.end();
    }
    return mark_done(h, st);
}

// sgm_match / sgm_match_f32 at level 1: 2-D copies between the caller's rows and the staging
// images in the pyramid buffer around a one-frame device batch.
int pyr_match_host(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, void* out,
                   size_t out_stride, bool f32)
{
    PyrPlan pl;
    MatchConfig coarse;
    int rc = pyramid_plan(h->cfg, W, H, pl, coarse, h->err);
    if (rc || (rc = config_status(h, h->cfg)) || (rc = ensure_stream(h))) return rc;
    const int ch = h->cfg.raw_ch == 3 ? 3 : 1;
    const size_t row = (size_t)W * ch;
    const PyrLayout l = pyr_layout(W, H, 1, row, true, ch == 3, fill_on(h->cfg));
    if ((rc = ensure_pyr_buf(h, l.total))) return rc;
    hipStream_t st = h->stream;
    if ((rc = order_after_last(h, st))) return rc;
    char* b = h->pyr_buf;
    HIP_TRY(hipMemcpy2DAsync(b + l.inL, row, L, stride, row, H, hipMemcpyHostToDevice, st), "H2D L");
    HIP_TRY(hipMemcpy2DAsync(b + l.inR, row, R, stride, row, H, hipMemcpyHostToDevice, st), "H2D R");
    const uint8_t* l1[1] = {(const uint8_t*)(b + l.inL)};
    const uint8_t* r1[1] = {(const uint8_t*)(b + l.inR)};
    int16_t* d16 = (int16_t*)(b + l.out);
    int16_t* o1[1] = {d16};
    if ((rc = pyr_device_batch(h, l1, r1, 1, W, H, row, nullptr, nullptr, 0, o1, (size_t)W, nullptr, true))) return rc;
    const void* dsrc = d16;
    const size_t es = f32 ? 4 : 2;
    if (f32) {
        HIP_TRY(sgm::launch_to_f32(d16, W, (float*)(b + l.outf), W, W, H, st), "to_f32");
        dsrc = b + l.outf;
    }
    HIP_TRY(hipMemcpy2DAsync(out, out_stride * es, dsrc, W * es, W * es, H, hipMemcpyDeviceToHost, st), "D2H");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    return mark_done(h, st);
}

}  // namespace sgm

// ==================================================================================== C-ABI
extern "C" {

void sgm_default_pyramid_params(sgm_pyramid_params* p)
{
    if (p) *p = kPyramidDefaults;
}

int sgm_set_pyramid_params(sgm_handle* h, const sgm_pyramid_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->cfg.pyr = *p;                  // checked at match time, like every parameter
    return SGM_OK;
}

int sgm_get_pyramid_params(const sgm_handle* h, sgm_pyramid_params* p)
{
    if (!h || !p) return SGM_ERR_ARG;
    *p = h->cfg.pyr;
    return SGM_OK;
}

int sgm_check_pyramid_params(const sgm_pyramid_params* p)
{
    if (!p) return SGM_ERR_ARG;
    std::string err;
    return pyramid_status(*p, err);
}

int sgm_pyramid_plan(const sgm_params* p, const sgm_bm_params* bm, const sgm_pyramid_params* pyr, int W, int H,
                     int out[6])
{
    if (!p || !pyr || !out) return SGM_ERR_ARG;
    MatchConfig c, coarse;
    c.params = *p;
    if (bm) c.bm = *bm;
    c.pyr = *pyr;
    std::string err;
    int rc = pyramid_status(c.pyr, err);
    if (rc) return rc;
    PyrPlan pl;
    if (c.pyr.level == 0) {
        Geom g;
        if ((rc = make_geom(c.params, W, H, g, err, &c.bm))) return rc;
        const int inv = (p->min_disparity - 1) * 16;
        pl = PyrPlan{W, H, p->min_disparity, p->num_disparities, inv, inv};
    } else if ((rc = pyramid_plan(c, W, H, pl, coarse, err))) {
        return rc;
    }
    out[0] = pl.Wc; out[1] = pl.Hc; out[2] = pl.mc; out[3] = pl.Dc; out[4] = pl.invalid_c; out[5] = pl.invalid;
    return SGM_OK;
}

// Both stage entry points stage their images in the pyramid buffer: host images in, one frame's
// planes, host images out.
int sgm_debug_pyr_down(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, uint8_t* outL,
                       uint8_t* outR)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!L || !R || !outL || !outR || W <= 0 || H <= 0 || W > 32767 || H > 32767 || stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    int rc = ensure_stream(h);
    if (rc) return rc;
    const PyrLayout l = pyr_layout(W, H, 1, (size_t)W, true, false, false);
    if ((rc = ensure_pyr_buf(h, l.total)) || (rc = order_after_last(h, h->stream))) return rc;
    hipStream_t st = h->stream;
    char* b = h->pyr_buf;
    char* fb = b + l.frames;
    const size_t Wc = (size_t)((W + 1) >> 1), Hc = (size_t)((H + 1) >> 1);
    HIP_TRY(hipMemcpy2DAsync(b + l.inL, W, L, stride, W, H, hipMemcpyHostToDevice, st), "H2D L");
    HIP_TRY(hipMemcpy2DAsync(b + l.inR, W, R, stride, W, H, hipMemcpyHostToDevice, st), "H2D R");
    HIP_TRY(sgm::launch_pyr_down((const uint8_t*)(b + l.inL), (const uint8_t*)(b + l.inR), W, W, H, (uint8_t*)(fb + l.Lc),
                                 (uint8_t*)(fb + l.Rc), (uint32_t*)(fb + l.KL), (uint32_t*)(fb + l.KR), st), "pyr_down");
    HIP_TRY(hipMemcpyAsync(outL, fb + l.Lc, Wc * Hc, hipMemcpyDeviceToHost, st), "D2H L");
    HIP_TRY(hipMemcpyAsync(outR, fb + l.Rc, Wc * Hc, hipMemcpyDeviceToHost, st), "D2H R");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    return mark_done(h, st);
}

int sgm_debug_pyr_refine(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride,
                         const int16_t* coarse, int m, int D, int mc, int radius, int subpixel, int16_t* out)
{
    if (!h) return SGM_ERR_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!L || !R || !coarse || !out || W <= 0 || H <= 0 || W > 32767 || H > 32767 || stride < (size_t)W)
        return fail(h, SGM_ERR_ARG, "bad buffers or sizes");
    if (radius < 1 || radius > 2) return fail(h, SGM_ERR_PARAM, "pyramid radius must be within 1..2");
    if (D <= 0 || D > 2048 || m < -4096 || m > 4096 || mc < -4096 || mc > 4096)
        return fail(h, SGM_ERR_PARAM, "disparity range out of bounds");
    int rc = ensure_stream(h);
    if (rc) return rc;
    const PyrLayout l = pyr_layout(W, H, 1, (size_t)W, true, false, false);
    if ((rc = ensure_pyr_buf(h, l.total)) || (rc = order_after_last(h, h->stream))) return rc;
    hipStream_t st = h->stream;
    char* b = h->pyr_buf;
    char* fb = b + l.frames;
    const size_t Wc = (size_t)((W + 1) >> 1), Hc = (size_t)((H + 1) >> 1);
    HIP_TRY(hipMemcpy2DAsync(b + l.inL, W, L, stride, W, H, hipMemcpyHostToDevice, st), "H2D L");
    HIP_TRY(hipMemcpy2DAsync(b + l.inR, W, R, stride, W, H, hipMemcpyHostToDevice, st), "H2D R");
    HIP_TRY(hipMemcpyAsync(fb + l.C, coarse, Wc * Hc * 2, hipMemcpyHostToDevice, st), "H2D coarse");
    HIP_TRY(sgm::launch_pyr_down((const uint8_t*)(b + l.inL), (const uint8_t*)(b + l.inR), W, W, H, (uint8_t*)(fb + l.Lc),
                                 (uint8_t*)(fb + l.Rc), (uint32_t*)(fb + l.KL), (uint32_t*)(fb + l.KR), st), "pyr_down");
    HIP_TRY(sgm::launch_pyr_refine((const uint32_t*)(fb + l.KL), (const uint32_t*)(fb + l.KR), (const int16_t*)(fb + l.C),
                                   Wc, W, H, m, D, mc, radius, subpixel, (int16_t*)(b + l.out), (size_t)W, st),
            "pyr_refine");
    HIP_TRY(hipMemcpyAsync(out, b + l.out, (size_t)W * H * 2, hipMemcpyDeviceToHost, st), "D2H");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    return mark_done(h, st);
}

}  // extern "C"
