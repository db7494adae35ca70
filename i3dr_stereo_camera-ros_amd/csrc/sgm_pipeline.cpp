// sgm_pipeline.cpp — the handle's device resources, the single-frame pipeline and the two batch
// schedulers. Everything runs asynchronously on the handle's stream; the entry points order calls.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "sgm_host.h"

namespace sgm {

int ensure_stream(sgm_handle* h)
{
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    if (!h->stream) HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), "hipStreamCreate");
    if (!h->done) HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming), "hipEventCreate");
    if (!h->n_cu) HIP_TRY(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device), "attr");
    return SGM_OK;
}

// Orders a call on stream `st` after the previous call that used the handle's workspace
// (on any stream): the workspace (codes, volumes, scratch) is shared by all calls.
int order_after_last(sgm_handle* h, hipStream_t st)
{
    if (h->done_stream && h->done_stream != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0), "hipStreamWaitEvent");
    return SGM_OK;
}

// Marks the end of a call's work on `st` (see order_after_last).
int mark_done(sgm_handle* h, hipStream_t st)
{
    HIP_TRY(hipEventRecord(h->done, st), "hipEventRecord");
    h->done_stream = st;
    return SGM_OK;
}

// Records the next pool event on the handle's stream; returns its index or -1.
long record_event(sgm_handle* h)
{
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        h->ev_pool.push_back(e);
    }
    if (hipEventRecord(h->ev_pool[h->ev_used], h->stream) != hipSuccess) return -1;
    return (long)h->ev_used++;
}

int stage_index(sgm_handle* h, const char* name, double bytes)
{
    for (int i = 0; i < h->nstages; i++)
        if (std::strcmp(h->stage_name[i], name) == 0) { h->stage_bytes[i] = bytes; return i; }
    if (h->nstages == SGM_MAX_STAGES) return -1;
    h->stage_name[h->nstages] = name;
    h->stage_bytes[h->nstages] = bytes;
    return h->nstages++;
}

int ensure_ws(sgm_handle* h, size_t bytes)
{
    if (h->ws.size >= bytes) return SGM_OK;
    h->items_key[0].clear();       // contents (the path work lists) do not survive
    h->items_key[1].clear();
    if (h->ws.base) {
        (void)hipStreamSynchronize(h->stream);
        if (h->done_stream) (void)hipEventSynchronize(h->done);
        (void)hipFree(h->ws.base);
        h->ws.base = nullptr;
        h->ws.size = 0;
    }
    hipError_t e = hipMalloc(&h->ws.base, bytes);
    if (e != hipSuccess) {
        h->ws.base = nullptr;
        return fail(h, SGM_ERR_ALLOC, std::string("hipMalloc workspace: ") + hipGetErrorString(e));
    }
    h->ws.size = bytes;
    return SGM_OK;
}

int ensure_pin(sgm_handle* h, size_t bytes)
{
    if (h->pin_size >= bytes) return SGM_OK;
    if (h->pin) { (void)hipStreamSynchronize(h->stream); (void)hipHostFree(h->pin); h->pin = nullptr; h->pin_size = 0; }
    hipError_t e = hipHostMalloc((void**)&h->pin, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { h->pin = nullptr; return fail(h, SGM_ERR_ALLOC, "hipHostMalloc staging"); }
    h->pin_size = bytes;
    return SGM_OK;
}

// The INTER_CUBIC weight table on the device, built on the host once per handle.
int ensure_cubic_table(sgm_handle* h)
{
    if (h->cubic_tab) return SGM_OK;
    std::vector<int16_t> tab(32 * 32 * 16);
    sgm::cubic_table(tab.data());
    int16_t* d = nullptr;
    hipError_t e = hipMalloc(&d, tab.size() * 2);
    if (e != hipSuccess) return hip_fail(h, e, "hipMalloc cubic table");
    e = hipMemcpy(d, tab.data(), tab.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(h, e, "upload cubic table"); }
    h->cubic_tab = d;
    return SGM_OK;
}

// Device work list of the census path launch for (g, only_dir), uploaded on `st` when the
// geometry or the workspace changed. Returns the entry count (< 0: error).
int path_items(sgm_handle* h, const Layout& l, const Geom& g, unsigned dir_mask, int group, hipStream_t st,
               const uint32_t** dev, int up_group)
{
    const int w = group > 1 || up_group > 0 ? 1 : 0;
    uint32_t* d = (uint32_t*)((char*)h->ws.base + l.items[w]);
    *dev = d;
    char key[160];
    snprintf(key, sizeof key, "%d %d %d %d %x %d %d %d %d %p", g.W, g.H, g.D, g.minD, dir_mask, group, up_group, h->n_cu,
             l.np, (void*)d);
    const int n = sgm::census_path_items(g, dir_mask, h->n_cu, group, nullptr, 0, up_group);
    if (h->items_key[w] == key) return n;
    if (n > l.n_items[w]) return fail(h, SGM_ERR_ARG, "path work list larger than its workspace slot");
    if (n > h->items_cap) {
        if (h->items_pin) (void)hipHostFree(h->items_pin);
        h->items_pin = nullptr;
        h->items_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&h->items_pin, (size_t)n * 4, hipHostMallocDefault), "hipHostMalloc");
        h->items_cap = n;
    }
    sgm::census_path_items(g, dir_mask, h->n_cu, group, h->items_pin, h->items_cap, up_group);
    HIP_TRY(hipMemcpyAsync(d, h->items_pin, (size_t)n * 4, hipMemcpyHostToDevice, st), "H2D items");
    HIP_TRY(hipStreamSynchronize(st), "sync");    // geometry changes are rare: never leave the pinned copy in flight
    h->items_key[w] = key;
    return n;
}

// Post filters of one finished frame (src = the WTA output in `tmp` when a median runs).
// tmp_off: element offset of this frame's raw image in `tmp` (a pipelined group holds one
// raw image per frame).
int run_post(sgm_handle* h, const Layout& l, const Geom& g, int16_t* dOut, size_t out_stride, StageRec& rec,
             size_t tmp_off)
{
    const sgm_params& p = h->cfg.params;
    char* ws = (char*)h->ws.base;
    const double WH = (double)g.W * g.H;
    const int16_t* raw = (const int16_t*)(ws + l.tmp) + tmp_off;
    const bool med = use_median(p), spk = use_speckle(p);
    // with hole filling the filters below leave their result in this frame's image in front of it
    int16_t* const fOut = dOut;
    const size_t f_stride = out_stride;
    dOut = post_image(l, g, ws, tmp_off / ((size_t)g.W * g.H), dOut);
    out_stride = post_stride(l, g, out_stride);
    if (med && !spk) {
        rec.begin("median3", 4 * WH);
        HIP_TRY(sgm::launch_median3(raw, g.W, dOut, out_stride, g.W, g.H, h->stream), "median3");
    }
    if (spk) {   // with a median, the speckle tiles apply it first (one launch less)
        rec.begin(med ? "median3+speckle" : "speckle", (med ? 4 : 0) * WH + 14 * WH);
        HIP_TRY(sgm::launch_speckle(med ? raw : nullptr, g.W, dOut, out_stride, g.W, g.H, g.invalid,
                                    p.speckle_window_size, speckle_scale(p.mode) * p.speckle_range, (int*)(ws + l.lab),
                                    (int*)(ws + l.cnt), h->stream),
                "speckle");
    }
    if (l.fill) {
        // the rectangle: where the mode can produce a disparity (BM: also its row range)
        const sgm_fill_params& f = h->cfg.fill;
        const bool bm = p.mode == SGM_MODE_OCV_BM;
        const int x0 = g.width1 > 0 ? g.minX1 : 0, x1 = g.width1 > 0 ? g.maxX1 : 0;
        const int y0 = bm ? std::min(g.SW2, g.H) : 0, y1 = bm ? std::max(g.H - g.SW2, y0) : g.H;
        rec.begin("fill", 4 * WH);
        HIP_TRY(sgm::launch_fill_holes(dOut, out_stride, fOut, f_stride, g.W, g.H, g.invalid, f.mode, f.max_gap,
                                       f.min_neighbours, x0, y0, x1, y1, ws + l.fpl, h->stream),
                "fill");
    }
    return SGM_OK;
}

// Runs the whole pipeline on device buffers, asynchronously on h->stream.
// copy_r (census mode): dR is not written yet; the left image's census is launched first, then
// copy_r() issues the right image's copy and returns the event that completes it, and the right
// image's census waits on that event (a pageable copy can hold the host until it is done, so the
// left census must already be queued). outf (census mode without median / speckles): the WTA
// writes the final rows as float to outf (a mapped host buffer, row stride outf_stride floats)
// and dOut is not written. raw (OCV / BM modes, rectification set): dL / dR are raw frames
// (stride = raw stride) that the k_rectify_pair pre-pass rectifies into the grey planes; *raw
// names the frame's rectified-output images, and rect_ev (may be null) is recorded after the
// pre-pass (sgm_node_frame copies the rectified images back from there on its copy stream).
int run_pipeline(sgm_handle* h, const Layout& l, const Geom& g, const uint8_t* dL, const uint8_t* dR, size_t stride,
                 int16_t* dOut, size_t out_stride, const std::function<hipEvent_t()>& copy_r, float* outf,
                 size_t outf_stride, const RectOut* raw, hipEvent_t rect_ev)
{
    const sgm_params& p = h->cfg.params;
    char* ws = (char*)h->ws.base;
    hipStream_t st = h->stream;
    const bool med = use_median(p);
    int16_t* tmp = (int16_t*)(ws + l.tmp);
    // the disparity producer writes to `tmp` when a median follows, else directly to dOut
    int16_t* dst = med ? tmp : post_image(l, g, ws, 0, dOut);
    const size_t dst_stride = med ? (size_t)g.W : post_stride(l, g, out_stride);
    const double WH = (double)g.W * g.H;
    const double cells = (double)std::max(g.width1, 0) * g.H * g.D;
    StageRec rec{h};
    if (h->profiling) h->prof_frames++;
    const int ch = h->cfg.raw_ch == 3 ? 3 : 1;
    // census with a non-default window: its own launch on 8UC1 planes (colour frames converted
    // into the grey planes first, like the OCV modes'). Both images are needed at once, so the
    // right image's copy is issued and waited for up front.
    const bool win = census_win_on(h->cfg) && g.width1 > 0;
    const bool split_r = copy_r && !win;
    if (copy_r && win) {
        const hipEvent_t r_ready = copy_r();
        if (!r_ready) return SGM_ERR_DEVICE;
        HIP_TRY(hipStreamWaitEvent(st, r_ready, 0), "hipStreamWaitEvent");
    }
    if (raw && p.mode != SGM_MODE_CENSUS8 && g.width1 > 0) {
        // raw frames (the node's imageCb): both images through the handle's maps into the grey
        // planes, colour converted after the remap, then the unchanged pipeline on those. Bytes:
        // 16 B/px of maps and ch B/px of source per pair read, 2 B/px of grey and ch B/px per
        // rectified image written.
        uint8_t* GL = (uint8_t*)(ws + l.grayL);
        uint8_t* GR = (uint8_t*)(ws + l.grayR);
        rec.begin("rectify", (16 + 2 * ch + 2 + ch * ((raw->L ? 1 : 0) + (raw->R ? 1 : 0))) * WH);
        HIP_TRY(sgm::launch_rectify_pair(h->rect, dL, dR, stride, ch, h->cfg.gray_set, g.W, g.H, GL, GR, raw->L,
                                         raw->R, raw->stride, st), "rectify");
        if (rect_ev) HIP_TRY(hipEventRecord(rect_ev, st), "hipEventRecord");   // the rectified images are written
        dL = GL; dR = GR; stride = g.W;
    } else if (ch == 3 && (p.mode != SGM_MODE_CENSUS8 || win) && g.width1 > 0) {
        // colour frames: COLOR_BGR2GRAY of both images into the handle's grey planes, then the
        // unchanged pipeline on those (the census mode with its default window converts inside
        // its tiles instead)
        uint8_t* GL = (uint8_t*)(ws + l.grayL);
        uint8_t* GR = (uint8_t*)(ws + l.grayR);
        rec.begin("gray", 6 * WH + 2 * WH);
        HIP_TRY(sgm::launch_bgr2gray(dL, dR, stride, g.W, g.H, GL, GR, g.W, h->cfg.gray_set, st), "gray");
        dL = GL; dR = GR; stride = g.W;
    }
    if (g.width1 <= 0) {
        rec.begin("fill_invalid", 2 * WH);
        HIP_TRY(sgm::launch_fill16(dst, dst_stride, g.W, g.H, g.invalid, st), "fill");
    } else if (p.mode == SGM_MODE_OCV_BM) {
        // pre-filter of both images, then the fused SAD + WTA kernel (no volume in HBM: it reads
        // the two pre-filtered images, L2-resident, and writes the disparity)
        uint8_t* PL = (uint8_t*)(ws + l.bmL);
        uint8_t* PR = (uint8_t*)(ws + l.bmR);
        rec.begin("bm_prefilter", 4 * WH);
        HIP_TRY(sgm::launch_bm_prefilter(dL, dR, stride, g.W, g.H, g.ftzero, PL, PR, st), "bm_prefilter");
        rec.begin("bm_match", 2 * WH + 2 * WH + 2 * (double)g.width1 * (g.H - 2 * g.SW2));
        HIP_TRY(sgm::launch_bm_match(PL, PR, g, l.bm, dst, dst_stride, ws + l.bmV, nullptr, nullptr, st), "bm_match");
    } else if (p.mode == SGM_MODE_CENSUS8) {
        uint64_t* cL = (uint64_t*)(ws + l.cL[0]);
        uint64_t* cR = (uint64_t*)(ws + l.cR[0]);
        uint8_t* vols = (uint8_t*)(ws + l.vols[0]);
        rec.begin(win ? "census_win" : "census", (win ? 2 : 2 * ch) * WH + 16 * WH);
        if (win) {    // dL / dR are 8UC1 here (colour frames went through the grey planes above)
            HIP_TRY(sgm::launch_census_planes(h->cfg.cwin, dL, dR, stride, g.W, g.H, cL, cR, st), "census_win");
        } else if (split_r) {
            HIP_TRY(sgm::launch_census(dL, nullptr, stride, g.W, g.H, cL, nullptr, st, ch, h->cfg.gray_set), "census L");
            const hipEvent_t r_ready = copy_r();
            if (!r_ready) return SGM_ERR_DEVICE;
            HIP_TRY(hipStreamWaitEvent(st, r_ready, 0), "hipStreamWaitEvent");
            HIP_TRY(sgm::launch_census(dR, nullptr, stride, g.W, g.H, cR, nullptr, st, ch, h->cfg.gray_set), "census R");
        } else {
            HIP_TRY(sgm::launch_census(dL, dR, stride, g.W, g.H, cL, cR, st, ch, h->cfg.gray_set), "census");
        }
        const uint32_t* items;
        const int n_items = path_items(h, l, g, sgm::census_dir_mask(l.np), 1, st, &items);
        if (n_items < 0) return n_items;
        sgm::PathFrames pf{};
        pf.cL[0] = cL; pf.cR[0] = cR; pf.vols[0] = vols; pf.n = 1; pf.np = l.np;
        sgm::WtaFrames wf{};
        wf.vols[0] = vols; wf.out[0] = dst; wf.n = 1;
        if (outf) { wf.outf[0] = outf; wf.outf_stride = outf_stride; }
        rec.begin(l.np == 4 ? "paths4" : "paths8", l.np * cells);
        HIP_TRY(sgm::launch_census_paths(pf, l.vol_bytes, g, items, n_items, st), "paths");
        rec.begin("wta_lr", l.np * cells + 2 * WH);
        HIP_TRY(sgm::launch_census_wta(wf, l.vol_bytes, g, dst_stride, st, l.np), "wta");
    } else {
        const int fullDP = p.mode == SGM_MODE_OCV_HH8;
        const int mask = fullDP ? 0xFF : 0xCD;   // SGBM5: dirs 0,2,3,6,7
        const int ndir = fullDP ? 8 : 5;
        int16_t* A = (int16_t*)(ws + l.bufA);
        int16_t* B = (int16_t*)(ws + l.bufB);
        void* V = ws + l.ovols;
        const size_t ncells = (size_t)g.width1 * g.H * g.D;
        Geom gg = g;
        if (g.wide == 2) {             // the cost kernel raises the flag, the gated launches read it
            gg.ovf = (int*)(ws + l.ovf);
            HIP_TRY(hipMemsetAsync(gg.ovf, 0, sizeof(int), st), "hipMemsetAsync");
        }
        const double es = g.wide == 1 && !(g.compat & SGM_OCV_SIMD_SAT) ? 4 : 2;   // gated: the int16 case
        const bool vwta = ocv_vwta_on(g, fullDP);
        // the plain kernels' volumes as deficit planes where they fit (the stage byte bases below stay
        // those of int16 volumes)
        gg.evol = sgm::ocv_evol_mode(gg, mask, vwta ? sgm::ocv_vwta_dir(ndir) : -1);
        rec.begin("ocv_cost", 2 * WH + 2 * cells);
        HIP_TRY(sgm::launch_ocv_cost(dL, dR, stride, gg, fullDP, (uint8_t*)(ws + l.planes), A, B, st), "ocv_cost");
        if (vwta) {
            // the vertical direction of the last group fused with the WTA (k_ocv_vwta), then
            // disp2 + LR of each row from the per-pixel results (the census rowfin)
            const int fd = sgm::ocv_vwta_dir(ndir);
            uint64_t* res = (uint64_t*)(ws + l.ores);
            // the unfused stages' byte basis (C' counted once, in the paths stage)
            rec.begin("ocv_paths", 2 * cells + es * cells * (ndir - 1));
            HIP_TRY(sgm::launch_ocv_paths(A, A, V, ncells, gg, mask, st, fd), "ocv_paths");
            rec.begin("ocv_vwta", es * cells * (ndir - 1) + 8 * WH);
            HIP_TRY(sgm::launch_ocv_vwta(A, A, V, ncells, ndir, gg, res, st), "ocv_vwta");
            sgm::WtaFrames wf{};
            wf.res[0] = res; wf.out[0] = dst; wf.n = 1;
            rec.begin("ocv_rowfin", 8 * WH + 2 * WH);
            HIP_TRY(sgm::launch_census_rowfin(wf, g, dst_stride, st), "ocv_rowfin");
        } else {
            rec.begin("ocv_paths", 2 * cells + es * cells * ndir);
            HIP_TRY(sgm::launch_ocv_paths(A, A, V, ncells, gg, mask, st), "ocv_paths");
            rec.begin("ocv_wta_lr", es * cells * ndir + 2 * WH);
            HIP_TRY(sgm::launch_ocv_wta(A, V, ncells, ndir, gg, dst, dst_stride, st), "ocv_wta");
        }
    }
    int rc = run_post(h, l, g, dOut, out_stride, rec);
    if (rc) return rc;
    rec.end();
    return SGM_OK;
}

// Census-mode frame pipeline on h->stream, in groups of l.group frames.
// up+WTA scheme (l.up_wta, the default):
//   census(G0) | fused[paths7(G0) + census(G1)] | fused[paths7(Gk) + upWTA(Gk-1) + census(Gk+1)]
//   rowfin(Gk-1) post(Gk-1) ... | fused[paths8(Glast) + upWTA(Glast-1)] rowfin post | wta(Glast) post
// paths7 = the seven directions other than dir 1 (volumes written); upWTA = the dir-1 sweep
// of the previous group with its WTA fused (census_sgm.hip UpWta: volume 1 is never stored),
// rowfin = disp2 + LR of those rows. Codes rotate over three sets (group k+1's census runs
// beside group k-1's dir-1 sweep), volumes over two.
// Earlier scheme (SGM_UPWTA=0):
//   census(G0) | fused[paths(G0) + census(G1)] | fused[paths(Gk) + wta(Gk-1) + census(Gk+1)] post(Gk-1)
//   ... | wta(Glast) post
// The census of group k+1 writes the code set of group k-1, whose path sweeps finished in
// the previous launch.
// With 4 census paths (l.np == 4: dirs 0, 1, 6, 7, four slices per volume set) the same
// schemes run with paths3 (dirs 0, 6, 7) / paths4 in place of paths7 / paths8.
// With a median the WTA of a group writes each frame's raw disparity to its own scratch image
// (post filters read it), so no frame's output is overwritten before its median.
// With h->rect_on, dLs / dRs are raw images (stride = raw stride) rectified inside the census
// (the census tiles read remap(raw)), and rectLs / rectRs (may be null) receive the
// rectified images. node (sgm_node_frame, one frame): see NodeOut in sgm_host.h.
int run_batch_census(sgm_handle* h, const Layout& l, const Geom& g, const uint8_t* const* dLs,
                     const uint8_t* const* dRs, int n, size_t stride, int16_t* const* outs, size_t out_stride,
                     uint8_t* const* rectLs, uint8_t* const* rectRs, size_t rect_stride, FrameHooks* hooks,
                     const NodeOut* node)
{
    const sgm_params& p = h->cfg.params;
    char* ws = (char*)h->ws.base;
    hipStream_t st = h->stream;
    const bool med = use_median(p);
    const double WH = (double)g.W * g.H;
    const double cells = (double)g.width1 * g.H * g.D;
    const int G = l.group;
    const bool up = l.up_wta;
    const int ng = (n + G - 1) / G;
    const uint32_t* items;
    const int np = l.np;           // paths summed: 8, or 4 (dirs 0, 1, 6, 7; the names below follow it)
    const int ch = h->cfg.raw_ch == 3 ? 3 : 1;
    // algorithmic bytes of one frame's census: ch B/px read and 8 B/px of codes written per image,
    // plus, for colour frames, 3 B/px per rectified image written
    const double census_bytes = (2 * ch + 16 + (ch == 3 ? 3 * ((rectLs ? 1 : 0) + (rectRs ? 1 : 0)) : 0)) * WH;
    const int n_items = path_items(h, l, g, sgm::census_dir_mask(np), G, st, &items, up ? G : 0);
    if (n_items < 0) return n_items;
    StageRec rec{h};
    if (h->profiling) h->prof_frames += n;
    auto frames_of = [&](int k) { return std::min(G, n - k * G); };
    auto code_set = [&](int k, int f) { return (up ? k % 3 : k & 1) * G + f; };
    auto path_frames = [&](int k) {
        sgm::PathFrames pf{};
        pf.n = frames_of(k);
        pf.np = np;
        for (int f = 0; f < pf.n; f++) {
            pf.cL[f] = (const uint64_t*)(ws + l.cL[code_set(k, f)]);
            pf.cR[f] = (const uint64_t*)(ws + l.cR[code_set(k, f)]);
            pf.vols[f] = (uint8_t*)(ws + l.vols[(k & 1) * G + f]);
        }
        return pf;
    };
    size_t dst_stride = med ? (size_t)g.W : post_stride(l, g, out_stride);
    auto wta_frames = [&](int k) {
        sgm::WtaFrames wf{};
        wf.n = frames_of(k);
        for (int f = 0; f < wf.n; f++) {
            wf.vols[f] = (const uint8_t*)(ws + l.vols[(k & 1) * G + f]);
            wf.out[f] = med ? (int16_t*)(ws + l.tmp) + (size_t)f * g.W * g.H : post_image(l, g, ws, f, outs[k * G + f]);
            if (up) {
                wf.cL[f] = (const uint64_t*)(ws + l.cL[code_set(k, f)]);
                wf.cR[f] = (const uint64_t*)(ws + l.cR[code_set(k, f)]);
                wf.res[f] = (uint64_t*)(ws + l.res[f]);
            }
        }
        return wf;
    };
    auto census_frames = [&](int k) {
        sgm::CensusFrames cf{};
        cf.n = frames_of(k);
        cf.stride = stride;
        cf.rect_stride = rect_stride;
        cf.ch = ch;
        cf.gray = h->cfg.gray_set;
        if (h->rect_on) cf.rect = h->rect;
        for (int f = 0; f < cf.n; f++) {
            cf.L[f] = dLs[k * G + f];
            cf.R[f] = dRs[k * G + f];
            cf.cL[f] = (uint64_t*)(ws + l.cL[code_set(k, f)]);
            cf.cR[f] = (uint64_t*)(ws + l.cR[code_set(k, f)]);
            cf.rectL[f] = rectLs ? rectLs[k * G + f] : nullptr;
            cf.rectR[f] = rectRs ? rectRs[k * G + f] : nullptr;
        }
        return cf;
    };
    // hooks of group k (no-ops without hooks)
    auto hk_in = [&](int k) { return hooks ? hooks->inputs(k * G, frames_of(k)) : 0; };
    auto hk_free = [&](int k) { return hooks ? hooks->outputs_free(k * G, frames_of(k)) : 0; };
    auto hk_done = [&](int k) { return hooks ? hooks->outputs_done(k * G, frames_of(k)) : 0; };
    // A non-default window (sgm_set_census_window): the census of group k is a launch of its own
    // on the stream (stage census_win, all images of the group at once) and the fused launches get
    // an empty CensusFrames. Colour and / or raw frames first go through the OCV modes' pre-pass,
    // frame by frame into the group's grey planes (stage rectify, which also writes the requested
    // rectified images, or gray).
    const bool win = census_win_on(h->cfg);
    const bool pre = census_win_prepass(h->cfg, h->rect_on);
    auto census_win_group = [&](int k) -> int {
        sgm::WinImages wi{};
        wi.n = 2 * frames_of(k);
        wi.stride = pre ? (size_t)g.W : stride;
        for (int f = 0; f < frames_of(k); f++) {
            const int i = k * G + f;
            const uint8_t* pl = dLs[i];
            const uint8_t* pr = dRs[i];
            if (pre) {
                uint8_t* GL = (uint8_t*)(ws + l.grayL) + (size_t)f * g.W * g.H;
                uint8_t* GR = (uint8_t*)(ws + l.grayR) + (size_t)f * g.W * g.H;
                if (h->rect_on) {
                    uint8_t* rl = rectLs ? rectLs[i] : nullptr;
                    uint8_t* rr = rectRs ? rectRs[i] : nullptr;
                    rec.begin("rectify", (16 + 2 * ch + 2 + ch * ((rl ? 1 : 0) + (rr ? 1 : 0))) * WH);
                    HIP_TRY(sgm::launch_rectify_pair(h->rect, pl, pr, stride, ch, h->cfg.gray_set, g.W, g.H, GL, GR, rl, rr,
                                                     rect_stride, st), "rectify");
                    if (node && node->rect_ev) HIP_TRY(hipEventRecord(node->rect_ev, st), "hipEventRecord");
                } else {
                    rec.begin("gray", 6 * WH + 2 * WH);
                    HIP_TRY(sgm::launch_bgr2gray(pl, pr, stride, g.W, g.H, GL, GR, g.W, h->cfg.gray_set, st), "gray");
                }
                pl = GL; pr = GR;
            }
            wi.src[2 * f] = pl; wi.out[2 * f] = (uint64_t*)(ws + l.cL[code_set(k, f)]);
            wi.src[2 * f + 1] = pr; wi.out[2 * f + 1] = (uint64_t*)(ws + l.cR[code_set(k, f)]);
        }
        rec.begin("census_win", (2 + 16) * WH * frames_of(k));
        HIP_TRY(sgm::launch_census_win(wi, g.W, g.H, h->cfg.cwin, st), "census_win");
        return SGM_OK;
    };
    int hrc = hk_in(0);
    if (hrc) return hrc;
    if (win) {
        if ((hrc = census_win_group(0))) return hrc;
    } else if (h->rect_on) {    // remap + census of the first group, one launch
        rec.begin("rectify+census", (census_bytes + 16 * WH) * frames_of(0));
        HIP_TRY(sgm::launch_census_tiles(census_frames(0), g.W, g.H, st), "rectify+census");
        if (node && node->rect_ev) HIP_TRY(hipEventRecord(node->rect_ev, st), "hipEventRecord");
    } else {
        for (int f = 0; f < frames_of(0); f++) {
            rec.begin("census", census_bytes);
            HIP_TRY(sgm::launch_census(dLs[f], dRs[f], stride, g.W, g.H, (uint64_t*)(ws + l.cL[code_set(0, f)]),
                                       (uint64_t*)(ws + l.cR[code_set(0, f)]), st, ch, h->cfg.gray_set), "census");
        }
    }
    for (int k = 0; k <= ng; k++) {
        // this launch reads the inputs of group k + 1 (census in the tail) and writes the
        // disparities of group k - 1 (WTA, or up+WTA and the row finish after it)
        if (k + 1 < ng && ng > 1 && (hrc = hk_in(k + 1))) return hrc;
        if (k > 0 && (hrc = hk_free(k - 1))) return hrc;
        // a non-default window: the next group's census ahead of this launch instead of in its tail
        if (win && k + 1 < ng && (hrc = census_win_group(k + 1))) return hrc;
        if (up && k < ng) {
            // the last group sweeps all eight directions (its WTA rows follow alone: a lone
            // launch of up+WTA blocks would be one long latency-bound chain per column block)
            const bool last = k == ng - 1;
            sgm::PathFrames pf = path_frames(k);
            pf.skip_dirs = last ? 0u : 2u;
            const sgm::WtaFrames wf = k > 0 ? wta_frames(k - 1) : sgm::WtaFrames{};
            const sgm::CensusFrames cf = k + 1 < ng && !win ? census_frames(k + 1) : sgm::CensusFrames{};
            // stage name and algorithmic bytes (the canonical dataflow: the dir-1 volume of an
            // up+WTA frame counted as written and read, as if it existed) from the launch's parts
            const char* name8 = last ? (wf.n ? "paths8+up_wta" : "paths8")
                                     : (wf.n ? (cf.n ? "paths7+up_wta+census" : "paths7+up_wta")
                                             : (cf.n ? "paths7+census" : "paths7"));
            const char* name4 = last ? (wf.n ? "paths4+up_wta" : "paths4")
                                     : (wf.n ? (cf.n ? "paths3+up_wta+census" : "paths3+up_wta")
                                             : (cf.n ? "paths3+census" : "paths3"));
            rec.begin(np == 4 ? name4 : name8,
                      (last ? np : np - 1) * cells * pf.n + ((np + 1) * cells + 2 * WH) * wf.n + census_bytes * cf.n);
            HIP_TRY(sgm::launch_census_fused(pf, wf, cf, l.vol_bytes, g, items, n_items, dst_stride, true, st),
                    "fused");
            if (wf.n) {
                rec.begin("rowfin", 10 * WH * wf.n);
                HIP_TRY(sgm::launch_census_rowfin(wf, g, dst_stride, st), "rowfin");
            }
        } else if (k == ng) {
            rec.begin("wta_lr", (np * cells + 2 * WH) * frames_of(k - 1));
            sgm::WtaFrames wf = wta_frames(k - 1);
            const bool rows = node && node->rows;     // sgm_node_frame: DisparityImage rows from this launch
            if (rows) { wf.outf[0] = node->rows; wf.outf_stride = node->stride; }
            HIP_TRY(sgm::launch_census_wta(wf, l.vol_bytes, g, dst_stride, st, np, rows ? &node->win : nullptr), "wta");
        } else if (ng == 1) {
            rec.begin(np == 4 ? "paths4" : "paths8", np * cells * frames_of(0));
            HIP_TRY(sgm::launch_census_paths(path_frames(0), l.vol_bytes, g, items, n_items, st), "paths");
        } else {
            const sgm::WtaFrames wf = k > 0 ? wta_frames(k - 1) : sgm::WtaFrames{};
            const sgm::CensusFrames cf = k + 1 < ng && !win ? census_frames(k + 1) : sgm::CensusFrames{};
            const char* name8 = wf.n ? (cf.n ? "paths8+wta_lr+census" : "paths8+wta_lr") : (cf.n ? "paths8+census" : "paths8");
            const char* name4 = wf.n ? (cf.n ? "paths4+wta_lr+census" : "paths4+wta_lr") : (cf.n ? "paths4+census" : "paths4");
            rec.begin(np == 4 ? name4 : name8,
                      np * cells * frames_of(k) + (np * cells + 2 * WH) * wf.n + census_bytes * cf.n);
            HIP_TRY(sgm::launch_census_fused(path_frames(k), wf, cf, l.vol_bytes, g, items, n_items, dst_stride, false,
                                             st),
                    "fused");
        }
        if (k > 0) {
            const int k1 = k - 1;
            for (int f = 0; f < frames_of(k1); f++) {
                int rc = run_post(h, l, g, outs[k1 * G + f], out_stride, rec, (size_t)f * g.W * g.H);
                if (rc) return rc;
            }
            if ((hrc = hk_done(k1))) return hrc;
        }
    }
    rec.end();
    return SGM_OK;
}

// sgm_set_raw_format stores anything; a match needs 1 or 3 channels and a known grey set
int raw_format_status(sgm_handle* h, const MatchConfig& c)
{
    if (c.raw_ch != 1 && c.raw_ch != 3)
        return fail(h, SGM_ERR_PARAM, "raw format: channels must be 1 or 3 (sgm_set_raw_format), got " +
                                          std::to_string(c.raw_ch));
    if (c.gray_set != SGM_GRAY_Y14 && c.gray_set != SGM_GRAY_Y15)
        return fail(h, SGM_ERR_PARAM, "raw format: unknown grey set " + std::to_string(c.gray_set));
    return SGM_OK;
}
// the entry points whose frame rings and band copies move one byte per pixel
int refuse_colour(sgm_handle* h, const char* what)
{
    const int rc = raw_format_status(h, h->cfg);
    if (rc) return rc;
    if (h->cfg.raw_ch == 3)
        return fail(h, SGM_ERR_UNSUPPORTED, std::string(what) + " takes mono frames only (sgm_set_raw_format: 3 channels)");
    return SGM_OK;
}
// the overlap tile modes: a band filled alone would differ from the frame at its seams
int refuse_fill(sgm_handle* h, const char* what)
{
    if (fill_on(h->cfg))
        return fail(h, SGM_ERR_UNSUPPORTED, std::string(what) + " does not fill holes (sgm_set_fill_params: switch it off)");
    return SGM_OK;
}
// bytes per pixel of the frames a match takes
size_t raw_bpp(const sgm_handle* h) { return h->cfg.raw_ch == 3 ? 3 : 1; }

// Geometry, layout and workspace of a W x H frame under configuration c (the handle's own, or
// a copy of it that a debug entry point adjusted).
// what a match checks of a configuration besides the geometry (make_geom)
int config_status(sgm_handle* h, const MatchConfig& c)
{
    int rc;
    if (c.params.mode == SGM_MODE_CENSUS8 && c.census_paths != 4 && c.census_paths != 8)
        return fail(h, SGM_ERR_PARAM, "census paths must be 4 or 8 (sgm_set_census_paths), got " +
                                          std::to_string(c.census_paths));
    if (c.params.mode == SGM_MODE_CENSUS8 && (rc = census_window_status(c.cwin, h->err))) return rc;
    if ((rc = raw_format_status(h, c))) return rc;
    if ((rc = fill_params_status(c.fill, h->err))) return rc;
    return pyramid_status(c.pyr, h->err);
}

int prepare(sgm_handle* h, const MatchConfig& c, int W, int H, bool host_io, Geom& g, Layout& l, int group, bool rect)
{
    int rc = make_geom(c.params, W, H, g, h->err, &c.bm);
    if (rc) return rc;
    if ((rc = config_status(h, c))) return rc;
    if ((rc = ensure_stream(h))) return rc;
    l = make_layout(c, g, host_io, group, h->n_cu, rect);
    // the uploaded path work lists live in the workspace: any other use of it invalidates them, also
    // a census call that carves it differently (a single frame after a pipelined batch of the same
    // geometry finds its list's offset inside the batch's second volume set)
    char sig[128];
    snprintf(sig, sizeof sig, "%zu %zu %zu %d %d", l.total, l.items[0], l.items[1], l.group, (int)l.up_wta);
    if (c.params.mode != SGM_MODE_CENSUS8 || h->layout_sig != sig) { h->items_key[0].clear(); h->items_key[1].clear(); }
    h->layout_sig = sig;
    return ensure_ws(h, l.total);
}

// OCV-mode batch (sgm_match_device_batch on an OpenCV mode): frames dealt round-robin over
// S same-device lanes (own stream + workspace each; SGM_OCV_STREAMS, default 4, 1 = one
// frame after another on the handle's stream). Lane 0 is h itself (its workspace is the one
// the caller prepared); lanes 1.. are sub-handles, opened only while the device's free memory
// holds their workspace (the shipped 2448x2048 D=480 block-21 frame needs 27-70 GB per
// workspace, by mode and OpenCV build), and a lane whose allocation fails ends the list. Every
// lane starts after the work already on h->stream, and h->stream waits for every lane, so the
// call keeps the single-stream contract. With h->rect_on the frames are raw: every lane gets the
// handle's rectification state (the maps and the weight table stay the handle's) and plans its
// workspace with the grey planes, and frame i's rectified-output pointers go to the lane that
// runs frame i.
int run_batch_ocv(sgm_handle* h, const Layout& l0, const Geom& g0, int W, int H, const uint8_t* const* dLs,
                  const uint8_t* const* dRs, int n, size_t stride, int16_t* const* outs, size_t out_stride,
                  uint8_t* const* rectLs, uint8_t* const* rectRs, size_t rect_stride)
{
    const int Smax = ocv_batch_lanes(n);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    const size_t reserve = std::max<size_t>(total_b / 64, (size_t)1 << 30);   // headroom for the caller
    std::vector<Geom> g(1, g0);
    std::vector<Layout> l(1, l0);
    while ((int)h->par.size() < Smax - 1) h->par.push_back(nullptr);
    int S = 1;
    for (int s = 1; s < Smax; s++) {
        sgm_handle*& q = h->par[s - 1];
        const size_t have = q ? q->ws.size : 0;
        const size_t extra = have >= l0.total ? 0 : l0.total;
        if (extra + reserve > free_b) break;
        if (!q && sgm_create(&q, h->device) != SGM_OK) break;
        q->cfg = h->cfg;
        q->rect = h->rect;
        q->rect_on = h->rect_on;
        Geom gq;
        Layout lq;
        if (prepare(q, q->cfg, W, H, false, gq, lq, 0, h->rect_on) != SGM_OK) {   // e.g. an allocation failure: fewer lanes
            q->err.clear();
            break;
        }
        free_b -= std::min(free_b, extra);
        g.push_back(gq);
        l.push_back(lq);
        S = s + 1;
    }
    if (S > 1) {
        if (!h->par_ev) HIP_TRY(hipEventCreateWithFlags(&h->par_ev, hipEventDisableTiming), "hipEventCreate");
        HIP_TRY(hipEventRecord(h->par_ev, h->stream), "hipEventRecord");
        for (int s = 1; s < S; s++) HIP_TRY(hipStreamWaitEvent(h->par[s - 1]->stream, h->par_ev, 0), "hipStreamWaitEvent");
    }
    for (int i = 0; i < n; i++) {
        const int s = i % S;
        sgm_handle* q = s ? h->par[s - 1] : h;
        const RectOut ro{rectLs ? rectLs[i] : nullptr, rectRs ? rectRs[i] : nullptr, rect_stride};
        const int rc = run_pipeline(q, l[s], g[s], dLs[i], dRs[i], stride, outs[i], out_stride, nullptr, nullptr, 0,
                                    h->rect_on ? &ro : nullptr);
        if (rc) return q == h ? rc : fail(h, rc, q->err);
    }
    for (int s = 1; s < S; s++) {
        sgm_handle* q = h->par[s - 1];
        HIP_TRY(hipEventRecord(q->done, q->stream), "hipEventRecord");
        q->done_stream = q->stream;
        HIP_TRY(hipStreamWaitEvent(h->stream, q->done, 0), "hipStreamWaitEvent");
    }
    // lanes whose workspaces take more than a quarter of the device are not kept past the call
    // (a later call on h, or another handle, may need that memory): the call waits for them
    // (SGM_OCV_KEEP_LANES=1 keeps them: the A/B of profiles/r04_ocv_lanes_ab.jsonl)
    const char* keep = std::getenv("SGM_OCV_KEEP_LANES");
    if ((size_t)(S - 1) * l0.total > total_b / 4 && !(keep && std::atoi(keep))) {
        for (int s = 1; s < S; s++) {
            sgm_handle* q = h->par[s - 1];
            HIP_TRY(hipStreamSynchronize(q->stream), "hipStreamSynchronize");
            HIP_TRY(hipFree(q->ws.base), "hipFree lane workspace");
            q->ws = Workspace{};
            q->items_key[0].clear();
            q->items_key[1].clear();
        }
    }
    return SGM_OK;
}

// Host images in, host disparity out (sgm_match: int16; sgm_match_f32: the CV_32FC1 the
// node's matcher contract wants, converted on the device). The reference's path is
// matcherOpenCVSGBM.cpp:17-44 (compute, then convertTo CV_32FC1), called per frame from
// generate_disparity.cpp:334-368. Every copy is one 2-D DMA between the caller's (pageable)
// rows and the workspace: measured on the MI355X box (tools/probe/host_copy.cpp,
// profiles/r04_host_copy.txt), a pageable 1920x1080 H2D takes 58 us against 42 us of CPU
// packing + 45 us of pinned DMA, and the 8.3 MB float D2H runs at the same 53 GB/s into
// pageable or pinned memory — staging buffers would only add copies.
// A caller may page-lock `out` with sgm_host_register (the adapter does, for its persistent
// disparity_lr): the D2H then needs no runtime staging, 1920x1080 f32 forwardMatch 1.95-1.97
// vs 1.97-1.99 ms pageable (profiles/r04_host_copy_ab.jsonl). Copying the rows back in 4 bands
// behind a banded WTA measured no gain (1.97-2.00 ms): a quarter-frame WTA launch (270 row
// workgroups) runs below the full launch's efficiency by about what the overlap saves.
int match_host(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, void* out,
               size_t out_stride, bool f32)
{
    Geom g;
    Layout l;
    int rc = prepare(h, h->cfg, W, H, true, g, l);
    if (rc || (rc = order_after_last(h, h->stream))) return rc;
    hipStream_t st = h->stream;
    const size_t es = f32 ? 4 : 2;
    char* ws = (char*)h->ws.base;
    const sgm_params& p = h->cfg.params;
    const bool census = p.mode == SGM_MODE_CENSUS8 && g.width1 > 0;
    // census mode: the left image's census runs while the right image is copied (second stream)
    if (census) {
        if (!h->cpy) HIP_TRY(hipStreamCreateWithFlags(&h->cpy, hipStreamNonBlocking), "hipStreamCreate");
        if (!h->cpy_ev) HIP_TRY(hipEventCreateWithFlags(&h->cpy_ev, hipEventDisableTiming), "hipEventCreate");
        HIP_TRY(hipEventRecord(h->cpy_ev, st), "hipEventRecord");        // the workspace is free
        HIP_TRY(hipStreamWaitEvent(h->cpy, h->cpy_ev, 0), "hipStreamWaitEvent");
    }
    const size_t row = (size_t)W * raw_bpp(h);    // bytes of an input row (8UC3 with colour frames)
    HIP_TRY(hipMemcpy2DAsync(ws + l.inL, row, L, stride, row, H, hipMemcpyHostToDevice, st), "H2D L");
    // f32 output that is the WTA's own (census, no median / speckles) into a registered, mapped
    // host buffer: the WTA writes the float rows there itself (no to-float pass, no copy back)
    float* outf = nullptr;
    if (f32 && census && !use_median(p) && !use_speckle(p) && !l.fill) {
        const size_t need = out_stride * 4 * (size_t)(H - 1) + (size_t)W * 4;
        for (const auto& r : h->regs)
            if (r.dev && (char*)out >= r.host && (char*)out + need <= r.host + r.bytes) {
                outf = (float*)(r.dev + ((char*)out - r.host));
                break;
            }
    }
    int16_t* d16 = (int16_t*)(ws + l.out);
    std::function<hipEvent_t()> copy_r;
    if (census) {
        copy_r = [&]() -> hipEvent_t {
            hipError_t e = hipMemcpy2DAsync(ws + l.inR, row, R, stride, row, H, hipMemcpyHostToDevice, h->cpy);
            if (e == hipSuccess) e = hipEventRecord(h->cpy_ev, h->cpy);
            if (e != hipSuccess) { hip_fail(h, e, "H2D R"); return nullptr; }
            return h->cpy_ev;
        };
    } else {
        HIP_TRY(hipMemcpy2DAsync(ws + l.inR, row, R, stride, row, H, hipMemcpyHostToDevice, st), "H2D R");
    }
    rc = run_pipeline(h, l, g, (const uint8_t*)(ws + l.inL), (const uint8_t*)(ws + l.inR), row, d16, W, copy_r, outf,
                      out_stride);
    if (rc) return rc;
    if (outf) {
        HIP_TRY(hipStreamSynchronize(st), "sync");
        return mark_done(h, st);
    }
    const void* dsrc = d16;
    if (f32) {
        HIP_TRY(sgm::launch_to_f32(d16, W, (float*)(ws + l.outf), W, W, H, st), "to_f32");
        dsrc = ws + l.outf;
    }
    HIP_TRY(hipMemcpy2DAsync(out, out_stride * es, dsrc, W * es, W * es, H, hipMemcpyDeviceToHost, st), "D2H");
    HIP_TRY(hipStreamSynchronize(st), "sync");
    return mark_done(h, st);
}

}  // namespace sgm
