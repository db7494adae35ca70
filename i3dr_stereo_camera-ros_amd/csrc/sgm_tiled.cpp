// sgm_tiled.cpp — one huge frame over several devices: the overlap tile mode (host and device
// buffers) and the exact tile mode. Sub-handles come from open_subs / run_on_subs (sgm_host.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "sgm_host.h"

using namespace sgm;

namespace {

// Enables dev -> peer access; true when it is in effect (enabled now or before, or dev == peer).
bool enable_peer(int dev, int peer)
{
    if (dev == peer) return true;
    int ok = 0;
    if (hipDeviceCanAccessPeer(&ok, dev, peer) != hipSuccess || !ok) {
        (void)hipGetLastError();
        return false;
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(dev) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    (void)hipGetLastError();
    if (prev >= 0) (void)hipSetDevice(prev);
    return e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
}

static bool enable_peer_pair(int a, int b)
{
    const bool ab = enable_peer(a, b), ba = enable_peer(b, a);
    return ab && ba;
}

}  // namespace

extern "C" {

int sgm_match_tiled(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, int16_t* disp,
                    size_t out_stride, int n_bands, int halo, const int* devices, int n_dev)
{
    if (!h) return SGM_ERR_ARG;
    if (!L || !R || !disp || W <= 0 || H <= 0 || stride < (size_t)W || out_stride < (size_t)W || n_bands < 1 ||
        halo < 0)
        return fail(h, SGM_ERR_ARG, "bad buffers, sizes, band count or halo");
    if (int rf = refuse_colour(h, "sgm_match_tiled")) return rf;
    if (int rf = refuse_pyramid(h, "sgm_match_tiled")) return rf;
    if (int rf = refuse_fill(h, "sgm_match_tiled")) return rf;
    n_bands = std::min(n_bands, H);
    std::vector<int> devs;
    int rc = open_subs(h, devices, n_dev, devs);
    if (rc) return rc;
    const int nd = (int)devs.size();
    return run_on_subs(h, devs, [&](int t, sgm_handle* sub) {
        std::vector<int16_t> band;
        for (int b = t; b < n_bands; b += nd) {
            const int c0 = (int)((long long)b * H / n_bands), c1 = (int)((long long)(b + 1) * H / n_bands);
            const int e0 = std::max(0, c0 - halo), e1 = std::min(H, c1 + halo);
            band.resize((size_t)W * (e1 - e0));
            int r = sgm_match(sub, L + (size_t)e0 * stride, R + (size_t)e0 * stride, W, e1 - e0, stride, band.data(),
                              (size_t)W);
            if (r) return r;
            for (int y = c0; y < c1; y++)
                std::memcpy(disp + (size_t)y * out_stride, band.data() + (size_t)(y - e0) * W, sizeof(int16_t) * W);
        }
        return (int)SGM_OK;
    });
}

}  // extern "C"

// Overlap tile mode on device buffers (the C5 frame already in HBM of h's device): band b's
// rows + halo go device -> devices[b % n] (xGMI peer copy), are matched there by
// sgm_match_device on that device's sub-handle, and the band's own rows come back into
// d_disp. Each device's bands run on its own host thread and stream.
static int tiled_copy(void* dst, int ddev, size_t dpitch, const void* src, int sdev, size_t spitch, size_t width,
                      size_t rows, bool peer_ok, hipStream_t st)
{
    if (ddev != sdev && dpitch == width && spitch == width) {      // contiguous rows: one peer copy
        const hipError_t e = hipMemcpyPeerAsync(dst, ddev, src, sdev, width * rows, st);
        return e == hipSuccess ? 0 : (int)e;
    }
    // strided rows within a device, or between devices whose peer access is confirmed both ways
    // (enable_peer_pair): one 2-D copy over the unified address space. Peer copies between
    // devices without peer mappings take one hipMemcpyPeerAsync per row (the runtime stages them).
    // (Between distinct physical devices this path has not run on hardware: the leased boxes have
    // one GPU)
    if (ddev == sdev || peer_ok) {
        const hipError_t e = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDefault, st);
        if (e == hipSuccess) return 0;
        if (ddev == sdev) return (int)e;
        (void)hipGetLastError();
    }
    for (size_t r = 0; r < rows; r++) {
        const hipError_t e2 = hipMemcpyPeerAsync((char*)dst + r * dpitch, ddev, (const char*)src + r * spitch, sdev,
                                                 width, st);
        if (e2 != hipSuccess) return (int)e2;
    }
    return 0;
}

extern "C" int sgm_match_tiled_device(sgm_handle* h, const uint8_t* dL, const uint8_t* dR, int W, int H,
                                      size_t stride, int16_t* dOut, size_t out_stride, int n_bands, int halo,
                                      const int* devices, int n_dev, void* stream)
{
    if (!h) return SGM_ERR_ARG;
    if (!dL || !dR || !dOut || W <= 0 || H <= 0 || stride < (size_t)W || out_stride < (size_t)W || n_bands < 1 ||
        halo < 0)
        return fail(h, SGM_ERR_ARG, "bad buffers, sizes, band count or halo");
    if (int rf = refuse_colour(h, "sgm_match_tiled_device")) return rf;
    if (int rf = refuse_pyramid(h, "sgm_match_tiled_device")) return rf;
    if (int rf = refuse_fill(h, "sgm_match_tiled_device")) return rf;
    if (h->rect_on) return fail(h, SGM_ERR_UNSUPPORTED, "the tile mode takes rectified images");
    n_bands = std::min(n_bands, H);
    std::vector<int> devs;
    int rc = open_subs(h, devices, n_dev, devs);
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if ((rc = ensure_stream(h))) return rc;
        if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize caller");
        if (h->done_stream) HIP_TRY(hipEventSynchronize(h->done), "hipEventSynchronize");
    }
    std::vector<char> peer_ok(devs.size(), 0);           // peer access confirmed both ways
    for (size_t i = 0; i < devs.size(); i++) peer_ok[i] = enable_peer_pair(devs[i], h->device) ? 1 : 0;
    const int nd = (int)devs.size(), hdev = h->device;
    return run_on_subs(h, devs, [&](int t, sgm_handle* sub) {
        for (int b = t; b < n_bands; b += nd) {
            const int c0 = (int)((long long)b * H / n_bands), c1 = (int)((long long)(b + 1) * H / n_bands);
            const int e0 = std::max(0, c0 - halo), e1 = std::min(H, c1 + halo), He = e1 - e0;
            const size_t img = align_up((size_t)W * He), need = 2 * img + (size_t)W * He * 2;
            int r = ensure_stream(sub);
            if (r) return r;
            if (sub->io_dev_size < need) {
                (void)hipStreamSynchronize(sub->stream);
                if (sub->io_dev) { (void)hipFree(sub->io_dev); sub->io_dev = nullptr; sub->io_dev_size = 0; }
                if (hipMalloc(&sub->io_dev, need) != hipSuccess)
                    return fail(sub, SGM_ERR_ALLOC, "hipMalloc band buffers");
                sub->io_dev_size = need;
            }
            uint8_t* bl = (uint8_t*)sub->io_dev;
            uint8_t* br = bl + img;
            int16_t* bo = (int16_t*)(br + img);
            const bool pk = peer_ok[t] != 0;
            if ((r = tiled_copy(bl, sub->device, W, dL + (size_t)e0 * stride, hdev, stride, W, He, pk, sub->stream)) ||
                (r = tiled_copy(br, sub->device, W, dR + (size_t)e0 * stride, hdev, stride, W, He, pk, sub->stream)))
                return fail(sub, SGM_ERR_DEVICE, std::string("band input copy: ") + hipGetErrorString((hipError_t)r));
            if ((r = sgm_match_device(sub, bl, br, W, He, W, bo, W, nullptr))) return r;
            if ((r = tiled_copy(dOut + (size_t)c0 * out_stride, hdev, out_stride * 2, bo + (size_t)(c0 - e0) * W,
                                sub->device, (size_t)W * 2, (size_t)W * 2, c1 - c0, pk, sub->stream)))
                return fail(sub, SGM_ERR_DEVICE, std::string("band output copy: ") + hipGetErrorString((hipError_t)r));
            if (hipStreamSynchronize(sub->stream) != hipSuccess) return fail(sub, SGM_ERR_DEVICE, "band stream");
        }
        return (int)SGM_OK;
    });
}

// ------------------------------------------------------------------ exact tile mode ----
// SURVEY §8(e) "single huge frame", exact mode. Band b (rows [c0, c1)) runs on its own
// handle: census of its rows (+3 * step image rows of halo, the reach of the census window, so the
// codes equal the full frame's),
// horizontal scans (band-local), then its downward sweeps continue the lines of band b-1
// from band b-1's last volume row and its upward sweeps those of band b+1 from its first
// row. The boundary rows (3 directions x width1 x D u8 per seam and sweep) move between
// devices with hipMemcpyPeerAsync (xGMI); the two chains run top-down and bottom-up
// concurrently (separate streams), so the frame's critical path is H row steps per sweep
// direction, whatever the band count. The WTA of a band needs only its own rows.
namespace {

constexpr unsigned kDirsHoriz = 0xC0u, kDirsDown = 0x0Du, kDirsUp = 0x32u;

struct BandLayout {
    size_t inL = 0, inR = 0, cL = 0, cR = 0, vols = 0, vol_bytes = 0, items[3] = {}, bnd[2] = {}, bnd_slot = 0, raw = 0;
    int n_items[3] = {};
    size_t total = 0;
};

BandLayout make_band_layout(const Geom& g, int He)
{
    BandLayout l;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + std::max<size_t>(bytes, 1)); return o; };
    const size_t w1 = (size_t)std::max(g.width1, 0);    // width1 <= 0: no paths, all invalid
    const size_t cells = w1 * g.H * g.D;
    l.inL = take((size_t)g.W * He);
    l.inR = take((size_t)g.W * He);
    auto take_codes = [&](size_t n) { return take((n + 2 * sgm::kCodeMargin) * 8) + 8 * sgm::kCodeMargin; };
    l.cL = take_codes((size_t)g.W * He);
    l.cR = take_codes((size_t)g.W * He);
    l.vol_bytes = align_up(cells + kTrashBytes);
    l.vols = take(l.vol_bytes * 8);
    const unsigned masks[3] = {kDirsHoriz, kDirsDown, kDirsUp};
    for (int i = 0; i < 3; i++) {
        l.n_items[i] = w1 ? sgm::census_path_items(g, masks[i], 1, 1, nullptr, 0) : 0;
        l.items[i] = take((size_t)l.n_items[i] * 4);
    }
    // + 512 B: lanes past D (D < 16 * DPL) read beyond the last pixel before being masked
    l.bnd_slot = align_up(w1 * g.D + 512);
    l.bnd[0] = take(3 * l.bnd_slot);
    l.bnd[1] = take(3 * l.bnd_slot);
    l.raw = take((size_t)g.W * g.H * 2);
    l.total = off;
    return l;
}

hipError_t copy_between(void* dst, int ddev, const void* src, int sdev, size_t n, hipStream_t st)
{
    return ddev == sdev ? hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, st)
                        : hipMemcpyPeerAsync(dst, ddev, src, sdev, n, st);
}

// Stream 2 + events of a band handle; the three path work lists uploaded for g.
int band_prepare(sgm_handle* b, const Geom& g, const BandLayout& l)
{
    sgm_handle* h = b;                            // for HIP_TRY
    int rc = ensure_stream(b);
    if (rc) return rc;
    if (!b->stream2) HIP_TRY(hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking), "hipStreamCreate");
    for (hipEvent_t& e : b->bev)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    if ((rc = ensure_ws(b, l.total))) return rc;
    char key[160];
    snprintf(key, sizeof key, "band %d %d %d %d %d %zu %p", g.W, g.H, g.D, g.minD, b->n_cu, l.total, b->ws.base);
    if (b->items_key[0] == key) return SGM_OK;
    const unsigned masks[3] = {kDirsHoriz, kDirsDown, kDirsUp};
    std::vector<uint32_t> v;
    for (int i = 0; i < 3 && g.width1 > 0; i++) {
        const int n = sgm::census_path_items(g, masks[i], b->n_cu, 1, nullptr, 0);
        if (n != l.n_items[i]) return fail(b, SGM_ERR_ARG, "band work list size mismatch");
        v.resize(n);
        sgm::census_path_items(g, masks[i], b->n_cu, 1, v.data(), n);
        HIP_TRY(hipMemcpy((char*)b->ws.base + l.items[i], v.data(), (size_t)n * 4, hipMemcpyHostToDevice), "H2D items");
    }
    b->items_key[0] = key;
    b->items_key[1].clear();
    return SGM_OK;
}

int run_tiled_exact(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride, int16_t* disp,
                    size_t out_stride, int n_bands, const std::vector<int>& devs)
{
    const sgm_params& p = h->cfg.params;
    Geom gf;
    int rc = make_geom(p, W, H, gf, h->err);
    if (rc || (rc = fill_params_status(h->cfg.fill, h->err))) return rc;
    if (p.mode != SGM_MODE_CENSUS8) return fail(h, SGM_ERR_UNSUPPORTED, "the exact tile mode runs in the census mode");
    // the seam exchange carries three directions per sweep family (bnd_slot_of): 8 paths only
    if (h->cfg.census_paths != 8)
        return fail(h, SGM_ERR_UNSUPPORTED, "the exact tile mode runs with 8 census paths (sgm_set_census_paths)");
    if ((rc = census_window_status(h->cfg.cwin, h->err))) return rc;
    const sgm_census_window cw = h->cfg.cwin;
    const int ih = 3 * cw.step;       // image rows a band's census needs beyond its own: the window's reach
    const int nb = n_bands;
    while ((int)h->bands.size() < nb) h->bands.push_back(nullptr);
    std::vector<int> c(nb + 1);
    for (int b = 0; b <= nb; b++) c[b] = (int)((long long)b * H / nb);
    std::vector<Geom> g(nb);
    std::vector<BandLayout> bl(nb);
    for (int b = 0; b < nb; b++) {
        const int dev = devs[b % devs.size()];
        sgm_handle*& bh = h->bands[b];
        if (bh && bh->device != dev) { sgm_destroy(bh); bh = nullptr; }
        if (!bh && (rc = sgm_create(&bh, dev))) return fail(h, rc, "cannot open device " + std::to_string(dev));
        bh->cfg = h->cfg;
        if ((rc = make_geom(p, W, c[b + 1] - c[b], g[b], h->err))) return rc;
        const int e0 = std::max(0, c[b] - ih), e1 = std::min(H, c[b + 1] + ih);
        bl[b] = make_band_layout(g[b], e1 - e0);
        if ((rc = band_prepare(bh, g[b], bl[b]))) return fail(h, rc, "band " + std::to_string(b) + ": " + bh->err);
        if ((rc = ensure_pin(bh, 2 * (size_t)W * (e1 - e0)))) return fail(h, rc, bh->err);
    }
    for (int b = 0; b < nb; b++) {
        if (b > 0) enable_peer(h->bands[b]->device, h->bands[b - 1]->device);
        if (b + 1 < nb) enable_peer(h->bands[b]->device, h->bands[b + 1]->device);
        enable_peer(h->bands[b]->device, h->device);
    }
    if ((rc = ensure_stream(h))) return rc;
    const Layout pl = make_post_layout(p, gf, fill_on(h->cfg));
    if ((rc = ensure_ws(h, pl.total))) return rc;
    if ((rc = ensure_pin(h, (size_t)W * H * 2))) return rc;
    const bool med = use_median(p);
    char* pws = (char*)h->ws.base;
    int16_t* frame_raw = med ? (int16_t*)(pws + pl.tmp) : post_image(pl, gf, pws, 0, (int16_t*)(pws + pl.out));
    const size_t cells_row = (size_t)std::max(gf.width1, 0) * gf.D;

    auto ws = [&](int b, size_t off) { return (char*)h->bands[b]->ws.base + off; };
    auto fail_band = [&](int b, hipError_t e, const char* where) {
        for (sgm_handle* s : h->bands)
            if (s && s->stream) { (void)hipSetDevice(s->device); (void)hipStreamSynchronize(s->stream);
                                   (void)hipStreamSynchronize(s->stream2); }
        return fail(h, SGM_ERR_DEVICE, "band " + std::to_string(b) + " " + where + ": " + hipGetErrorString(e));
    };
#define BAND_TRY(b, expr, where)                          \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return fail_band(b, e_, where); \
    } while (0)
    enum { EV_CENSUS = 0, EV_DOWN = 1, EV_UP = 2, EV_GATHER = 3 };
    // SGM_TILE_TIMES=<file>: measurement mode — every band step runs alone (synchronised
    // before and after) and its duration on the band's device is appended to the file as
    // "band kind ms" lines (the per-band inputs of the multi-device critical-path model in
    // DESIGN.md §7). Never set in production runs.
    struct TileTimes {           // closed / destroyed on every return path
        FILE* f = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~TileTimes() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (f) std::fclose(f);
        }
    } tt;
    if (const char* tf = std::getenv("SGM_TILE_TIMES")) tt.f = std::fopen(tf, "a");
    FILE*& tt_file = tt.f;
    hipEvent_t& tt0 = tt.e0;
    hipEvent_t& tt1 = tt.e1;
    auto tt_begin = [&](int b, hipStream_t s) {
        if (!tt_file) return;
        (void)hipSetDevice(h->bands[b]->device);
        (void)hipDeviceSynchronize();
        if (!tt0) { (void)hipEventCreate(&tt0); (void)hipEventCreate(&tt1); }
        (void)hipEventRecord(tt0, s);
    };
    auto tt_end = [&](int b, const char* kind, hipStream_t s) {
        if (!tt_file) return;
        float ms = 0.f;
        (void)hipEventRecord(tt1, s);
        (void)hipEventSynchronize(tt1);
        (void)hipEventElapsedTime(&ms, tt0, tt1);
        std::fprintf(tt_file, "%d %s %.4f\n", b, kind, ms);
    };
    // 1. inputs, census, horizontal scans (band-local)
    for (int b = 0; b < nb; b++) {
        sgm_handle* bh = h->bands[b];
        BAND_TRY(b, hipSetDevice(bh->device), "hipSetDevice");
        const int e0 = std::max(0, c[b] - ih), e1 = std::min(H, c[b + 1] + ih), He = e1 - e0;
        const size_t n = (size_t)W * He;
        for (int y = 0; y < He; y++) {
            std::memcpy(bh->pin + (size_t)y * W, L + (size_t)(e0 + y) * stride, W);
            std::memcpy(bh->pin + n + (size_t)y * W, R + (size_t)(e0 + y) * stride, W);
        }
        tt_begin(b, bh->stream);
        BAND_TRY(b, hipMemcpyAsync(ws(b, bl[b].inL), bh->pin, n, hipMemcpyHostToDevice, bh->stream), "H2D");
        BAND_TRY(b, hipMemcpyAsync(ws(b, bl[b].inR), bh->pin + n, n, hipMemcpyHostToDevice, bh->stream), "H2D");
        tt_end(b, "h2d", bh->stream);
        tt_begin(b, bh->stream);
        BAND_TRY(b, sgm::launch_census_planes(cw, (const uint8_t*)ws(b, bl[b].inL), (const uint8_t*)ws(b, bl[b].inR), W, W,
                                              He, (uint64_t*)ws(b, bl[b].cL), (uint64_t*)ws(b, bl[b].cR), bh->stream),
                 "census");
        tt_end(b, "census", bh->stream);
        BAND_TRY(b, hipEventRecord(bh->bev[EV_CENSUS], bh->stream), "event");
    }
    auto frames = [&](int b) {
        sgm::PathFrames pf{};
        const size_t skip = (size_t)(c[b] - std::max(0, c[b] - ih)) * W;  // codes of the band's first row
        pf.cL[0] = (const uint64_t*)ws(b, bl[b].cL) + skip;
        pf.cR[0] = (const uint64_t*)ws(b, bl[b].cR) + skip;
        pf.vols[0] = (uint8_t*)ws(b, bl[b].vols);
        pf.n = 1;
        return pf;
    };
    if (gf.width1 > 0) {
        for (int b = 0; b < nb; b++) {
            sgm_handle* bh = h->bands[b];
            BAND_TRY(b, hipSetDevice(bh->device), "hipSetDevice");
            tt_begin(b, bh->stream);
            BAND_TRY(b, sgm::launch_census_paths(frames(b), bl[b].vol_bytes, g[b], (const uint32_t*)ws(b, bl[b].items[0]),
                                                 bl[b].n_items[0], bh->stream), "horizontal paths");
            tt_end(b, "horiz", bh->stream);
        }
        // 2. downward chain, top to bottom: band b continues band b-1's last row
        static const int down_dirs[3] = {0, 2, 3}, up_dirs[3] = {1, 4, 5};
        for (int b = 0; b < nb; b++) {
            sgm_handle* bh = h->bands[b];
            BAND_TRY(b, hipSetDevice(bh->device), "hipSetDevice");
            if (b > 0) BAND_TRY(b, hipStreamWaitEvent(bh->stream, h->bands[b - 1]->bev[EV_DOWN], 0), "wait");
            tt_begin(b, bh->stream);
            BAND_TRY(b, sgm::launch_census_paths(frames(b), bl[b].vol_bytes, g[b], (const uint32_t*)ws(b, bl[b].items[1]),
                                                 bl[b].n_items[1], bh->stream,
                                                 b > 0 ? (const uint8_t*)ws(b, bl[b].bnd[0]) : nullptr, nullptr,
                                                 bl[b].bnd_slot), "down paths");
            tt_end(b, "down", bh->stream);
            if (b + 1 < nb) {
                tt_begin(b, bh->stream);
                const size_t last = (size_t)(g[b].H - 1) * cells_row;
                for (int k = 0; k < 3; k++)
                    BAND_TRY(b, copy_between(ws(b + 1, bl[b + 1].bnd[0] + k * bl[b + 1].bnd_slot), h->bands[b + 1]->device,
                                             ws(b, bl[b].vols + down_dirs[k] * bl[b].vol_bytes + last), bh->device,
                                             cells_row, bh->stream), "boundary copy");
                tt_end(b, "copy_down", bh->stream);
            }
            BAND_TRY(b, hipEventRecord(bh->bev[EV_DOWN], bh->stream), "event");
        }
        // 3. upward chain, bottom to top, on the second streams: band b continues band b+1's first row
        for (int b = nb - 1; b >= 0; b--) {
            sgm_handle* bh = h->bands[b];
            BAND_TRY(b, hipSetDevice(bh->device), "hipSetDevice");
            BAND_TRY(b, hipStreamWaitEvent(bh->stream2, bh->bev[EV_CENSUS], 0), "wait");
            if (b + 1 < nb) BAND_TRY(b, hipStreamWaitEvent(bh->stream2, h->bands[b + 1]->bev[EV_UP], 0), "wait");
            tt_begin(b, bh->stream2);
            BAND_TRY(b, sgm::launch_census_paths(frames(b), bl[b].vol_bytes, g[b], (const uint32_t*)ws(b, bl[b].items[2]),
                                                 bl[b].n_items[2], bh->stream2, nullptr,
                                                 b + 1 < nb ? (const uint8_t*)ws(b, bl[b].bnd[1]) : nullptr,
                                                 bl[b].bnd_slot), "up paths");
            tt_end(b, "up", bh->stream2);
            if (b > 0) {
                tt_begin(b, bh->stream2);
                for (int k = 0; k < 3; k++)
                    BAND_TRY(b, copy_between(ws(b - 1, bl[b - 1].bnd[1] + k * bl[b - 1].bnd_slot), h->bands[b - 1]->device,
                                             ws(b, bl[b].vols + up_dirs[k] * bl[b].vol_bytes), bh->device, cells_row,
                                             bh->stream2), "boundary copy");
                tt_end(b, "copy_up", bh->stream2);
            }
            BAND_TRY(b, hipEventRecord(bh->bev[EV_UP], bh->stream2), "event");
        }
    }
    // 4. WTA of each band (after its three path launches), gathered into the primary's frame
    for (int b = 0; b < nb; b++) {
        sgm_handle* bh = h->bands[b];
        BAND_TRY(b, hipSetDevice(bh->device), "hipSetDevice");
        int16_t* raw = (int16_t*)ws(b, bl[b].raw);
        if (gf.width1 > 0) {
            BAND_TRY(b, hipStreamWaitEvent(bh->stream, bh->bev[EV_UP], 0), "wait");
            sgm::WtaFrames wf{};
            wf.vols[0] = (const uint8_t*)ws(b, bl[b].vols); wf.out[0] = raw; wf.n = 1;
            tt_begin(b, bh->stream);
            BAND_TRY(b, sgm::launch_census_wta(wf, bl[b].vol_bytes, g[b], W, bh->stream), "wta");
            tt_end(b, "wta", bh->stream);
        } else {
            BAND_TRY(b, sgm::launch_fill16(raw, W, W, g[b].H, gf.invalid, bh->stream), "fill");
        }
        tt_begin(b, bh->stream);
        BAND_TRY(b, copy_between(frame_raw + (size_t)c[b] * W, h->device, raw, bh->device, (size_t)W * g[b].H * 2,
                                 bh->stream), "gather");
        tt_end(b, "gather", bh->stream);
        BAND_TRY(b, hipEventRecord(bh->bev[EV_GATHER], bh->stream), "event");
    }
#undef BAND_TRY
    // 5. post filters on the assembled frame (median / speckles need no band seams), D2H
    HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
    for (int b = 0; b < nb; b++) HIP_TRY(hipStreamWaitEvent(h->stream, h->bands[b]->bev[EV_GATHER], 0), "wait");
    StageRec rec{h};
    int16_t* out = (int16_t*)(pws + pl.out);
    if (tt_file) {
        (void)hipDeviceSynchronize();
        (void)hipEventRecord(tt0, h->stream);
    }
    if ((rc = run_post(h, pl, gf, out, W, rec))) return rc;
    rec.end();
    if (tt_file) {
        float ms = 0.f;
        (void)hipEventRecord(tt1, h->stream);
        (void)hipEventSynchronize(tt1);
        (void)hipEventElapsedTime(&ms, tt0, tt1);
        std::fprintf(tt_file, "-1 post %.4f\n", ms);
    }
    HIP_TRY(hipMemcpyAsync(h->pin, out, (size_t)W * H * 2, hipMemcpyDeviceToHost, h->stream), "D2H");
    HIP_TRY(hipStreamSynchronize(h->stream), "sync");
    const int16_t* src = (const int16_t*)h->pin;
    for (int y = 0; y < H; y++) std::memcpy(disp + (size_t)y * out_stride, src + (size_t)y * W, 2 * (size_t)W);
    return SGM_OK;
}

}  // namespace

extern "C" {

int sgm_match_tiled_exact(sgm_handle* h, const uint8_t* L, const uint8_t* R, int W, int H, size_t stride,
                          int16_t* disp, size_t out_stride, int n_bands, const int* devices, int n_dev)
{
    if (!h) return SGM_ERR_ARG;
    if (!L || !R || !disp || W <= 0 || H <= 0 || stride < (size_t)W || out_stride < (size_t)W || n_bands < 1)
        return fail(h, SGM_ERR_ARG, "bad buffers, sizes or band count");
    if (int rf = refuse_colour(h, "sgm_match_tiled_exact")) return rf;
    if (int rf = refuse_pyramid(h, "sgm_match_tiled_exact")) return rf;
    std::vector<int> devs;
    if (!devices || n_dev <= 0) {
        for (int i = 0; i < sgm_device_count(); i++) devs.push_back(i);
    } else {
        devs.assign(devices, devices + n_dev);
    }
    if (devs.empty()) return fail(h, SGM_ERR_DEVICE, "no HIP device");
    std::lock_guard<std::mutex> lk(h->mu);
    return run_tiled_exact(h, L, R, W, H, stride, disp, out_stride, std::min(n_bands, H), devs);
}

}  // extern "C"
