// sgm_plan.cpp — everything that decides without touching the device: parameter validation and
// geometry, the workspace carve-up, and the environment / build knobs that pick a scheme.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "sgm_host.h"

// measurement-only build knob (tools/build_variant.sh ... sgm_plan.cpp)
#ifndef SGM_VOL_PAD_BYTES
#define SGM_VOL_PAD_BYTES 0    // extra bytes per census volume slot
#endif

namespace sgm {

// effective parameters — identical rules to the oracle (oracle/sgm_oracle.c effective())
// cv::filterSpeckles' maxDiff per unit of sgm_params.speckle_range: StereoSGBM passes
// 16 * speckleRange (its disparities are x16), StereoBM passes speckleRange unscaled.
constexpr int kSpeckleScaleSgbm = 16;
constexpr int kSpeckleScaleBm = 1;
int speckle_scale(int mode) { return mode == SGM_MODE_OCV_BM ? kSpeckleScaleBm : kSpeckleScaleSgbm; }

// SGM_MODE_OCV_BM: nothing is repaired (the validation step of the BM specification).
static int make_geom_bm(const sgm_params& p, const sgm_bm_params& bm, int W, int H, Geom& g, std::string& err)
{
    if (bm.prefilter_size < 5 || bm.prefilter_size > 255 || bm.prefilter_size % 2 == 0) {
        err = "StereoBM: preFilterSize must be odd and within 5..255";
        return SGM_ERR_PARAM;
    }
    if (p.prefilter_cap < 1 || p.prefilter_cap > 63) { err = "StereoBM: preFilterCap must be within 1..63"; return SGM_ERR_PARAM; }
    const int w = p.block_size;
    if (w < 5 || w > 255 || w % 2 == 0 || w >= std::min(W, H)) {
        err = "StereoBM: SADWindowSize must be odd, within 5..255 and smaller than the image";
        return SGM_ERR_PARAM;
    }
    if (bm.texture_threshold < 0) { err = "StereoBM: texture threshold must be non-negative"; return SGM_ERR_PARAM; }
    if (p.uniqueness_ratio < 0) { err = "StereoBM: uniqueness ratio must be non-negative"; return SGM_ERR_PARAM; }
    if (p.disp12_max_diff >= 0) {
        err = "StereoBM: disp12MaxDiff >= 0 (validateDisparity) is not implemented; -1 switches it off";
        return SGM_ERR_UNSUPPORTED;
    }
    g = Geom{};
    g.W = W; g.H = H;
    g.minD = p.min_disparity; g.D = p.num_disparities;
    g.SW2 = g.SH2 = w / 2;
    g.ftzero = p.prefilter_cap;
    g.uniq = p.uniqueness_ratio;
    g.bm_tex = bm.texture_threshold;
    g.subpix = 1;
    g.invalid = (g.minD - 1) * 16;
    // column range [X0, X1): s = D - 1 + minD, X0 = max(s, 0), X1 = min(W, W + minD)
    g.minX1 = std::max(g.D - 1 + g.minD, 0);
    g.maxX1 = std::min(W, W + g.minD);
    g.width1 = (g.minX1 >= W || g.maxX1 <= 0 || g.maxX1 <= g.minX1) ? 0 : g.maxX1 - g.minX1;
    return SGM_OK;
}

int make_geom(const sgm_params& p, int W, int H, Geom& g, std::string& err, const sgm_bm_params* bm)
{
    if (W <= 0 || H <= 0) { err = "image size must be positive"; return SGM_ERR_ARG; }
    if (W > 32767 || H > 32767) { err = "image larger than 32767 pixels"; return SGM_ERR_UNSUPPORTED; }
    if (p.mode < SGM_MODE_OCV_SGBM5 || p.mode > SGM_MODE_OCV_BM) { err = "unknown mode"; return SGM_ERR_PARAM; }
    if (p.num_disparities <= 0 || p.num_disparities % 16 != 0) {
        err = "numDisparities must be a positive multiple of 16 (OpenCV: CV_Assert(D % 16 == 0))";
        return SGM_ERR_PARAM;
    }
    // OCV modes: up to 2048 (the node's cfg range, i3DR_Disparity.cfg:27); census mode: 512
    // (its u8 path engine keeps at most 32 disparities per lane of a 16-lane line)
    const int max_d = p.mode == SGM_MODE_CENSUS8 ? 512 : 2048;
    if (p.num_disparities > max_d) {
        err = p.mode == SGM_MODE_CENSUS8 ? "numDisparities > 512 is not supported in the census mode"
                                         : "numDisparities > 2048 is not supported";
        return SGM_ERR_UNSUPPORTED;
    }
    if (p.mode == SGM_MODE_OCV_BM) return make_geom_bm(p, bm ? *bm : kBmDefaults, W, H, g, err);
    g = Geom{};
    g.W = W; g.H = H;
    g.minD = p.min_disparity; g.D = p.num_disparities;
    const int maxD = g.minD + g.D;
    if (p.mode == SGM_MODE_CENSUS8) {
        g.P1 = p.p1 > 0 ? p.p1 : 10;
        g.P2 = std::max(p.p2 > 0 ? p.p2 : 120, g.P1 + 1);
        if (g.P2 > 193) g.P2 = 193;                   // u8 path costs: 62 + P2 <= 255
        if (g.P1 >= g.P2) g.P1 = g.P2 - 1;
        g.subpix = p.subpixel != 0; g.lr = p.lr_check != 0;
        g.SW2 = 4; g.SH2 = 3; g.ftzero = 0;
    } else {
        const int sw = p.block_size > 0 ? p.block_size : 5;
        g.SW2 = sw / 2; g.SH2 = sw / 2;
        g.ftzero = std::max(p.prefilter_cap, 15) | 1;
        g.P1 = p.p1 > 0 ? p.p1 : 2;
        g.P2 = std::max(p.p2 > 0 ? p.p2 : 5, g.P1 + 1);
        g.subpix = 1; g.lr = 1;
        // A pixel cost is <= 2*ftzero + 63 (BT of the prefiltered image + raw BT >> 2), so
        // C = box sum + P2 stays in int16 below this bound, and then every path cost lies in
        // [C - P2, C]: int16 volumes are exact. Above it C may wrap (OpenCV's CostType) and a
        // path cost can leave int16, while OpenCV adds the int value into S: int32 volumes.
        // When the bound allows it, the cost kernel flags the C' values that do leave int16 and
        // only frames with such a value take the int32 volumes (Geom::wide == 2): real images
        // stay far below the bound (the reference launch config, block 21: bound 41 413).
        // SGM_OCV_WIDE=1 forces int32 volumes; SGM_OCV_GATE=0 takes them whenever the bound allows.
        // The SIMD branches (ocv_compat SGM_OCV_SIMD_SAT) saturate instead, and agree with the
        // plain kernels until a C' exceeds 32767 - P2 (then (short)(minLr + P2) can wrap): their
        // flagged kernels are the sequential saturating cost and saturating int16 paths / sums.
        g.compat = p.ocv_compat & (SGM_OCV_COL0_LEGACY | SGM_OCV_SIMD_SAT | SGM_OCV_LANE_TIE);
        const bool sat = (g.compat & SGM_OCV_SIMD_SAT) != 0;
        g.ovf_thr = sat ? 32767 - g.P2 : 32767;
        const long long cmax = (long long)(2 * g.SW2 + 1) * (2 * g.SH2 + 1) * (2 * g.ftzero + 63) + g.P2 +
                               (sat ? g.P2 : 0);
        const char* wide_env = std::getenv("SGM_OCV_WIDE");
        const char* gate_env = std::getenv("SGM_OCV_GATE");
        if (wide_env && std::atoi(wide_env) != 0) g.wide = 1;
        else if (cmax > 32767) g.wide = (gate_env && std::atoi(gate_env) == 0) ? 1 : 2;
        else g.wide = 0;
    }
    g.uniq = p.uniqueness_ratio >= 0 ? p.uniqueness_ratio : 10;
    g.disp12 = p.disp12_max_diff > 0 ? p.disp12_max_diff : 1;
    g.minX1 = std::max(maxD, 0);
    g.maxX1 = W + std::min(g.minD, 0);
    g.width1 = g.maxX1 - g.minX1;
    g.invalid = (g.minD - 1) * 16;
    return SGM_OK;
}

bool use_median(const sgm_params& p)
{
    if (p.mode == SGM_MODE_OCV_BM) return false;   // cv::StereoBM has no median
    return p.mode != SGM_MODE_CENSUS8 || p.median != 0;
}

// the speckle filter of a frame: BM also needs speckle_range >= 0 (OpenCV's condition)
bool use_speckle(const sgm_params& p)
{
    return p.speckle_window_size > 0 && (p.mode != SGM_MODE_OCV_BM || p.speckle_range >= 0);
}

// Pipelined census batches with D <= 256 fuse the upward vertical sweep with the WTA
// (census_sgm.hip UpWta) unless SGM_UPWTA=0 (the earlier scheme: 8 volumes written, WTA rows
// interleaved).
static bool use_up_wta()
{
    const char* e = std::getenv("SGM_UPWTA");
    return !e || std::atoi(e) != 0;
}

// rect: the frames are raw (sgm_set_rectification) and a pre-pass rectifies them into the grey
// planes: the OCV and BM modes, and the census mode with a non-default window.
Layout make_layout(const MatchConfig& c, const Geom& g, bool host_io, int group, int n_cu, bool rect)
{
    const sgm_params& p = c.params;
    const int ch = c.raw_ch;
    Layout l;
    l.np = c.census_paths == 4 ? 4 : 8;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + std::max<size_t>(bytes, 1)); return o; };
    auto take_codes = [&](size_t n) { return take((n + 2 * sgm::kCodeMargin) * 8) + 8 * sgm::kCodeMargin; };
    const size_t WH = (size_t)g.W * g.H;
    const size_t cells = (size_t)std::max(g.width1, 0) * g.H * g.D;
    if (p.mode == SGM_MODE_OCV_BM) {
        l.bmL = take(WH);
        l.bmR = take(WH);
        l.bm = sgm::bm_plan(g, n_cu);
        l.bmV = take(l.bm.vbytes);
    } else if (p.mode == SGM_MODE_CENSUS8) {
        l.vol_bytes = align_up(cells + kTrashBytes);   // + trash slot for masked stores
#if SGM_VOL_PAD_BYTES > 0
        // extra bytes per volume slot (a measurement build: tools/build_variant.sh, -DSGM_VOL_PAD_BYTES=N)
        l.vol_bytes = align_up(l.vol_bytes + (size_t)std::min<long long>(SGM_VOL_PAD_BYTES, 1LL << 30));
#endif
        l.group = std::max(group, 1);
        // D > 256 (32 disparities per lane, 2 waves/SIMD) keeps the earlier scheme: its up+WTA
        // blocks are long latency-bound chains (C5 batch: 32.3 vs 23.3 ms per frame)
        l.up_wta = group > 0 && use_up_wta() && g.D <= 256;
        const int sets = group > 0 ? 2 * l.group : 1;
        for (int i = 0; i < sets; i++) l.vols[i] = take(l.vol_bytes * l.np);
        const unsigned mask = sgm::census_dir_mask(l.np);
        for (int i = 0; i < (l.up_wta ? 3 * l.group : sets); i++) {
            l.cL[i] = take_codes(WH);
            l.cR[i] = take_codes(WH);
        }
        if (l.up_wta)
            for (int i = 0; i < l.group; i++) l.res[i] = take((WH + 64) * 8);
        if (g.width1 > 0) {
            l.n_items[0] = sgm::census_path_items(g, mask, 1, 1, nullptr, 0);
            l.items[0] = take((size_t)l.n_items[0] * 4);
            if (group > 0) {
                l.n_items[1] = sgm::census_path_items(g, mask, 1, l.group, nullptr, 0, l.up_wta ? l.group : 0);
                l.items[1] = take((size_t)l.n_items[1] * 4);
            }
        }
    } else {
        // the packed BT planes (16 B/px) only for frames whose cost stage takes the fused kernel
        l.planes = take(sgm::ocv_cost_takes_fused(g) ? sgm::ocv_planes_total(g.W, g.H) : sgm::ocv_planes_bytes(g.W, g.H));
        l.bufA = take(cells * 2);
        l.bufB = take(cells * 2);
        const size_t es = g.wide && !(g.compat & SGM_OCV_SIMD_SAT) ? 4 : 2;   // int32 / int16 path volumes
        // + slack: the path kernel's trash slots (64 lanes x 32 values) and the WTA's last pixel
        // group of the last row, which reads 3 pixels past the volume
        l.ovols = take(es * (sgm::ocv_vol_elems(cells, es) * (p.mode == SGM_MODE_OCV_HH8 ? 8 : 5) + 64 * 32 +
                             (size_t)8 * g.D));
        l.ovf = take(sizeof(int));
        l.ores = take(WH * 8);
    }
    l.tmp = take(WH * 2 * (size_t)std::max(group, 1));   // raw disparity before the median (per frame of a group)
    if (p.speckle_window_size > 0) { l.lab = take(WH * 4); l.cnt = take(WH * 4); }
    if ((ch == 3 || rect) && p.mode != SGM_MODE_CENSUS8) { l.grayL = take(WH); l.grayR = take(WH); }
    // census with a non-default window: k_census_win reads one grey plane pair per frame of a group
    if (census_win_prepass(c, rect)) { l.grayL = take(WH * l.group); l.grayR = take(WH * l.group); }
    if (host_io) { l.inL = take(WH * ch); l.inR = take(WH * ch); l.out = take(WH * 2); l.outf = take(WH * 4); }
    if (fill_on(c)) {
        l.fill = true;
        l.fsrc = take(WH * 2 * (size_t)std::max(group, 1));
        l.fpl = take(sgm::fill_plane_bytes(g.W, g.H));
    }
    l.total = off;
    return l;
}

// Post-filter workspace of the assembled frame on the primary handle.
Layout make_post_layout(const sgm_params& p, const Geom& g, bool fill)
{
    Layout l;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + std::max<size_t>(bytes, 1)); return o; };
    const size_t WH = (size_t)g.W * g.H;
    l.tmp = take(WH * 2);
    l.out = take(WH * 2);
    if (p.speckle_window_size > 0) { l.lab = take(WH * 4); l.cnt = take(WH * 4); }
    if (fill) {
        l.fill = true;
        l.fsrc = take(WH * 2);
        l.fpl = take(sgm::fill_plane_bytes(g.W, g.H));
    }
    l.total = off;
    return l;
}

// sgm_set_fill_params stores anything; with a mode other than OFF a match (and sgm_fill_holes)
// needs a known mode, a gap of 1..255 and 1..8 neighbours
int fill_params_status(const sgm_fill_params& f, std::string& err)
{
    if (f.mode == SGM_FILL_OFF) return SGM_OK;
    if (f.mode != SGM_FILL_BACKGROUND && f.mode != SGM_FILL_MEDIAN) {
        err = "hole filling: unknown mode " + std::to_string(f.mode);
        return SGM_ERR_PARAM;
    }
    if (f.max_gap < 1 || f.max_gap > 255) {
        err = "hole filling: max_gap must be within 1..255, got " + std::to_string(f.max_gap);
        return SGM_ERR_PARAM;
    }
    if (f.min_neighbours < 1 || f.min_neighbours > 8) {
        err = "hole filling: min_neighbours must be within 1..8, got " + std::to_string(f.min_neighbours);
        return SGM_ERR_PARAM;
    }
    return SGM_OK;
}

// sgm_set_census_window stores anything; a census match needs one of the 24 windows
int census_window_status(const sgm_census_window& w, std::string& err)
{
    if (census_window_ok(w)) return SGM_OK;
    err = "census window: taps_x must be 3, 5, 7 or 9, taps_y 3, 5 or 7 and step 1 or 2 (sgm_set_census_window), got " +
          std::to_string(w.taps_x) + "x" + std::to_string(w.taps_y) + "/" + std::to_string(w.step);
    return SGM_ERR_PARAM;
}

// OpenCV modes: the vertical direction of the last group fused with the WTA (k_ocv_vwta)
// instead of paths + k_ocv_wta16. One wave per column walks H steps and does the pixel WTAs
// itself, so it needs frames with many cells per column chain (interleaved A/B,
// profiles/r03_ocv_vwta_ab.jsonl, ms per frame off -> on: shipped 2448x2048 D=480 MODE_SGBM
// 14.54 -> 13.93, MODE_HH 21.82 -> 21.63; 1080p D=128 MODE_SGBM 1.85 -> 2.11, MODE_HH 2.55 ->
// 2.48; C1 0.23 -> 0.41). SGM_OCV_VWTA = 0 / 1 forces it off / on (parity tests run both).
// D <= 128 with uniqueness < 100 keeps the row WTA in both modes since it is packed
// (k_ocv_wta16_pk, which also lets the paths write deficit volumes): 1080p D=128 MODE_HH
// 2.25 -> 1.97 ms (profiles/r05_ocv_hh_vwta_ab.jsonl), 4096x3000 D=128 MODE_SGBM 9.49-9.65 ->
// 8.63; at 4096x3000 D=256 MODE_HH the fused kernel stays ahead (28.3-28.6 against 30.0 ms,
// profiles/r05_ocv_12mp_vwta_ab.jsonl), so wider ranges keep the thresholds below.
bool ocv_vwta_on(const Geom& g, int fullDP)
{
    if (const char* e = std::getenv("SGM_OCV_VWTA")) return std::atoi(e) != 0;
    if (g.D <= 128 && g.uniq < 100) return false;
    return (double)g.width1 * g.H * g.D >= (fullDP ? 2.0e8 : 1.0e9);
}

// Frames per pipelined launch: 2 (more path blocks than resident workgroup slots, so the
// dispatcher balances the CUs) unless the batch is shorter; SGM_GROUP overrides (1..4).
int batch_group(int n)
{
    const char* env = std::getenv("SGM_GROUP");
    const int g = env ? std::atoi(env) : 2;
    return std::max(1, std::min({g, sgm::kMaxGroup, n}));
}

// Lanes of an OCV-mode frame batch (run_batch_ocv): SGM_OCV_STREAMS, default 4, at most 8.
int ocv_batch_lanes(int n)
{
    const char* e = std::getenv("SGM_OCV_STREAMS");
    const int s = e ? std::atoi(e) : 4;
    return std::max(1, std::min({s, n, 8}));
}

}  // namespace sgm
