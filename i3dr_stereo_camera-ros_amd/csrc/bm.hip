// bm.hip — SGM_MODE_OCV_BM: cv::StereoBM (XSOBEL pre-filter + fused SAD block matching).
//
// Two launches per frame (BM section):
//   k_bm_prefilter  both images in one launch, u8 -> u8 (clamped x-Sobel + cap)
//   k_bm_match      fused SAD + winner-takes-all + texture / uniqueness tests + sub-pixel
// The SAD volume never exists in HBM. A workgroup (8 or 16 waves) owns a strip of TX output
// columns plus a halo of w2 columns on each side and marches down RB output rows. Per row step:
//   * the entering and the leaving row of both pre-filtered images are staged in LDS (fetched
//     into registers one step ahead, so the loads fly during the previous row's WTA);
//   * V[j][e], the vertical running sum of |PL - PR| of strip column j at disparity index e
//     over the 2*w2 + 1 rows of the window, lives in LDS (u16 when w^2 * 2c <= 65535, else
//     u32): v_sad_u8 adds the entering row's |diff| and subtracts the leaving row's, which is
//     recomputed from the staged rows, not stored. Wave i takes columns i, i + waves, ...;
//   * a wave owns a run of output columns of the strip: lane l holds the horizontal box sums
//     of e = l + 64k (k < K) in registers and slides them along x (add the entering column
//     sum, subtract the leaving one: two conflict-free LDS reads per cell);
//   * per pixel the wave reduces (SAD << 11 | e) to the first minimum (wave_min: DPP), reads the
//     two neighbours with v_readlane, and decides uniqueness by counting the values at or below
//     the bound with one ballot per chunk: no second pass over memory. The sub-pixel division
//     and the store run once per 64 pixels, one pixel per lane.
// The edge workgroups also write FILTERED to the frame's border columns and rows.
// e = D - 1 - (d - minD): e = 0 is the largest disparity (OpenCV scans in this order and keeps
// the first minimum, so equal minima resolve to the largest disparity).
#include "sgm_device.h"
#include "sgm_launch.h"

#include <cstdlib>

namespace sgm {

constexpr int kBmMaxWaves = 16;
// waves of a workgroup: 16, or 8 for D > 1024 (32 chunks per lane need more than 128 VGPRs)
__host__ __device__ constexpr int bm_waves(int k) { return k > 16 ? kBmMaxWaves / 2 : kBmMaxWaves; }
constexpr int kBmPf = 4;                      // staged bytes a thread prefetches per row step
// LDS bytes of one staged row of NC strip columns: the left pixels, the right segment (4-B multiples)
__host__ __device__ constexpr int bm_stage_l(int nc) { return (nc + 3) & ~3; }
__host__ __device__ constexpr int bm_stage_r(int nc, int D) { return (nc + D + 3) & ~3; }
constexpr size_t kBmLdsBudget = 128 * 1024;   // of the 160 KB of a gfx950 CU

// XSOBEL pre-filter of both images (blockIdx.z): reflect-101 rows, columns 0 and W-1 = cap,
// and the whole last row = cap when H is odd (OpenCV's loop handles two rows per step).
__global__ __launch_bounds__(256) void k_bm_prefilter(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R,
                                                      size_t stride, int W, int H, int cap,
                                                      uint8_t* __restrict__ PL, uint8_t* __restrict__ PR)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const uint8_t* __restrict__ src = blockIdx.z ? R : L;
    uint8_t* __restrict__ dst = blockIdx.z ? PR : PL;
    int v = cap;
    if (x >= 1 && x <= W - 2 && !((H & 1) && y == H - 1)) {
        const int ya = y > 0 ? y - 1 : 1, yb = y < H - 1 ? y + 1 : H - 2;
        const uint8_t* a = src + (size_t)ya * stride + x;
        const uint8_t* b = src + (size_t)y * stride + x;
        const uint8_t* c = src + (size_t)yb * stride + x;
        const int s = (a[1] - a[-1]) + 2 * (b[1] - b[-1]) + (c[1] - c[-1]);
        v = min(max(s, -cap), cap) + cap;
    }
    dst[(size_t)y * W + x] = (uint8_t)v;
}

hipError_t launch_bm_prefilter(const uint8_t* L, const uint8_t* R, size_t stride, int W, int H, int cap, uint8_t* PL,
                               uint8_t* PR, hipStream_t st)
{
    hipLaunchKernelGGL(k_bm_prefilter, dim3((W + 255) / 256, H, R ? 2 : 1), dim3(256), 0, st, L, R, stride, W, H, cap,
                       PL, PR);
    return hipGetLastError();
}

// Tiling of the fused kernel for a geometry. SGM_BM_VGLOBAL=1 forces the HBM column sums
// (the parity tests run both).
BmPlan bm_plan(const Geom& g, int n_cu)
{
    BmPlan p{};
    const int w2 = g.SW2, w = 2 * w2 + 1;
    p.wide = (long long)w * w * 2 * g.ftzero > 65535 ? 1 : 0;
    p.nk = (g.D + 63) / 64;
    p.Dp = p.nk * 64;
    const size_t es = p.wide ? 4 : 2;
    // per strip column: the column sums, the texture sum and 4 staged bytes (two rows x two images)
    const size_t per_col = (size_t)p.Dp * es + 4 + 4;
    const char* env = std::getenv("SGM_BM_VGLOBAL");
    const size_t fixed = 2 * ((size_t)p.Dp + 8) + 16;        // the staged right segments' D bytes + padding
    const int max_nc = (int)((kBmLdsBudget - fixed) / per_col);
    if (!(env && std::atoi(env) != 0) && max_nc >= w + 3) {
        p.TX = std::min(max_nc - 2 * w2, 128);
    } else {
        p.vglobal = 1;
        p.TX = 32;
    }
    const int width1 = std::max(g.width1, 1), rows = std::max(g.H - 2 * w2, 1);
    // bands of at least the window height: a band recomputes 2*w2 rows of column sums before its
    // first output row
    const int max_bands = std::max(1, rows / std::max(8, 2 * w2));
    const int cus = std::max(n_cu, 1);
    p.TX = std::min(p.TX, width1);
    // narrower strips while the frame cannot give every CU two workgroups (16 waves each: a row
    // step is a chain of LDS and DPP latencies, so a strip's columns and pixels are spread over
    // many waves and a CU holds 32 of them)
    while (p.TX > 32 && ((width1 + p.TX - 1) / p.TX) * max_bands < 2 * cus) p.TX = (p.TX + 1) / 2;
    p.nsx = (width1 + p.TX - 1) / p.TX;
    p.TX = (width1 + p.nsx - 1) / p.nsx;
    const size_t nc = (size_t)p.TX + 2 * w2;
    const size_t stage = 2 * (size_t)bm_stage_l((int)nc) + 2 * (size_t)bm_stage_r((int)nc, p.Dp);
    p.lds = nc * 4 + stage + (p.vglobal ? 0 : nc * p.Dp * es);
    // workgroups that fill the CUs in whole rounds (rounded down: one round fewer beats a tail)
    // 16 waves on the large strips (one workgroup per CU: many waves hide its LDS latencies), 8 on
    // the small ones, where the per-wave fixed work of a row step (its warm-up columns) dominates
    p.waves = p.lds > 48 * 1024 ? bm_waves(p.nk) : kBmMaxWaves / 2;
    const int per_cu = (int)std::min<size_t>(32 / p.waves, std::max<size_t>(1, (160 * 1024) / std::max<size_t>(p.lds, 1)));
    const int target = cus * per_cu;
    p.nsy = std::min(std::max(target / p.nsx, 1), max_bands);
    p.RB = (rows + p.nsy - 1) / p.nsy;
    p.nsy = (rows + p.RB - 1) / p.RB;
    p.vbytes = p.vglobal ? (size_t)p.nsx * p.nsy * nc * p.Dp * es : 0;
    return p;
}

// T: the column-sum type (uint16_t / uint32_t); K: 64-disparity chunks per lane (>= plan.nk);
// VG: the column sums live in the workspace (gV) instead of LDS. blockDim.x / 64 waves.
template <typename T, int K, bool VG>
__global__ __launch_bounds__(bm_waves(K) * 64) void k_bm_match(const uint8_t* __restrict__ PL,
                                                               const uint8_t* __restrict__ PR, Geom g, BmPlan pl,
                                                               int16_t* __restrict__ out, size_t ostride, T* gV,
                                                               int* __restrict__ dbg_vol, int* __restrict__ dbg_tex)
{
    extern __shared__ uint32_t lds_bm[];
    constexpr int kVU = K <= 8 ? 2 : 1;                     // columns of the vertical step in flight
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwv = blockDim.x >> 6, nth = blockDim.x;
    const int W = g.W, D = g.D, w2 = g.SW2, cap = g.ftzero, Dp = pl.Dp, nk = pl.nk;
    const int s = D - 1 + g.minD;
    const int xs = g.minX1 + blockIdx.x * pl.TX;            // first output column of the strip
    const int nx = min(pl.TX, g.maxX1 - xs);
    const int y0 = w2 + blockIdx.y * pl.RB;                 // first output row of the band
    const int ny = min(pl.RB, g.H - w2 - y0);
    const int NC = nx + 2 * w2, NCmax = pl.TX + 2 * w2;
    int* Vt = (int*)lds_bm;                                 // texture column sums
    // the entering and the leaving row of both pre-filtered images, staged per row step: the strip's
    // left pixels (clamped columns) and the right segment [rc(0), rc(NC - 1) + D)
    const int stL = bm_stage_l(NCmax), stR = bm_stage_r(NCmax, Dp);
    uint8_t* sLn = (uint8_t*)(lds_bm + NCmax);
    uint8_t* sLo = sLn + stL;
    uint8_t* sRn = sLo + stL;
    uint8_t* sRo = sRn + stR;
    // the column sums: LDS behind the staged rows, or this workgroup's slice of the workspace
    auto vbase = [&]() {
        if constexpr (VG) return gV + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * NCmax * Dp;
        else return (T*)(sRo + stR);
    };
    auto V = vbase();
    for (int i = threadIdx.x; i < NC * Dp; i += nth) V[i] = 0;
    for (int i = threadIdx.x; i < NC; i += nth) Vt[i] = 0;
    __syncthreads();
    // FILTERED around the computed area: the edge workgroups own the frame's border columns / rows
    {
        const int cx0 = blockIdx.x == 0 ? 0 : xs, cx1 = blockIdx.x == gridDim.x - 1 ? W : xs + nx;
        const int ry0 = blockIdx.y == 0 ? 0 : y0, ry1 = blockIdx.y == gridDim.y - 1 ? g.H : y0 + ny;
        const int cw = cx1 - cx0;
        if (cw != nx || ry1 - ry0 != ny)
            for (int i = threadIdx.x; i < cw * (ry1 - ry0); i += nth) {
                const int yy = ry0 + i / cw, xx = cx0 + i % cw;
                if (yy < y0 || yy >= y0 + ny || xx < xs || xx >= xs + nx)
                    out[(size_t)yy * ostride + xx] = (int16_t)g.invalid;
            }
    }

    const int npw = (nx + nwv - 1) / nwv;                   // output columns of a wave
    const int px0 = wv * npw, px1 = min(nx, px0 + npw);
    const int rfirst = y0 - w2, rend = y0 + ny + w2;
    const int rc0 = min(max(xs - w2 - s, 0), W - D);
    const int segR = min(max(xs - w2 + NC - 1 - s, 0), W - D) - rc0 + D;
    const int nstage = NC + segR;                           // staged bytes of one row (left, then right)

    // Row r's bytes are fetched into registers one row step ahead (kBmPf per thread, the loads fly
    // during the WTA of the row before) and committed to LDS at the top of their step; bytes past
    // kBmPf * blockDim (very wide searches) are copied at the commit.
    uint8_t pfn[kBmPf], pfo[kBmPf];
    auto stage_src = [&](int i, int row) -> const uint8_t* {
        return i < NC ? PL + (size_t)row * W + min(max(xs - w2 + i, 0), W - 1)
                      : PR + (size_t)row * W + rc0 + (i - NC);
    };
    auto prefetch = [&](int row) {
        const int rold = row - (2 * w2 + 1) >= rfirst ? row - (2 * w2 + 1) : row;
#pragma unroll
        for (int q = 0; q < kBmPf; q++) {
            const int i = threadIdx.x + q * nth;
            if (i < nstage) { pfn[q] = *stage_src(i, row); pfo[q] = *stage_src(i, rold); }
        }
    };
    auto commit = [&](int row) {
        const int rold = row - (2 * w2 + 1) >= rfirst ? row - (2 * w2 + 1) : row;
#pragma unroll
        for (int q = 0; q < kBmPf; q++) {
            const int i = threadIdx.x + q * nth;
            if (i < nstage) {
                if (i < NC) { sLn[i] = pfn[q]; sLo[i] = pfo[q]; }
                else { sRn[i - NC] = pfn[q]; sRo[i - NC] = pfo[q]; }
            }
        }
        for (int i = threadIdx.x + kBmPf * nth; i < nstage; i += nth) {
            const uint8_t vn = *stage_src(i, row), vo = *stage_src(i, rold);
            if (i < NC) { sLn[i] = vn; sLo[i] = vo; }
            else { sRn[i - NC] = vn; sRo[i - NC] = vo; }
        }
    };
    prefetch(rfirst);
    // lanes of the last chunk that hold a real disparity index
    const unsigned long long lastmask = (D & 63) ? (1ull << (D & 63)) - 1 : ~0ull;

    for (int r = rfirst; r < rend; r++) {
        // ---- vertical step: row r enters, row r - (2*w2 + 1) leaves
        const bool has_old = r - (2 * w2 + 1) >= rfirst;
        commit(r);
        __syncthreads();
        if (r + 1 < rend) prefetch(r + 1);
        // lanes past D (the last chunk of a D that is no multiple of 64) repeat disparity index
        // D - 1: their sums tie with it and lose to its smaller index, so nothing is predicated
        if (has_old) {
#pragma unroll kVU
            for (int j = wv; j < NC; j += nwv) {
                const int rcj = min(max(xs - w2 + j - s, 0), W - D) - rc0;
                const unsigned pln = sLn[j], plo = sLo[j];
                auto v = V + (size_t)j * Dp;
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (k < nk) {
                        unsigned t = __builtin_amdgcn_sad_u8(pln, sRn[rcj + min(lane + 64 * k, D - 1)], v[lane + 64 * k]);
                        t -= __builtin_amdgcn_sad_u8(plo, sRo[rcj + min(lane + 64 * k, D - 1)], 0u);
                        v[lane + 64 * k] = (T)t;
                    }
                if (lane == 0) Vt[j] += abs((int)pln - cap) - abs((int)plo - cap);
            }
        } else {
#pragma unroll kVU
            for (int j = wv; j < NC; j += nwv) {
                const int rcj = min(max(xs - w2 + j - s, 0), W - D) - rc0;
                const unsigned pln = sLn[j];
                auto v = V + (size_t)j * Dp;
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (k < nk) v[lane + 64 * k] = (T)__builtin_amdgcn_sad_u8(pln, sRn[rcj + min(lane + 64 * k, D - 1)], v[lane + 64 * k]);
                if (lane == 0) Vt[j] += abs((int)pln - cap);
            }
        }
        __syncthreads();
        // ---- horizontal slide + WTA of output row y
        const int y = r - w2;
        if (y >= y0 && px0 < px1) {
            int Hs[K];
            int Ts = 0;
#pragma unroll
            for (int k = 0; k < K; k++) Hs[k] = 0;
            for (int j = px0; j <= px0 + 2 * w2; j++) {
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (k < nk) Hs[k] += (int)V[(size_t)j * Dp + lane + 64 * k];
                Ts += Vt[j];
            }
            // lane i keeps the WTA result of the wave's pixel px0 + 64*n + i; the sub-pixel term and
            // the store run once per 64 pixels, one pixel per lane
            int k_min = 0, k_ind = -1, k_p = 0, k_n = 0;
            for (int px = px0; px < px1; px++) {
                const int X = xs + px;
                if (dbg_vol) {
                    const size_t pix = (size_t)y * g.width1 + (X - g.minX1);
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (k < nk && lane + 64 * k < D) dbg_vol[pix * D + lane + 64 * k] = Hs[k];
                    if (lane == 0 && dbg_tex) dbg_tex[pix] = Ts;
                }
                // first minimum in e order: lane-local over k (e ascends with k), then across lanes
                int minsad, mind;
                if constexpr (sizeof(T) == 2) {         // SAD < 2^16, e < 2^11: one key, one reduction
                    int key = 0x7FFFFFFF;
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (k < nk) key = min(key, (Hs[k] << 11) | (lane + 64 * k));
                    key = wave_min(key);
                    minsad = key >> 11;
                    mind = key & 2047;
                } else {
                    int bv = 0x7FFFFFFF, be = 0;
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (k < nk && Hs[k] < bv) { bv = Hs[k]; be = lane + 64 * k; }
                    minsad = wave_min(bv);
                    mind = wave_min(bv == minsad ? be : 0x7FFFFFFF);
                }
                // SAD[-1] := SAD[1], SAD[D] := SAD[D - 2]
                const int ep = mind + 1 < D ? mind + 1 : D - 2;
                const int en = mind > 0 ? mind - 1 : 1;
                int p = 0, n = 0;
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (k < nk) {
                        if ((ep >> 6) == k) p = __builtin_amdgcn_readlane(Hs[k], ep & 63);
                        if ((en >> 6) == k) n = __builtin_amdgcn_readlane(Hs[k], en & 63);
                    }
                bool bad = Ts < g.bm_tex;
                if (!bad && g.uniq > 0) {
                    // minsad + minsad * u / 100: minsad < 2^23, so 32 bits hold the product up to u = 255
                    // (a division by a constant); larger ratios take the 64-bit division
                    int thr;
                    if (g.uniq <= 255) {
                        thr = minsad + (int)((unsigned)minsad * (unsigned)g.uniq / 100u);
                    } else {
                        const long long t64 = (long long)minsad + (long long)minsad * g.uniq / 100;
                        thr = (int)min(t64, (long long)0x7FFFFFFF);
                    }
                    // any e outside [mind - 1, mind + 1] with SAD <= thr: count every e at or below the
                    // bound (one ballot per chunk) and take off the up to three inside the window
                    int cnt = 0;
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (k < nk) {
                            unsigned long long m = __ballot(Hs[k] <= thr);
                            if (k == nk - 1) m &= lastmask;
                            cnt += __builtin_popcountll(m);
                        }
                    const int inside = 1 + (mind > 0 && n <= thr ? 1 : 0) + (mind + 1 < D && p <= thr ? 1 : 0);
                    bad = cnt > inside;
                }
                const int slot = (px - px0) & 63;
                if (lane == slot) { k_min = minsad; k_ind = bad ? -1 : mind; k_p = p; k_n = n; }
                if (slot == 63 || px + 1 == px1) {
                    if (lane <= slot) {
                        int res = g.invalid;
                        if (k_ind >= 0) {
                            const int q = k_p + k_n - 2 * k_min + abs(k_p - k_n);
                            int frac;
                            if constexpr (sizeof(T) == 2) frac = tdiv((k_p - k_n) * 256, max(q, 1));   // |num| < 2^24
                            else frac = (k_p - k_n) * 256 / max(q, 1);
                            res = ((D - k_ind - 1 + g.minD) * 256 + (q ? frac : 0) + 15) >> 4;
                        }
                        out[(size_t)y * ostride + X - slot + lane] = (int16_t)res;
                    }
                }
                if (px + 1 < px1) {
#pragma unroll
                    for (int k = 0; k < K; k++)
                        if (k < nk)
                            Hs[k] += (int)V[(size_t)(px + 1 + 2 * w2) * Dp + lane + 64 * k] -
                                     (int)V[(size_t)px * Dp + lane + 64 * k];
                    Ts += Vt[px + 1 + 2 * w2] - Vt[px];
                }
            }
        }
        // no barrier here: the commit of the next step only writes the staged rows (last read before
        // the barrier above), and the barrier after it orders this step's V reads before its V writes
    }
}

template <typename T, int K, bool VG>
static hipError_t bm_launch(const uint8_t* PL, const uint8_t* PR, const Geom& g, const BmPlan& pl, int16_t* out,
                            size_t ostride, void* gV, int* dbg_vol, int* dbg_tex, hipStream_t st)
{
    if (pl.lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bm_match<T, K, VG>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_bm_match<T, K, VG>), dim3(pl.nsx, pl.nsy), dim3(pl.waves * 64), pl.lds, st, PL, PR, g, pl,
                       out, ostride, (T*)gV, dbg_vol, dbg_tex);
    return hipGetLastError();
}

template <typename T, bool VG>
static hipError_t bm_launch_k(const uint8_t* PL, const uint8_t* PR, const Geom& g, const BmPlan& pl, int16_t* out,
                              size_t ostride, void* gV, int* dbg_vol, int* dbg_tex, hipStream_t st)
{
    if (pl.nk <= 1) return bm_launch<T, 1, VG>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
    if (pl.nk <= 2) return bm_launch<T, 2, VG>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
    if (pl.nk <= 4) return bm_launch<T, 4, VG>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
    if (pl.nk <= 8) return bm_launch<T, 8, VG>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
    if (pl.nk <= 16) return bm_launch<T, 16, VG>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
    return bm_launch<T, 32, VG>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
}

template <typename T>
static hipError_t bm_launch_v(const uint8_t* PL, const uint8_t* PR, const Geom& g, const BmPlan& pl, int16_t* out,
                              size_t ostride, void* gV, int* dbg_vol, int* dbg_tex, hipStream_t st)
{
    return pl.vglobal ? bm_launch_k<T, true>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st)
                      : bm_launch_k<T, false>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
}

// The whole frame: the fused kernel over rows [w2, H - w2) x columns
// [X0, X1). PL / PR: the pre-filtered images (row pitch W). gV: pl.vbytes of workspace when
// pl.vglobal. dbg_vol / dbg_tex (may be null): sgm_debug_bm_sad.
hipError_t launch_bm_match(const uint8_t* PL, const uint8_t* PR, const Geom& g, const BmPlan& pl, int16_t* out,
                           size_t ostride, void* gV, int* dbg_vol, int* dbg_tex, hipStream_t st)
{
    if (g.width1 <= 0 || g.H - 2 * g.SW2 <= 0 || g.D > 2048) return launch_fill16(out, ostride, g.W, g.H, g.invalid, st);
    return pl.wide ? bm_launch_v<uint32_t>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st)
                   : bm_launch_v<uint16_t>(PL, PR, g, pl, out, ostride, gV, dbg_vol, dbg_tex, st);
}

}  // namespace sgm
