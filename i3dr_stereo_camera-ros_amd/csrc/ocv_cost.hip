// ocv_cost.hip — the cost stage of the OpenCV-StereoSGBM-compatible modes (ocv_device.h): C'.
//   k_ocv_prefilter  Sobel-x prefilter + raw channel, columns 0 / W-1 forced to ftzero
//   k_ocv_cost_fused pixel cost + vertical box + horizontal box + P2 in one pass (the default
//                    for frames that fill the chip, ocv_cost_fusable)
//   k_ocv_pixhsum    Birchfield-Tomasi cost of both channels (raw >> 2) and the horizontal
//                    SAD box (replicate clamp to [0, width1)) in one pass through LDS;
//                    k_ocv_pixcost + k_ocv_hsum unfused when the LDS tile would not fit
//   k_ocv_vsum_seg   vertical box + P2 offset + OpenCV's bottom-row quirk:
//                    rows with y + SH2 >= H are never recomputed (MODE_SGBM keeps the
//                    last computed row, MODE_HH keeps the P2 initialisation)
//   k_ocv_*_sat, k_ocv_vsum_sat2   OpenCV's SIMD cost loop for the flagged SIMD_SAT frames
#include "ocv_device.h"
#include "sgm_launch.h"
#include <algorithm>
#include <atomic>
#include <cstdlib>

namespace sgm {

// bt (optional, the fused cost's input): the Birchfield-Tomasi intervals of both channels at x,
// packed u | lo << 8 | hi << 16, from the prefiltered / raw values at x - 1, x, x + 1 computed in
// the thread (what bt_lohi reads from the planes)
// Four adjacent pixels per thread (round 5; was one, with ~15 byte loads each): the 8 source bytes
// x0 - 2 .. x0 + 5 of the three rows feed the six prefiltered values x0 - 1 .. x0 + 4 (the BT
// intervals need both neighbours), and the four pixels of each plane go out as one dword / dwordx4
// store where the address is aligned (else byte / dword stores).
__global__ __launch_bounds__(256) void k_ocv_prefilter(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R,
                                                       size_t stride, int W, int H, int ftzero,
                                                       uint8_t* __restrict__ planes /* 4 x W x H */,
                                                       uint32_t* __restrict__ bt /* 4 x W x H, or null */)
{
    const int x0 = 4 * (blockIdx.x * 256 + threadIdx.x), y = blockIdx.y;
    if (x0 >= W) return;
    const int img = blockIdx.z;
    const uint8_t* src = img ? R : L;
    uint8_t* pf = planes + (size_t)(2 * img) * W * H;
    uint8_t* raw = planes + (size_t)(2 * img + 1) * W * H;
    const size_t o = (size_t)y * W + x0;
    const uint8_t* r = src + (size_t)y * stride;
    const uint8_t* n = y > 0 ? r - stride : r;
    const uint8_t* s = y < H - 1 ? r + stride : r;
    // source bytes x0 - 2 + i (clamped reads: the columns they reach outside [1, W - 2] are forced
    // to ftzero below)
    int cr[8], cn[8], cs[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int xx = min(max(x0 - 2 + i, 0), W - 1);
        cr[i] = r[xx]; cn[i] = n[xx]; cs[i] = s[xx];
    }
    int p[6], q[6];                                      // columns x0 - 1 + j; 0 and W - 1 are ftzero
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const int xx = x0 - 1 + j;
        const int v = (cr[j + 2] - cr[j]) * 2 + cn[j + 2] - cn[j] + cs[j + 2] - cs[j];
        const bool edge = xx <= 0 || xx >= W - 1;
        p[j] = edge ? ftzero : min(max(v, -ftzero), ftzero) + ftzero;
        q[j] = edge ? ftzero : cr[j + 1];
    }
    const bool full = x0 + 3 < W && (((uintptr_t)(pf + o) | (uintptr_t)(raw + o)) & 3) == 0;
    if (full) {
        *(uint32_t*)(pf + o) = (uint32_t)p[1] | (uint32_t)p[2] << 8 | (uint32_t)p[3] << 16 | (uint32_t)p[4] << 24;
        *(uint32_t*)(raw + o) = (uint32_t)q[1] | (uint32_t)q[2] << 8 | (uint32_t)q[3] << 16 | (uint32_t)q[4] << 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (x0 + k < W) { pf[o + k] = (uint8_t)p[k + 1]; raw[o + k] = (uint8_t)q[k + 1]; }
    }
    if (!bt) return;
    // bt_lohi of pixel k with neighbours k - 1 and k + 1 (the frame's first / last column takes
    // itself as the missing neighbour)
    auto pack = [&](const int (&a)[6], int k) {
        const int u = a[k + 1];
        const int l = x0 + k > 0 ? a[k] : u, rr = x0 + k < W - 1 ? a[k + 2] : u;
        const int ul = (u + l) / 2, ur = (u + rr) / 2;
        return (uint32_t)u | (uint32_t)min(min(ul, ur), u) << 8 | (uint32_t)max(max(ul, ur), u) << 16;
    };
    const size_t plane = (size_t)W * H;
    uint32_t* bp = bt + (size_t)(2 * img) * plane + o;
    uint32_t* bq = bt + (size_t)(2 * img + 1) * plane + o;
    if (x0 + 3 < W && (((uintptr_t)bp | (uintptr_t)bq) & 15) == 0) {
        *(uint4*)bp = make_uint4(pack(p, 0), pack(p, 1), pack(p, 2), pack(p, 3));
        *(uint4*)bq = make_uint4(pack(q, 0), pack(q, 1), pack(q, 2), pack(q, 3));
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (x0 + k < W) { bp[k] = pack(p, k); bq[k] = pack(q, k); }
    }
}

__device__ __forceinline__ void bt_lohi(const uint8_t* a, int x, int W, int& u, int& lo, int& hi)
{
    u = a[x];
    const int ul = x > 0 ? (u + a[x - 1]) / 2 : u;
    const int ur = x < W - 1 ? (u + a[x + 1]) / 2 : u;
    lo = min(min(ul, ur), u);
    hi = max(max(ul, ur), u);
}


__device__ __forceinline__ void pixcost_cell(const uint8_t* __restrict__ planes, const Geom& g, int x1, int y,
                                             int16_t* __restrict__ cost)
{
    const int x = x1 + g.minX1;
    const size_t plane = (size_t)g.W * g.H;
    int c_u[2], c_lo[2], c_hi[2];
#pragma unroll
    for (int c = 0; c < 2; c++) bt_lohi(planes + c * plane + (size_t)y * g.W, x, g.W, c_u[c], c_lo[c], c_hi[c]);
    int16_t* out = cost + ((size_t)y * g.width1 + x1) * g.D;
    for (int d = threadIdx.x; d < g.D; d += 256) {
        const int xr = x - g.minD - d;
        int acc = 0;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int v, v0, v1;
            bt_lohi(planes + (2 + c) * plane + (size_t)y * g.W, xr, g.W, v, v0, v1);
            const int c0 = max(0, max(c_u[c] - v1, v0 - c_u[c]));
            const int c1 = max(0, max(v - c_hi[c], c_lo[c] - v));
            acc += min(c0, c1) >> (c == 0 ? 0 : 2);
        }
        out[d] = (int16_t)acc;
    }
}

// grid (width1, H), block 256 over d
__global__ __launch_bounds__(256) void k_ocv_pixcost(const uint8_t* __restrict__ planes, Geom g,
                                                     int16_t* __restrict__ cost)
{
    pixcost_cell(planes, g, blockIdx.x, blockIdx.y, cost);
}

// thread per (y, d): running horizontal box along x
__global__ __launch_bounds__(256) void k_ocv_hsum(const int16_t* __restrict__ pix, Geom g, int16_t* __restrict__ hs)
{
    const int d = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (d >= g.D) return;
    const size_t rb = (size_t)y * g.width1 * g.D + d;
    const int W1 = g.width1, SW2 = g.SW2;
    int s = pix[rb] * (SW2 + 1);
    for (int i = 1; i <= SW2; i++) s += pix[rb + (size_t)min(i, W1 - 1) * g.D];
    hs[rb] = (int16_t)s;
    for (int x = 1; x < W1; x++) {
        s += pix[rb + (size_t)min(x + SW2, W1 - 1) * g.D] - pix[rb + (size_t)max(x - SW2 - 1, 0) * g.D];
        hs[rb + (size_t)x * g.D] = (int16_t)s;
    }
}

// Pixel cost + horizontal SAD box fused: one block per XB output pixels x DC disparities of
// a row (blockIdx.z: the disparity chunk). Chunking the disparities lets a block take many
// output columns (few halo columns recomputed) at any D: with all D in one block it could
// take only 32 columns, and a 21-wide box recomputed 52 columns per 32 outputs (the shipped
// 2448x2048 D=480 block-21 config: 5.38 -> 3.38 ms).
// Every value is handled as a packed pair of ADJACENT DISPARITIES (d, d+1) in one u32, the
// layout of the output volume, so the box and its stores take one op per two cells:
//   stage:  the Birchfield-Tomasi intervals (u, lo, hi) of both channels of the NX = XB + 2*SW2
//           left columns, each duplicated into both halves of a u32, 6 words per column; the
//           right entries the cells reach (r = 0 .. NX + DC - 2), indexed j = M - 1 - r, as pair
//           words W[j] = (entry j, entry j + 1) per plane: the right entries of (d, d+1) at one
//           column are W[j] of d (low = d, high = d + 1). Records of 6 words (+ 1 pad) per j,
//           even and odd j apart: the lanes of a wave read j, j + 2, ... at a stride of 7 words
//           (conflict-free), the planes at immediate offsets;
//   cost:   P[k][dp] = the cells (k, 2dp) and (k, 2dp + 1): 12 u32 reads at immediate offsets
//           from two running addresses, packed u16 saturating subtracts (max(a - b, 0) in one
//           op): 16 packed ops for two cells;
//   edges:  staged columns outside [0, width1) take the edge column's P (the running sum's
//           replicate rule), in a short pass that only edge blocks run;
//   box:    thread (segment, dp) slides its window over the segment's outputs: two u32 LDS
//           reads, one packed subtract and add, one u32 store per two cells (u16 wrap-around
//           = OpenCV's int16 truncation of the int sum).
constexpr int kPixXB = 96;             // output columns per block (32-128 measured: 96 best at the shipped config)
constexpr int kPixDC = 128;            // disparities per block
__host__ __device__ inline int pix_xb(const Geom& g) { return g.D >= kPixDC ? kPixXB : kPixXB * 2; }
__host__ __device__ inline int pix_dc(const Geom& g) { return g.D < kPixDC ? g.D : kPixDC; }
struct PixGeo {
    int XB, DC, NX, M, PP;      // NX even >= XB + 2*SW2; M: right pair words (j < M);
                                // PP: P's row pitch in u32 (odd below 64 pairs: rows spread over banks)
    __host__ __device__ PixGeo(const Geom& g) {
        XB = pix_xb(g); DC = pix_dc(g);
        NX = (XB + 2 * g.SW2 + 1) & ~1;
        M = ((NX + DC) & ~1) + 2;                   // even, > NX + DC - 1; M / 2 records per parity
        PP = DC / 2 >= 64 ? DC / 2 : DC / 2 + 1;
    }
    __host__ __device__ size_t bytes() const { return (size_t)4 * ((size_t)NX * PP + 6 * NX + 7 * M); }
};
__host__ inline size_t pix_lds_bytes(const Geom& g) { return PixGeo(g).bytes(); }
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
template <bool GATED>      // GATED: only for the flagged frames (the fused cost made C' for the others)
__global__ __launch_bounds__(256) void k_ocv_pixhsum(const uint8_t* __restrict__ planes, Geom g,
                                                     int16_t* __restrict__ hs)
{
    if (GATED && !ocv_flagged(g)) return;
    extern __shared__ uint32_t lds_pix32[];
    const PixGeo pg(g);
    const int XB = pg.XB, DCmax = pg.DC, NX = pg.NX, M = pg.M, PP = pg.PP;
    const int y = blockIdx.y, x0 = blockIdx.x * XB, tid = threadIdx.x;
    const int d0 = blockIdx.z * DCmax, DC = min(DCmax, g.D - d0), DPC = DC / 2;   // D % 16 == 0: DC even
    const int SW2 = g.SW2;
    const size_t plane = (size_t)g.W * g.H;
    uint32_t* P = lds_pix32;                               // [NX][PP] packed (d, d+1)
    uint32_t* Lx = P + (size_t)NX * PP;                    // [NX][6]: (u, lo, hi) of channel 0, then 1
    uint32_t* Rw = Lx + 6 * NX;                            // [j & 1][j >> 1][7] pair words, same plane order
    const int MH = M / 2;
    // staged column k <-> x = minX1 + x0 - SW2 + k (not clamped: out-of-frame columns get
    // clamped BT entries and are replaced by the edge pass); right entry r <-> xr = x(0) - minD - (d0 + DC - 1) + r
    const int xs = g.minX1 + x0 - SW2;
    for (int i = tid; i < 2 * NX; i += 256) {
        const int c = i / NX, k = i - c * NX;
        int u, lo, hi;
        bt_lohi(planes + c * plane + (size_t)y * g.W, min(max(xs + k, 0), g.W - 1), g.W, u, lo, hi);
        uint32_t* o = Lx + 6 * k + 3 * c;
        o[0] = (uint32_t)u * 0x10001u; o[1] = (uint32_t)lo * 0x10001u; o[2] = (uint32_t)hi * 0x10001u;
    }
    const int xr0 = xs - g.minD - (d0 + DC - 1);
    const int NRr = NX + DC - 1;                           // right entries the cells reach
    uint16_t* Rh = (uint16_t*)Rw;
    for (int i = tid; i < 2 * NRr; i += 256) {
        const int c = i / NRr, r = i - c * NRr;
        int v, lo, hi;
        bt_lohi(planes + (2 + c) * plane + (size_t)y * g.W, min(max(xr0 + r, 0), g.W - 1), g.W, v, lo, hi);
        // entry j = M - 1 - r: low half of word j, high half of word j - 1 (j >= 2)
        const int j = M - 1 - r;
        uint16_t* lo16 = Rh + 2 * (7 * ((j & 1) * MH + (j >> 1)) + 3 * c);
        uint16_t* hi16 = Rh + 2 * (7 * (((j - 1) & 1) * MH + ((j - 1) >> 1)) + 3 * c) + 1;
        lo16[0] = (uint16_t)v; lo16[2] = (uint16_t)lo; lo16[4] = (uint16_t)hi;
        hi16[0] = (uint16_t)v; hi16[2] = (uint16_t)lo; hi16[4] = (uint16_t)hi;
    }
    __syncthreads();
    // thread -> disparity pair dp (fixed), columns k = kg, kg + tpd, ...
    // cell (k, d): r = k + DC - 1 - d, j = M - 1 - r = M - DC - k + d; the pair (2dp, 2dp + 1)
    // reads word j of d = 2dp (entries j and j + 1 = the right entries of d and d + 1). tpd is
    // even, so a thread's j keeps its parity (j = k mod 2) and steps tpd / 2 records down.
    const int tpd = (256 / DPC) & ~1, dp = tid % DPC, kg = tid / DPC;
    if (kg < tpd) {
        auto sat = [](u16x2_t a, u16x2_t b) { return __builtin_elementwise_sub_sat(a, b); };
        auto w = [](const uint32_t* p, int o) { return __builtin_bit_cast(u16x2_t, p[o]); };
        const uint32_t* Lk = Lx + 6 * kg;
        const int j0 = M - DC - kg + 2 * dp;
        const uint32_t* Rk = Rw + 7 * ((j0 & 1) * MH + (j0 >> 1));
        uint32_t* Pk = P + (size_t)kg * PP + dp;
        for (int k = kg; k < NX; k += tpd, Lk += 6 * tpd, Rk -= 7 * (tpd / 2), Pk += tpd * PP) {
            u16x2_t m[2];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const u16x2_t u = w(Lk, 3 * c), ulo = w(Lk, 3 * c + 1), uhi = w(Lk, 3 * c + 2);
                const u16x2_t v = w(Rk, 3 * c), v0 = w(Rk, 3 * c + 1), v1 = w(Rk, 3 * c + 2);
                const u16x2_t c0 = __builtin_elementwise_max(sat(u, v1), sat(v0, u));
                const u16x2_t c1 = __builtin_elementwise_max(sat(v, uhi), sat(ulo, v));
                m[c] = __builtin_elementwise_min(c0, c1);
            }
            *Pk = __builtin_bit_cast(uint32_t, m[0] + (m[1] >> (u16x2_t){2, 2}));
        }
    }
    __syncthreads();
    const int nout = min(XB, g.width1 - x0);
    const int klo = SW2 - x0, khi = g.width1 - 1 - x0 + SW2;   // staged columns inside [0, width1)
    if (klo > 0 || khi < NX - 1) {                              // uniform: an edge block
        const int nlo = max(klo, 0), nhi = max(NX - 1 - khi, 0);
        for (int i = tid; i < (nlo + nhi) * DPC; i += 256) {
            const int e = i / DPC, p = i - e * DPC;
            const int k = e < nlo ? e : khi + 1 + (e - nlo);
            P[(size_t)k * PP + p] = P[(size_t)(e < nlo ? klo : khi) * PP + p];
        }
        __syncthreads();
    }
    // horizontal box: thread (segment, dp) slides its window over the segment's outputs
    int16_t* dst = hs + ((size_t)y * g.width1 + x0) * g.D + d0;
    const int nseg = max(256 / DPC, 1), seglen = (nout + nseg - 1) / nseg, BW = 2 * SW2;
    for (int t = tid; t < nseg * DPC; t += 256) {
        const int seg = t / DPC, p = t - seg * DPC;
        const int xa = seg * seglen, xb = min(xa + seglen, nout);
        if (xa >= xb) continue;
        const uint32_t* Pd = P + p;
        u16x2_t sum = {0, 0};
        for (int u = 0; u <= BW; u++) sum += __builtin_bit_cast(u16x2_t, Pd[(size_t)(xa + u) * PP]);
        uint32_t* o = (uint32_t*)(dst + (size_t)xa * g.D) + p;
        *o = __builtin_bit_cast(uint32_t, sum);
        for (int xo = xa + 1; xo < xb; xo++) {
            sum += __builtin_bit_cast(u16x2_t, Pd[(size_t)(xo + BW) * PP]) - __builtin_bit_cast(u16x2_t, Pd[(size_t)(xo - 1) * PP]);
            o += g.D / 2;
            *o = __builtin_bit_cast(uint32_t, sum);
        }
    }
}

// Vertical box + P2 offset + the bottom-row rule, in segments of kVsumRows rows per thread
// (each segment starts from its own window sum; rows y >= 1 with y + SH2 >= H repeat the
// value of row max(H - SH2 - 1, 0) in MODE_SGBM, or are P2 in MODE_HH). A thread owns two
// adjacent disparities (one u32 of the row: width1 * D is even), int sums per half (the
// overflow flag needs the true value), one u32 load per row and window edge, one u32 store.
// SGM_OCV_COL0_LEGACY (OpenCV 3.x, `for (x = D; ...)`): column 0 keeps its row-0 value for
// y >= 1 (MODE_SGBM's single C row) or the P2 initialisation (MODE_HH's per-row C).
// Overflow flag (Geom::wide == 2): a C' above g.ovf_thr (32767: int16 volumes no longer exact
// for the scalar branch; 32767 - P2 for SIMD_SAT, where (short)(minLr + P2) could wrap), or a
// horizontal sum that left int16 (its u16 word has the sign bit: every true sum is >= 0).
constexpr int kVsumRows = 64;
__global__ __launch_bounds__(256) void k_ocv_vsum_seg(const int16_t* __restrict__ hs, Geom g, int fullDP,
                                                      int16_t* __restrict__ C)
{
    const int i = blockIdx.x * 256 + threadIdx.x;         // pair index in a row
    const size_t rs = (size_t)g.width1 * g.D / 2;          // u32 per row
    if (i >= (int)rs) return;
    const uint32_t* h32 = (const uint32_t*)hs;
    uint32_t* C32 = (uint32_t*)C;
    const int H = g.H, SH2 = g.SH2;
    const int y0 = blockIdx.y * kVsumRows, y1 = min(H, y0 + kVsumRows);
    auto lo16 = [](uint32_t w) { return (int)(int16_t)(uint16_t)w; };
    auto hi16 = [](uint32_t w) { return (int)w >> 16; };
    uint32_t signs = 0;                                    // OR of every loaded sum word
    auto window = [&](int y, int& s0, int& s1) {
        s0 = 0; s1 = 0;
        for (int k = y - SH2; k <= y + SH2; k++) {
            const uint32_t w = h32[(size_t)min(max(k, 0), H - 1) * rs + i];
            s0 += lo16(w); s1 += hi16(w);
            signs |= w;
        }
    };
    bool ovf = false;                                      // a C' above ovf_thr (Geom::wide == 2)
    const int ylast = max(H - SH2 - 1, 0);                 // last row whose window is recomputed
    const bool tail = y1 - 1 >= 1 && y1 - 1 + SH2 >= H;    // the segment reaches the repeated rows
    int rep0 = g.P2, rep1 = g.P2;
    if (!fullDP && tail) { int t0, t1; window(ylast, t0, t1); rep0 += t0; rep1 += t1; }
    // column 0 under COL0_LEGACY: every row y >= 1 holds z (row 0's value, or P2 in MODE_HH)
    const bool c0 = (g.compat & SGM_OCV_COL0_LEGACY) && i < g.D / 2;
    int z0 = g.P2, z1 = g.P2;
    if (c0 && !fullDP) { int t0, t1; window(0, t0, t1); z0 += t0; z1 += t1; }
    int s0, s1;
    window(y0, s0, s1);
    // rows in chunks of 8: the chunk's 16 entering / leaving rows are loaded together (clamped
    // rows, used only where the window slides), so a thread keeps 16 loads in flight
    constexpr int U = 8;
    for (int yb = y0; yb < y1; yb += U) {
        uint32_t ha[U], hb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int y = min(yb + u, y1 - 1);
            ha[u] = h32[(size_t)min(y + SH2, H - 1) * rs + i];
            hb[u] = h32[(size_t)max(y - SH2 - 1, 0) * rs + i];
            signs |= ha[u];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int y = yb + u;
            if (y >= y1) break;                            // uniform over the block
            int v0, v1;
            if (y == 0 || y + SH2 < H) {
                if (y > y0) { s0 += lo16(ha[u]) - lo16(hb[u]); s1 += hi16(ha[u]) - hi16(hb[u]); }
                v0 = g.P2 + s0; v1 = g.P2 + s1;
            } else {
                v0 = rep0; v1 = rep1;
            }
            if (c0 && y > 0) { v0 = z0; v1 = z1; }
            ovf |= max(v0, v1) > g.ovf_thr;
            C32[(size_t)y * rs + i] = ((uint32_t)v0 & 0xFFFFu) | ((uint32_t)v1 << 16);
        }
    }
    ovf |= (signs & 0x80008000u) != 0;
    if (g.wide == 2 && g.ovf) {                            // one atomic per wave that saw one
        const uint64_t b = __ballot(ovf);
        if (b && (int)(threadIdx.x & 63) == __builtin_ctzll(b)) atomicOr(g.ovf, 1);
    }
}

// ---- SGM_OCV_SIMD_SAT frames the overflow flag marks: OpenCV's SIMD cost loop, exactly ------
// (gated: each kernel returns at once unless the frame takes the flagged path). The SIMD
// branch saturates the running sums of rows y >= 1 — the horizontal sums of image rows
// k > SH2 ((h - sub) + add) and the vertical update ((Cprev - hsumSub) + hsumAdd) — so a value
// that saturated once changes every later one: sequential sums, one thread per (row, d) or per
// (column, d) pair; rows k <= SH2 and row y = 0 keep the scalar int16 wrap.
// grid-stride over the (x1, y) cells of the frame, block 256 over d
__global__ __launch_bounds__(256) void k_ocv_pixcost_sat(const uint8_t* __restrict__ planes, Geom g,
                                                         int16_t* __restrict__ cost)
{
    if (!ocv_flagged(g)) return;
    const int n = g.width1 * g.H;
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const int y = it / g.width1;
        pixcost_cell(planes, g, it - y * g.width1, y, cost);
    }
}

// thread per (image row k, d): the running horizontal box along x
__global__ __launch_bounds__(256) void k_ocv_hsum_sat(const int16_t* __restrict__ pix, Geom g, int16_t* __restrict__ hs)
{
    if (!ocv_flagged(g)) return;
    const int d = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (d >= g.D) return;
    const size_t rb = (size_t)k * g.width1 * g.D + d;
    const int W1 = g.width1, SW2 = g.SW2;
    int s = pix[rb] * (SW2 + 1);
    for (int i = 1; i <= SW2; i++) s += pix[rb + (size_t)min(i, W1 - 1) * g.D];
    int h = (int16_t)s;                                   // first column: scalar, int16 store
    hs[rb] = (int16_t)h;
    const bool sat = k > g.SH2;                            // computed for an output row y >= 1
    for (int x = 1; x < W1; x++) {
        const int a = pix[rb + (size_t)min(x + SW2, W1 - 1) * g.D];
        const int b = pix[rb + (size_t)max(x - SW2 - 1, 0) * g.D];
        h = sat ? sat16(sat16(h - b) + a) : (int)(int16_t)(h + a - b);
        hs[rb + (size_t)x * g.D] = (int16_t)h;
    }
}

// thread per (column, d): C' down the rows (OpenCV's row loop with the SIMD vertical update)
__global__ __launch_bounds__(256) void k_ocv_vsum_sat(const int16_t* __restrict__ hs, Geom g, int fullDP,
                                                      int16_t* __restrict__ C)
{
    if (!ocv_flagged(g)) return;
    const size_t rc = (size_t)g.width1 * g.D;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rc) return;
    const int H = g.H, SH2 = g.SH2;
    const bool c0 = (g.compat & SGM_OCV_COL0_LEGACY) && i < (size_t)g.D;
    int c = g.P2;                                          // row 0: P2 + the clamped window (int16 wrap)
    for (int k = -SH2; k <= SH2; k++) c += hs[(size_t)min(max(k, 0), H - 1) * rc + i];
    c = (int16_t)c;
    C[i] = (int16_t)c;
    for (int y = 1; y < H; y++) {
        if (y + SH2 < H) {
            if (!c0) c = sat16(sat16(c - hs[(size_t)max(y - SH2 - 1, 0) * rc + i]) + hs[(size_t)(y + SH2) * rc + i]);
            else if (fullDP) c = g.P2;
        } else if (fullDP) {
            c = g.P2;                                      // MODE_HH: never recomputed, the P2 init
        }                                                  // MODE_SGBM: the last computed row
        C[(size_t)y * rc + i] = (int16_t)c;
    }
}

// ---- the whole cost stage in one pass: pixel cost + vertical box + horizontal box + P2 ------
// (replaces k_ocv_pixhsum + k_ocv_vsum_seg, whose 2 B/cell horizontal-sum volume went to HBM
// and was read back twice: 1.71 GB moved for 0.50 GB of C' at 1080p D=128, PMC r03). The box
// is separable and OpenCV's int16 wrap is arithmetic mod 2^16, so the vertical sums can come
// first: a block owns a tile of XB output columns x DC disparities over a band of rows and walks
// the band's rows (+ SH2 above and below) once. Per row:
//   staging threads (waves 4-7): the BT intervals of the row (k_ocv_prefilter writes them) into LDS in
//       k_ocv_pixhsum's formats (left columns duplicated into both halves of a word, right
//       entries as pair words of adjacent disparities);
//   every thread: the pixel costs of its staged column k and I disparity pairs (packed u16 ops,
//       the left words kept in registers), and its vertical window sums V: V += P - P(row - R),
//       the last R = 2*SH2 + 1 rows of P in registers (the slot is picked by a uniform switch,
//       so every ring slot is a static register); V of the row to LDS;
//   box threads (every wave for R <= 9, else waves 0-3): the horizontal box (2*SW2+1 = R wide:
//       OpenCV's block is square) of the previous row's V: a segment of L output columns per
//       thread and pair, its L + R - 1 window values read from LDS at once (staged columns
//       outside [0, width1) read as the edge column: OpenCV's replicate rule) and slid over in
//       registers, + P2, stored as int16 (u16 wrap = OpenCV's CostType store);
// one barrier per row (staging, V and the box double-buffered). The true sums are exact in u16
// when (2*SW2+1)(2*SH2+1)(2*ftzero+63) <= 65535 (the launcher's condition), so the overflow flag
// of Geom::wide == 2 is max(box) > ovf_thr - P2, as k_ocv_vsum_seg computes it (no horizontal sum
// can leave int16 under that bound). OpenCV's bottom-row rule: the band holding the last computed
// row ylast = max(H - SH2 - 1, 0) also writes the rows below it (its last values in MODE_SGBM, P2
// in MODE_HH); COL0_LEGACY's column is written by k_ocv_col0_legacy afterwards.
// Block ids are dealt XCD-aware: the DC-chunks of one tile (and then the next strip of the band)
// run back to back on one XCD, so the partial lines of their C' rows merge in that L2.
constexpr int kFuseNX = 128;              // staged columns per block: 4 threads per column (256, 1024-thread blocks
                                          // one per CU: ocv_cost 2.0 -> 3.2 ms, profiles/r05_ocv_cost_nx256_ab.jsonl)
constexpr int kFuseThreads = 4 * kFuseNX;
constexpr int kFuseHalf = kFuseThreads / 2;   // waves 0 .. W/2 - 1: box (R > 9); the rest: staging
__host__ __device__ inline int fuse_xb(const Geom& g) { return kFuseNX - 2 * g.SW2; }
// rows per barrier: RB rows of pixel costs, boxes and staging between two barriers, the box RB
// rows behind the pixel costs and the staging RB rows ahead, over 2 * RB LDS buffers each: two
// rows for boxes wider than 9
__host__ __device__ constexpr int fuse_rb(int R) { return R > 9 ? 2 : 1; }
// words of LDS that hold ring slot 0 (R > 9: hipcc had spilled it to scratch): one per ring
// register of every thread
__host__ __device__ constexpr int fuse_ring0_words(int r, int dpc)
{
    // RQ ring registers per thread: I = dpc / 4 disparity pairs, two per register as bytes
    return r > 9 ? dpc / 8 * kFuseThreads : 0;
}
struct FuseGeo {
    int DC, M, MH;
    __host__ __device__ FuseGeo(int dpc) {
        DC = 2 * dpc;
        M = ((kFuseNX + DC) & ~1) + 2;
        MH = M / 2;
        // 32 pairs per block: the odd-entry half starts at MH = 101 (not 97), which makes the
        // pixel-cost reads of a 32-lane half hit 32 distinct banks (2-way before: SQ_LDS_BANK_CONFLICT
        // 44 % of the LDS cycles at 1080p block 5, profiles/r04_ocv_cost_pmc_fused_final_1080p.txt)
        if (dpc == 32) MH += ((5 - MH % 8) + 8) % 8;
    }
    __host__ __device__ int stage_words() const { return 6 * kFuseNX + 14 * MH; }
    // + ring slot 0 in LDS for boxes wider than 9 (fuse_ring0_words)
    __host__ __device__ size_t lds_bytes(int dpc, int rb, int r = 0) const {
        return (size_t)4 * 2 * rb * (stage_words() + kFuseNX * dpc) + (size_t)4 * fuse_ring0_words(r, dpc);
    }
};
struct FuseGrid {
    int strips, bands, chunks, band_rows, ncomp, total, per_xcd;
};
constexpr uint32_t kFuseDrop = 0x80000000u;      // a byte offset past every C' row descriptor's range
// TRK: what the overflow flag tracks (ocv_fuse_track): 0 nothing (no gate), 1 the max of C' itself
// (box + P2 below 2^16 whatever the pixels; P2 taken off at the end), 2 the max of C' - P2
// C' stores through a row descriptor (scalar offsets, no per-store VALU) for boxes up to this size
// (1080p block 5: 0.221 -> 0.217 ms; the shipped block 21: 2.00 -> 2.05 ms, so not there;
// profiles/r05_ocv_pk_cost_ab.jsonl)
constexpr int kFuseBufSt = 9;
// As measured (profiles/r04_ocv_cost_ring_ab_v2.jsonl; cost stage, 1080p block 5 / the shipped
// 2448x2048 D=480 block 21): the pixel-cost ring as bytes 0.234 -> 0.231 / 3.17 -> 3.01 ms, plus
// <= 128 VGPRs (4 waves per SIMD) asked for R > 9 (two blocks per CU at 36 B of spills) -> 2.86 ms;
// the box reads are issued after the V store: before the pixel costs measured 3.73 ms at R = 21
// (the window registers live across the pixel-cost phase), no gain at R = 5
template <int R, int DPC, int I, int TRK>
__global__ __launch_bounds__(kFuseThreads) __attribute__((amdgpu_waves_per_eu(R > 9 ? 4 : 1)))
void k_ocv_cost_fused(const uint32_t* __restrict__ bt, Geom g, int fullDP,
                                                                 FuseGrid fg, int16_t* __restrict__ C)
{
    // every Geom / FuseGrid field the kernel reads, as scalars: a by-value struct that any
    // lambda captures by reference is otherwise given an address (copied to scratch)
    const int gW = g.W, gH = g.H, gD = g.D, gP2 = g.P2, gw1 = g.width1, gminD = g.minD, gminX1 = g.minX1;
    const int gSW2 = g.SW2, gSH2 = g.SH2, gcompat = g.compat, govf_thr = g.ovf_thr;
    int* const govf = g.ovf;
    const int fg_strips = fg.strips, fg_chunks = fg.chunks, fg_band_rows = fg.band_rows, fg_ncomp = fg.ncomp;
    const int fg_total = fg.total, fg_per_xcd = fg.per_xcd;
    static_assert(DPC / I * kFuseNX == kFuseThreads, "4 threads per staged column");
    static_assert(R <= 21, "ring slots: cases 0..20 below");
    constexpr int TPC = DPC / I;
    extern __shared__ uint32_t lds_fuse[];
    const FuseGeo fz(DPC);
    const int DC = fz.DC, M = fz.M, MH = fz.MH, NX = kFuseNX;
    const int SW2 = gSW2, SH2 = gSH2, XB = NX - 2 * SW2;
    // XCD-aware deal: XCD x = blockIdx.x % 8 runs logical tiles x * per_xcd, x * per_xcd + 1, ...
    const int lid = (blockIdx.x & 7) * fg_per_xcd + (blockIdx.x >> 3);
    if (lid >= fg_total) return;
    const int chunk = lid % fg_chunks, tile = lid / fg_chunks;
    const int strip = tile % fg_strips, band = tile / fg_strips;
    const int x0 = strip * XB, d0 = chunk * DC;
    const int y0 = band * fg_band_rows, y1 = min(fg_ncomp, y0 + fg_band_rows);
    const int nv = (y1 - y0) + 2 * SH2;                      // rows of P the band needs
    const int t = threadIdx.x;
    constexpr int RB = fuse_rb(R), NBUF = 2 * RB;
    uint32_t* S0 = lds_fuse;                                 // staging, NBUF buffers
    uint32_t* V0 = lds_fuse + NBUF * fz.stage_words();       // V rows [NX][DPC], NBUF buffers
    auto Sbuf = [&](int r) { return S0 + (r % NBUF) * fz.stage_words(); };
    const int xs = gminX1 + x0 - SW2;                       // staged column k <-> image x = xs + k
    const int xr0 = xs - gminD - (d0 + DC - 1);             // right entry r <-> xr0 + r
    const size_t plane = (size_t)gW * gH;
    // staging (waves 4-7, beside the box of waves 0-3): entry st of the 2 * NX left entries (one
    // each) and entries st, st + kFuseHalf of the 2 * NRr right ones; the bt words of row v + 2 are
    // loaded while row v + 1's are written to LDS, so a global load's latency spans a whole phase
    const int st = t - kFuseHalf;
    const int NRr = NX + DC - 1;
    const int cl = st >= NX, kl = st - cl * NX;
    const int cr0 = st >= NRr, r0 = st - cr0 * NRr;
    static_assert(2 * kFuseNX <= kFuseHalf, "one staging thread per left entry");
    const bool has1 = st + kFuseHalf < 2 * NRr;
    const int cr1 = st + kFuseHalf >= NRr, r1 = st + kFuseHalf - cr1 * NRr;
    // 32-bit element offsets off the uniform base (4 planes < 2^32 elements: the launcher's
    // condition), one register each instead of a 64-bit pointer
    const uint32_t oL = (uint32_t)(cl * plane) + (uint32_t)min(max(xs + kl, 0), gW - 1);
    const uint32_t oR0 = (uint32_t)((2 + cr0) * plane) + (uint32_t)min(max(xr0 + r0, 0), gW - 1);
    const uint32_t oR1 = (uint32_t)((2 + cr1) * plane) + (uint32_t)min(max(xr0 + r1, 0), gW - 1);
    uint32_t wl = 0, wr0 = 0, wr1 = 0;
    auto stage_load = [&](int v) {
        const uint32_t ro = (uint32_t)(min(max(y0 - SH2 + v, 0), gH - 1) * gW);
        wl = bt[oL + ro];
        wr0 = bt[oR0 + ro];
        wr1 = has1 ? bt[oR1 + ro] : 0u;
    };
    auto put_right = [&](uint16_t* Rh, int c, int r, uint32_t w) {
        const int j = M - 1 - r;
        uint16_t* lo16 = Rh + 2 * (7 * ((j & 1) * MH + (j >> 1)) + 3 * c);
        uint16_t* hi16 = Rh + 2 * (7 * (((j - 1) & 1) * MH + ((j - 1) >> 1)) + 3 * c) + 1;
        const uint16_t v = w & 0xFF, lo = (w >> 8) & 0xFF, hi = (w >> 16) & 0xFF;
        lo16[0] = v; lo16[2] = lo; lo16[4] = hi;
        hi16[0] = v; hi16[2] = lo; hi16[4] = hi;
    };
    auto stage_store = [&](uint32_t* S) {
        uint32_t* o = S + 6 * kl + 3 * cl;
        o[0] = (wl & 0xFFu) * 0x10001u; o[1] = ((wl >> 8) & 0xFFu) * 0x10001u; o[2] = ((wl >> 16) & 0xFFu) * 0x10001u;
        uint16_t* Rh = (uint16_t*)(S + 6 * NX);
        put_right(Rh, cr0, r0, wr0);
        if (has1) put_right(Rh, cr1, r1, wr1);
    };
    // P + ring + V: staged column kc, pairs tq*I .. tq*I + I - 1; the last R rows of P in
    // registers, slot v mod R picked by a uniform switch (static register indices, one copy of
    // the row code)
    const int kc = t / TPC, tq = t % TPC;
    // the thread's first right-entry word of staging buffer 0 (loop-invariant, kept opaque so the
    // per-row reads are one base add + ds_read2 immediates, not one add per read: the folded
    // 6*NX*4-byte constant had pushed every read2 offset out of its 1020-byte range)
    int rk_off = 6 * NX + 7 * (((M - DC - kc + 2 * tq * I) & 1) * MH + ((M - DC - kc + 2 * tq * I) >> 1));
    asm volatile("" : "+v"(rk_off));
    // a pixel cost is <= 2*ftzero + 63 <= 255 (the launcher's condition), so the ring keeps
    // bytes, two disparity pairs per register
    constexpr int RQ = I / 2;
    uint32_t ring[RQ][R];
    uint32_t Vs[I];
#pragma unroll
    for (int q = 0; q < I; q++) Vs[q] = 0;
#pragma unroll
    for (int q = 0; q < RQ; q++)
#pragma unroll
        for (int s2 = 0; s2 < R; s2++) ring[q][s2] = 0;
    // ring slot 0 in LDS for wide boxes (each thread its own words: no barrier; read and written
    // once every R rows): at <= 128 VGPRs hipcc spilled that slot to scratch, whose reload put a
    // vmcnt(0) wait (the row's C' stores and BT loads) into every R-th row
    constexpr bool kRing0Lds = fuse_ring0_words(R, DPC) > 0;
    uint32_t* ring0 = lds_fuse + NBUF * fz.stage_words() + NBUF * kFuseNX * DPC + t;
    if constexpr (kRing0Lds) {
#pragma unroll
        for (int q = 0; q < RQ; q++) ring0[q * kFuseThreads] = 0;
    }
    auto sat = [](u16x2_t a, u16x2_t b) { return __builtin_elementwise_sub_sat(a, b); };
    auto wd = [](const uint32_t* p, int o) { return __builtin_bit_cast(u16x2_t, p[o]); };
    // box: thread (segment, pair); NB box threads, L outputs per segment, the NL = L + R - 1
    // window values of a segment read from LDS at once (one wait, not one per output)
    constexpr int NB = R <= 9 ? kFuseThreads : kFuseHalf;    // every wave for small boxes, else waves 0-3
    constexpr int NSEG = NB / DPC;
    constexpr int L = (kFuseNX - (R - 1) + NSEG - 1) / NSEG;
    constexpr int NL = L + R - 1;
    const int nout = min(XB, gw1 - x0);
    const int klo = max(SW2 - x0, 0), khi = min(gw1 - 1 - x0 + SW2, NX - 1);
    const bool edge = klo > 0 || khi < NX - 1;               // uniform: strips at the frame's sides
    const int bp = t % DPC, bseg = t / DPC;
    const int xa = bseg * L, xb = min(xa + L, nout);
    // the last chunk of a frame whose D is not a multiple of DC holds pairs past D: computed
    // (their right entries clamp inside the row) but never stored nor flagged
    const bool pok = d0 + 2 * bp < gD;
    u16x2_t bmax = {0, 0};                                   // flag: the largest box sum seen
    const bool col0 = (gcompat & SGM_OCV_COL0_LEGACY) && x0 == 0;
    const u16x2_t p2v = {(unsigned short)gP2, (unsigned short)gP2};
    uint32_t* C32 = (uint32_t*)C;
    const size_t rowC = (size_t)gw1 * gD / 2;         // u32 per C' row
    const bool last_band = y1 == fg_ncomp;
    int v_cur = 0;                                           // the row of the loop below
    if (t >= kFuseHalf) {
        for (int r = 0; r < RB && r < nv; r++) {
            stage_load(r);
            stage_store(Sbuf(r));
        }
        if (RB < nv) stage_load(RB);
    }
    __syncthreads();
    auto box_load = [&](u16x2_t (&w)[NL]) __attribute__((always_inline)) {
        const uint32_t* Vp = V0 + ((v_cur - RB) % NBUF) * NX * DPC + bp;
        if (edge) {                                          // staged columns outside the frame: the edge column
#pragma unroll
            for (int i = 0; i < NL; i++) w[i] = wd(Vp, min(max(xa + i, klo), khi) * DPC);
        } else {
#pragma unroll
            for (int i = 0; i < NL; i++) {
                // only the last segment's window passes the staged row (L * NSEG >= XB)
                const int k = i > NX - 1 - (NSEG - 1) * L ? min(xa + i, NX - 1) : xa + i;
                w[i] = wd(Vp, k * DPC);
            }
        }
    };
    int slot = 0;
    for (int v = 0; v < nv + RB; v++) {
        v_cur = v;
        uint32_t* S = Sbuf(v);
        // the box of row v - RB (its V written RB iterations ago, a barrier between)
        const bool dobox = t < NB && v >= RB && v - RB >= 2 * SH2 && xa < xb;
        u16x2_t w[NL];
        if (v < nv) {
            const uint32_t* Lk = S + 6 * kc;
            u16x2_t u[2], ulo[2], uhi[2];
#pragma unroll
            for (int c = 0; c < 2; c++) { u[c] = wd(Lk, 3 * c); ulo[c] = wd(Lk, 3 * c + 1); uhi[c] = wd(Lk, 3 * c + 2); }
            const uint32_t* Rk = S + rk_off;
            uint32_t P[I];
            // kPipe: the right entries of pair q + 1 read from LDS before pair q's arithmetic (else
            // hipcc issues each pair's reads just before their use), for boxes wider than 9 (already
            // at 128 VGPRs: shipped block 21 cost 1.856 -> 1.838 ms; at 1080p block 5 it took 128 ->
            // 155 VGPRs, one block per CU, 0.206 -> 0.256 ms; profiles/r06_ocv_cost_pipe_ab.jsonl)
            constexpr bool kPipe = R > 9;
            u16x2_t rw[2][6];
            auto rload = [&](int q, u16x2_t (&r)[6]) {
#pragma unroll
                for (int k = 0; k < 6; k++) r[k] = wd(Rk, 7 * q + k);
            };
            if constexpr (kPipe) {
                rload(0, rw[0]);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int q = 0; q < I; q++) {
                if constexpr (kPipe) {
                    if (q + 1 < I) rload(q + 1, rw[(q + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    rload(q, rw[q & 1]);
                }
                const u16x2_t (&r)[6] = rw[q & 1];
                u16x2_t m[2];
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    const u16x2_t vv = r[3 * c], v0 = r[3 * c + 1], v1 = r[3 * c + 2];
                    const u16x2_t c0 = __builtin_elementwise_max(sat(u[c], v1), sat(v0, u[c]));
                    const u16x2_t c1 = __builtin_elementwise_max(sat(vv, uhi[c]), sat(ulo[c], vv));
                    m[c] = __builtin_elementwise_min(c0, c1);
                }
                P[q] = __builtin_bit_cast(uint32_t, m[0] + (m[1] >> (u16x2_t){2, 2}));
                if constexpr (kPipe) __builtin_amdgcn_sched_barrier(0);
            }
            auto upd = [&](auto ss) {
                constexpr int s2 = decltype(ss)::value;
                auto vupd = [&](int q, uint32_t old) {
                    Vs[q] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2_t, Vs[q]) + __builtin_bit_cast(u16x2_t, P[q]) -
                                                         __builtin_bit_cast(u16x2_t, old));
                };
#pragma unroll
                for (int h = 0; h < RQ; h++) {
                    const uint32_t o = (kRing0Lds && s2 == 0) ? ring0[h * kFuseThreads] : ring[h][s2];
                    vupd(2 * h, __builtin_amdgcn_perm(o, o, 0x0C010C00u));       // bytes 0, 1 -> u16 lanes
                    vupd(2 * h + 1, __builtin_amdgcn_perm(o, o, 0x0C030C02u));   // bytes 2, 3
                    const uint32_t nw = __builtin_amdgcn_perm(P[2 * h + 1], P[2 * h], 0x06040200u);
                    if (kRing0Lds && s2 == 0) ring0[h * kFuseThreads] = nw;
                    else ring[h][s2] = nw;
                }
            };
            switch (slot) {
#define SGM_RING_CASE(n) case n: if constexpr (n < R) upd(std::integral_constant<int, n>{}); break;
            SGM_RING_CASE(0) SGM_RING_CASE(1) SGM_RING_CASE(2) SGM_RING_CASE(3) SGM_RING_CASE(4) SGM_RING_CASE(5)
            SGM_RING_CASE(6) SGM_RING_CASE(7) SGM_RING_CASE(8) SGM_RING_CASE(9) SGM_RING_CASE(10) SGM_RING_CASE(11)
            SGM_RING_CASE(12) SGM_RING_CASE(13) SGM_RING_CASE(14) SGM_RING_CASE(15) SGM_RING_CASE(16)
            SGM_RING_CASE(17) SGM_RING_CASE(18) SGM_RING_CASE(19) SGM_RING_CASE(20)
#undef SGM_RING_CASE
            default: break;
            }
            slot = slot + 1 == R ? 0 : slot + 1;
            if (v >= 2 * SH2) {
                uint32_t* Vout = V0 + (v % NBUF) * NX * DPC + kc * DPC + tq * I;
                // exactly the thread's I words (I = 2 at DPC = 8: one 8-byte store, 8-byte aligned)
                if constexpr (I % 4 == 0) {
#pragma unroll
                    for (int q = 0; q < I; q += 4) *(uint4*)(Vout + q) = make_uint4(Vs[q], Vs[q + 1], Vs[q + 2], Vs[q + 3]);
                } else {
                    static_assert(I % 2 == 0, "pairs of words per thread");
#pragma unroll
                    for (int q = 0; q < I; q += 2) *(uint2*)(Vout + q) = make_uint2(Vs[q], Vs[q + 1]);
                }
            }
        }
        if (dobox) {                                         // the box of row v - RB
            const int y = y0 + (v - RB) - 2 * SH2;
            const bool tail = last_band && y == fg_ncomp - 1;
            box_load(w);
            // the window sum starts at P2, so the slid sum IS C' (mod 2^16, OpenCV's CostType wrap)
            u16x2_t sum = w[0] + p2v;
#pragma unroll
            for (int i = 1; i < R; i++) sum += w[i];
            // 32-bit element offsets off the uniform C' base (C' < 2^32 words: the launcher's
            // condition)
            const uint32_t ob = (uint32_t)y * (uint32_t)rowC + (uint32_t)(((x0 + xa) * gD + d0) / 2 + bp);
            // stores through a descriptor of the row (wave-uniform base, SGPRs): the lane's byte
            // offset in one VGPR and output j's step as the scalar offset, no per-store VALU
            const __amdgpu_buffer_rsrc_t crow = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(C32 + (size_t)y * rowC), 0, (int)(rowC * 4), 0x00020000);
            const uint32_t vb = 4u * (uint32_t)(((x0 + xa) * gD + d0) / 2 + bp);
            if constexpr (R <= kFuseBufSt) {
                // branch-free: an output past the segment's end goes to an offset past the range,
                // where the hardware drops it, and the flag's max is a select (1080p block 5 cost
                // 0.210 -> 0.204 ms; at R = 21 the same form measured 2.00 against 1.97 for the
                // branches below, and the branches with descriptor stores 2.02: profiles/
                // r05_ocv_cost_box_ab.jsonl, r05_ocv_cost_box2_ab.jsonl)
                const int nj = xb - xa;                      // outputs of the segment (> 0)
                const bool skip0 = col0 && xa == 0 && y > 0; // COL0_LEGACY's column: not in the flag
#pragma unroll
                for (int j = 0; j < L; j++) {
                    if (j > 0) sum += w[j + R - 1] - w[j - 1];
                    const bool ok = j < nj && pok;
                    if constexpr (TRK != 0) {
                        const u16x2_t cand = __builtin_elementwise_max(bmax, TRK == 1 ? sum : sum - p2v);
                        bmax = (ok && !(j == 0 && skip0)) ? cand : bmax;
                    }
                    __builtin_amdgcn_raw_buffer_store_b32(as_u(sum), crow, ok ? (int)vb : (int)kFuseDrop, j * gD * 2, 0);
                }
            } else {
#pragma unroll
                for (int j = 0; j < L; j++) {
                    if (j > 0) sum += w[j + R - 1] - w[j - 1];
                    if (xa + j < xb && pok) {
                        if constexpr (TRK != 0)
                            if (!(col0 && xa + j == 0 && y > 0))
                                bmax = __builtin_elementwise_max(bmax, TRK == 1 ? sum : sum - p2v);
                        C32[ob + (uint32_t)(j * (gD / 2))] = as_u(sum);
                    }
                }
            }
            if (tail) {                                      // OpenCV's bottom rows: never recomputed
                // (the row's values slid again from the registers: reading the stores back would
                // put a vmcnt(0) wait into every row of the loop)
                sum = w[0] + p2v;
#pragma unroll
                for (int i = 1; i < R; i++) sum += w[i];
                uint32_t* o = C32 + ob;
#pragma unroll
                for (int j = 0; j < L; j++) {
                    if (j > 0) sum += w[j + R - 1] - w[j - 1];
                    const uint32_t c = fullDP ? gP2 * 0x10001u : as_u(sum);
                    if (xa + j < xb && pok)
                        for (int yy = y + 1; yy < gH; yy++) o[(size_t)(yy - y) * rowC] = c;
                    o += gD / 2;
                }
            }
        }
        if (t >= kFuseHalf && v + RB < nv) {
            stage_store(Sbuf(v + RB));
            if (v + RB + 1 < nv) stage_load(v + RB + 1);
        }
        // every write of iteration v is read RB iterations later and every buffer is rewritten
        // 2 * RB iterations after its reads: one barrier per RB iterations orders both
        if ((v + 1) % RB == 0) __syncthreads();
    }
    if (TRK != 0 && govf && t < NB) {
        const int m = max((int)bmax[0], (int)bmax[1]) - (TRK == 1 ? gP2 : 0);
        const bool ovf = m > govf_thr - gP2;
        const uint64_t b = __ballot(ovf);
        if (b && (int)(threadIdx.x & 63) == __builtin_ctzll(b)) atomicOr(govf, 1);
    }
}

// COL0_LEGACY after the fused cost: column x1 = 0 of rows y >= 1 holds row 0's value (MODE_SGBM's
// single C row is never updated there) or the P2 initialisation (MODE_HH)
__global__ __launch_bounds__(256) void k_ocv_col0_legacy(Geom g, int fullDP, int16_t* __restrict__ C)
{
    const int np = g.D / 2;                               // u32 pairs of column 0
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (g.H - 1) * np) return;
    const int y = 1 + i / np, pr = i - (y - 1) * np;
    uint32_t* C32 = (uint32_t*)C;
    C32[(size_t)y * g.width1 * np + pr] = fullDP ? ((uint32_t)g.P2 & 0xFFFFu) * 0x10001u : C32[pr];
}

// The SIMD_SAT flagged frames whose horizontal sums cannot saturate: when
// (2*SW2 + 1) * (2*ftzero + 63) <= 32767 every running horizontal sum of the SIMD loop stays in
// int16 (it is a box of pixel costs <= 2*ftzero + 63, and (h - sub) + add never leaves
// [-maxP, 32767]), so the plain horizontal sums hs (k_ocv_pixhsum) ARE the SIMD branch's and only
// the vertical update saturates: C_y = sat(sat(C_{y-1} - hs[y-SH2-1]) + hs[y+SH2]). That chain is
// sequential per (column, d), so a thread owns a pair of adjacent disparities (packed saturating
// i16 ops, v_pk_sub_i16 / v_pk_add_i16 with clamp) and walks every row; the grid covers
// width1 * D / 2 pairs (437 K threads at the shipped 2448x2048 D=480 config). Each hs row is read
// from HBM once, as it enters the window, U rows ahead of the chain, and kept in the thread's
// LDS ring (R = 2*SH2 + 1 slots) until it leaves: 2 B read + 2 B written per cell. The old
// k_ocv_pixcost_sat / k_ocv_hsum_sat / k_ocv_vsum_sat chain (one int16 per thread, no prefetch)
// stays for the configs whose horizontal sums can saturate (boxes wider than ~171 columns).
__host__ __device__ inline bool ocv_hsum_cannot_saturate(const Geom& g)
{
    return (2 * g.SW2 + 1) * (2 * g.ftzero + 63) <= 32767;
}
__host__ inline int vsum_sat2_unroll(const Geom& g)
{
    const int R = 2 * g.SH2 + 1;
    return R >= 8 ? 8 : R >= 4 ? 4 : R >= 2 ? 2 : 1;
}
template <int U>
__global__ __launch_bounds__(256) void k_ocv_vsum_sat2(const int16_t* __restrict__ hs, Geom g, int fullDP,
                                                       int16_t* __restrict__ C)
{
    if (!ocv_flagged(g)) return;
    extern __shared__ uint32_t ring_sat[];                 // [R][256]: slot s of thread t at s * 256 + t
    const int t = threadIdx.x, i = blockIdx.x * 256 + t;
    const size_t rs = (size_t)g.width1 * g.D / 2;           // u32 pairs per row
    if (i >= (int)rs) return;                               // no barriers below: the ring is per thread
    const uint32_t* h32 = (const uint32_t*)hs;
    uint32_t* C32 = (uint32_t*)C;
    const int H = g.H, SH2 = g.SH2, R = 2 * SH2 + 1;
    uint32_t* ring = ring_sat + t;
    auto lo16 = [](uint32_t w) { return (int)(int16_t)(uint16_t)w; };
    auto hi16 = [](uint32_t w) { return (int)w >> 16; };
    auto S = [](uint32_t w) { return __builtin_bit_cast(s16x2_t, w); };
    // row 0: P2 + the clamped window, int sums wrapped to int16 (the scalar y == 0 loop)
    int s0 = 0, s1 = 0;
    for (int k = 0; k <= SH2; k++) {
        const uint32_t w = h32[(size_t)min(k, H - 1) * rs + i];
        if (k < H) ring[k * 256] = w;                       // rows 0 .. SH2 enter the ring (k < R)
        const int m = k == 0 ? SH2 + 1 : 1;                 // row 0 weighs SH2 + 1 (clamped rows above)
        s0 += m * lo16(w); s1 += m * hi16(w);
    }
    uint32_t c = ((uint32_t)(g.P2 + s0) & 0xFFFFu) | ((uint32_t)(g.P2 + s1) << 16);
    C32[i] = c;
    const bool col0 = (g.compat & SGM_OCV_COL0_LEGACY) && i < g.D / 2;
    const uint32_t p2w = ((uint32_t)g.P2 & 0xFFFFu) * 0x10001u;
    const int ylast = H - SH2 - 1;                           // rows y <= ylast add row y + SH2
    // ring slot of row y - SH2 - 1 (= the slot row y + SH2 takes: they are R rows apart), kept
    // as a running counter (no modulo in the loop); rows y <= SH2 subtract row 0 (slot 0) and
    // add row y + SH2 < R into slot y + SH2
    int q0 = (R - SH2) % R;                                  // its value at y = 1
    for (int yb = 1; yb < H; yb += U) {
        uint32_t add[U], sub[U];
        int slot[U];
#pragma unroll
        for (int u = 0; u < U; u++) {                        // entering rows (clamped: used only if y <= ylast)
            const int y = yb + u;
            int q = q0 + u;
            q = q >= R ? q - R : q;                          // U <= R
            slot[u] = y <= SH2 ? y + SH2 : q;
            add[u] = h32[(size_t)min(y + SH2, H - 1) * rs + i];
            sub[u] = ring[(y <= SH2 ? 0 : q) * 256];         // leaving rows: none of this group's (U <= R)
        }
        q0 += U;
        q0 = q0 >= R ? q0 - R : q0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int y = yb + u;
            if (y >= H) break;
            if (y <= ylast) {
                if (!col0)
                    c = __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(
                            __builtin_elementwise_sub_sat(S(c), S(sub[u])), S(add[u])));
                else if (fullDP)
                    c = p2w;
                ring[slot[u] * 256] = add[u];
            } else if (fullDP) {
                c = p2w;                                     // MODE_HH: never recomputed, the P2 init
            }                                                // MODE_SGBM: the last computed row
            C32[(size_t)y * rs + i] = c;
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------
// The fused cost applies: R = 2*SH2 + 1 <= 21 (the register ring; SH2 <= 10 leaves XB >= 108 of
// the 128 staged columns) and every sum exact in u16.
__host__ inline bool ocv_cost_fusable(const Geom& g)
{
    const long long B = (long long)(2 * g.SW2 + 1) * (2 * g.SH2 + 1) * (2 * g.ftzero + 63);
    const char* e = std::getenv("SGM_OCV_FUSED");
    // default: frames with enough tiles x bands to fill the chip (10^8 cells: C1 measured 0.10
    // fused vs 0.053 ms; 1080p block 5 0.29 vs 0.42, the shipped block-21 config 3.18 vs 3.79 ms,
    // profiles/r04_ocv_cost_box_ab.jsonl)
    const bool dflt = (double)g.width1 * g.H * g.D >= 1e8;
    return g.SH2 <= 10 && g.SW2 == g.SH2 && B <= 65535 && 2 * g.ftzero + 63 <= 255 &&
           (double)g.W * g.H * 4 < 4294967296.0 && (double)g.width1 * g.H * g.D / 2 < 4294967296.0 && g.width1 > 0 && (e ? std::atoi(e) != 0 : dflt);
}

// Disparity pairs per block row (DC = 2 * DPC disparities): 32 only for R <= 9 (its I = 8
// pairs per thread keep 8 R-slot rings in registers), else 16, or 8 (I = 2: 95 VGPRs at R = 21
// against 165 for 16, i.e. two blocks per CU instead of one); SGM_FUSE_DPC forces one.
static int fuse_dpc(const Geom& g)
{
    const int R = 2 * g.SH2 + 1;
    // D % 32 == 16 from D = 256 on: 16 pairs with a half-empty last chunk (<= 6 % of the pixel-cost
    // work wasted) beat 8 pairs, whose blocks stage the same BT rows for half the disparities (the
    // processing launch's D = 752 block 21: profiles/r06_ocv_cost_dpc_ab.jsonl)
    int dpc = (R <= 9 && g.D % 64 == 0) ? 32 : (g.D % 32 == 0 || g.D >= 256) ? 16 : 8;
    if (const char* e = std::getenv("SGM_FUSE_DPC")) {
        const int f = std::atoi(e);
        if ((f == 32 && R <= 9 && g.D % 64 == 0) || f == 16 || f == 8) dpc = f;
    }
    return dpc;
}

// The overflow flag's tracking (k_ocv_cost_fused's TRK): none without the gate (Geom::wide != 2);
// the max of C' when box + P2 stays below 2^16 for any pixels (a pixel cost is <= 2*ftzero + 63),
// so the slid sum that starts at P2 is compared as it is stored; else the max of C' - P2
static int ocv_fuse_track(const Geom& g)
{
    if (g.wide != 2) return 0;
    const long long B = (long long)(2 * g.SW2 + 1) * (2 * g.SH2 + 1) * (2 * g.ftzero + 63);
    return B + g.P2 <= 65535 ? 1 : 2;
}

template <int R, int TRK>
static void launch_cost_fused_rt(const uint32_t* bt, const Geom& g, int fullDP, const FuseGrid& fg, int16_t* C,
                                 hipStream_t st)
{
    const dim3 grid(fg.per_xcd * 8), block(kFuseThreads);
    const int dpc = fuse_dpc(g);
    if constexpr (R <= 9) {
        if (dpc == 32) {
            hipLaunchKernelGGL((k_ocv_cost_fused<R, 32, 8, TRK>), grid, block, FuseGeo(32).lds_bytes(32, fuse_rb(R), R), st, bt, g,
                               fullDP, fg, C);
            return;
        }
    }
    // blocks above 64 KB of LDS (R > 9: two rows per barrier plus ring slot 0) ask for it
    auto allow = [](const void* k, size_t lds) {
        if (lds > 65536) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    };
    if (dpc == 16) {
        const size_t lds = FuseGeo(16).lds_bytes(16, fuse_rb(R), R);
        allow(reinterpret_cast<const void*>(&k_ocv_cost_fused<R, 16, 4, TRK>), lds);
        hipLaunchKernelGGL((k_ocv_cost_fused<R, 16, 4, TRK>), grid, block, lds, st, bt, g, fullDP, fg, C);
    } else {
        const size_t lds = FuseGeo(8).lds_bytes(8, fuse_rb(R), R);
        allow(reinterpret_cast<const void*>(&k_ocv_cost_fused<R, 8, 2, TRK>), lds);
        hipLaunchKernelGGL((k_ocv_cost_fused<R, 8, 2, TRK>), grid, block, lds, st, bt, g, fullDP, fg, C);
    }
}

template <int R>
static void launch_cost_fused_r(const uint32_t* bt, const Geom& g, int fullDP, const FuseGrid& fg, int16_t* C,
                                hipStream_t st)
{
    switch (ocv_fuse_track(g)) {
    case 0: launch_cost_fused_rt<R, 0>(bt, g, fullDP, fg, C, st); break;
    case 1: launch_cost_fused_rt<R, 1>(bt, g, fullDP, fg, C, st); break;
    default: launch_cost_fused_rt<R, 2>(bt, g, fullDP, fg, C, st); break;
    }
}

static FuseGrid fuse_grid(const Geom& g)
{
    FuseGrid fg{};
    const int dpc = fuse_dpc(g);
    const int XB = fuse_xb(g);
    fg.strips = (g.width1 + XB - 1) / XB;
    fg.chunks = (g.D + 2 * dpc - 1) / (2 * dpc);   // the last one partly past D when 2 * dpc does not divide D
    fg.ncomp = std::max(g.H - g.SH2 - 1, 0) + 1;             // rows 0 .. ylast are computed
    const long long tiles = (long long)fg.strips * fg.chunks;
    // bands: about four rounds of blocks over the chip's slots (two 512-thread blocks per CU, every
    // instantiation at <= 128 VGPRs), bands of about max(64, 8*SH2) rows or more so the 2*SH2
    // warm-up rows stay a small share. Measured (profiles/r04_ocv_cost_rows_ab.jsonl): the shipped block-21
    // config 2.43 ms at the earlier ~ncomp*tiles/1024 rows (507: 1275 blocks, 2.5 rounds) against
    // 2.06 at 256 rows (2040 blocks), 2.10-2.11 at 128-160; 1080p block 5 best at 64 rows
    // slot count of the calling thread's current device, cached per device (launches run from
    // several host threads at once: per-device atomics, each written with the same value)
    static std::atomic<int> slots_of[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    int slots = dev < 64 ? slots_of[dev].load(std::memory_order_relaxed) : 0;
    if (!slots) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        slots = (2 * 128 / kFuseNX) * cus;             // 512-thread blocks: two per CU
        if (dev < 64) slots_of[dev].store(slots, std::memory_order_relaxed);
    }
    const int min_rows = std::max(64, 8 * g.SH2);
    const long long nb = std::max<long long>(1, std::min<long long>((4LL * slots + tiles / 2) / std::max(tiles, 1LL),
                                                                    (fg.ncomp + min_rows - 1) / min_rows));
    const char* e = std::getenv("SGM_FUSE_ROWS");
    fg.band_rows = e ? std::max(std::atoi(e), 1) : (int)((fg.ncomp + nb - 1) / nb);
    fg.bands = (fg.ncomp + fg.band_rows - 1) / fg.band_rows;
    fg.total = (int)(tiles * fg.bands);
    fg.per_xcd = (fg.total + 7) / 8;
    return fg;
}

// C' of the frame into bufA (bufB: scratch, the horizontal sums of the unfused kernels).
// Default: k_ocv_prefilter (with the BT planes) + k_ocv_cost_fused (+ k_ocv_col0_legacy) when ocv_cost_fusable, else
// k_ocv_pixhsum (or k_ocv_pixcost + k_ocv_hsum) + k_ocv_vsum_seg. SIMD_SAT frames that take the
// flagged kernels (Geom::wide != 0 and the overflow flag) get the exact SIMD cost written over
// it, by kernels that return at once on the other frames: the vertical SIMD update over the
// plain horizontal sums (k_ocv_vsum_sat2; after the fused cost, a gated k_ocv_pixhsum makes
// those sums first) when the horizontal sums cannot saturate, else the sequential chain
// (pixel costs -> bufA, horizontal sums -> bufB, C' -> bufA).
// The frame's cost stage takes k_ocv_cost_fused (and so reads the packed BT planes after the
// prefilter planes): the workspace layout reserves those 16 B/px only then.
// wide == 1 with SIMD_SAT: every launch after the cost reads the SIMD cost, the plain C' is never used.
bool ocv_cost_takes_fused(const Geom& g)
{
    const bool simd_only = g.wide == 1 && (g.compat & SGM_OCV_SIMD_SAT);
    return !simd_only && ocv_cost_fusable(g);
}

hipError_t launch_ocv_cost(const uint8_t* L, const uint8_t* R, size_t stride, const Geom& g, int fullDP,
                           uint8_t* planes, int16_t* bufA, int16_t* bufB, hipStream_t st)
{
    const size_t lds = pix_lds_bytes(g);
    const bool simd_only = g.wide == 1 && (g.compat & SGM_OCV_SIMD_SAT);
    const bool fused = ocv_cost_takes_fused(g);
    uint32_t* bt = fused ? (uint32_t*)(planes + ocv_planes_bytes(g.W, g.H)) : nullptr;
    hipLaunchKernelGGL(k_ocv_prefilter, dim3((g.W + 1023) / 1024, g.H, 2), dim3(256), 0, st, L, R, stride, g.W, g.H,
                       g.ftzero, planes, bt);
    const bool sat2 = g.wide && (g.compat & SGM_OCV_SIMD_SAT) && ocv_hsum_cannot_saturate(g) && lds <= 64 * 1024 &&
                      (size_t)(2 * g.SH2 + 1) * 256 * 4 <= 64 * 1024 && !std::getenv("SGM_OCV_SAT_SEQ");
    if (simd_only) {
        if (sat2) {                    // the horizontal sums for k_ocv_vsum_sat2
            const int XB = pix_xb(g), DC = pix_dc(g);
            hipLaunchKernelGGL(k_ocv_pixhsum<true>, dim3((g.width1 + XB - 1) / XB, g.H, (g.D + DC - 1) / DC), dim3(256),
                               lds, st, planes, g, bufB);
        }
    } else if (fused) {
        const FuseGrid fg = fuse_grid(g);
        switch (g.SH2) {
        case 0: launch_cost_fused_r<1>(bt, g, fullDP, fg, bufA, st); break;
        case 1: launch_cost_fused_r<3>(bt, g, fullDP, fg, bufA, st); break;
        case 2: launch_cost_fused_r<5>(bt, g, fullDP, fg, bufA, st); break;
        case 3: launch_cost_fused_r<7>(bt, g, fullDP, fg, bufA, st); break;
        case 4: launch_cost_fused_r<9>(bt, g, fullDP, fg, bufA, st); break;
        case 5: launch_cost_fused_r<11>(bt, g, fullDP, fg, bufA, st); break;
        case 6: launch_cost_fused_r<13>(bt, g, fullDP, fg, bufA, st); break;
        case 7: launch_cost_fused_r<15>(bt, g, fullDP, fg, bufA, st); break;
        case 8: launch_cost_fused_r<17>(bt, g, fullDP, fg, bufA, st); break;
        case 9: launch_cost_fused_r<19>(bt, g, fullDP, fg, bufA, st); break;
        default: launch_cost_fused_r<21>(bt, g, fullDP, fg, bufA, st); break;
        }
        if ((g.compat & SGM_OCV_COL0_LEGACY) && g.H > 1)
            hipLaunchKernelGGL(k_ocv_col0_legacy, dim3(((g.H - 1) * (g.D / 2) + 255) / 256), dim3(256), 0, st, g, fullDP,
                               bufA);
        if (sat2) {                    // the flagged frames' horizontal sums for k_ocv_vsum_sat2
            const int XB = pix_xb(g), DC = pix_dc(g);
            hipLaunchKernelGGL(k_ocv_pixhsum<true>, dim3((g.width1 + XB - 1) / XB, g.H, (g.D + DC - 1) / DC), dim3(256),
                               lds, st, planes, g, bufB);
        }
    } else {
        if (lds <= 64 * 1024) {
            const int XB = pix_xb(g), DC = pix_dc(g);
            hipLaunchKernelGGL(k_ocv_pixhsum<false>, dim3((g.width1 + XB - 1) / XB, g.H, (g.D + DC - 1) / DC), dim3(256),
                               lds, st, planes, g, bufB);
        } else {            // very wide boxes x wide ranges: the unfused pair (no LDS staging)
            hipLaunchKernelGGL(k_ocv_pixcost, dim3(g.width1, g.H), dim3(256), 0, st, planes, g, bufA);
            hipLaunchKernelGGL(k_ocv_hsum, dim3((g.D + 255) / 256, g.H), dim3(256), 0, st, bufA, g, bufB);
        }
        hipLaunchKernelGGL(k_ocv_vsum_seg, dim3((g.width1 * g.D / 2 + 255) / 256, (g.H + kVsumRows - 1) / kVsumRows),
                           dim3(256), 0, st, bufB, g, fullDP, bufA);
    }
    if (g.wide && (g.compat & SGM_OCV_SIMD_SAT)) {
        const size_t rc = (size_t)g.width1 * g.D;
        if (sat2) {
            const size_t ring = (size_t)(2 * g.SH2 + 1) * 256 * 4;
            const dim3 grid((unsigned)((rc / 2 + 255) / 256));
            switch (vsum_sat2_unroll(g)) {
            case 8: hipLaunchKernelGGL(k_ocv_vsum_sat2<8>, grid, dim3(256), ring, st, bufB, g, fullDP, bufA); break;
            case 4: hipLaunchKernelGGL(k_ocv_vsum_sat2<4>, grid, dim3(256), ring, st, bufB, g, fullDP, bufA); break;
            case 2: hipLaunchKernelGGL(k_ocv_vsum_sat2<2>, grid, dim3(256), ring, st, bufB, g, fullDP, bufA); break;
            default: hipLaunchKernelGGL(k_ocv_vsum_sat2<1>, grid, dim3(256), ring, st, bufB, g, fullDP, bufA); break;
            }
        } else {
            hipLaunchKernelGGL(k_ocv_pixcost_sat, dim3(std::min(g.width1 * g.H, 8192)), dim3(256), 0, st, planes, g, bufA);
            hipLaunchKernelGGL(k_ocv_hsum_sat, dim3((g.D + 255) / 256, g.H), dim3(256), 0, st, bufA, g, bufB);
            hipLaunchKernelGGL(k_ocv_vsum_sat, dim3((unsigned)((rc + 255) / 256)), dim3(256), 0, st, bufB, g, fullDP, bufA);
        }
    }
    return hipGetLastError();
}

}  // namespace sgm
