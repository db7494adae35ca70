// fill.hip — the hole-filling post filter (sgm_set_fill_params, stage `fill`): a bounded
// 8-direction nearest-valid interpolation of the final int16 disparity. Specified by this project
// (tests/fill_reference.py is the numpy statement), integer and order-independent, bit-exact.
//
// For a hole p (in == invalid, inside the fill rectangle) each of the 8 directions contributes the
// first pixel within max_gap steps that lies in the image and is not invalid; the result is the
// second-lowest (BACKGROUND) or the lower median (MEDIAN) of those candidates, or invalid when
// fewer than min_neighbours exist. Every candidate is read from the input.
//
// Shape (k_fill): the nearest valid value along a direction is a carry
//   near_r(p) = valid(p - r) ? (in[p - r], 1) : (near_r(p - r).value, age + 1), dropped past age G,
// so a scan that starts G steps ahead of a pixel reproduces its carry exactly, and the frame is cut
// into independent blocks: BW output columns x BH output rows, one thread per column of the block's
// T = BW + 2G column span (G halo columns each side). The block marches down from G rows above its
// band with the three carries from above (vertical in the thread, the two diagonals handed one
// thread sideways through LDS each row), parks the three candidates of every hole in three int16
// planes, then marches up from G rows below with the three carries from below; on the way up each
// output row also takes its left / right candidates from the row staged in LDS (values + one
// validity bit mask per wave), sorts the eight with a fixed compare-exchange network and writes the
// pixel. A thread reads back only plane cells that it wrote itself. No flags, no atomics, nothing
// crosses a workgroup.
#include <algorithm>

#include "sgm_device.h"
#include "sgm_launch.h"

namespace sgm {

namespace {

constexpr int kFillNone = 0x7FFFFFFF;   // "no candidate": sorts behind every int16
constexpr int kFillMaxT = 1024;

struct FillArgs {
    const int16_t* src; size_t sstride;
    int16_t* dst; size_t dstride;
    int16_t* planes; size_t plane_elems;   // three W x H planes (row stride W)
    int W, H, invalid, mode, G, N;
    int x0, y0, x1, y1;
    int BW, BH;
};

// a carry: the value in the low 16 bits, its age (0 = none) above
__device__ __forceinline__ unsigned carry_of(int a) { return ((unsigned)a & 0xFFFFu) | (1u << 16); }
__device__ __forceinline__ unsigned carry_step(unsigned c, int a, bool valid, int G)
{
    if (valid) return carry_of(a);
    const unsigned age = c >> 16;
    return (age == 0 || (int)age >= G) ? 0u : c + (1u << 16);
}
__device__ __forceinline__ int carry_value(unsigned c) { return (c >> 16) ? (int)(int16_t)(c & 0xFFFFu) : kFillNone; }

__device__ __forceinline__ void cswap(int& a, int& b) { const int t = min(a, b); b = max(a, b); a = t; }

// the selection rule on up to eight candidates (kFillNone = absent); returns `invalid` below N
__device__ __forceinline__ int fill_select(int c0, int c1, int c2, int c3, int c4, int c5, int c6, int c7, int mode,
                                           int N, int invalid)
{
    const int n = (c0 != kFillNone) + (c1 != kFillNone) + (c2 != kFillNone) + (c3 != kFillNone) + (c4 != kFillNone) +
                  (c5 != kFillNone) + (c6 != kFillNone) + (c7 != kFillNone);
    // 19-exchange sorting network of eight
    cswap(c0, c1); cswap(c2, c3); cswap(c4, c5); cswap(c6, c7);
    cswap(c0, c2); cswap(c1, c3); cswap(c4, c6); cswap(c5, c7);
    cswap(c1, c2); cswap(c5, c6); cswap(c0, c4); cswap(c3, c7);
    cswap(c1, c5); cswap(c2, c6);
    cswap(c1, c4); cswap(c3, c6);
    cswap(c2, c4); cswap(c3, c5);
    cswap(c3, c4);
    if (n == 0 || n < N) return invalid;
    const int k = mode == 1 ? (n >= 2 ? 1 : 0) : (n - 1) >> 1;    // second lowest / lower median (k <= 3)
    int v = c0;
    v = k == 1 ? c1 : v;
    v = k == 2 ? c2 : v;
    v = k == 3 ? c3 : v;
    return v;
}

__global__ __launch_bounds__(kFillMaxT) void k_fill(const FillArgs A)
{
    __shared__ unsigned sL[2][kFillMaxT], sR[2][kFillMaxT];   // the diagonal carries of a row, by parity
    __shared__ int16_t sval[2][kFillMaxT];                     // the row's values
    __shared__ unsigned long long smask[2][kFillMaxT / 64];    // ... and one validity mask per wave
    const int T = blockDim.x, tid = threadIdx.x, G = A.G;
    const int c0 = blockIdx.x * A.BW, r0 = blockIdx.y * A.BH;
    const int r1 = min(r0 + A.BH, A.H);
    const int x = c0 - G + tid;
    const bool in_x = x >= 0 && x < A.W;
    const bool out_col = tid >= G && tid < G + A.BW && x < A.W;     // x >= c0 >= 0 there
    const bool rect_x = x >= A.x0 && x < A.x1;
    // blocks the rectangle does not touch (or a plain copy): no sweep
    const bool work = A.mode != 0 && c0 < A.x1 && c0 + A.BW > A.x0 && r0 < A.y1 && r1 > A.y0;
    if (!work) {
        if (out_col)
            for (int y = r0; y < r1; y++) A.dst[(size_t)y * A.dstride + x] = A.src[(size_t)y * A.sstride + x];
        return;
    }
    const int16_t* col = A.src + (in_x ? x : 0);
    int16_t* pU = A.planes + (in_x ? x : 0);
    int16_t* pL = pU + A.plane_elems;
    int16_t* pR = pL + A.plane_elems;

    // ---- down: candidates from above (up, up-left, up-right) of the band's holes into the planes
    {
        const int ys = max(r0 - G, 0);
        unsigned cU = 0, cL = 0, cR = 0;
        int a_next = in_x ? col[(size_t)ys * A.sstride] : A.invalid;
        for (int y = ys; y < r1; y++) {
            const int a = a_next;
            if (y + 1 < r1 && in_x) a_next = col[(size_t)(y + 1) * A.sstride];
            const bool valid = a != A.invalid;
            if (y >= r0 && out_col && !valid && rect_x && y >= A.y0 && y < A.y1) {
                const size_t o = (size_t)y * A.W;
                const int u = carry_value(cU), l = carry_value(cL), r = carry_value(cR);
                pU[o] = (int16_t)(u == kFillNone ? A.invalid : u);
                pL[o] = (int16_t)(l == kFillNone ? A.invalid : l);
                pR[o] = (int16_t)(r == kFillNone ? A.invalid : r);
            }
            const int par = y & 1;
            cU = carry_step(cU, a, valid, G);
            sL[par][tid] = carry_step(cL, a, valid, G);     // what (x + 1, y + 1) sees up-left
            sR[par][tid] = carry_step(cR, a, valid, G);     // what (x - 1, y + 1) sees up-right
            __syncthreads();
            cL = tid > 0 ? sL[par][tid - 1] : 0u;
            cR = tid + 1 < T ? sR[par][tid + 1] : 0u;
        }
    }
    __syncthreads();    // the LDS rows change hands

    // ---- up: candidates from below, the row's left / right ones, selection, output
    {
        const int ye = min(r1 - 1 + G, A.H - 1);
        const int lane = tid & 63, wv = tid >> 6, nw = T >> 6;
        unsigned cD = 0, cL = 0, cR = 0;
        int a_next = in_x ? col[(size_t)ye * A.sstride] : A.invalid;
        for (int y = ye; y >= r0; y--) {
            const int a = a_next;
            if (y > r0 && in_x) a_next = col[(size_t)(y - 1) * A.sstride];
            const bool valid = a != A.invalid;
            const int par = y & 1;
            const bool out_row = y < r1;             // block-uniform
            const unsigned nL = carry_step(cL, a, valid, G), nR = carry_step(cR, a, valid, G);
            sL[par][tid] = nL;                       // what (x + 1, y - 1) sees down-left
            sR[par][tid] = nR;                       // what (x - 1, y - 1) sees down-right
            if (out_row) {
                sval[par][tid] = (int16_t)a;
                const unsigned long long m = __ballot(valid);
                if (lane == 0) smask[par][wv] = m;
            }
            __syncthreads();
            if (out_row && out_col) {
                int v = a;
                if (!valid && rect_x && y >= A.y0 && y < A.y1) {
                    // nearest valid to the left / right within G columns of the staged row
                    int cl = kFillNone, cr = kFillNone;
                    {
                        unsigned long long m = smask[par][wv] & ((1ull << lane) - 1ull);
                        int j = -1;
                        if (m) j = wv * 64 + 63 - __builtin_clzll(m);
                        else
                            for (int k = wv - 1; k >= 0 && tid - (k * 64 + 63) <= G; k--) {
                                m = smask[par][k];
                                if (m) { j = k * 64 + 63 - __builtin_clzll(m); break; }
                            }
                        if (j >= 0 && tid - j <= G) cl = sval[par][j];
                    }
                    {
                        unsigned long long m = lane == 63 ? 0ull : smask[par][wv] & (~0ull << (lane + 1));
                        int j = -1;
                        if (m) j = wv * 64 + __builtin_ctzll(m);
                        else
                            for (int k = wv + 1; k < nw && k * 64 - tid <= G; k++) {
                                m = smask[par][k];
                                if (m) { j = k * 64 + __builtin_ctzll(m); break; }
                            }
                        if (j >= 0 && j - tid <= G) cr = sval[par][j];
                    }
                    const size_t o = (size_t)y * A.W;
                    const int u = pU[o], ul = pL[o], ur = pR[o];
                    v = fill_select(cl, cr, u == A.invalid ? kFillNone : u, carry_value(cD),
                                    ul == A.invalid ? kFillNone : ul, ur == A.invalid ? kFillNone : ur,
                                    carry_value(cL), carry_value(cR), A.mode, A.N, A.invalid);
                }
                A.dst[(size_t)y * A.dstride + x] = (int16_t)v;
            }
            cD = carry_step(cD, a, valid, G);
            cL = tid > 0 ? sL[par][tid - 1] : 0u;
            cR = tid + 1 < T ? sR[par][tid + 1] : 0u;
        }
    }
}

}  // namespace

// Threads per block for a gap: the column span of a block is T = BW + 2G.
static int fill_threads(int G) { return G <= 48 ? 256 : G <= 160 ? 512 : kFillMaxT; }

size_t fill_plane_bytes(int W, int H) { return 3 * (((size_t)W * H * 2 + 255) / 256 * 256); }

// src -> dst (never the same image). mode 0 copies. planes: fill_plane_bytes(W, H) of device
// memory (not read or written in mode 0). The caller has checked G in 1..255 and N in 1..8 for a
// mode other than 0, and 0 <= x0 <= x1 <= W, 0 <= y0 <= y1 <= H.
hipError_t launch_fill_holes(const int16_t* src, size_t sstride, int16_t* dst, size_t dstride, int W, int H,
                             int invalid, int mode, int G, int N, int x0, int y0, int x1, int y1, void* planes,
                             hipStream_t st)
{
    if (mode == 0 || x1 <= x0 || y1 <= y0) { mode = 0; G = 1; }
    if (G < 1 || G > 255) return hipErrorInvalidValue;
    FillArgs a{};
    a.src = src; a.sstride = sstride; a.dst = dst; a.dstride = dstride;
    a.planes = (int16_t*)planes; a.plane_elems = fill_plane_bytes(W, H) / 6;
    a.W = W; a.H = H; a.invalid = invalid; a.mode = mode; a.G = G; a.N = N;
    a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1;
    const int T = fill_threads(G);
    a.BW = T - 2 * G;
    // rows per band: a block marches BH + G rows down and as many up, and a 1080p frame's blocks are
    // all resident at once, so short bands finish sooner than the halo rows they repeat cost
    a.BH = std::min(std::max(2 * G, 16), 32);
    const dim3 grid((W + a.BW - 1) / a.BW, (H + a.BH - 1) / a.BH);
    hipLaunchKernelGGL(k_fill, grid, dim3(T), 0, st, a);
    return hipGetLastError();
}

}  // namespace sgm
