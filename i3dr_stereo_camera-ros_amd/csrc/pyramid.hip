// pyramid.hip — the two kernels of the half-resolution pyramid level (sgm_set_pyramid_params) for
// gfx950. tests/pyramid_reference.py is the executable statement of what they compute.
//
// k_pyr_down: both 8UC1 images of a pair in one launch (grid z = image). A workgroup of 256 threads
// owns a 64 x 16 pixel block; its LDS tile carries a halo of 2 (the 5x5 census), 20 rows of 72
// bytes (1440 B), loaded with replicate clamping. From the tile it writes
//   - the block's 32 x 8 coarse pixels, one per thread: (a + b + c + d + 2) >> 2 of the 2x2 cell whose
//     odd column / row is clamped to the image (the clamped tile holds exactly those values);
//   - the 24-bit 5x5 census code of every pixel as a u32 plane (raster over dy, dx = -2..2, centre
//     skipped, LSB first), four pixels per thread, lane = column.
// k_pyr_refine<RAD>: one thread per full-resolution pixel, a workgroup of 64 x 4 pixels. A pixel
// reads its coarse disparity, gathers the 3 x 3 left codes around it and the 3 x (2 RAD + 5) right
// codes around x - d0 through the caches (neighbouring pixels share all but one column), forms
// h(d) = sum of 9 popcounts for the 2 RAD + 3 disparities d0 - RAD - 1 .. d0 + RAD + 1, picks the
// candidate k = 0, -1, +1, .. (strict <) inside [m, m + D - 1] and interpolates with its two
// neighbours. All arrays are indexed by unrolled constants: registers only, no LDS, no scratch.
#include <algorithm>

#include "sgm_device.h"
#include "sgm_launch.h"

namespace sgm {

namespace {

constexpr int kDownW = 64, kDownH = 16, kDownPitch = 72, kDownRows = kDownH + 4;

struct PyrDownArgs {
    const uint8_t* src[2];
    uint8_t* dst[2];
    uint32_t* code[2];
    size_t stride;
    int W, H, Wc, Hc;
};

__global__ __launch_bounds__(256) void k_pyr_down(PyrDownArgs A)
{
    __shared__ uint8_t tile[kDownRows * kDownPitch];
    const int z = blockIdx.z;
    const uint8_t* __restrict__ src = A.src[z];
    const int bx = blockIdx.x * kDownW, by = blockIdx.y * kDownH;
    const int tid = threadIdx.x;
    for (int i = tid; i < kDownRows * (kDownW + 4); i += 256) {
        const int r = i / (kDownW + 4), c = i - r * (kDownW + 4);
        const int y = min(max(by + r - 2, 0), A.H - 1), x = min(max(bx + c - 2, 0), A.W - 1);
        tile[r * kDownPitch + c] = src[(size_t)y * A.stride + x];
    }
    __syncthreads();
    {   // one coarse pixel per thread
        const int cx = tid & 31, cy = tid >> 5;
        const int xc = (bx >> 1) + cx, yc = (by >> 1) + cy;
        if (xc < A.Wc && yc < A.Hc) {
            const uint8_t* t = tile + (2 * cy + 2) * kDownPitch + 2 * cx + 2;
            const int s = t[0] + t[1] + t[kDownPitch] + t[kDownPitch + 1];
            A.dst[z][(size_t)yc * A.Wc + xc] = (uint8_t)((s + 2) >> 2);
        }
    }
    const int tx = tid & 63, ty0 = tid >> 6;
    const int x = bx + tx;
    if (x >= A.W) return;
#pragma unroll
    for (int r = 0; r < kDownH / 4; r++) {
        const int ty = ty0 + 4 * r, y = by + ty;
        if (y >= A.H) break;
        const uint8_t* t = tile + ty * kDownPitch + tx;      // the window's top left corner
        const uint32_t c = t[2 * kDownPitch + 2];
        uint32_t code = 0;
        int bit = 0;
#pragma unroll
        for (int dy = 0; dy < 5; dy++)
#pragma unroll
            for (int dx = 0; dx < 5; dx++) {
                if (dy == 2 && dx == 2) continue;
                code |= (uint32_t)(t[dy * kDownPitch + dx] < c) << bit;
                bit++;
            }
        A.code[z][(size_t)y * A.W + x] = code;
    }
}

struct PyrRefineArgs {
    const uint32_t* KL;
    const uint32_t* KR;
    const int16_t* coarse;      // Wc x Hc, row stride cstride
    size_t cstride;
    int16_t* out;
    size_t ostride;
    int W, H, m, D, invalid_c, invalid, x_lo, x_hi, subpix;
};

// eight waves per SIMD: the gathers are latency the other waves hide, and 65 VGPRs would cost one
template <int RAD>
__global__ __launch_bounds__(256, 8) void k_pyr_refine(PyrRefineArgs A)
{
    constexpr int NT = 2 * RAD + 3;      // disparities d0 - RAD - 1 .. d0 + RAD + 1
    constexpr int NC = NT + 2;           // right-code columns x - d0 - (RAD + 2) .. x - d0 + (RAD + 2)
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.W || y >= A.H) return;
    int16_t* o = A.out + (size_t)y * A.ostride + x;
    const int c = A.coarse[(size_t)(y >> 1) * A.cstride + (x >> 1)];
    if (x < A.x_lo || x >= A.x_hi || c == A.invalid_c) { *o = (int16_t)A.invalid; return; }
    const int d0 = (2 * c + 8) >> 4;
    const int dmax = A.m + A.D - 1;
    if (d0 + RAD < A.m || d0 - RAD > dmax) { *o = (int16_t)A.invalid; return; }    // no candidate in range
    int h[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) h[t] = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const size_t row = (size_t)min(max(y + j - 1, 0), A.H - 1) * A.W;
        uint32_t kl[3], kr[NC];
#pragma unroll
        for (int i = 0; i < 3; i++) kl[i] = A.KL[row + min(max(x + i - 1, 0), A.W - 1)];
#pragma unroll
        for (int e = 0; e < NC; e++) kr[e] = A.KR[row + min(max(x - d0 + e - (RAD + 2), 0), A.W - 1)];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int i = 0; i < 3; i++) h[t] += __popc(kl[i] ^ kr[i - t + 2 * RAD + 2]);
    }
    int best = 1 << 20, ds = 0, cm = 0, cp = 0;
#pragma unroll
    for (int n = 0; n < 2 * RAD + 1; n++) {
        const int k = n == 0 ? 0 : (n & 1 ? -((n + 1) / 2) : n / 2);     // 0, -1, +1, -2, +2
        const int d = d0 + k, t = k + RAD + 1;
        if (d >= A.m && d <= dmax && h[t] < best) { best = h[t]; ds = d; cm = h[t - 1]; cp = h[t + 1]; }
    }
    int off = 0;
    if (A.subpix && ds > A.m && ds < dmax) {
        const int den = cm + cp - 2 * best;
        if (cm >= best && cp >= best && den > 0) off = ((cm - cp) * 16 + den) / (2 * den);
    }
    *o = (int16_t)(ds * 16 + off);
}

}  // namespace

// Both images of a pair: coarse images (row stride (W + 1) / 2) and u32 code planes (row stride W).
hipError_t launch_pyr_down(const uint8_t* L, const uint8_t* R, size_t stride, int W, int H, uint8_t* Lc, uint8_t* Rc,
                           uint32_t* KL, uint32_t* KR, hipStream_t st)
{
    PyrDownArgs a{};
    a.src[0] = L; a.src[1] = R; a.dst[0] = Lc; a.dst[1] = Rc; a.code[0] = KL; a.code[1] = KR;
    a.stride = stride; a.W = W; a.H = H; a.Wc = (W + 1) >> 1; a.Hc = (H + 1) >> 1;
    const dim3 grid((W + kDownW - 1) / kDownW, (H + kDownH - 1) / kDownH, 2);
    hipLaunchKernelGGL(k_pyr_down, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

// coarse: ((W + 1) / 2) x ((H + 1) / 2) int16 with row stride cstride; out: W x H int16. The
// caller has checked radius in 1..2.
hipError_t launch_pyr_refine(const uint32_t* KL, const uint32_t* KR, const int16_t* coarse, size_t cstride, int W,
                             int H, int m, int D, int mc, int radius, int subpixel, int16_t* out, size_t ostride,
                             hipStream_t st)
{
    if (radius < 1 || radius > 2) return hipErrorInvalidValue;
    PyrRefineArgs a{};
    a.KL = KL; a.KR = KR; a.coarse = coarse; a.cstride = cstride; a.out = out; a.ostride = ostride;
    a.W = W; a.H = H; a.m = m; a.D = D; a.invalid_c = (mc - 1) * 16; a.invalid = (m - 1) * 16;
    a.x_lo = std::max(m + D, 0); a.x_hi = W + std::min(m, 0); a.subpix = subpixel != 0;
    const dim3 grid((W + 63) / 64, (H + 3) / 4), block(64, 4);
    if (radius == 1) hipLaunchKernelGGL(k_pyr_refine<1>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_pyr_refine<2>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace sgm
