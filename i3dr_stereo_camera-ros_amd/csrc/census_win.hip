// census_win.hip — census codes of a selectable window (sgm_set_census_window) for gfx950.
//
// A window is (taps_x, taps_y, step): taps_x x taps_y comparisons, `step` pixels apart, centred on
// the pixel. Tap (j, i) sets the bit the offset (dy = j, dx = i) has in the 9x7 code of
// census_sgm.hip (raster over dy = -3..3, dx = -4..4, centre skipped, LSB first); the bits of the
// taps a window does not have are 0. So a code stays a uint64_t of at most 62 bits, a dense
// (step 1) window's code is the 9x7 code AND-ed with the window's mask, and everything after the
// codes (Hamming cost <= 62, the u8 path engine, WTA, post filters) runs unchanged.
//
// One kernel family, k_census_win<STEP, TAPS_X, TAPS_Y>: 8UC1 planes in, codes out, every image
// of a pipeline group (left and right of up to kMaxGroup frames) in one launch. A workgroup of
// 256 threads owns a 64 x 32 pixel block like census_block. Its LDS tile has a halo of 4 * STEP
// columns and 3 * STEP rows whatever the tap counts: (32 + 6 STEP) rows of 64 + 8 STEP bytes,
// 38 x 72 at step 1 and 44 x 80 (3520 B) at step 2. A wave works on one tile row at a time, lane =
// column: the 32 lanes of a half wave read 8 or 9 consecutive dwords of one row, four lanes per
// dword (a broadcast), so the reads are conflict-free at any pitch and the pitch is just the row
// length, a multiple of 4. A window row is 3 (step 1) or 5 (step 2) aligned u32 LDS reads joined
// by v_alignbyte into dwords of window bytes; at step 2 the taps are bytes 0 and 2 of each. Every
// tap costs the two VALU of census_bit (SDWA byte compare, add with carry); a run of absent taps
// costs one shift. Rows and dwords a window has no tap in are never read.
#include "sgm_device.h"
#include "sgm_launch.h"

namespace sgm {

namespace {

constexpr int kWinWG = 256;
constexpr int kWinRows = 32;     // block: 64 columns x 32 rows

template <int STEP, int TAPS_X, int TAPS_Y>
__device__ __forceinline__ uint64_t census_win_code(const uint8_t* tile, int ty, int tx)
{
    constexpr int PITCH = 64 + 8 * STEP;
    constexpr int RX = (TAPS_X - 1) / 2, RY = (TAPS_Y - 1) / 2;
    constexpr int NW = STEP == 1 ? 3 : 5;          // dwords of a window row
    static_assert(PITCH % 4 == 0, "u32 rows");
    const uint32_t* t32 = (const uint32_t*)tile + (PITCH / 4) * ty + (tx >> 2);
    const int sb = tx & 3;
    const uint32_t c = tile[(ty + 3 * STEP) * PITCH + tx + 4 * STEP];
    uint32_t lo = 0, hi = 0;
    int pend_lo = 0, pend_hi = 0;                  // absent taps since the word's last bit (constants once unrolled)
#pragma unroll
    for (int dy = 6; dy >= 0; dy--) {
        const bool row_in = dy - 3 >= -RY && dy - 3 <= RY;
        uint32_t a[NW] = {};
        if (row_in) {
            const uint32_t* r = t32 + (PITCH / 4) * (STEP * dy);
            // window bytes 4k .. 4k+3 of the row; only the dwords that hold a tap are read
#pragma unroll
            for (int k = 0; k < NW; k++) {
                const int b0 = STEP * (4 - RX), b1 = STEP * (4 + RX);     // first / last tap byte
                if (4 * k + 3 < b0 || 4 * k > b1) continue;
                a[k] = k + 1 < NW ? __builtin_amdgcn_alignbyte(r[k + 1], r[k], sb)
                                  : __builtin_amdgcn_alignbyte(r[k], r[k], sb);   // the last: its low byte only
            }
        }
#pragma unroll
        for (int dx = 8; dx >= 0; dx--) {
            if (dy == 3 && dx == 4) continue;
            const int k = dy * 9 + dx - (dy * 9 + dx > 31 ? 1 : 0);    // bit index in the 9x7 code
            const bool in = row_in && dx - 4 >= -RX && dx - 4 <= RX;
            const int byte = STEP * dx;
            if (k >= 32) {
                if (!in) { pend_hi++; continue; }
                if (pend_hi) { hi <<= pend_hi; pend_hi = 0; }
                census_bit(hi, a[byte >> 2], c, byte & 3);
            } else {
                if (!in) { pend_lo++; continue; }
                if (pend_lo) { lo <<= pend_lo; pend_lo = 0; }
                census_bit(lo, a[byte >> 2], c, byte & 3);
            }
        }
    }
    lo <<= pend_lo;
    hi <<= pend_hi;
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// blockIdx.x: the 64 x 32 block of an image, blockIdx.y: the image (wi.src / wi.out, < wi.n)
template <int STEP, int TAPS_X, int TAPS_Y>
__global__ __launch_bounds__(kWinWG) void k_census_win(WinImages wi, int W, int H)
{
    constexpr int PITCH = 64 + 8 * STEP, TH = kWinRows + 6 * STEP;
    __shared__ __attribute__((aligned(16))) uint8_t tile[TH * PITCH];
    // selects, not a dynamic index: that would copy the kernel argument to scratch
    const int img = blockIdx.y;
    const uint8_t* src = wi.src[0];
    uint64_t* out = wi.out[0];
#pragma unroll
    for (int i = 1; i < 2 * kMaxGroup; i++) {
        src = img == i ? wi.src[i] : src;
        out = img == i ? wi.out[i] : out;
    }
    const int bx = (W + 63) / 64, by = blockIdx.x / bx;
    const int x0 = (blockIdx.x - by * bx) * 64, y0 = by * kWinRows;
    for (int i = threadIdx.x; i < TH * PITCH; i += kWinWG) {
        const int ty = i / PITCH, tx = i - ty * PITCH;
        const int yy = min(max(y0 + ty - 3 * STEP, 0), H - 1), xx = min(max(x0 + tx - 4 * STEP, 0), W - 1);
        tile[i] = src[(size_t)yy * wi.stride + xx];
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, x = x0 + tx;
    if (x >= W) return;
    for (int ty = threadIdx.x >> 6; ty < kWinRows; ty += kWinWG / 64) {
        const int y = y0 + ty;
        if (y >= H) break;
        out[(size_t)y * W + x] = census_win_code<STEP, TAPS_X, TAPS_Y>(tile, ty, tx);
    }
}

template <int STEP, int TAPS_X, int TAPS_Y>
void launch_win(const WinImages& wi, int W, int H, hipStream_t st)
{
    dim3 grid(((W + 63) / 64) * ((H + kWinRows - 1) / kWinRows), wi.n);
    hipLaunchKernelGGL((k_census_win<STEP, TAPS_X, TAPS_Y>), grid, dim3(kWinWG), 0, st, wi, W, H);
}

template <int STEP, int TAPS_X>
bool launch_win_y(const WinImages& wi, int W, int H, int taps_y, hipStream_t st)
{
    switch (taps_y) {
    case 3: launch_win<STEP, TAPS_X, 3>(wi, W, H, st); return true;
    case 5: launch_win<STEP, TAPS_X, 5>(wi, W, H, st); return true;
    case 7: launch_win<STEP, TAPS_X, 7>(wi, W, H, st); return true;
    default: return false;
    }
}

template <int STEP>
bool launch_win_x(const WinImages& wi, int W, int H, int taps_x, int taps_y, hipStream_t st)
{
    switch (taps_x) {
    case 3: return launch_win_y<STEP, 3>(wi, W, H, taps_y, st);
    case 5: return launch_win_y<STEP, 5>(wi, W, H, taps_y, st);
    case 7: return launch_win_y<STEP, 7>(wi, W, H, taps_y, st);
    case 9: return launch_win_y<STEP, 9>(wi, W, H, taps_y, st);
    default: return false;
    }
}

}  // namespace

// Codes of the wi.n images of wi (8UC1 planes of W x H, row stride wi.stride) under window cw.
// A window census_window_ok refuses is hipErrorInvalidValue (the callers validate first).
hipError_t launch_census_win(const WinImages& wi, int W, int H, const sgm_census_window& cw, hipStream_t st)
{
    if (wi.n <= 0) return hipSuccess;
    if (wi.n > 2 * kMaxGroup || !census_window_ok(cw)) return hipErrorInvalidValue;
    const bool ok = cw.step == 1 ? launch_win_x<1>(wi, W, H, cw.taps_x, cw.taps_y, st)
                                 : launch_win_x<2>(wi, W, H, cw.taps_x, cw.taps_y, st);
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// The codes of one 8UC1 image pair (R may be null: the left image alone) under cw: the 9x7 kernel
// of census_sgm.hip for the default window, k_census_win for any other.
hipError_t launch_census_planes(const sgm_census_window& cw, const uint8_t* L, const uint8_t* R, size_t stride, int W,
                                int H, uint64_t* cL, uint64_t* cR, hipStream_t st)
{
    if (census_window_default(cw)) return launch_census(L, R, stride, W, H, cL, cR, st);
    WinImages wi{};
    wi.src[0] = L; wi.out[0] = cL;
    wi.src[1] = R; wi.out[1] = cR;
    wi.n = R ? 2 : 1;
    wi.stride = stride;
    return launch_census_win(wi, W, H, cw, st);
}

}  // namespace sgm
