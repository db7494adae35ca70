// rectify.hip — the node's rectify() on the device:
//   cv::initUndistortRectifyMap(K, D, R, P, size, CV_32FC1, map_x, map_y)
//   cv::remap(raw, rect, map_x, map_y, INTER_CUBIC, BORDER_CONSTANT)
// (generate_disparity.cpp:370-386, rectify.cpp:111-127). The reference recomputes the map on
// every frame on the CPU; here it is computed once per calibration (k_rectify_map, double
// precision, the scalar OpenCV loop) and every frame is one HBM-bound remap pass
// (k_remap_cubic: 8 B of map + 1 B out per pixel, the 4x4 source taps from L1/L2).
//
//  k_rectify_map   one thread per map row: the row start i*ir1 + ir2 (etc.) advanced by
//                  += ir0 per column exactly as the scalar loop does (the rounding of the
//                  running sums is part of the result), then the rational + tangential +
//                  thin-prism distortion model, identity tilt, stored as float.
//  k_remap_cubic   OpenCV's fixed-point bicubic remap for u8: X = cvRound(map_x * 32) ->
//                  integer part X >> 5 (saturated to short), fraction X & 31; 16 int16 weights
//                  of the 32 x 32 sub-pixel table (cubic_table, built on the host exactly as
//                  initInterTab2D builds it); taps outside the image read 0 (BORDER_CONSTANT);
//                  dst = sat_u8((sum + 2^14) >> 15).
//  k_remap_cubic_c3 the same for interleaved 8UC3 (the node rectifies colour frames as they
//                  arrive, generate_disparity.cpp:651-652): channels are independent in OpenCV's
//                  remapBicubic, so one map look-up and weight row serve three accumulators.
//  k_bgr2gray      cv::cvtColor(COLOR_BGR2GRAY) 8UC3 -> 8UC1 (generate_disparity.cpp:406-416) in
//                  its 14-bit (OpenCV 3.x) or 15-bit (4.x) coefficients, over the bytes in memory
//                  order; restated, unverified against OpenCV.
//  k_rectify_pair  the pre-pass of the OCV / BM modes on raw frames: both images of a pair
//                  remapped (and, for colour, converted after the remap) into the handle's grey
//                  planes and the caller's rectified images, 4 pixels per thread.
//
// FMA contraction is off for this file: the double map and the float cubic coefficients
// are bit-identical to the scalar C++ evaluation (oracle/sgm_oracle.py rectify_map /
// cubic_table / remap_cubic).
#include "sgm_device.h"
#include "sgm_launch.h"

#include <cmath>

#pragma clang fp contract(off)

namespace sgm {

constexpr int kInterBits = 5;
constexpr int kInterTab = 1 << kInterBits;       // 32 sub-pixel positions per axis
constexpr int kCoefBits = 15;
constexpr int kCoefScale = 1 << kCoefBits;

struct RectMap {
    double ir[9];                                // (P[:, :3] * R)^-1, row-major
    double fx, fy, u0, v0;
    double k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4;
};

__global__ __launch_bounds__(64) void k_rectify_map(RectMap m, int W, int H, float* __restrict__ mx,
                                                    float* __restrict__ my, size_t stride)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= H) return;
    const double* ir = m.ir;
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    float* rx = mx + (size_t)i * stride;
    float* ry = my + (size_t)i * stride;
    for (int j = 0; j < W; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        const double w = 1. / _w, x = _x * w, y = _y * w;
        const double x2 = x * x, y2 = y * y;
        const double r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = (1 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2) / (1 + ((m.k6 * r2 + m.k5) * r2 + m.k4) * r2);
        const double xd = (x * kr + m.p1 * _2xy + m.p2 * (r2 + 2 * x2) + m.s1 * r2 + m.s2 * r2 * r2);
        const double yd = (y * kr + m.p1 * (r2 + 2 * y2) + m.p2 * _2xy + m.s3 * r2 + m.s4 * r2 * r2);
        // identity tilt matrix times (xd, yd, 1), Matx order: s = 0; s += a(i,k) * b(k)
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        t0 += 1.0 * xd; t0 += 0.0 * yd; t0 += 0.0 * 1.0;
        t1 += 0.0 * xd; t1 += 1.0 * yd; t1 += 0.0 * 1.0;
        t2 += 0.0 * xd; t2 += 0.0 * yd; t2 += 1.0 * 1.0;
        const double inv = t2 != 0.0 ? 1. / t2 : 1;
        const double u = m.fx * inv * t0 + m.u0;
        const double v = m.fy * inv * t1 + m.v0;
        rx[j] = (float)u;
        ry[j] = (float)v;
    }
}

// One output pixel per thread; a 64 x 4 block covers 64 consecutive columns of 4 rows.
__global__ __launch_bounds__(256) void k_remap_cubic(const uint8_t* __restrict__ src, size_t sstride, int sw, int sh,
                                                     const float* __restrict__ mx, const float* __restrict__ my,
                                                     size_t mstride, int W, int H, const int16_t* __restrict__ tab,
                                                     uint8_t* __restrict__ dst, size_t dstride)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t m = (size_t)y * mstride + x;
    dst[(size_t)y * dstride + x] = remap_cubic_px(src, sstride, sw, sh, mx[m], my[m], tab);
}

// The same for interleaved 8UC3 (strides in bytes): the map and the weight row of a pixel are
// read once for its three channels (remap_cubic_px3); 3 B out per pixel as byte stores.
__global__ __launch_bounds__(256) void k_remap_cubic_c3(const uint8_t* __restrict__ src, size_t sstride, int sw, int sh,
                                                        const float* __restrict__ mx, const float* __restrict__ my,
                                                        size_t mstride, int W, int H, const int16_t* __restrict__ tab,
                                                        uint8_t* __restrict__ dst, size_t dstride)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t m = (size_t)y * mstride + x;
    const uint32_t v = remap_cubic_px3(src, sstride, sw, sh, mx[m], my[m], tab);
    uint8_t* d = dst + (size_t)y * dstride + 3 * (size_t)x;
    d[0] = (uint8_t)v;
    d[1] = (uint8_t)(v >> 8);
    d[2] = (uint8_t)(v >> 16);
}

// cv::cvtColor(COLOR_BGR2GRAY), 8UC3 -> 8UC1 (gray_px): a thread converts 4 consecutive pixels
// of a row, 12 B in as three dwords and 4 B out as one when both row segments are dword-aligned
// and whole, byte by byte otherwise (odd strides, the row's tail). blockIdx.z selects the image
// of a pair (the matchers' pre-pass converts left and right in one launch).
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1,
                                                  size_t sstride, int W, int H, uint8_t* __restrict__ dst0,
                                                  uint8_t* __restrict__ dst1, size_t dstride, int set)
{
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const uint8_t* s = (blockIdx.z ? src1 : src0) + (size_t)y * sstride + 3 * (size_t)x;
    uint8_t* d = (blockIdx.z ? dst1 : dst0) + (size_t)y * dstride + x;
    if (x + 4 <= W && (((uintptr_t)s | (uintptr_t)d) & 3) == 0) {
        const uint32_t a = ((const uint32_t*)s)[0], b = ((const uint32_t*)s)[1], c = ((const uint32_t*)s)[2];
        const uint32_t g0 = gray_px(a & 255, (a >> 8) & 255, (a >> 16) & 255, set);
        const uint32_t g1 = gray_px(a >> 24, b & 255, (b >> 8) & 255, set);
        const uint32_t g2 = gray_px((b >> 16) & 255, b >> 24, c & 255, set);
        const uint32_t g3 = gray_px((c >> 8) & 255, (c >> 16) & 255, c >> 24, set);
        *(uint32_t*)d = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    } else {
        const int n = min(4, W - x);
        for (int i = 0; i < n; i++) d[i] = (uint8_t)gray_px(s[3 * i], s[3 * i + 1], s[3 * i + 2], set);
    }
}

// The node's imageCb ahead of an OCV / BM match (generate_disparity.cpp:651-652, :406-416): both
// raw images of a frame pair rectified in one launch, blockIdx.z selects the image. CH == 1:
// grey = remap(raw); CH == 3: the colour pixel is remapped first and then converted (the node's
// order: a grey image is never remapped). The grey plane (row stride W) feeds the matcher, the
// rectified image (8UC1 / 8UC3, may be null) goes to the caller.
// A thread owns 4 consecutive pixels of a row: its two map segments as one 16-byte load each, the
// grey bytes as one dword and the 12 colour bytes as three, wherever the segment is whole and
// the address aligned; element by element otherwise (odd strides or bases, the row's tail).
// The remap itself runs transposed: in step i lane t computes pixel 64 i + t of its wave's 256,
// so the 16 tap loads of a step read neighbouring bytes across the wave as in k_remap_cubic
// (with each lane on its own 4 pixels they are 4 pixels apart: 0.100 against 0.082 ms for the
// mono pair at 2448 x 2048). The map values go to the computing lanes and the pixels back to
// their owners through LDS (12 KB per block, a region per wave). No pixel needs a neighbourhood,
// so there is no image tile and no halo: the 4 x 4 taps come from L1 / L2.
struct RectPair {
    const uint8_t* src0; const uint8_t* src1;     // raw images, sw x sh, row stride sstride bytes
    const float* mx0; const float* my0;           // maps of image 0 / 1, W x H, row stride mstride floats
    const float* mx1; const float* my1;
    uint8_t* gray0; uint8_t* gray1;               // W x H, row stride W
    uint8_t* rect0; uint8_t* rect1;               // W x H x CH, row stride rstride bytes, or null
    size_t sstride, mstride, rstride;
    int sw, sh, W, H, set;
    const int16_t* tab;
};

template <int CH>
__global__ __launch_bounds__(256) void k_rectify_pair(RectPair p)
{
    __shared__ __align__(16) float s_mx[4][256];          // per wave: the maps of its 256 pixels
    __shared__ __align__(16) float s_my[4][256];
    __shared__ __align__(16) uint32_t s_px[4][256];       // ... and their remapped values (CH bytes each)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 256, x = x0 + lane * 4, y = blockIdx.y * 4 + wv;
    const bool row = y < p.H, own = row && x < p.W;
    const bool z = blockIdx.z != 0;
    const uint8_t* __restrict__ src = z ? p.src1 : p.src0;
    const int n = min(4, p.W - x);
    if (own) {
        const float* rx = (z ? p.mx1 : p.mx0) + (size_t)y * p.mstride + x;
        const float* ry = (z ? p.my1 : p.my0) + (size_t)y * p.mstride + x;
        float4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (n == 4 && (((uintptr_t)rx | (uintptr_t)ry) & 15) == 0) {
            a = *(const float4*)rx; b = *(const float4*)ry;
        } else {
            a.x = rx[0]; b.x = ry[0];
            if (n > 1) { a.y = rx[1]; b.y = ry[1]; }
            if (n > 2) { a.z = rx[2]; b.z = ry[2]; }
            if (n > 3) { a.w = rx[3]; b.w = ry[3]; }
        }
        *(float4*)&s_mx[wv][4 * lane] = a;
        *(float4*)&s_my[wv][4 * lane] = b;
    }
    __syncthreads();
    // pixels past the row's end are not computed (their map values were not read either)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k = 64 * i + lane;
        if (row && x0 + k < p.W) {
            const float fx = s_mx[wv][k], fy = s_my[wv][k];
            s_px[wv][k] = CH == 3 ? remap_cubic_px3(src, p.sstride, p.sw, p.sh, fx, fy, p.tab)
                                  : (uint32_t)remap_cubic_px(src, p.sstride, p.sw, p.sh, fx, fy, p.tab);
        }
    }
    __syncthreads();
    if (!own) return;
    const uint4 q = *(const uint4*)&s_px[wv][4 * lane];
    const uint32_t v0 = q.x, v1 = n > 1 ? q.y : 0, v2 = n > 2 ? q.z : 0, v3 = n > 3 ? q.w : 0;
    uint8_t* g = (z ? p.gray1 : p.gray0) + (size_t)y * p.W + x;
    uint8_t* r = z ? p.rect1 : p.rect0;
    if (r) r += (size_t)y * p.rstride + (size_t)CH * x;
    uint32_t gq = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);      // CH == 1: the four grey bytes
    if (CH == 3) {
        if (r) {
            if (n == 4 && ((uintptr_t)r & 3) == 0) {
                ((uint32_t*)r)[0] = v0 | (v1 << 24);
                ((uint32_t*)r)[1] = (v1 >> 8) | (v2 << 16);
                ((uint32_t*)r)[2] = (v2 >> 16) | (v3 << 8);
            } else {
                r[0] = (uint8_t)v0; r[1] = (uint8_t)(v0 >> 8); r[2] = (uint8_t)(v0 >> 16);
                if (n > 1) { r[3] = (uint8_t)v1; r[4] = (uint8_t)(v1 >> 8); r[5] = (uint8_t)(v1 >> 16); }
                if (n > 2) { r[6] = (uint8_t)v2; r[7] = (uint8_t)(v2 >> 8); r[8] = (uint8_t)(v2 >> 16); }
                if (n > 3) { r[9] = (uint8_t)v3; r[10] = (uint8_t)(v3 >> 8); r[11] = (uint8_t)(v3 >> 16); }
            }
        }
        gq = (uint32_t)gray_px(v0 & 255, (v0 >> 8) & 255, v0 >> 16, p.set) |
             ((uint32_t)gray_px(v1 & 255, (v1 >> 8) & 255, v1 >> 16, p.set) << 8) |
             ((uint32_t)gray_px(v2 & 255, (v2 >> 8) & 255, v2 >> 16, p.set) << 16) |
             ((uint32_t)gray_px(v3 & 255, (v3 >> 8) & 255, v3 >> 16, p.set) << 24);
    } else if (r) {
        if (n == 4 && ((uintptr_t)r & 3) == 0) {
            *(uint32_t*)r = gq;
        } else {
            r[0] = (uint8_t)gq;
            if (n > 1) r[1] = (uint8_t)(gq >> 8);
            if (n > 2) r[2] = (uint8_t)(gq >> 16);
            if (n > 3) r[3] = (uint8_t)(gq >> 24);
        }
    }
    if (n == 4 && ((uintptr_t)g & 3) == 0) {
        *(uint32_t*)g = gq;
    } else {
        g[0] = (uint8_t)gq;
        if (n > 1) g[1] = (uint8_t)(gq >> 8);
        if (n > 2) g[2] = (uint8_t)(gq >> 16);
        if (n > 3) g[3] = (uint8_t)(gq >> 24);
    }
}

// ---- host -------------------------------------------------------------------------------

// imgwarp.cpp interpolateCubic (float, A = -0.75)
static void cubic_coeffs(float x, float* c)
{
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// initInterTab2D(INTER_CUBIC, fixpt = true): [32 * 32][16] int16, entry fy * 32 + fx
void cubic_table(int16_t* tab)
{
    float t1[kInterTab][4];
    const float scale = 1.f / kInterTab;
    for (int i = 0; i < kInterTab; i++) cubic_coeffs(i * scale, t1[i]);
    for (int i = 0; i < kInterTab; i++)
        for (int j = 0; j < kInterTab; j++) {
            int16_t* it = tab + (size_t)(i * kInterTab + j) * 16;
            int isum = 0;
            for (int k1 = 0; k1 < 4; k1++) {
                const float vy = t1[i][k1];
                for (int k2 = 0; k2 < 4; k2++) {
                    const float v = vy * t1[j][k2];
                    const float sv = v * (float)kCoefScale;
                    const long r = std::lrint(sv);          // cvRound: half to even
                    it[k1 * 4 + k2] = (int16_t)std::min(std::max(r, -32768L), 32767L);
                    isum += it[k1 * 4 + k2];
                }
            }
            if (isum != kCoefScale) {    // the difference goes to one tap of rows/columns 2..3
                const int diff = isum - kCoefScale;
                int Mk1 = 2, Mk2 = 2, mk1 = 2, mk2 = 2;
                for (int k1 = 2; k1 < 4; k1++)
                    for (int k2 = 2; k2 < 4; k2++) {
                        if (it[k1 * 4 + k2] < it[mk1 * 4 + mk2]) mk1 = k1, mk2 = k2;
                        else if (it[k1 * 4 + k2] > it[Mk1 * 4 + Mk2]) Mk1 = k1, Mk2 = k2;
                    }
                if (diff < 0) it[Mk1 * 4 + Mk2] = (int16_t)(it[Mk1 * 4 + Mk2] - diff);
                else it[mk1 * 4 + mk2] = (int16_t)(it[mk1 * 4 + mk2] - diff);
            }
        }
}

// (P[:, :3] * R)^-1: the product summed k = 0..2 in order, cv::invert's 3x3 closed form.
// Returns false when singular.
bool rectify_inverse(const double* P, const double* R, double* ir)
{
    double m[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += P[i * 4 + k] * (R ? R[k * 3 + j] : (k == j ? 1.0 : 0.0));
            m[i * 3 + j] = s;
        }
    auto M = [&](int r, int c) { return m[r * 3 + c]; };
    const double det = M(0, 0) * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) - M(0, 1) * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0)) +
                       M(0, 2) * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0));
    if (det == 0.0) return false;
    const double d = 1. / det;
    ir[0] = (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * d;
    ir[1] = (M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * d;
    ir[2] = (M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * d;
    ir[3] = (M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * d;
    ir[4] = (M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * d;
    ir[5] = (M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * d;
    ir[6] = (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * d;
    ir[7] = (M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * d;
    ir[8] = (M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * d;
    return true;
}

// K 3x3, dist[12] = k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, ir from rectify_inverse
hipError_t launch_rectify_map(const double* K, const double* dist, const double* ir, int W, int H, float* mx,
                              float* my, size_t stride, hipStream_t st)
{
    RectMap m;
    for (int i = 0; i < 9; i++) m.ir[i] = ir[i];
    m.fx = K[0]; m.fy = K[4]; m.u0 = K[2]; m.v0 = K[5];
    m.k1 = dist[0]; m.k2 = dist[1]; m.p1 = dist[2]; m.p2 = dist[3]; m.k3 = dist[4];
    m.k4 = dist[5]; m.k5 = dist[6]; m.k6 = dist[7];
    m.s1 = dist[8]; m.s2 = dist[9]; m.s3 = dist[10]; m.s4 = dist[11];
    hipLaunchKernelGGL(k_rectify_map, dim3((H + 63) / 64), dim3(64), 0, st, m, W, H, mx, my, stride);
    return hipGetLastError();
}

hipError_t launch_remap_cubic(const uint8_t* src, size_t sstride, int sw, int sh, const float* mx, const float* my,
                              size_t mstride, int W, int H, const int16_t* tab, uint8_t* dst, size_t dstride,
                              hipStream_t st)
{
    hipLaunchKernelGGL(k_remap_cubic, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, src, sstride, sw, sh, mx, my,
                       mstride, W, H, tab, dst, dstride);
    return hipGetLastError();
}

hipError_t launch_remap_cubic_c3(const uint8_t* src, size_t sstride, int sw, int sh, const float* mx, const float* my,
                                 size_t mstride, int W, int H, const int16_t* tab, uint8_t* dst, size_t dstride,
                                 hipStream_t st)
{
    hipLaunchKernelGGL(k_remap_cubic_c3, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, st, src, sstride, sw, sh, mx,
                       my, mstride, W, H, tab, dst, dstride);
    return hipGetLastError();
}

// src1 / dst1 null: one image
hipError_t launch_bgr2gray(const uint8_t* src0, const uint8_t* src1, size_t sstride, int W, int H, uint8_t* dst0,
                           uint8_t* dst1, size_t dstride, int set, hipStream_t st)
{
    hipLaunchKernelGGL(k_bgr2gray, dim3((W + 255) / 256, (H + 3) / 4, src1 ? 2 : 1), dim3(256), 0, st, src0, src1,
                       sstride, W, H, dst0, dst1, dstride, set);
    return hipGetLastError();
}

// Both raw images of a frame pair (ch 1: 8UC1, 3: 8UC3, sstride / rstride in bytes) through
// rect.map into the grey planes (row stride W) and, where not null, the rectified images.
hipError_t launch_rectify_pair(const RectifyIn& rect, const uint8_t* rawL, const uint8_t* rawR, size_t sstride, int ch,
                               int gray_set, int W, int H, uint8_t* grayL, uint8_t* grayR, uint8_t* rectL,
                               uint8_t* rectR, size_t rstride, hipStream_t st)
{
    const RectPair p{rawL, rawR, rect.map[0], rect.map[1], rect.map[2], rect.map[3], grayL, grayR, rectL, rectR,
                     sstride, rect.map_stride, rstride, rect.src_w, rect.src_h, W, H, gray_set, rect.tab};
    const dim3 grid((W + 255) / 256, (H + 3) / 4, 2);
    if (ch == 3) hipLaunchKernelGGL(k_rectify_pair<3>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_rectify_pair<1>, grid, dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace sgm
