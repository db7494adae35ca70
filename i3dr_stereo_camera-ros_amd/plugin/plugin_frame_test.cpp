// plugin_frame_test — C++ driver of the plugin core's node frame (MatcherCore::imageCb over
// sgm_node_frame).
// Modes:  plugin_frame_test abi      (sizeof and the offset of every field of sgm_camera_info and
//                                     sgm_node_frame_io, which tests/test_node_frame_host.py compares
//                                     with the ctypes mirrors of the Python package; no GPU)
//         plugin_frame_test window f T depth_min depth_max
//                                    (the bits of MatcherCore::disparityWindow's two floats; no GPU)
//         plugin_frame_test frame <bm|sgbm5|hh8|census> <1|3> <0|1>
//                                    (imageCb of one generated 224x96 raw pair, mono or colour, at
//                                     the node defaults, interpolation off or on; prints the window
//                                     and an FNV-1a checksum of both rectified images and of the
//                                     DisparityImage floats, which tests/test_gpu_node_frame.py
//                                     compares with the Python image_cb on the same pair; needs a GPU)
// The pair is generated here from a 32-bit LCG (the Python test runs the same generator): per
// channel c a noise plane N_c, B_c(x, y) = (N_c(x, y) + N_c(x + 1, y) + N_c(x, y + 1) +
// N_c(x + 1, y + 1) + 2) >> 2, left = B(x), right(x) = B(x + s(y)) with s(y) = 20 + y / 16; channels
// interleaved. The calibration is the pair of CameraInfos written below.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_sgm_core.h"

static int fail(const char* m) { std::fprintf(stderr, "FAIL: %s\n", m); return 1; }

static const int kW = 224, kH = 96;
static const double kF = 712.5, kT = 0.119;

static void driver_frame(int ch, std::vector<uint8_t>& L, std::vector<uint8_t>& R)
{
    const int NW = kW + 32, NH = kH + 1;
    std::vector<int> N((size_t)ch * NH * NW);
    uint32_t s = 7331u;
    for (auto& v : N) { s = s * 1664525u + 1013904223u; v = (int)((s >> 24) & 255u); }
    L.assign((size_t)kW * kH * ch, 0);
    R.assign((size_t)kW * kH * ch, 0);
    auto B = [&](int c, int x, int y) {
        const int* p = &N[((size_t)c * NH + y) * NW + x];
        return (uint8_t)((p[0] + p[1] + p[NW] + p[NW + 1] + 2) >> 2);
    };
    for (int y = 0; y < kH; y++) {
        const int sh = 20 + y / 16;
        for (int x = 0; x < kW; x++)
            for (int c = 0; c < ch; c++) {
                L[((size_t)y * kW + x) * ch + c] = B(c, x, y);
                R[((size_t)y * kW + x) * ch + c] = B(c, x + sh, y);
            }
    }
}

// Two plumb_bob cameras of a 224x96 sensor: the same small rotation, slightly different principal
// point and first radial coefficient (the rows of the two rectified images stay aligned).
static void driver_calib(sgm_camera_info& l, sgm_camera_info& r)
{
    const double K[9] = {201.6, 0, 115.3, 0, 203.616, 45.9, 0, 0, 1};
    const double D[5] = {-0.21, 0.07, 0.0012, -0.0009, -0.011};
    const double Rm[9] = {0.99995, -0.008, 0.006, 0.00806, 0.99992, -0.0095, -0.00592, 0.00955, 0.99994};
    const double P[12] = {197.568, 0, 107.0, -24.192, 0, 197.568, 49.5, 0, 0, 0, 1, 0};
    std::memset(&l, 0, sizeof l);
    std::memcpy(l.K, K, sizeof K);
    std::memcpy(l.D, D, sizeof D);
    l.n_dist = 5;
    l.has_R = 1;
    std::memcpy(l.R, Rm, sizeof Rm);
    std::memcpy(l.P, P, sizeof P);
    r = l;
    l.P[3] = 0.0;
    r.K[2] += 0.75;
    r.D[0] += 0.01;
}

static unsigned long long fnv1a(const void* data, size_t n)
{
    unsigned long long h = 1469598103934665603ULL;
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 1099511628211ULL; }
    return h;
}

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

#define OFF(T, f) std::printf("offset " #T "." #f " %zu\n", offsetof(T, f))

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "abi")) {
        std::printf("sizeof sgm_camera_info %zu\n", sizeof(sgm_camera_info));
        OFF(sgm_camera_info, K); OFF(sgm_camera_info, D); OFF(sgm_camera_info, n_dist); OFF(sgm_camera_info, has_R);
        OFF(sgm_camera_info, R); OFF(sgm_camera_info, P);
        std::printf("sizeof sgm_node_frame_io %zu\n", sizeof(sgm_node_frame_io));
        OFF(sgm_node_frame_io, struct_size); OFF(sgm_node_frame_io, raw_left); OFF(sgm_node_frame_io, raw_right);
        OFF(sgm_node_frame_io, raw_stride); OFF(sgm_node_frame_io, width); OFF(sgm_node_frame_io, height);
        OFF(sgm_node_frame_io, min_disparity); OFF(sgm_node_frame_io, max_disparity); OFF(sgm_node_frame_io, rect_left);
        OFF(sgm_node_frame_io, rect_right); OFF(sgm_node_frame_io, rect_stride); OFF(sgm_node_frame_io, disparity);
        OFF(sgm_node_frame_io, disparity_stride); OFF(sgm_node_frame_io, depth); OFF(sgm_node_frame_io, depth_stride);
        OFF(sgm_node_frame_io, q5); OFF(sgm_node_frame_io, depth_min); OFF(sgm_node_frame_io, depth_max);
        return 0;
    }
    if (!std::strcmp(mode, "window") && argc == 6) {
        float lo, hi;
        sgm_hip::MatcherCore::disparityWindow(std::strtod(argv[2], nullptr), std::strtod(argv[3], nullptr),
                                              std::strtod(argv[4], nullptr), std::strtod(argv[5], nullptr), &lo, &hi);
        std::printf("min_disp %08x max_disp %08x\n", bits(lo), bits(hi));
        return 0;
    }
    if (!std::strcmp(mode, "frame") && argc == 5) {
        const char* names[4] = {"sgbm5", "hh8", "census", "bm"};     // SGM_MODE_* order
        int m = -1;
        for (int i = 0; i < 4; i++) if (!std::strcmp(argv[2], names[i])) m = i;
        const int ch = std::atoi(argv[3]), interp = std::atoi(argv[4]);
        if (m < 0 || (ch != 1 && ch != 3)) return fail("frame <bm|sgbm5|hh8|census> <1|3> <0|1>");
        std::vector<uint8_t> L, R;
        driver_frame(ch, L, R);
        sgm_camera_info cl, cr;
        driver_calib(cl, cr);
        sgm_hip::MatcherCore core(0, m);
        // updateMatcher() with the node defaults (generate_disparity.cpp:90-112, :241-261)
        core.setDisparityRange(64, kW);
        core.setWindowSize(15);
        core.setMinDisparity(9);
        core.setUniquenessRatio(15);
        core.setSpeckleFilterRange(4);
        core.setSpeckleFilterWindow(100);
        core.setPreFilterCap(31);
        core.setP1(200.0f);
        core.setP2(400.0f);
        core.setTextureThreshold(10);
        core.setPreFilterSize(9);
        core.setInterpolation(interp != 0);
        // the right matcher's disparities are negative: a window that holds them
        const double zmin = interp ? -20.0 : 0.5, zmax = interp ? -0.5 : 20.0;
        float lo, hi;
        sgm_hip::MatcherCore::disparityWindow(kF, kT, zmin, zmax, &lo, &hi);
        std::printf("min_disp %08x max_disp %08x\n", bits(lo), bits(hi));
        const size_t row = (size_t)kW * ch;
        std::vector<uint8_t> rl(row * kH, 0x5A), rr(row * kH, 0x5A);
        std::vector<float> disp((size_t)kW * kH, -1.0f);
        for (int k = 0; k < 2; k++)      // the second frame reuses the maps
            if (core.imageCb(L.data(), R.data(), kW, kH, ch, row, cl, cr, kF, kT, zmin, zmax, rl.data(), rr.data(), row,
                             disp.data(), kW) != 0)
                return fail("imageCb");
        if (core.mapBuilds() != 1) return fail("two frames of one calibration built the maps more than once");
        std::printf("rect_left hash %016llx\n", fnv1a(rl.data(), rl.size()));
        std::printf("rect_right hash %016llx\n", fnv1a(rr.data(), rr.size()));
        std::printf("disparity hash %016llx\n", fnv1a(disp.data(), disp.size() * sizeof(float)));
        core.setDisparityRange(24, kW);          // not a multiple of 16: the parameter-error path, -1
        std::vector<float> keep(disp);
        if (core.imageCb(L.data(), R.data(), kW, kH, ch, row, cl, cr, kF, kT, zmin, zmax, rl.data(), rr.data(), row,
                         disp.data(), kW) != -1)
            return fail("D = 24 accepted");
        if (std::memcmp(keep.data(), disp.data(), keep.size() * sizeof(float))) return fail("a failed frame wrote its output");
        std::printf("frame ok\n");
        return 0;
    }
    return fail("usage: plugin_frame_test abi | window f T depth_min depth_max | frame <mode> <1|3> <0|1>");
}
