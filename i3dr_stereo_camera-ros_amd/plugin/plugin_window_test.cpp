// plugin_window_test — C++ driver of the plugin core with a census window.
// Modes:  plugin_window_test env     (prints the window and the cfg flag a fresh core takes from
//                                     SGM_HIP_CENSUS_WINDOW, then the window after setWindowSize(s)
//                                     for a list of slider values, then the effect of
//                                     setCensusWindow; no GPU)
//         plugin_window_test match   (forwardMatch and backwardMatch16 of one generated 144x56 frame
//                                     with the window (7, 7, 2), chosen through the cfg route:
//                                     setWindowSize(11); prints the parameter blocks of both matches
//                                     and an FNV-1a checksum of each disparity image, which
//                                     tests/test_gpu_census_window_plugin.py compares with the
//                                     checksum of tests/census_window_reference.py; needs a GPU)
// The frame is plugin_paths_test's (the Python tests run the same generator,
// census_paths_reference.driver_frame): B(x, y) = (N(x, y) + N(x + 1, y) + 1) >> 1 of 32-bit LCG noise
// N, left = B, right(x) = B(x + s(y)), s(y) = 5 + y / 16.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_sgm_core.h"

static int fail(const char* m) { std::fprintf(stderr, "FAIL: %s\n", m); return 1; }

static const int kW = 144, kH = 56;
static const int kSizes[] = {-7, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17, 21, 255};

static void driver_frame(std::vector<uint8_t>& L, std::vector<uint8_t>& R)
{
    const int NW = kW + 16;
    std::vector<int> N((size_t)kH * NW);
    uint32_t s = 2024u;
    for (auto& v : N) { s = s * 1664525u + 1013904223u; v = (int)((s >> 24) & 255u); }
    L.assign((size_t)kW * kH, 0);
    R.assign((size_t)kW * kH, 0);
    for (int y = 0; y < kH; y++) {
        const int sh = 5 + y / 16;
        for (int x = 0; x < kW; x++) {
            L[(size_t)y * kW + x] = (uint8_t)((N[(size_t)y * NW + x] + N[(size_t)y * NW + x + 1] + 1) >> 1);
            R[(size_t)y * kW + x] = (uint8_t)((N[(size_t)y * NW + x + sh] + N[(size_t)y * NW + x + sh + 1] + 1) >> 1);
        }
    }
}

static unsigned long long fnv1a(const std::vector<int16_t>& d)
{
    unsigned long long h = 1469598103934665603ULL;
    for (int16_t v : d)
        for (int b = 0; b < 2; b++) { h ^= (unsigned long long)(((uint16_t)v >> (8 * b)) & 255u); h *= 1099511628211ULL; }
    return h;
}

static void print_params(const char* tag, const sgm_params& p)
{
    const int* v = (const int*)&p;
    std::printf("%s params", tag);
    for (size_t i = 0; i < sizeof(sgm_params) / sizeof(int); i++) std::printf(" %d", v[i]);
    std::printf("\n");
}

static void print_window(const char* tag, const sgm_census_window& w)
{
    std::printf("%s %d %d %d\n", tag, w.taps_x, w.taps_y, w.step);
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "env";
    if (!std::strcmp(mode, "env")) {
        sgm_hip::MatcherCore m(0, SGM_MODE_CENSUS8);
        print_window("env window", m.censusWindow());
        std::printf("env cfg %d\n", m.censusWindowFollowsSize() ? 1 : 0);
        for (int s : kSizes) {
            m.setWindowSize(s);
            if (m.params().block_size != s) return fail("setWindowSize lost block_size");
            std::printf("size %d window %d %d %d\n", s, m.censusWindow().taps_x, m.censusWindow().taps_y,
                        m.censusWindow().step);
        }
        m.setCensusWindow(5, 3, 2);
        print_window("set window", m.censusWindow());
        m.setCensusWindow(4, 0, -1);               // stored as given
        print_window("set window", m.censusWindow());
        return 0;
    }
    if (!std::strcmp(mode, "match")) {
        std::vector<uint8_t> L, R;
        driver_frame(L, R);
        sgm_hip::MatcherCore m(0, SGM_MODE_CENSUS8);
        m.setMinDisparity(0);
        m.setDisparityRange(32, kW);
        m.setUniquenessRatio(10);
        m.setP1(8.0f);
        m.setP2(64.0f);
        m.setDisp12MaxDiff(1);
        m.setSpeckleFilterWindow(20);
        m.setSpeckleFilterRange(2);
        m.setCensusPaths(8);
        m.setCensusWindowFollowsSize(true);      // what SGM_HIP_CENSUS_WINDOW=cfg switches on
        m.setWindowSize(11);                     // -> (7, 7, 2)
        print_window("window", m.censusWindow());
        print_params("forward", m.params());
        print_params("backward", sgm_hip::MatcherCore::rightMatcherParams(m.params()));
        std::vector<float> f((size_t)kW * kH);
        std::vector<int16_t> fwd((size_t)kW * kH), bwd((size_t)kW * kH);
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch");
        for (size_t i = 0; i < f.size(); i++) fwd[i] = (int16_t)f[i];
        std::printf("forward hash %016llx\n", fnv1a(fwd));
        if (m.backwardMatch16(L.data(), R.data(), kW, kH, kW, bwd.data(), kW) != 0) return fail("backwardMatch16");
        std::printf("backward hash %016llx\n", fnv1a(bwd));
        m.setCensusWindowFollowsSize(false);
        m.setWindowSize(15);                     // no longer followed: the window stays (7, 7, 2)
        if (m.censusWindow().taps_x != 7 || m.censusWindow().step != 2) return fail("setWindowSize moved the window");
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch again");
        for (size_t i = 0; i < f.size(); i++) fwd[i] = (int16_t)f[i];
        std::printf("again hash %016llx\n", fnv1a(fwd));
        m.setCensusWindow(4, 7, 1);              // not a window: the parameter-error path, -1
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != -1) return fail("4x7 accepted");
        std::printf("window match ok\n");
        return 0;
    }
    return fail("usage: plugin_window_test env | match");
}
