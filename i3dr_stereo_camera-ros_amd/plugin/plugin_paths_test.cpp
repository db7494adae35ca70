// plugin_paths_test — C++ driver of the plugin core with the census mode's 4-path set.
// Modes:  plugin_paths_test env     (prints the path count a fresh core takes from
//                                    SGM_HIP_CENSUS_PATHS, then the effect of setCensusPaths; no GPU)
//         plugin_paths_test match   (4-path forwardMatch and backwardMatch16 of one generated
//                                    144x56 frame through the core; prints the parameter blocks of
//                                    both matches and an FNV-1a checksum of each disparity image,
//                                    which tests/test_gpu_census_paths.py compares with the checksum
//                                    of the reference composed from the oracle's stages; needs a GPU)
// The frame is generated here from a 32-bit LCG (the Python test runs the same generator):
// B(x, y) = (N(x, y) + N(x + 1, y) + 1) >> 1 of LCG noise N, left = B, right(x) = B(x + s(y)) with
// the shift s(y) = 5 + y / 16: a pair whose disparity steps down the image.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_sgm_core.h"

static int fail(const char* m) { std::fprintf(stderr, "FAIL: %s\n", m); return 1; }

static const int kW = 144, kH = 56;

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

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "env";
    if (!std::strcmp(mode, "env")) {
        sgm_hip::MatcherCore m(0, SGM_MODE_CENSUS8);
        std::printf("env paths %d\n", m.censusPaths());
        m.setCensusPaths(4);
        if (m.censusPaths() != 4) return fail("setCensusPaths");
        std::printf("set paths %d\n", m.censusPaths());
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
        m.setCensusPaths(4);
        print_params("forward", m.params());
        print_params("backward", sgm_hip::MatcherCore::rightMatcherParams(m.params()));
        std::vector<float> f((size_t)kW * kH);
        std::vector<int16_t> fwd((size_t)kW * kH), bwd((size_t)kW * kH);
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch");
        for (size_t i = 0; i < f.size(); i++) fwd[i] = (int16_t)f[i];
        std::printf("forward hash %016llx\n", fnv1a(fwd));
        if (m.backwardMatch16(L.data(), R.data(), kW, kH, kW, bwd.data(), kW) != 0) return fail("backwardMatch16");
        std::printf("backward hash %016llx\n", fnv1a(bwd));
        m.setCensusPaths(5);                     // neither 4 nor 8: the parameter-error path, -1
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != -1) return fail("5 paths accepted");
        std::printf("paths match ok\n");
        return 0;
    }
    return fail("usage: plugin_paths_test env | match");
}
