// plugin_pyramid_test — C++ driver of the plugin core with the pyramid level.
// Modes:  plugin_pyramid_test env     (prints what a fresh core takes from SGM_HIP_PYRAMID, then the
//                                      level after setDownsampleScale(1), (0.5), (0.25) and (0.75),
//                                      and after setPyramidLevel(1) and a further
//                                      setDownsampleScale(1); no GPU)
//         plugin_pyramid_test match   (census forwardMatch of plugin_paths_test's 144x56 frame through
//                                      the core at level 0, at level 1, and with the scale driving the
//                                      level (0.5 and 1); prints an FNV-1a checksum of each disparity
//                                      image, which tests/test_gpu_pyramid.py compares with the engine's
//                                      own images; needs a GPU)
// The frame: B(x, y) = (N(x, y) + N(x + 1, y) + 1) >> 1 of 32-bit LCG noise N, left = B,
// right(x) = B(x + s(y)) with s(y) = 5 + y / 16.
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

static unsigned long long fnv1a(const std::vector<float>& f)
{
    unsigned long long h = 1469598103934665603ULL;
    for (float x : f) {
        const int16_t v = (int16_t)x;
        for (int b = 0; b < 2; b++) { h ^= (unsigned long long)(((uint16_t)v >> (8 * b)) & 255u); h *= 1099511628211ULL; }
    }
    return h;
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "env";
    if (!std::strcmp(mode, "env")) {
        sgm_hip::MatcherCore m(0, SGM_MODE_CENSUS8);
        std::printf("env level %d follow %d\n", m.pyramidLevel(), m.pyramidFollowsScale() ? 1 : 0);
        const double scales[] = {1.0, 0.5, 0.25, 0.75};
        for (double s : scales) {
            m.setDownsampleScale(s);
            std::printf("scale %.2f level %d\n", s, m.pyramidLevel());
        }
        m.setPyramidLevel(1);
        if (m.pyramidLevel() != 1) return fail("setPyramidLevel");
        m.setDownsampleScale(1.0);
        std::printf("set level %d\n", m.pyramidLevel());
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
        m.setSpeckleFilterWindow(0);
        m.setSpeckleFilterRange(0);
        m.setHoleFilling(SGM_FILL_OFF);
        std::vector<float> f((size_t)kW * kH);
        m.setPyramidFollowsScale(false);
        for (int level = 0; level < 2; level++) {
            m.setPyramidLevel(level);
            m.setDownsampleScale(level ? 1.0 : 0.5);       // not followed: changes nothing
            if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch");
            std::printf("level%d hash %016llx\n", level, fnv1a(f));
        }
        m.setPyramidFollowsScale(true);
        m.setDownsampleScale(0.5);
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch scale 0.5");
        std::printf("scale_half hash %016llx\n", fnv1a(f));
        m.setDownsampleScale(1.0);
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch scale 1");
        std::printf("scale_one hash %016llx\n", fnv1a(f));
        std::vector<int16_t> b((size_t)kW * kH);
        m.setDownsampleScale(0.5);                          // the right matcher inherits the level
        if (m.backwardMatch16(L.data(), R.data(), kW, kH, kW, b.data(), kW) != 0) return fail("backwardMatch16");
        std::vector<float> bf(b.begin(), b.end());
        std::printf("backward_half hash %016llx\n", fnv1a(bf));
        m.setPyramidFollowsScale(false);
        m.setPyramidLevel(2);                               // the parameter-error path, -1
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != -1) return fail("level 2 accepted");
        std::printf("pyramid match ok\n");
        return 0;
    }
    return fail("usage: plugin_pyramid_test env | match");
}
