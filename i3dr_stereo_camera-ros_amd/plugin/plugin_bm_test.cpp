// plugin_bm_test — C++ driver of the plugin core in SGM_MODE_OCV_BM (cv::StereoBM).
// Modes:  plugin_bm_test setters   (cv::StereoBM::create(64, 9) start, setters, right matcher; no GPU)
//         plugin_bm_test match     (forward + backward match of one generated 48x96 frame against
//                                   the values tests/golden/make_golden_bm.py printed for the
//                                   numpy reference tests/bm_reference.py; needs a GPU)
// The frame is regenerated here (a 32-bit LCG, make_golden_bm.py driver_frame() is the same
// generator): B(x, y) = (N(x, y) + N(x + 1, y) + 1) >> 1 of LCG noise N, left = B, right(x) =
// B(x + 7): a pair with a constant disparity of 7.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_sgm_core.h"

static int fail(const char* m) { std::fprintf(stderr, "FAIL: %s\n", m); return 1; }

static const int kW = 96, kH = 48, kShift = 7;

// values printed by tests/golden/make_golden_bm.py (reference: tests/bm_reference.py)
static const unsigned long long kForwardHash = 0x6f9b2abb7c7dc8e6ULL;
static const unsigned long long kBackwardHash = 0xd0706a7a00d959b7ULL;
static const int kForwardValid = 1298, kBackwardValid = 1320;
static const int kForwardSample = 113, kBackwardSample = -113;   // forward (24, 80), backward (24, 10)

static void driver_frame(std::vector<uint8_t>& L, std::vector<uint8_t>& R)
{
    const int NW = kW + 8;
    std::vector<int> N((size_t)kH * NW);
    uint32_t s = 12345u;
    for (auto& v : N) { s = s * 1664525u + 1013904223u; v = (int)((s >> 24) & 255u); }
    L.assign((size_t)kW * kH, 0);
    R.assign((size_t)kW * kH, 0);
    for (int y = 0; y < kH; y++)
        for (int x = 0; x < kW; x++) {
            L[(size_t)y * kW + x] = (uint8_t)((N[(size_t)y * NW + x] + N[(size_t)y * NW + x + 1] + 1) >> 1);
            R[(size_t)y * kW + x] =
                (uint8_t)((N[(size_t)y * NW + x + kShift] + N[(size_t)y * NW + x + kShift + 1] + 1) >> 1);
        }
}

static unsigned long long fnv1a(const std::vector<int16_t>& d)
{
    unsigned long long h = 1469598103934665603ULL;
    for (int16_t v : d)
        for (int b = 0; b < 2; b++) { h ^= (unsigned long long)(((uint16_t)v >> (8 * b)) & 255u); h *= 1099511628211ULL; }
    return h;
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "setters";
    if (!std::strcmp(mode, "setters")) {
        sgm_hip::MatcherCore m(0, SGM_MODE_OCV_BM);
        const sgm_params& p = m.params();
        if (p.mode != SGM_MODE_OCV_BM || p.min_disparity != 0 || p.num_disparities != 64 || p.block_size != 9 ||
            p.prefilter_cap != 31 || p.uniqueness_ratio != 15 || p.speckle_window_size != 0 || p.disp12_max_diff != -1 ||
            m.bmParams().texture_threshold != 10 || m.bmParams().prefilter_size != 9)
            return fail("StereoBM::create(64, 9) defaults");
        m.setTextureThreshold(25);
        m.setPreFilterSize(11);
        m.setMinDisparity(9);
        m.setSpeckleFilterWindow(100);
        m.setSpeckleFilterRange(4);
        if (m.bmParams().texture_threshold != 25 || m.bmParams().prefilter_size != 11) return fail("BM setters");
        const sgm_params r = sgm_hip::MatcherCore::rightMatcherParams(m.params());
        const sgm_bm_params rb = sgm_hip::MatcherCore::rightMatcherBmParams(m.bmParams());
        if (r.min_disparity != -(9 + 64) + 1 || r.num_disparities != 64 || r.block_size != 9 || r.uniqueness_ratio != 0 ||
            r.speckle_window_size != 0 || r.disp12_max_diff != -1 || rb.texture_threshold != 0 || rb.prefilter_size != 11)
            return fail("right matcher params");
        if (sgm_check_bm_params(&m.params(), &m.bmParams(), 640, 480) != SGM_OK) return fail("check");
        m.setWindowSize(10);
        if (sgm_check_bm_params(&m.params(), &m.bmParams(), 640, 480) != SGM_ERR_PARAM) return fail("even window");
        std::printf("bm setters ok\n");
        return 0;
    }
    if (!std::strcmp(mode, "match")) {
        std::vector<uint8_t> L, R;
        driver_frame(L, R);
        sgm_hip::MatcherCore m(0, SGM_MODE_OCV_BM);
        std::vector<float> f((size_t)kW * kH);
        std::vector<int16_t> fwd((size_t)kW * kH), bwd((size_t)kW * kH);
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch");
        int valid = 0;
        for (size_t i = 0; i < f.size(); i++) { fwd[i] = (int16_t)f[i]; valid += fwd[i] != -16; }
        std::printf("forward hash %016llx valid %d sample %d\n", fnv1a(fwd), valid, (int)fwd[24 * kW + 80]);
        if (fnv1a(fwd) != kForwardHash || valid != kForwardValid || fwd[24 * kW + 80] != kForwardSample)
            return fail("forward match differs from the reference");
        if (m.backwardMatch16(L.data(), R.data(), kW, kH, kW, bwd.data(), kW) != 0) return fail("backwardMatch");
        valid = 0;
        for (int16_t v : bwd) valid += v != (-63 - 1) * 16;
        std::printf("backward hash %016llx valid %d sample %d\n", fnv1a(bwd), valid, (int)bwd[24 * kW + 10]);
        if (fnv1a(bwd) != kBackwardHash || valid != kBackwardValid || bwd[24 * kW + 10] != kBackwardSample)
            return fail("backward match differs from the reference");
        m.setWindowSize(10);                     // an even window: the cv::Exception path, -1
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != -1) return fail("even window accepted");
        std::printf("bm match ok\n");
        return 0;
    }
    return fail("usage: plugin_bm_test setters | match");
}
