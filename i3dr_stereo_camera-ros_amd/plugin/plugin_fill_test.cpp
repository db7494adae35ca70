// plugin_fill_test — C++ driver of the plugin core with the hole filter.
// Modes:  plugin_fill_test env     (prints what a fresh core takes from SGM_HIP_FILL and
//                                   SGM_HIP_FILL_WHEN, the filter a match would run with interp off
//                                   and on, and whether interp on still means Q3; then the effect of
//                                   setHoleFilling; no GPU)
//         plugin_fill_test match   (census forwardMatch of one generated 144x56 frame through the
//                                   core with the filter off, background and median, and under
//                                   "when = interp" with interp on and off; prints an FNV-1a checksum
//                                   of each disparity image, which tests/test_gpu_fuzz_fill.py compares
//                                   with the oracle's match followed by tests/fill_reference.py; needs
//                                   a GPU)
// The frame is plugin_paths_test's, B(x, y) = (N(x, y) + N(x + 1, y) + 1) >> 1 of 32-bit LCG noise N,
// left = B, right(x) = B(x + s(y)) with s(y) = 5 + y / 16, except that the right image's 12 x 6
// patches with (x / 12 + y / 6) % 3 == 0 hold unrelated noise, N(NW - 1 - x, H - 1 - y): nothing
// matches there, so the window has holes for the filter to fill.
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
            if ((x / 12 + y / 6) % 3 == 0) R[(size_t)y * kW + x] = (uint8_t)N[(size_t)(kH - 1 - y) * NW + (NW - 1 - x)];
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

static void print_fill(const char* tag, const sgm_fill_params& f)
{
    std::printf("%s %d %d %d\n", tag, f.mode, f.max_gap, f.min_neighbours);
}

int main(int argc, char** argv)
{
    const char* mode = argc > 1 ? argv[1] : "env";
    if (!std::strcmp(mode, "env")) {
        sgm_hip::MatcherCore m(0, SGM_MODE_CENSUS8);
        print_fill("env fill", m.holeFilling());
        print_fill("interp off", m.effectiveFill());
        std::printf("q3 off %d\n", m.q3() ? 1 : 0);
        m.setInterpolation(true);
        print_fill("interp on", m.effectiveFill());
        std::printf("q3 on %d\n", m.q3() ? 1 : 0);
        m.setHoleFilling(SGM_FILL_MEDIAN, 7, 3);
        const sgm_fill_params& f = m.holeFilling();
        if (f.mode != SGM_FILL_MEDIAN || f.max_gap != 7 || f.min_neighbours != 3) return fail("setHoleFilling");
        print_fill("set fill", f);
        return 0;
    }
    if (!std::strcmp(mode, "match")) {
        std::vector<uint8_t> L, R;
        driver_frame(L, R);
        sgm_hip::MatcherCore m(0, SGM_MODE_CENSUS8);
        m.setMinDisparity(0);
        m.setDisparityRange(32, kW);
        m.setUniquenessRatio(40);
        m.setP1(8.0f);
        m.setP2(64.0f);
        m.setDisp12MaxDiff(1);
        m.setSpeckleFilterWindow(0);
        m.setSpeckleFilterRange(0);
        m.setFillWhenInterp(false);
        std::vector<float> f((size_t)kW * kH);
        struct { const char* tag; int mode, gap, n; } runs[] = {
            {"off", SGM_FILL_OFF, 16, 2}, {"background", SGM_FILL_BACKGROUND, 16, 2}, {"median", SGM_FILL_MEDIAN, 3, 1}};
        for (const auto& r : runs) {
            m.setHoleFilling(r.mode, r.gap, r.n);
            if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch");
            std::printf("%s hash %016llx\n", r.tag, fnv1a(f));
        }
        // the interp flag drives the filter: on = the forward disparity filled (not Q3), off = unfilled
        m.setFillWhenInterp(true);
        m.setHoleFilling(SGM_FILL_OFF, 16, 2);
        m.setInterpolation(true);
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch interp on");
        std::printf("interp_on hash %016llx\n", fnv1a(f));
        m.setInterpolation(false);
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != 0) return fail("forwardMatch interp off");
        std::printf("interp_off hash %016llx\n", fnv1a(f));
        m.setFillWhenInterp(false);
        m.setHoleFilling(SGM_FILL_MEDIAN, 256, 2);        // the parameter-error path, -1
        if (m.forwardMatch(L.data(), R.data(), kW, kH, kW, f.data(), kW) != -1) return fail("gap 256 accepted");
        std::printf("fill match ok\n");
        return 0;
    }
    return fail("usage: plugin_fill_test env | match");
}
