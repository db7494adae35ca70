// sgm_launch.h — the host launchers and host helpers that the .hip files define and the
// C-ABI sources call. This is their only declaration (default arguments included): every
// file that defines one includes it, so the compiler checks each definition against it.
#pragma once

#include "sgm_device.h"

namespace sgm {

// census_sgm.hip
hipError_t launch_census(const uint8_t* L, const uint8_t* R, size_t stride, int W, int H, uint64_t* cL, uint64_t* cR,
                         hipStream_t st, int ch = 1, int gray = 0);
int census_path_items(const Geom& g, unsigned dir_mask, int n_slots, int group, uint32_t* out, int cap,
                      int up_group = 0);
int census_vol_group(int D);
hipError_t launch_census_paths(const PathFrames& pf, size_t vol_bytes, const Geom& g, const uint32_t* items,
                               int n_items, hipStream_t st, const uint8_t* bnd_down = nullptr,
                               const uint8_t* bnd_up = nullptr, size_t bnd_slot = 0);
hipError_t launch_census_wta(const WtaFrames& wf, size_t vol_bytes, const Geom& g, size_t out_stride, hipStream_t st,
                             int np = 8, const MsgWin* msg = nullptr);
hipError_t launch_census_tiles(const CensusFrames& cf, int W, int H, hipStream_t st);
hipError_t launch_census_fused(const PathFrames& pf, const WtaFrames& wf, const CensusFrames& cf, size_t vol_bytes,
                               const Geom& g, const uint32_t* items, int n_items, size_t out_stride, bool up_wta,
                               hipStream_t st);
hipError_t launch_census_rowfin(const WtaFrames& wf, const Geom& g, size_t out_stride, hipStream_t st);

// census_win.hip
hipError_t launch_census_win(const WinImages& wi, int W, int H, const sgm_census_window& cw, hipStream_t st);
hipError_t launch_census_planes(const sgm_census_window& cw, const uint8_t* L, const uint8_t* R, size_t stride, int W,
                                int H, uint64_t* cL, uint64_t* cR, hipStream_t st);

// rectify.hip
hipError_t launch_rectify_map(const double* K, const double* dist, const double* ir, int W, int H, float* mx,
                              float* my, size_t stride, hipStream_t st);
hipError_t launch_remap_cubic(const uint8_t* src, size_t sstride, int sw, int sh, const float* mx, const float* my,
                              size_t mstride, int W, int H, const int16_t* tab, uint8_t* dst, size_t dstride,
                              hipStream_t st);
hipError_t launch_remap_cubic_c3(const uint8_t* src, size_t sstride, int sw, int sh, const float* mx, const float* my,
                                 size_t mstride, int W, int H, const int16_t* tab, uint8_t* dst, size_t dstride,
                                 hipStream_t st);
hipError_t launch_bgr2gray(const uint8_t* src0, const uint8_t* src1, size_t sstride, int W, int H, uint8_t* dst0,
                           uint8_t* dst1, size_t dstride, int set, hipStream_t st);
hipError_t launch_rectify_pair(const RectifyIn& rect, const uint8_t* rawL, const uint8_t* rawR, size_t sstride, int ch,
                               int gray_set, int W, int H, uint8_t* grayL, uint8_t* grayR, uint8_t* rectL,
                               uint8_t* rectR, size_t rstride, hipStream_t st);
void cubic_table(int16_t* tab);
bool rectify_inverse(const double* P, const double* R, double* ir);

// post.hip
hipError_t launch_median3(const int16_t* src, size_t sstride, int16_t* dst, size_t dstride, int W, int H,
                          hipStream_t st);
hipError_t launch_speckle(const int16_t* med, size_t mstride, int16_t* d, size_t stride, int W, int H, int newVal,
                          int maxSize, int maxDiff, int* lab, int* cnt, hipStream_t st);
hipError_t launch_fill16(int16_t* d, size_t stride, int W, int H, int v, hipStream_t st);
hipError_t launch_to_f32(const int16_t* s, size_t ss, float* d, size_t ds, int W, int H, hipStream_t st);

// fill.hip
size_t fill_plane_bytes(int W, int H);
hipError_t launch_fill_holes(const int16_t* src, size_t sstride, int16_t* dst, size_t dstride, int W, int H,
                             int invalid, int mode, int G, int N, int x0, int y0, int x1, int y1, void* planes,
                             hipStream_t st);

// depth.hip
hipError_t launch_disp_to_msg(const int16_t* disp, size_t disp_stride, int W, int H, float min_disp, float max_disp,
                              float* out, size_t out_stride, hipStream_t st);
hipError_t launch_depth_points(const float* disp, size_t disp_stride, int W, int H, const float qf[5], double zmin,
                               double zmax, const uint8_t* color, size_t color_stride, int channels, float* depth,
                               size_t depth_stride, float4* points, int max_points, int* row_count, int* row_off,
                               hipStream_t st);
hipError_t launch_msg_tail(const int16_t* disp, size_t disp_stride, int W, int H, float min_disp, float max_disp,
                           float* msg, size_t msg_stride, const float qf[5], double zmin, double zmax, float* depth,
                           size_t depth_stride, hipStream_t st);

// ocv_cost.hip
hipError_t launch_ocv_cost(const uint8_t* L, const uint8_t* R, size_t stride, const Geom& g, int fullDP,
                           uint8_t* planes, int16_t* bufA, int16_t* bufB, hipStream_t st);
bool ocv_cost_takes_fused(const Geom& g);

// ocv_sgm.hip (paths, WTA)
hipError_t launch_ocv_paths(const int16_t* C, const int16_t* Csat, void* vols, size_t cells, const Geom& g,
                            int dirmask, hipStream_t st, int skipdir = -1);
hipError_t launch_ocv_vwta(const int16_t* C, const int16_t* Csat, const void* vols, size_t cells, int ndir,
                           const Geom& g, uint64_t* res, hipStream_t st);
int ocv_vwta_dir(int ndir);
hipError_t launch_ocv_wta(const int16_t* C, const void* vols, size_t cells, int ndir, const Geom& g, int16_t* out,
                          size_t out_stride, hipStream_t st);
int ocv_evol_mode(const Geom& g, int dirmask, int skipdir);

// pyramid.hip
hipError_t launch_pyr_down(const uint8_t* L, const uint8_t* R, size_t stride, int W, int H, uint8_t* Lc, uint8_t* Rc,
                           uint32_t* KL, uint32_t* KR, hipStream_t st);
hipError_t launch_pyr_refine(const uint32_t* KL, const uint32_t* KR, const int16_t* coarse, size_t cstride, int W,
                             int H, int m, int D, int mc, int radius, int subpixel, int16_t* out, size_t ostride,
                             hipStream_t st);

// bm.hip
hipError_t launch_bm_prefilter(const uint8_t* L, const uint8_t* R, size_t stride, int W, int H, int cap, uint8_t* PL,
                               uint8_t* PR, hipStream_t st);
BmPlan bm_plan(const Geom& g, int n_cu);
hipError_t launch_bm_match(const uint8_t* PL, const uint8_t* PR, const Geom& g, const BmPlan& pl, int16_t* out,
                           size_t ostride, void* gV, int* dbg_vol, int* dbg_tex, hipStream_t st);

}  // namespace sgm
