// ocv_device.h — what at least two sources of the OpenCV-StereoSGBM-compatible modes
// (SGM_MODE_OCV_SGBM5 / _HH8) use: ocv_cost.hip (the cost stage, C') and ocv_sgm.hip (the path
// and WTA stages).
//
// The modes are bit-exact with the CPU restatement oracle/sgm_oracle.c `ocv_match` (which follows
// OpenCV's sequential raster loop), every stage re-expressed in parallel form.
// Volumes: int16 while no path cost can leave int16; otherwise (Geom::wide, e.g. the shipped
// 2448x2048 D=480 block-21 config) int32 path volumes, gated per frame by the cost kernel's
// overflow flag ("OpenCV semantics targets"); in the plain int16 regime with P2 <= 511
// a volume slot may hold the 9-bit deficits e = C' - L instead of L (Geom::evol).
// A helper that only one source uses stays in that source, even if it looks general; no launch_*
// is declared here (sgm_launch.h).
#pragma once
#include "sgm_device.h"

namespace sgm {

__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }
typedef short s16x2_t __attribute__((ext_vector_type(2)));

}  // namespace sgm
