"""MI355X-native SGM disparity engine — Python host mirror of the reference's plugin surface.

The compute path is libsgm_hip.so (hand-written HIP for gfx950, csrc/) behind the C-ABI in
include/sgm_hip.h. This module binds it with ctypes and mirrors, name for name, the
reference's host-side interface for the hot path so tests read like the reference's code:

  * `MatcherHIPSGM`      — AbstractStereoMatcher subclass semantics
                           (reference include/stereoMatcher/abstractStereoMatcher.h:12-92,
                            setters as src/stereoMatcher/matcherOpenCVSGBM.cpp:53-110)
  * `stereo_match`       — generate_disparity.cpp:334-368
  * `process_disparity`  — generate_disparity.cpp:398-456 (x1/16, depth window, MISSING_Z)
  * `parameter_callback` — generate_disparity.cpp:735-845 (cfg sanitising, matcher swap)
  * `image_cb`           — generate_disparity.cpp:635-713 (raw frames + CameraInfo -> rectified
                           images + DisparityImage, one device call in every mode)
  * `image_cb_host`      — the same through sgm_node_frame on host arrays (`Engine.node_frame`), no torch

There is no CPU fallback: if the HIP library is missing or no device is visible, matching
fails loudly (MatcherHIPSGM.forwardMatch returns -1 exactly like the OpenCV wrapper on an
exception, and `Engine` raises).
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libsgm_hip.so")

ABI_VERSION = 5     # include/sgm_hip.h SGM_ABI_VERSION
MODE_OCV_SGBM5 = 0
MODE_OCV_HH8 = 1
MODE_CENSUS8 = 2
MODE_OCV_BM = 3     # cv::StereoBM, the node's default algorithm (restated, unverified against OpenCV)

SGM_OK, SGM_ERR_ARG, SGM_ERR_PARAM, SGM_ERR_DEVICE, SGM_ERR_ALLOC, SGM_ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5

# reference enum (cfg/i3DR_Disparity.cfg:11-17) + the new entry this engine adds
CV_StereoBM, CV_StereoSGBM, I3DR_StereoSGM, CV_StereoBMCuda, CV_StereoBPCuda, CV_StereoCSBPCuda = range(6)
HIP_StereoSGM = 6
HIP_StereoBM = 7     # the same engine in MODE_OCV_BM

MISSING_Z = 10000.0  # image_geometry::StereoCameraModel::MISSING_Z

# sgm_params.ocv_compat: the OpenCV build the OCV modes reproduce (include/sgm_hip.h SGM_OCV_*)
OCV_COL0_LEGACY, OCV_SIMD_SAT, OCV_LANE_TIE = 1, 2, 4
COMPAT_SCALAR = 0                                               # scalar 4.x restatement
COMPAT_NOETIC = OCV_SIMD_SAT                                    # noetic x86-64 (OpenCV 4.2)
COMPAT_MELODIC = OCV_COL0_LEGACY | OCV_SIMD_SAT | OCV_LANE_TIE  # melodic x86-64 (OpenCV 3.2), default
COMPAT_NAMES = {"scalar": COMPAT_SCALAR, "noetic": COMPAT_NOETIC, "melodic": COMPAT_MELODIC}

# COLOR_BGR2GRAY coefficient sets (include/sgm_hip.h SGM_GRAY_*), over a pixel's bytes in memory order
GRAY_Y14 = 0   # OpenCV 3.2 (melodic): (c0*1868 + c1*9617 + c2*4899 + 2^13) >> 14
GRAY_Y15 = 1   # OpenCV 4.x (noetic):  (c0*3735 + c1*19235 + c2*9798 + 2^14) >> 15, unverified against OpenCV
GRAY_COEFFS = {GRAY_Y14: (1868, 9617, 4899, 14), GRAY_Y15: (3735, 19235, 9798, 15)}

# hole filling (include/sgm_hip.h SGM_FILL_*): off, second-lowest candidate, lower median
FILL_OFF, FILL_BACKGROUND, FILL_MEDIAN = 0, 1, 2
FILL_NAMES = {"off": FILL_OFF, "background": FILL_BACKGROUND, "median": FILL_MEDIAN}


def ocv_compat_from_env(default=COMPAT_MELODIC):
    """SGM_HIP_OCV_COMPAT = melodic | noetic | scalar | <bits> (the adapters read the same
    variable)."""
    raw = os.environ.get("SGM_HIP_OCV_COMPAT")
    v = (raw or "").strip().lower()
    if not v:
        return default
    if v in COMPAT_NAMES:
        return COMPAT_NAMES[v]
    try:
        return int(v, 0) & 7
    except ValueError:      # the C++ adapter core (hip_sgm_core.cpp) warns and keeps the default too
        sys.stderr.write(f'SGM_HIP_OCV_COMPAT="{raw}" is not melodic | noetic | scalar | <bits>: using {default}\n')
        return default


def census_paths_from_env(default=8):
    """SGM_HIP_CENSUS_PATHS = 4 | 8: the census mode's path set (the C++ adapter core reads the same
    variable). Any integer is passed on (one other than 4 or 8 fails at match
    time); an unparseable value warns and keeps the default, as hip_sgm_core.cpp does."""
    raw = os.environ.get("SGM_HIP_CENSUS_PATHS")
    v = (raw or "").strip(" \t\n\v\f\r")
    if not v:
        return default
    body = v[1:] if v[0] in "+-" else v
    if not (body.isascii() and body.isdigit()) or abs(int(v)) > 1000000:
        sys.stderr.write(f'SGM_HIP_CENSUS_PATHS="{raw}" is not 4 or 8: using {default}\n')
        return default
    return int(v)


CENSUS_WINDOW_DEFAULT = (9, 7, 1)


def census_window_from_size(size):
    """The census window of a correlation_window_size slider value (sgm_census_window_from_size,
    the one table): (taps_x, taps_y, step)."""
    s = int(size) | 1
    if s <= 3:
        return (3, 3, 1)
    if s <= 9:
        return {5: (5, 5, 1), 7: (7, 7, 1), 9: (9, 7, 1)}[s]
    return (7, 7, 2) if s <= 13 else (9, 7, 2)


def census_window_from_env():
    """SGM_HIP_CENSUS_WINDOW = <tx>x<ty>[/<step>] | cfg (the C++ adapter core reads the same variable,
    INTEGRATION.md §10). Returns (window, follow_cfg): unset or empty: the default 9x7 window;
    "7x7" or "9x7/2": that window, passed on as it is (an invalid one fails at match time), each
    number 1 to 6 decimal digits; "cfg": setWindowSize drives the window through
    census_window_from_size. An unparsable value warns and keeps the default."""
    raw = os.environ.get("SGM_HIP_CENSUS_WINDOW")
    v = (raw or "").strip(" \t\n\v\f\r").lower()
    if not v:
        return CENSUS_WINDOW_DEFAULT, False
    if v == "cfg":
        return CENSUS_WINDOW_DEFAULT, True
    size, _, step = v.partition("/")
    tx, x, ty = size.partition("x")
    nums = [tx, ty] + ([step] if "/" in v else [])
    if not x or not all(n.isascii() and n.isdigit() and len(n) <= 6 for n in nums):
        sys.stderr.write(f'SGM_HIP_CENSUS_WINDOW="{raw}" is not <tx>x<ty>[/<step>] | cfg: using 9x7\n')
        return CENSUS_WINDOW_DEFAULT, False
    return (int(tx), int(ty), int(step) if "/" in v else 1), False


def fill_from_env():
    """SGM_HIP_FILL = off | background | median[:gap[:min]] -> (mode, max_gap, min_neighbours), the
    hole filter of the adapters (the C++ adapter core reads the same variable).
    gap and min are 1 to 6 decimal digits (defaults 16 and 2) and are passed on as they are: a value
    out of range fails at match time. Unset or empty: off. An unparsable value gives off and a note
    on stderr, as hip_sgm_core.cpp does."""
    raw = os.environ.get("SGM_HIP_FILL")
    v = (raw or "").strip(" \t\n\v\f\r").lower()
    if not v:
        return (FILL_OFF, 16, 2)
    parts = v.split(":")
    nums = parts[1:]
    if parts[0] not in FILL_NAMES or len(nums) > 2 or \
            not all(n.isascii() and n.isdigit() and len(n) <= 6 for n in nums):
        sys.stderr.write(f'SGM_HIP_FILL="{raw}" is not off | background | median[:gap[:min]]: hole filling off\n')
        return (FILL_OFF, 16, 2)
    return (FILL_NAMES[parts[0]], int(nums[0]) if len(nums) > 0 else 16, int(nums[1]) if len(nums) > 1 else 2)


def pyramid_from_env():
    """SGM_HIP_PYRAMID = 0 (default) | 1 | scale -> (level, follow_scale), the pyramid level of the
    adapters (the C++ adapter core reads the same variable). "scale":
    setDownsampleScale(s) drives the level (s <= 0.5: level 1, else 0). Unset or empty: level 0. Another
    value warns and means 0, as hip_sgm_core.cpp does."""
    raw = os.environ.get("SGM_HIP_PYRAMID")
    v = (raw or "").strip(" \t\n\v\f\r").lower()
    if v in ("", "0"):
        return 0, False
    if v == "1":
        return 1, False
    if v == "scale":
        return 0, True
    sys.stderr.write(f'SGM_HIP_PYRAMID="{raw}" is not 0 | 1 | scale: pyramid level 0\n')
    return 0, False


def fill_when_from_env():
    """SGM_HIP_FILL_WHEN = always (default) | interp: with "interp" the node's interp flag drives the
    hole filter (and replaces the Q3 right-view result); another value warns and means always."""
    raw = os.environ.get("SGM_HIP_FILL_WHEN")
    v = (raw or "").strip(" \t\n\v\f\r").lower()
    if v in ("", "always", "interp"):
        return v or "always"
    sys.stderr.write(f'SGM_HIP_FILL_WHEN="{raw}" is not always | interp: using always\n')
    return "always"


EXPORTS = [
    "sgm_device_count", "sgm_create", "sgm_destroy", "sgm_default_params", "sgm_set_params", "sgm_get_params",
    "sgm_check_params", "sgm_match", "sgm_match_f32", "sgm_match_device", "sgm_match_device_batch", "sgm_match_batch", "sgm_match_tiled",
    "sgm_match_tiled_device", "sgm_match_tiled_exact", "sgm_abi_version", "sgm_host_register", "sgm_host_unregister", "sgm_synchronize", "sgm_last_error",
    "sgm_set_profiling", "sgm_get_stage_times", "sgm_profiled_matches", "sgm_stage_name", "sgm_stage_bytes",
    "sgm_stage_launches", "sgm_disparity_to_msg", "sgm_calc_q", "sgm_depth_points", "sgm_rectify_map",
    "sgm_remap_cubic", "sgm_cubic_table", "sgm_set_rectification", "sgm_match_device_batch_rect", "sgm_debug_census",
    "sgm_debug_census_path", "sgm_debug_ocv_cost", "sgm_debug_median3", "sgm_debug_speckle", "sgm_debug_path_items",
    "sgm_default_bm_params", "sgm_set_bm_params", "sgm_get_bm_params", "sgm_check_bm_params", "sgm_debug_bm_prefilter",
    "sgm_debug_bm_sad", "sgm_set_census_paths", "sgm_get_census_paths",
    "sgm_bgr2gray", "sgm_remap_cubic_c3", "sgm_set_raw_format", "sgm_get_raw_format",
    "sgm_node_frame", "sgm_node_frame_map_builds",
    "sgm_default_fill_params", "sgm_set_fill_params", "sgm_get_fill_params", "sgm_check_fill_params",
    "sgm_fill_holes", "sgm_debug_fill",
    "sgm_default_census_window", "sgm_set_census_window", "sgm_get_census_window", "sgm_check_census_window",
    "sgm_census_window_from_size",
    "sgm_debug_bm_plan",
    "sgm_default_pyramid_params", "sgm_set_pyramid_params", "sgm_get_pyramid_params", "sgm_check_pyramid_params",
    "sgm_pyramid_plan", "sgm_debug_pyr_down", "sgm_debug_pyr_refine",
    "sgm_debug_post",
]


class SgmParams(ctypes.Structure):
    """`sgm_params` of include/sgm_hip.h."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "mode", "min_disparity", "num_disparities", "block_size", "p1", "p2",
        "uniqueness_ratio", "disp12_max_diff", "prefilter_cap", "speckle_window_size",
        "speckle_range", "subpixel", "lr_check", "median", "ocv_compat")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def copy(self, **kw):
        p = SgmParams()
        for n, _ in self._fields_:
            setattr(p, n, getattr(self, n))
        for k, v in kw.items():
            setattr(p, k, int(v))
        return p


class BmParams(ctypes.Structure):
    """`sgm_bm_params` of include/sgm_hip.h: the two cv::StereoBM values `sgm_params` has no field for."""
    _fields_ = [("texture_threshold", ctypes.c_int), ("prefilter_size", ctypes.c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def copy(self, **kw):
        b = BmParams(self.texture_threshold, self.prefilter_size)
        for k, v in kw.items():
            setattr(b, k, int(v))
        return b


class FillParams(ctypes.Structure):
    """`sgm_fill_params` of include/sgm_hip.h: the hole-filling post filter (mode FILL_*, max_gap
    1..255, min_neighbours 1..8)."""
    _fields_ = [("mode", ctypes.c_int), ("max_gap", ctypes.c_int), ("min_neighbours", ctypes.c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def copy(self, **kw):
        f = FillParams(self.mode, self.max_gap, self.min_neighbours)
        for k, v in kw.items():
            setattr(f, k, int(v))
        return f


class CensusWindow(ctypes.Structure):
    """sgm_census_window: taps_x x taps_y comparisons, `step` pixels apart."""
    _fields_ = [("taps_x", ctypes.c_int), ("taps_y", ctypes.c_int), ("step", ctypes.c_int)]

    def as_tuple(self):
        return (self.taps_x, self.taps_y, self.step)


class PyramidParams(ctypes.Structure):
    """`sgm_pyramid_params` of include/sgm_hip.h: level 0 (off) or 1 (half-resolution match refined at
    full resolution over +-radius disparities, radius 1..2)."""
    _fields_ = [("level", ctypes.c_int), ("radius", ctypes.c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


PYRAMID_PLAN_FIELDS = ("Wc", "Hc", "mc", "Dc", "invalid_c", "invalid")


class CameraInfo(ctypes.Structure):
    """`sgm_camera_info` of include/sgm_hip.h: one camera's K, D (n_dist of 12), R (has_R), P."""
    _fields_ = [("K", ctypes.c_double * 9), ("D", ctypes.c_double * 12), ("n_dist", ctypes.c_int),
                ("has_R", ctypes.c_int), ("R", ctypes.c_double * 9), ("P", ctypes.c_double * 12)]

    @classmethod
    def of(cls, info):
        """From a CameraInfo given as image_cb takes it (mapping, object or (K, D, R, P); R None: identity)."""
        if isinstance(info, cls):
            return info
        K, D, R, P = _camera_info(info)
        if len(D) > 12:
            raise ValueError("at most 12 distortion coefficients")
        c = cls()
        c.K[:] = K.ravel()
        c.D[:len(D)] = D
        c.n_dist = len(D)
        c.has_R = 0 if R is None else 1
        if R is not None:
            c.R[:] = R.ravel()
        c.P[:] = P.ravel()
        return c


class NodeFrameIO(ctypes.Structure):
    """`sgm_node_frame_io` of include/sgm_hip.h: the host buffers of one sgm_node_frame call."""
    _fields_ = [("struct_size", ctypes.c_size_t), ("raw_left", ctypes.c_void_p), ("raw_right", ctypes.c_void_p),
                ("raw_stride", ctypes.c_size_t), ("width", ctypes.c_int), ("height", ctypes.c_int),
                ("min_disparity", ctypes.c_float), ("max_disparity", ctypes.c_float),
                ("rect_left", ctypes.c_void_p), ("rect_right", ctypes.c_void_p), ("rect_stride", ctypes.c_size_t),
                ("disparity", ctypes.c_void_p), ("disparity_stride", ctypes.c_size_t),
                ("depth", ctypes.c_void_p), ("depth_stride", ctypes.c_size_t), ("q5", ctypes.POINTER(ctypes.c_double)),
                ("depth_min", ctypes.c_double), ("depth_max", ctypes.c_double)]


_lib = None


def load_library(path=None):
    """Load libsgm_hip.so (SGM_HIP_LIB overrides the in-tree path, e.g. for an experimental
    build); raises if it is missing (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("SGM_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"libsgm_hip.so not found at {path}: run build() / build_ext.py first")
    # One HIP runtime per process: torch ships its own libamdhip64 (SONAME libamdhip64.so.7).
    # Loading torch first makes the dynamic loader bind this library to that same copy, so
    # device pointers and streams from torch are valid here (and torch still finds the GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    P = ctypes.POINTER
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.sgm_device_count.restype = ci
    L.sgm_create.argtypes = [P(ctypes.c_void_p), ci]
    L.sgm_destroy.argtypes = [vp]
    L.sgm_destroy.restype = None
    L.sgm_default_params.argtypes = [P(SgmParams), ci]
    L.sgm_default_params.restype = None
    L.sgm_set_params.argtypes = [vp, P(SgmParams)]
    L.sgm_get_params.argtypes = [vp, P(SgmParams)]
    L.sgm_check_params.argtypes = [P(SgmParams), ci, ci]
    L.sgm_match.argtypes = [vp, vp, vp, ci, ci, sz, vp, sz]
    L.sgm_match_f32.argtypes = [vp, vp, vp, ci, ci, sz, vp, sz]
    L.sgm_match_device.argtypes = [vp, vp, vp, ci, ci, sz, vp, sz, vp]
    L.sgm_match_device_batch.argtypes = [vp, P(vp), P(vp), ci, ci, ci, sz, P(vp), sz, vp]
    L.sgm_match_batch.argtypes = [vp, P(vp), P(vp), ci, ci, ci, sz, P(vp), sz, P(ci), ci]
    L.sgm_match_tiled.argtypes = [vp, vp, vp, ci, ci, sz, vp, sz, ci, ci, P(ci), ci]
    L.sgm_match_tiled_device.argtypes = [vp, vp, vp, ci, ci, sz, vp, sz, ci, ci, P(ci), ci, vp]
    L.sgm_match_tiled_exact.argtypes = [vp, vp, vp, ci, ci, sz, vp, sz, ci, P(ci), ci]
    L.sgm_abi_version.restype = ci
    L.sgm_host_register.argtypes = [vp, vp, sz]
    L.sgm_host_unregister.argtypes = [vp, vp]
    if L.sgm_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: C-ABI version {L.sgm_abi_version()} != {ABI_VERSION} (include/sgm_hip.h "
                          "SGM_ABI_VERSION): rebuild the library")
    L.sgm_synchronize.argtypes = [vp]
    L.sgm_last_error.argtypes = [vp]
    L.sgm_last_error.restype = ctypes.c_char_p
    L.sgm_set_profiling.argtypes = [vp, ci]
    L.sgm_get_stage_times.argtypes = [vp, P(ctypes.c_float), ci]
    L.sgm_profiled_matches.argtypes = [vp]
    L.sgm_stage_name.argtypes = [vp, ci]
    L.sgm_stage_name.restype = ctypes.c_char_p
    L.sgm_stage_bytes.argtypes = [vp, ci]
    L.sgm_stage_launches.argtypes = [vp, ci]
    L.sgm_disparity_to_msg.argtypes = [vp, vp, sz, ci, ci, ctypes.c_float, ctypes.c_float, vp, sz, vp]
    L.sgm_calc_q.argtypes = [P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double)]
    L.sgm_calc_q.restype = None
    L.sgm_depth_points.argtypes = [vp, vp, sz, ci, ci, vp, sz, ci, P(ctypes.c_double), ctypes.c_double,
                                   ctypes.c_double, vp, sz, vp, ci, vp, vp]
    L.sgm_stage_bytes.restype = ctypes.c_double
    L.sgm_rectify_map.argtypes = [vp, P(ctypes.c_double), P(ctypes.c_double), ci, P(ctypes.c_double),
                                  P(ctypes.c_double), ci, ci, vp, vp, sz, vp]
    L.sgm_remap_cubic.argtypes = [vp, vp, sz, ci, ci, vp, vp, sz, ci, ci, vp, sz, vp]
    L.sgm_cubic_table.argtypes = [vp]
    L.sgm_set_rectification.argtypes = [vp, vp, vp, vp, vp, sz, ci, ci]
    L.sgm_match_device_batch_rect.argtypes = [vp, P(vp), P(vp), ci, ci, ci, sz, P(vp), P(vp), sz, P(vp), sz, vp]
    L.sgm_cubic_table.restype = None
    L.sgm_debug_census.argtypes = [vp, vp, ci, ci, sz, vp]
    L.sgm_debug_census_path.argtypes = [vp, vp, vp, ci, ci, sz, ci, vp]
    L.sgm_debug_ocv_cost.argtypes = [vp, vp, vp, ci, ci, sz, vp]
    L.sgm_debug_median3.argtypes = [vp, vp, ci, ci]
    L.sgm_debug_speckle.argtypes = [vp, vp, ci, ci, ci, ci, ci]
    L.sgm_debug_path_items.argtypes = [P(SgmParams), ci, ci, ctypes.c_uint, ci, ci, ci, vp, ci]
    L.sgm_default_bm_params.argtypes = [P(BmParams)]
    L.sgm_default_bm_params.restype = None
    L.sgm_set_bm_params.argtypes = [vp, P(BmParams)]
    L.sgm_get_bm_params.argtypes = [vp, P(BmParams)]
    L.sgm_check_bm_params.argtypes = [P(SgmParams), P(BmParams), ci, ci]
    L.sgm_set_census_paths.argtypes = [vp, ci]
    L.sgm_get_census_paths.argtypes = [vp, P(ci)]
    # the colour entry points came under ABI version 5: callers check for the symbols
    for name in ("sgm_bgr2gray", "sgm_remap_cubic_c3", "sgm_set_raw_format", "sgm_get_raw_format"):
        if not hasattr(L, name):
            raise ImportError(f"{path}: {name} is missing: rebuild the library")
    L.sgm_bgr2gray.argtypes = [vp, vp, sz, ci, ci, vp, sz, ci, vp]
    L.sgm_remap_cubic_c3.argtypes = [vp, vp, sz, ci, ci, vp, vp, sz, ci, ci, vp, sz, vp]
    L.sgm_set_raw_format.argtypes = [vp, ci, ci]
    L.sgm_get_raw_format.argtypes = [vp, P(ci), P(ci)]
    # sgm_node_frame came the same way
    for name in ("sgm_node_frame", "sgm_node_frame_map_builds"):
        if not hasattr(L, name):
            raise ImportError(f"{path}: {name} is missing: rebuild the library")
    L.sgm_node_frame.argtypes = [vp, P(CameraInfo), P(CameraInfo), P(NodeFrameIO)]
    L.sgm_node_frame_map_builds.argtypes = [vp]
    L.sgm_debug_bm_prefilter.argtypes = [vp, vp, ci, ci, sz, vp]
    L.sgm_debug_bm_sad.argtypes = [vp, vp, vp, ci, ci, sz, vp, vp]
    # ... and the hole-filling entry points
    for name in ("sgm_default_fill_params", "sgm_set_fill_params", "sgm_get_fill_params", "sgm_check_fill_params",
                 "sgm_fill_holes", "sgm_debug_fill"):
        if not hasattr(L, name):
            raise ImportError(f"{path}: {name} is missing: rebuild the library")
    L.sgm_default_fill_params.argtypes = [P(FillParams)]
    L.sgm_default_fill_params.restype = None
    L.sgm_set_fill_params.argtypes = [vp, P(FillParams)]
    L.sgm_get_fill_params.argtypes = [vp, P(FillParams)]
    L.sgm_check_fill_params.argtypes = [P(FillParams)]
    L.sgm_fill_holes.argtypes = [vp, vp, sz, ci, ci, ci, P(FillParams), ci, ci, ci, ci, vp, sz, vp]
    L.sgm_debug_fill.argtypes = [vp, vp, ci, ci, ci, P(FillParams), ci, ci, ci, ci]
    L.sgm_default_census_window.argtypes = [P(CensusWindow)]
    L.sgm_default_census_window.restype = None
    L.sgm_set_census_window.argtypes = [vp, P(CensusWindow)]
    L.sgm_get_census_window.argtypes = [vp, P(CensusWindow)]
    L.sgm_check_census_window.argtypes = [P(CensusWindow)]
    L.sgm_census_window_from_size.argtypes = [ci, P(CensusWindow)]
    if not hasattr(L, "sgm_debug_bm_plan"):
        raise ImportError(f"{path}: sgm_debug_bm_plan is missing: rebuild the library")
    L.sgm_debug_bm_plan.argtypes = [P(SgmParams), P(BmParams), ci, ci, ci, P(ci * 12)]
    # ... and the pyramid entry points
    for name in ("sgm_default_pyramid_params", "sgm_set_pyramid_params", "sgm_get_pyramid_params",
                 "sgm_check_pyramid_params", "sgm_pyramid_plan", "sgm_debug_pyr_down", "sgm_debug_pyr_refine"):
        if not hasattr(L, name):
            raise ImportError(f"{path}: {name} is missing: rebuild the library")
    L.sgm_default_pyramid_params.argtypes = [P(PyramidParams)]
    L.sgm_default_pyramid_params.restype = None
    L.sgm_set_pyramid_params.argtypes = [vp, P(PyramidParams)]
    L.sgm_get_pyramid_params.argtypes = [vp, P(PyramidParams)]
    L.sgm_check_pyramid_params.argtypes = [P(PyramidParams)]
    L.sgm_pyramid_plan.argtypes = [P(SgmParams), P(BmParams), P(PyramidParams), ci, ci, P(ci * 6)]
    L.sgm_debug_pyr_down.argtypes = [vp, vp, vp, ci, ci, sz, vp, vp]
    L.sgm_debug_pyr_refine.argtypes = [vp, vp, vp, ci, ci, sz, vp, ci, ci, ci, ci, ci, vp]
    # ... and the post filters as a match launches them
    if not hasattr(L, "sgm_debug_post"):
        raise ImportError(f"{path}: sgm_debug_post is missing: rebuild the library")
    L.sgm_debug_post.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
    _lib = L
    return L


def default_params(mode=MODE_CENSUS8, **kw):
    p = SgmParams()
    load_library().sgm_default_params(ctypes.byref(p), int(mode))
    for k, v in kw.items():
        setattr(p, k, int(v))
    return p


def default_bm_params(**kw):
    b = BmParams()
    load_library().sgm_default_bm_params(ctypes.byref(b))
    for k, v in kw.items():
        setattr(b, k, int(v))
    return b


def default_fill_params(**kw):
    f = FillParams()
    load_library().sgm_default_fill_params(ctypes.byref(f))
    for k, v in kw.items():
        setattr(f, k, int(v))
    return f


def default_pyramid_params(**kw):
    y = PyramidParams()
    load_library().sgm_default_pyramid_params(ctypes.byref(y))
    for k, v in kw.items():
        setattr(y, k, int(v))
    return y


def pyramid_plan(params, pyramid, width, height, bm_params=None):
    """sgm_pyramid_plan: the geometry a match of a width x height frame runs its matcher at, as a
    dict of PYRAMID_PLAN_FIELDS (host-only, needs no device); raises SGMError with the status a match
    would return."""
    out = (ctypes.c_int * 6)()
    rc = load_library().sgm_pyramid_plan(ctypes.byref(params), ctypes.byref(bm_params) if bm_params is not None else None,
                                         ctypes.byref(pyramid), int(width), int(height), ctypes.byref(out))
    if rc != SGM_OK:
        raise SGMError(rc, "sgm_pyramid_plan")
    return dict(zip(PYRAMID_PLAN_FIELDS, out))


def bm_geometry(params, width, height):
    """(X0, X1, width1, D, invalid) of MODE_OCV_BM: columns [X0, X1) are computed, X0 = max(D - 1 +
    minD, 0), X1 = min(W, W + minD); an empty range leaves the whole frame invalid."""
    minD, D = params.min_disparity, params.num_disparities
    x0, x1 = max(D - 1 + minD, 0), min(width, width + minD)
    w1 = 0 if (x0 >= width or x1 <= 0 or x1 <= x0) else x1 - x0
    return dict(X0=x0, X1=x1, width1=w1, D=D, invalid=(minD - 1) * 16)


BM_PLAN_FIELDS = ("TX", "nsx", "nsy", "RB", "waves", "lds", "vglobal", "wide", "nk", "Dp", "width1", "rows")


def bm_plan(params, bm_params, width, height, n_cu):
    """sgm_debug_bm_plan: the tiling of the fused MODE_OCV_BM kernel for a width x height frame on
    a device of n_cu compute units, as a dict of BM_PLAN_FIELDS (host-only, needs no device).
    SGM_BM_VGLOBAL applies as at a match."""
    out = (ctypes.c_int * 12)()
    rc = load_library().sgm_debug_bm_plan(ctypes.byref(params), ctypes.byref(bm_params), int(width), int(height),
                                          int(n_cu), ctypes.byref(out))
    if rc != SGM_OK:
        raise SGMError(rc, "sgm_debug_bm_plan")
    return dict(zip(BM_PLAN_FIELDS, out))


def device_count():
    return int(load_library().sgm_device_count())


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class SGMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sgm status {code}: {msg}")
        self.code = code


def effective_geometry(params, width, height):
    """(minX1, maxX1, width1, D, invalid) — OpenCV computeDisparitySGBM column range."""
    minD, D = params.min_disparity, params.num_disparities
    maxD = minD + D
    minX1 = max(maxD, 0)
    maxX1 = width + min(minD, 0)
    return dict(minX1=minX1, maxX1=maxX1, width1=maxX1 - minX1, D=D, invalid=(minD - 1) * 16)


class Engine:
    """Owning wrapper of one `sgm_handle` (one device, one stream, one workspace)."""

    def __init__(self, device=0, params=None):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.sgm_create(ctypes.byref(h), int(device))
        if rc != SGM_OK:
            raise SGMError(rc, f"cannot open HIP device {device} ({self.lib.sgm_device_count()} visible)")
        self.h = h
        self.device = device
        if params is not None:
            self.set_params(params)

    def close(self):
        if getattr(self, "h", None):
            self.lib.sgm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self):
        e = self.lib.sgm_last_error(self.h)
        return e.decode() if e else ""

    def _check(self, rc):
        if rc != SGM_OK:
            raise SGMError(rc, self.error())

    def set_params(self, p):
        self._check(self.lib.sgm_set_params(self.h, ctypes.byref(p)))

    def get_params(self):
        p = SgmParams()
        self._check(self.lib.sgm_get_params(self.h, ctypes.byref(p)))
        return p

    def set_bm_params(self, b):
        """The BM-only parameters (texture threshold, pre-filter size) of MODE_OCV_BM matches."""
        self._check(self.lib.sgm_set_bm_params(self.h, ctypes.byref(b)))

    def get_bm_params(self):
        b = BmParams()
        self._check(self.lib.sgm_get_bm_params(self.h, ctypes.byref(b)))
        return b

    def set_census_paths(self, paths):
        """Census mode: 8 aggregation paths (default) or 4 (down, up, left, right). Stored as given;
        a value other than 4 or 8 fails at match time."""
        self._check(self.lib.sgm_set_census_paths(self.h, int(paths)))

    def get_census_paths(self):
        n = ctypes.c_int()
        self._check(self.lib.sgm_get_census_paths(self.h, ctypes.byref(n)))
        return n.value

    def set_census_window(self, taps_x=9, taps_y=7, step=1):
        """Census mode: the census window, taps_x x taps_y comparisons `step` pixels apart (taps_x 3,
        5, 7 or 9, taps_y 3, 5 or 7, step 1 or 2; the default is the 9x7 window). Stored as given;
        an invalid window fails at match time."""
        w = CensusWindow(int(taps_x), int(taps_y), int(step))
        self._check(self.lib.sgm_set_census_window(self.h, ctypes.byref(w)))

    def get_census_window(self):
        w = CensusWindow()
        self._check(self.lib.sgm_get_census_window(self.h, ctypes.byref(w)))
        return w.as_tuple()

    def set_raw_format(self, channels=1, gray_set=GRAY_Y14):
        """The frames the match entry points take: 1 channel (8UC1, the default) or 3 (interleaved
        8UC3, converted on the device with COLOR_BGR2GRAY set `gray_set`; strides in bytes). Stored
        as given; other values fail at match time."""
        self._check(self.lib.sgm_set_raw_format(self.h, int(channels), int(gray_set)))

    def get_raw_format(self):
        c, g = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.sgm_get_raw_format(self.h, ctypes.byref(c), ctypes.byref(g)))
        return c.value, g.value

    def set_fill_params(self, f):
        """The hole-filling post filter of every match of this engine (FillParams; mode FILL_OFF
        switches it off). Stored as given; bad values fail at match time."""
        self._check(self.lib.sgm_set_fill_params(self.h, ctypes.byref(f)))

    def get_fill_params(self):
        f = FillParams()
        self._check(self.lib.sgm_get_fill_params(self.h, ctypes.byref(f)))
        return f

    def set_pyramid_params(self, y):
        """The pyramid level of every match of this engine (PyramidParams; level 1: a half-resolution
        match refined at full resolution). Stored as given; bad values fail at match time."""
        self._check(self.lib.sgm_set_pyramid_params(self.h, ctypes.byref(y)))

    def get_pyramid_params(self):
        y = PyramidParams()
        self._check(self.lib.sgm_get_pyramid_params(self.h, ctypes.byref(y)))
        return y

    def pyramid_plan(self, width, height):
        """pyramid_plan() of this engine's parameters, BM parameters and pyramid parameters."""
        return pyramid_plan(self.get_params(), self.get_pyramid_params(), width, height, self.get_bm_params())

    def pyr_down(self, left, right):
        """sgm_debug_pyr_down: both u8 images halved (2x2 box average, replicate clamping)."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        if left.ndim != 2 or left.shape != right.shape:
            raise ValueError("left/right must be equal-size 2-D u8 images")
        h, w = left.shape
        ol = np.empty(((h + 1) // 2, (w + 1) // 2), np.uint8)
        orr = np.empty_like(ol)
        self._check(self.lib.sgm_debug_pyr_down(self.h, _ptr(left), _ptr(right), w, h, w, _ptr(ol), _ptr(orr)))
        return ol, orr

    def pyr_refine(self, left, right, coarse, m, D, mc, radius=2, subpixel=True):
        """sgm_debug_pyr_refine: the level-1 refinement of a coarse int16 image on the full-resolution
        pair (m, D: the full-resolution range; mc: the coarse minimum)."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        coarse = np.ascontiguousarray(coarse, np.int16)
        if left.ndim != 2 or left.shape != right.shape:
            raise ValueError("left/right must be equal-size 2-D u8 images")
        h, w = left.shape
        if coarse.shape != ((h + 1) // 2, (w + 1) // 2):
            raise ValueError("coarse must be the ((h + 1) // 2, (w + 1) // 2) int16 image")
        out = np.empty((h, w), np.int16)
        self._check(self.lib.sgm_debug_pyr_refine(self.h, _ptr(left), _ptr(right), w, h, w, _ptr(coarse), int(m), int(D),
                                                  int(mc), int(radius), 1 if subpixel else 0, _ptr(out)))
        return out

    def fill_holes(self, d_src, src_stride, width, height, invalid, params, rect, d_dst, dst_stride, stream=None):
        """sgm_fill_holes on device pointers (int16 images, strides in elements): the holes of
        rect = (x0, y0, x1, y1) filled under `params`; asynchronous on `stream`."""
        x0, y0, x1, y1 = (int(v) for v in rect)
        self._check(self.lib.sgm_fill_holes(self.h, ctypes.c_void_p(d_src), int(src_stride), int(width), int(height),
                                            int(invalid), ctypes.byref(params), x0, y0, x1, y1,
                                            ctypes.c_void_p(d_dst), int(dst_stride), ctypes.c_void_p(stream or 0)))

    def fill(self, disp, invalid, params, rect=None):
        """The hole filter on a host int16 image (sgm_debug_fill); rect = (x0, y0, x1, y1), default the
        whole image. Returns the filled copy."""
        out = np.ascontiguousarray(disp, np.int16).copy()
        if out.ndim != 2:
            raise ValueError("disp must be a 2-D int16 image")
        h, w = out.shape
        x0, y0, x1, y1 = (int(v) for v in (rect if rect is not None else (0, 0, w, h)))
        self._check(self.lib.sgm_debug_fill(self.h, _ptr(out), w, h, int(invalid), ctypes.byref(params), x0, y0, x1, y1))
        return out

    def _host_pair(self, left, right):
        """Contiguous u8 host frames of a match: H x W, or H x W x 3 once set_raw_format(3, ..) was
        called. Returns (left, right, h, w, row bytes)."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        ch = 3 if self.get_raw_format()[0] == 3 else 1
        if left.shape != right.shape or left.ndim != (3 if ch == 3 else 2) or (ch == 3 and left.shape[2] != 3):
            raise ValueError("left/right must be equal-size 2-D u8 images" if ch == 1 else
                             "left/right must be equal-size H x W x 3 u8 images (set_raw_format: 3 channels)")
        h, w = left.shape[:2]
        return left, right, h, w, w * ch

    def match(self, left, right):
        left, right, h, w, row = self._host_pair(left, right)
        out = np.empty((h, w), np.int16)
        self._check(self.lib.sgm_match(self.h, _ptr(left), _ptr(right), w, h, row, _ptr(out), w))
        return out

    def match_f32(self, left, right, out=None):
        """sgm_match_f32: float32 disparity (x16 fixed point, the CV_32FC1 the node's matcher
        contract returns), converted on the device; `out` (float32 rows) is filled in place."""
        left, right, h, w, row = self._host_pair(left, right)
        if out is None:
            out = np.empty((h, w), np.float32)
        if out.dtype != np.float32 or out.shape != (h, w) or out.strides[1] != 4 or out.strides[0] < 4 * w:
            raise ValueError("out must be a float32 (h, w) row-strided array")
        self._check(self.lib.sgm_match_f32(self.h, _ptr(left), _ptr(right), w, h, row, _ptr(out), out.strides[0] // 4))
        return out

    def match_device(self, d_left, d_right, width, height, stride, d_out, out_stride, stream=None):
        """Device pointers (ints) already resident in HBM; async on `stream` (int handle)."""
        self._check(self.lib.sgm_match_device(self.h, ctypes.c_void_p(d_left), ctypes.c_void_p(d_right), width,
                                              height, stride, ctypes.c_void_p(d_out), out_stride,
                                              ctypes.c_void_p(stream) if stream else None))

    def match_device_batch(self, d_lefts, d_rights, width, height, stride, d_outs, out_stride, stream=None):
        """Frame batch of device pointers; census mode pipelines consecutive frames (the
        aggregation of frame i+1 shares one launch with the WTA of frame i)."""
        n = len(d_lefts)
        arr = ctypes.c_void_p * max(n, 1)
        self._check(self.lib.sgm_match_device_batch(self.h, arr(*d_lefts), arr(*d_rights), n, width, height, stride,
                                                    arr(*d_outs), out_stride,
                                                    ctypes.c_void_p(stream) if stream else None))

    def set_rectification(self, maps_left=None, maps_right=None, map_stride=0, src_width=0, src_height=0):
        """Raw inputs from now on: device matches rectify through the (map_x, map_y) device
        pointers of each camera (None, None: off), inside the census tiles in the census mode and
        in a pre-pass of each frame in the OCV and BM modes."""
        vp = ctypes.c_void_p
        ml = maps_left or (None, None)
        mr = maps_right or (None, None)
        self._check(self.lib.sgm_set_rectification(self.h, vp(ml[0]), vp(ml[1]), vp(mr[0]), vp(mr[1]), map_stride,
                                                   src_width, src_height))

    def match_device_batch_rect(self, d_lefts, d_rights, width, height, raw_stride, d_rect_lefts, d_rect_rights,
                                rect_stride, d_outs, out_stride, stream=None):
        """match_device_batch on raw frames that also returns the rectified images."""
        n = len(d_lefts)
        arr = ctypes.c_void_p * max(n, 1)
        rl = arr(*d_rect_lefts) if d_rect_lefts is not None else None
        rr = arr(*d_rect_rights) if d_rect_rights is not None else None
        self._check(self.lib.sgm_match_device_batch_rect(self.h, arr(*d_lefts), arr(*d_rights), n, width, height,
                                                         raw_stride, rl, rr, rect_stride, arr(*d_outs), out_stride,
                                                         ctypes.c_void_p(stream) if stream else None))

    def node_frame(self, left_raw, right_raw, info_left, info_right, min_disparity, max_disparity, rect_left=True,
                   rect_right=True, disparity=None, depth=None, q5=None, depth_min=0.0, depth_max=0.0):
        """sgm_node_frame on numpy arrays: the node's imageCb compute in one host call. left_raw /
        right_raw: u8 H x W, or H x W x 3 after set_raw_format(3, ..); row-strided views pass without
        a copy when both have one row stride. info_*: the cameras (CameraInfo, or what image_cb
        takes). rect_left / rect_right: True (a new array), None / False (not wanted) or a u8 array
        of the raw shape (row-strided, one stride for both) filled in place; disparity: None (a new
        array) or a float32 H x W row-strided array; depth: None / False, True or such an array, with
        q5 = (Q23, Q03, Q13, Q32, Q33). Returns (rect_left, rect_right, disparity, depth)."""
        ch = 3 if self.get_raw_format()[0] == 3 else 1

        def rows(a, dtype, isz):
            return (a.dtype == dtype and a.strides[-1] == isz and (a.ndim == 2 or a.strides[1] == 3 * isz) and
                    a.strides[0] >= a.shape[1] * (a.strides[1] if a.ndim == 3 else isz))

        left_raw, right_raw = np.asarray(left_raw), np.asarray(right_raw)
        if left_raw.shape != right_raw.shape or left_raw.ndim != (3 if ch == 3 else 2) or (ch == 3 and left_raw.shape[2] != 3):
            raise ValueError("left/right must be equal-size 2-D u8 images" if ch == 1 else
                             "left/right must be equal-size H x W x 3 u8 images (set_raw_format: 3 channels)")
        if not (rows(left_raw, np.uint8, 1) and rows(right_raw, np.uint8, 1) and left_raw.strides[0] == right_raw.strides[0]):
            left_raw, right_raw = np.ascontiguousarray(left_raw, np.uint8), np.ascontiguousarray(right_raw, np.uint8)
        h, w = left_raw.shape[:2]
        rect = [np.empty(left_raw.shape, np.uint8) if r is True else (None if r is None or r is False else r)
                for r in (rect_left, rect_right)]
        for r in rect:
            if r is not None and not (r.shape == left_raw.shape and rows(r, np.uint8, 1)):
                raise ValueError("a rectified output must be a u8 row-strided array of the raw frames' shape")
        if rect[0] is not None and rect[1] is not None and rect[0].strides[0] != rect[1].strides[0]:
            raise ValueError("the rectified outputs must have one common row stride")
        if disparity is None:
            disparity = np.empty((h, w), np.float32)
        if depth is True:
            depth = np.empty((h, w), np.float32)
        elif depth is False:
            depth = None
        for a in (disparity, depth):
            if a is not None and not (a.shape == (h, w) and a.ndim == 2 and rows(a, np.float32, 4) and a.strides[0] % 4 == 0):
                raise ValueError("disparity / depth must be float32 (h, w) row-strided arrays")
        io = NodeFrameIO()
        io.struct_size = ctypes.sizeof(NodeFrameIO)
        io.raw_left, io.raw_right, io.raw_stride = left_raw.ctypes.data, right_raw.ctypes.data, left_raw.strides[0]
        io.width, io.height = w, h
        io.min_disparity, io.max_disparity = float(min_disparity), float(max_disparity)
        io.rect_left = rect[0].ctypes.data if rect[0] is not None else None
        io.rect_right = rect[1].ctypes.data if rect[1] is not None else None
        io.rect_stride = next((r.strides[0] for r in rect if r is not None), 0)
        io.disparity, io.disparity_stride = disparity.ctypes.data, disparity.strides[0] // 4
        qv = None
        if depth is not None:
            io.depth, io.depth_stride = depth.ctypes.data, depth.strides[0] // 4
            if q5 is not None:
                qv = (ctypes.c_double * 5)(*[float(v) for v in q5])
                io.q5 = ctypes.cast(qv, ctypes.POINTER(ctypes.c_double))
        io.depth_min, io.depth_max = float(depth_min), float(depth_max)
        cl, cr = CameraInfo.of(info_left), CameraInfo.of(info_right)
        self._check(self.lib.sgm_node_frame(self.h, ctypes.byref(cl), ctypes.byref(cr), ctypes.byref(io)))
        return rect[0], rect[1], disparity, depth

    def node_frame_map_builds(self):
        """How often node_frame (re)built the cached rectification maps of this engine."""
        return int(self.lib.sgm_node_frame_map_builds(self.h))

    def synchronize(self):
        self._check(self.lib.sgm_synchronize(self.h))

    def match_batch(self, lefts, rights, devices=None, outs=None):
        """Host frames, sharded frame i -> devices[i % n] and streamed through pinned rings
        (sgm_match_batch). Row-strided views (one common row stride per side) are passed
        without a copy; `outs` (int16 arrays or row-strided views, one stride) are filled in
        place when given."""
        n = len(lefts)
        h, w = lefts[0].shape

        def rows(arrs, dtype):
            # a row-strided view passes as is; broadcast / overlapping / reversed views
            # (strides[0] < w * itemsize or <= 0) are compacted first
            arrs = [a if (a.dtype == dtype and a.ndim == 2 and a.strides[1] == a.itemsize and
                          a.strides[0] % a.itemsize == 0 and a.strides[0] >= w * a.itemsize)
                    else np.ascontiguousarray(a, dtype) for a in arrs]
            st = {a.strides[0] // a.itemsize for a in arrs}
            if len(st) != 1:   # one stride per side: compact the odd ones out
                arrs = [np.ascontiguousarray(a) for a in arrs]
                st = {w}
            return arrs, st.pop()

        lefts, sl = rows(lefts, np.uint8)
        rights, sr = rows(rights, np.uint8)
        if sl != sr:
            lefts = [np.ascontiguousarray(a) for a in lefts]
            rights = [np.ascontiguousarray(a) for a in rights]
            sl = w
        if outs is None:
            outs = [np.empty((h, w), np.int16) for _ in range(n)]
        so = {a.strides[0] // 2 for a in outs}
        if (len(so) != 1 or any(a.dtype != np.int16 or a.shape != (h, w) or a.strides[1] != 2 for a in outs)):
            raise ValueError("outs must be int16 (h, w) row-strided arrays with one common row stride")
        so = so.pop()
        arr = ctypes.c_void_p * max(n, 1)
        L = arr(*[a.ctypes.data for a in lefts])
        R = arr(*[a.ctypes.data for a in rights])
        O = arr(*[a.ctypes.data for a in outs])
        if devices:
            devs = (ctypes.c_int * len(devices))(*devices)
            nd = len(devices)
        else:
            devs, nd = None, 0
        self._check(self.lib.sgm_match_batch(self.h, L, R, n, w, h, sl, O, so, devs, nd))
        return outs

    def match_tiled(self, left, right, n_bands, halo, devices=None):
        """One frame split into row bands over the devices (overlap mode)."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        h, w = left.shape
        out = np.empty((h, w), np.int16)
        if devices:
            devs = (ctypes.c_int * len(devices))(*devices)
            nd = len(devices)
        else:
            devs, nd = None, 0
        self._check(self.lib.sgm_match_tiled(self.h, _ptr(left), _ptr(right), w, h, w, _ptr(out), w, n_bands, halo,
                                             devs, nd))
        return out

    def host_register(self, arr):
        """Page-lock a host array (sgm_host_register): matches into it copy out asynchronously."""
        self._check(self.lib.sgm_host_register(self.h, arr.ctypes.data, arr.nbytes))

    def host_unregister(self, arr):
        self._check(self.lib.sgm_host_unregister(self.h, arr.ctypes.data))

    def match_tiled_device(self, d_left, d_right, width, height, stride, d_out, out_stride, n_bands, halo,
                           devices=None, stream=None):
        """Overlap tile mode on device buffers of this engine's device (C5 frame resident in
        HBM): band b runs on devices[b % len(devices)], rows moved by peer copies."""
        if devices:
            devs = (ctypes.c_int * len(devices))(*devices)
            nd = len(devices)
        else:
            devs, nd = None, 0
        self._check(self.lib.sgm_match_tiled_device(self.h, d_left, d_right, width, height, stride, d_out, out_stride,
                                                    n_bands, halo, devs, nd, stream))

    def match_tiled_exact(self, left, right, n_bands, devices=None):
        """One frame split into row bands over the devices, exact mode: the
        bands' path sweeps continue across the seams through boundary-row exchanges, so the
        result equals match() for any band count."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        h, w = left.shape
        out = np.empty((h, w), np.int16)
        if devices:
            devs = (ctypes.c_int * len(devices))(*devices)
            nd = len(devices)
        else:
            devs, nd = None, 0
        self._check(self.lib.sgm_match_tiled_exact(self.h, _ptr(left), _ptr(right), w, h, w, _ptr(out), w, n_bands,
                                                   devs, nd))
        return out

    # -- profiling -------------------------------------------------------------------------
    def set_profiling(self, on=True):
        self._check(self.lib.sgm_set_profiling(self.h, 1 if on else 0))

    def profiled_matches(self):
        return int(self.lib.sgm_profiled_matches(self.h))

    def stage_launches(self):
        """{stage: number of launches recorded since profiling was enabled}"""
        return {self.lib.sgm_stage_name(self.h, i).decode(): int(self.lib.sgm_stage_launches(self.h, i))
                for i in range(len(self.stage_times()))}

    def stage_times(self):
        """[(stage, average ms per launch, algorithmic bytes per launch)], first-launch order"""
        buf = (ctypes.c_float * 16)()
        n = self.lib.sgm_get_stage_times(self.h, buf, 16)
        if n < 0:
            raise SGMError(n, self.error())
        return [(self.lib.sgm_stage_name(self.h, i).decode(), float(buf[i]),
                 float(self.lib.sgm_stage_bytes(self.h, i))) for i in range(n)]

    # -- stage entry points (parity tests) -------------------------------------------------
    # -- after the matcher (device pointers, async on `stream`) ------------------------------
    def disparity_to_msg(self, d_disp, disp_stride, width, height, min_disparity, max_disparity, d_out, out_stride,
                         stream=None):
        """DisparityImage float image from the int16 x16 disparity (generate_disparity.cpp:426-452)."""
        self._check(self.lib.sgm_disparity_to_msg(self.h, ctypes.c_void_p(d_disp), disp_stride, width, height,
                                                  float(min_disparity), float(max_disparity), ctypes.c_void_p(d_out),
                                                  out_stride, ctypes.c_void_p(stream) if stream else None))

    def depth_points(self, d_disp, disp_stride, width, height, q5, depth_min, depth_max, d_color=None,
                     color_stride=0, channels=0, d_depth=None, depth_stride=0, d_points=None, max_points=0,
                     d_num_points=None, stream=None):
        """disparity_to_depth.cpp:127-205; q5 = (Q23, Q03, Q13, Q32, Q33)."""
        q = (ctypes.c_double * 5)(*[float(v) for v in q5])
        vp = ctypes.c_void_p
        self._check(self.lib.sgm_depth_points(self.h, vp(d_disp), disp_stride, width, height, vp(d_color),
                                              color_stride, channels, q, float(depth_min), float(depth_max),
                                              vp(d_depth), depth_stride, vp(d_points), max_points,
                                              vp(d_num_points), vp(stream) if stream else None))

    def rectify_map(self, K, D, R, P, width, height, d_map_x, d_map_y, map_stride, stream=None):
        """initUndistortRectifyMap(K, D, R, P, (width, height), CV_32FC1) into device float maps
        (generate_disparity.cpp:379-380). R None = identity; D: 0/4/5/8/12 coefficients."""
        dv = ctypes.c_double
        k = (dv * 9)(*np.asarray(K, np.float64).ravel())
        dd = np.asarray([] if D is None else D, np.float64).ravel()
        darr = (dv * max(len(dd), 1))(*dd)
        r = (dv * 9)(*np.asarray(R, np.float64).ravel()) if R is not None else None
        pp = (dv * 12)(*np.asarray(P, np.float64).ravel())
        vp = ctypes.c_void_p
        self._check(self.lib.sgm_rectify_map(self.h, k, darr, len(dd), r, pp, width, height, vp(d_map_x),
                                             vp(d_map_y), map_stride, vp(stream) if stream else None))

    def remap_cubic(self, d_src, src_stride, src_w, src_h, d_map_x, d_map_y, map_stride, width, height, d_dst,
                    dst_stride, stream=None, channels=1):
        """cv::remap(src, dst, map_x, map_y, INTER_CUBIC, BORDER_CONSTANT) on device buffers
        (generate_disparity.cpp:383). channels = 3: src and dst are interleaved 8UC3 (H x W x 3),
        strides in bytes (sgm_remap_cubic_c3)."""
        if channels not in (1, 3):
            raise ValueError("remap_cubic takes 1 or 3 channels")
        vp = ctypes.c_void_p
        fn = self.lib.sgm_remap_cubic_c3 if channels == 3 else self.lib.sgm_remap_cubic
        self._check(fn(self.h, vp(d_src), src_stride, src_w, src_h, vp(d_map_x), vp(d_map_y), map_stride, width,
                       height, vp(d_dst), dst_stride, vp(stream) if stream else None))

    def bgr2gray(self, d_src, src_stride, width, height, d_dst, dst_stride, gray_set=GRAY_Y14, stream=None):
        """cv::cvtColor(COLOR_BGR2GRAY) on device buffers: 8UC3 (stride in bytes) -> 8UC1
        (generate_disparity.cpp:406-416), coefficient set GRAY_Y14 / GRAY_Y15."""
        vp = ctypes.c_void_p
        self._check(self.lib.sgm_bgr2gray(self.h, vp(d_src), src_stride, width, height, vp(d_dst), dst_stride,
                                          int(gray_set), vp(stream) if stream else None))

    def census(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.empty((h, w), np.uint64)
        self._check(self.lib.sgm_debug_census(self.h, _ptr(img), w, h, w, _ptr(out)))
        return out

    def census_path(self, left, right, direction):
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        h, w = left.shape
        e = effective_geometry(self.get_params(), w, h)
        vol = np.zeros((h, max(e["width1"], 0), e["D"]), np.uint8)
        self._check(self.lib.sgm_debug_census_path(self.h, _ptr(left), _ptr(right), w, h, w, int(direction),
                                                   _ptr(vol)))
        return vol

    def ocv_cost(self, left, right):
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        h, w = left.shape
        e = effective_geometry(self.get_params(), w, h)
        C = np.zeros((h, max(e["width1"], 0), e["D"]), np.int16)
        self._check(self.lib.sgm_debug_ocv_cost(self.h, _ptr(left), _ptr(right), w, h, w, _ptr(C)))
        return C

    def bm_prefilter(self, img):
        """MODE_OCV_BM: the XSOBEL pre-filtered image (u8)."""
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.empty((h, w), np.uint8)
        self._check(self.lib.sgm_debug_bm_prefilter(self.h, _ptr(img), w, h, w, _ptr(out)))
        return out

    def bm_sad(self, left, right):
        """MODE_OCV_BM, small frames: (SAD int32 [H][X1 - X0][D], texture int32 [H][X1 - X0]) of the
        fused kernel. The last SAD index is e = D - 1 - (d - minD): e = 0 is the largest disparity.
        Rows outside [w/2, H - w/2) are 0."""
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        h, w = left.shape
        e = bm_geometry(self.get_params(), w, h)
        sad = np.zeros((h, e["width1"], e["D"]), np.int32)
        tex = np.zeros((h, e["width1"]), np.int32)
        self._check(self.lib.sgm_debug_bm_sad(self.h, _ptr(left), _ptr(right), w, h, w, _ptr(sad), _ptr(tex)))
        return sad, tex

    def median3(self, disp):
        d = np.ascontiguousarray(disp, np.int16).copy()
        h, w = d.shape
        self._check(self.lib.sgm_debug_median3(self.h, _ptr(d), w, h))
        return d

    def filter_speckles(self, disp, new_val, max_size, max_diff):
        d = np.ascontiguousarray(disp, np.int16).copy()
        h, w = d.shape
        self._check(self.lib.sgm_debug_speckle(self.h, _ptr(d), w, h, new_val, max_size, max_diff))
        return d

    POST_CANARY = 0x5A5A

    def post(self, disp, median, new_val, max_size, max_diff, out_pad=0):
        """The post filters as a match launches them (sgm_debug_post): the median alone, the speckle
        filter alone or the fused median3+speckle, into an image of row stride W + out_pad that starts
        out as POST_CANARY everywhere. Returns (image[:, :W], pad_columns)."""
        d = np.ascontiguousarray(disp, np.int16)
        h, w = d.shape
        out = np.full((h, w + int(out_pad)), self.POST_CANARY, np.int16)
        self._check(self.lib.sgm_debug_post(self.h, _ptr(d), w, h, int(out_pad), int(bool(median)), int(new_val),
                                            int(max_size), int(max_diff), _ptr(out)))
        return out[:, :w].copy(), out[:, w:].copy()


def calc_q(K, P_right, P_left):
    """calc_q (disparity_to_depth.cpp:62-84) through the C-ABI: 4x4 float64 Q."""
    lib = load_library()
    dv = ctypes.c_double
    k = (dv * 9)(*np.asarray(K, np.float64).ravel())
    pr = (dv * 12)(*np.asarray(P_right, np.float64).ravel())
    pl = (dv * 12)(*np.asarray(P_left, np.float64).ravel())
    q = (dv * 16)()
    lib.sgm_calc_q(k, pr, pl, q)
    return np.array(q[:], np.float64).reshape(4, 4)


def _side_stream(torch):
    """A stream ordered after everything already queued on torch's current stream (the
    library's NULL-stream argument means the handle's own stream, not torch's)."""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    return st


def cubic_table():
    """The INTER_CUBIC int16 weight table of the library (host code, no device needed)."""
    lib = load_library()
    t = np.empty((1024, 16), np.int16)
    lib.sgm_cubic_table(t.ctypes.data_as(ctypes.c_void_p))
    return t


def rectify(engine, image, K, D, R, P, maps=None):
    """The node's rectify(image, camera_info) (generate_disparity.cpp:370-386) on the GPU:
    initUndistortRectifyMap + remap INTER_CUBIC / BORDER_CONSTANT. `maps` (map_x, map_y
    device tensors from a previous call) skips the map computation — the map depends only
    on the calibration. Returns (rectified u8 image as numpy, maps)."""
    import torch
    img = torch.as_tensor(np.ascontiguousarray(image, np.uint8)).cuda()
    h, w = img.shape[:2]
    ch = 3 if img.dim() == 3 else 1
    if maps is None:
        mx = torch.empty((h, w), dtype=torch.float32, device="cuda")
        my = torch.empty((h, w), dtype=torch.float32, device="cuda")
        maps = (mx, my)
    out = torch.empty(tuple(img.shape), dtype=torch.uint8, device="cuda")
    stream = _side_stream(torch)
    if len(maps) == 2:
        engine.rectify_map(K, D, R, P, w, h, maps[0].data_ptr(), maps[1].data_ptr(), w, stream.cuda_stream)
        maps = (maps[0], maps[1], True)
    engine.remap_cubic(img.data_ptr(), w * ch, w, h, maps[0].data_ptr(), maps[1].data_ptr(), w, w, h, out.data_ptr(),
                       w * ch, stream.cuda_stream, channels=ch)
    stream.synchronize()
    return out.cpu().numpy(), maps


def q_terms(Q):
    """The five Q entries the depth node uses (disparity_to_depth.cpp:134-138)."""
    Q = np.asarray(Q, np.float64)
    return (Q[2, 3], Q[0, 3], Q[1, 3], Q[3, 2], Q[3, 3])


def disp_info_to_depth(engine, disp_image, color, Q, depth_min=0.0, depth_max=100.0, gen_point_cloud=True):
    """dispInfoMsg2depthMsg (disparity_to_depth.cpp:94-218) on the GPU: the DisparityImage
    float image (+ MONO8/BGR8 color) -> (depth float32 HxW, points Nx3 float32, rgba N)."""
    import torch
    d = torch.as_tensor(np.ascontiguousarray(disp_image, np.float32)).cuda()
    h, w = d.shape
    c = None
    ch = 0
    if color is not None:
        c = torch.as_tensor(np.ascontiguousarray(color, np.uint8)).cuda()
        ch = 1 if c.dim() == 2 else 3
    depth = torch.empty((h, w), dtype=torch.float32, device="cuda")
    pts = torch.empty((h * w if gen_point_cloud else 1, 4), dtype=torch.float32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = _side_stream(torch)
    engine.depth_points(d.data_ptr(), w, w, h, q_terms(Q), depth_min, depth_max,
                        c.data_ptr() if c is not None else None, w * ch, ch, depth.data_ptr(), w,
                        pts.data_ptr() if gen_point_cloud else None, h * w if gen_point_cloud else 0,
                        n.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    k = int(n.item())
    p = pts[:k].cpu().numpy() if gen_point_cloud else np.zeros((0, 4), np.float32)
    return depth.cpu().numpy(), p[:, :3].copy(), p[:, 3].copy().view(np.uint32)


def right_matcher_params(p):
    """cv::ximgproc::createRightMatcher for a StereoSGBM: minD' = -(minD + D) + 1, same D /
    block / P1 / P2 / mode / preFilterCap, uniqueness 0, disp12MaxDiff 1e6, no speckle filter
    (reference calls it at matcherOpenCVSGBM.cpp:48)."""
    if p.mode == MODE_OCV_BM:
        return p.copy(min_disparity=-(p.min_disparity + p.num_disparities) + 1, uniqueness_ratio=0,
                      speckle_window_size=0, speckle_range=0)
    return p.copy(min_disparity=-(p.min_disparity + p.num_disparities) + 1, uniqueness_ratio=0,
                  disp12_max_diff=1000000, speckle_window_size=0)


def right_matcher_bm_params(b):
    """cv::ximgproc::createRightMatcher for a StereoBM (with right_matcher_params): minD' = -(minD + D)
    + 1, same D / block / caps, texture threshold 0, uniqueness 0, no speckle filter. Restated, not
    verified against ximgproc."""
    return b.copy(texture_threshold=0)


class MatcherHIPSGM:
    """`MatcherHIPSGM : AbstractStereoMatcher` host mirror.

    Same method names, argument meaning and error behaviour as the reference's
    MatcherOpenCVSGBM (matcherOpenCVSGBM.{h,cpp}); compute delegated to libsgm_hip.so.
    `mode` picks the engine mode (the reference's SGBM path never sets a mode, Q1, so the
    OpenCV-compatible default is MODE_SGBM = 5 directions; env SGM_HIP_MODE overrides).
    `census_paths` (census mode only): 8 or 4 aggregation paths; None reads env
    SGM_HIP_CENSUS_PATHS (default 8).
    Hole filling (setHoleFilling, env SGM_HIP_FILL) runs after every match of the adapter. With env
    SGM_HIP_FILL_WHEN=interp the interp flag drives it instead: setInterpolation(true) returns the
    forward disparity filled (mode background when SGM_HIP_FILL names none), not Q3's right-view
    image, and setInterpolation(false) returns it unfilled.
    """

    def __init__(self, param_file=" ", image_size=(0, 0), device=0, mode=None, census_paths=None):
        self.param_file = param_file
        self.image_size = (0, 0)          # Q5: the base ctor ignores _image_size
        self.downsample_scale = 1.0
        self.min_disparity = 0
        self.disparity_range = 64
        self.window_size = 9
        self.interpolate = False
        self.left = None
        self.right = None
        self.disparity_lr = None
        self.disparity_rl = None
        if mode is None:
            mode = int(os.environ.get("SGM_HIP_MODE", MODE_OCV_SGBM5))
        self.device = device
        self.mode = mode
        self.census_paths = census_paths_from_env(8) if census_paths is None else int(census_paths)
        self.fill = FillParams(*fill_from_env())
        self.fill_when = fill_when_from_env()
        # census mode: the census window; with SGM_HIP_CENSUS_WINDOW=cfg setWindowSize drives it
        self.census_window, self.census_window_cfg = census_window_from_env()
        # SGM_HIP_PYRAMID: the pyramid level; with "scale" setDownsampleScale drives it
        self.pyramid_level, self.pyramid_scale = pyramid_from_env()
        self.init()

    # --- AbstractStereoMatcher ----------------------------------------------------------
    def init(self):
        self.bm_params = default_bm_params()
        if self.mode == MODE_OCV_BM:
            # cv::StereoBM::create(64, 9) starting point (matcherOpenCVBlock.cpp): minDisparity 0,
            # 64 disparities, block 9, preFilterCap 31 / size 9, texture 10, uniqueness 15, no speckles
            self.params = default_params(self.mode, min_disparity=0, num_disparities=64, block_size=9,
                                         prefilter_cap=31, uniqueness_ratio=15, speckle_window_size=0,
                                         speckle_range=0, disp12_max_diff=-1)
            self._engine = None
            return
        # cv::StereoSGBM::create(64, 9, 5) equivalent starting point (matcherOpenCVSGBM.cpp:14)
        p = default_params(self.mode)
        p.ocv_compat = ocv_compat_from_env(p.ocv_compat)
        p.min_disparity, p.num_disparities, p.block_size = 64, 9, 5
        p.p1 = p.p2 = p.uniqueness_ratio = p.disp12_max_diff = p.prefilter_cap = 0
        p.speckle_window_size = p.speckle_range = 0
        self.params = p
        self._engine = None               # opened lazily at the first match (Q5 / §8b)

    def setImages(self, left, right):
        if left.shape != right.shape:
            sys.stderr.write("Images MUST be the same resolution\n")
            return
        # scale 1 (the node always passes 1): cv::resize short-circuits to a copy
        # H x W x 3 frames are kept as they are: the engine converts them on the device (_run)
        self.left = np.array(left, copy=True)
        self.right = np.array(right, copy=True)
        self.image_size = (self.left.shape[1], self.left.shape[0])

    def setDownsampleScale(self, scale=1.0):
        # no CPU resize ever happens: under SGM_HIP_PYRAMID=scale a scale <= 0.5 selects pyramid level 1
        # (the engine halves the pair on the device), otherwise the value is stored and ignored
        self.downsample_scale = scale
        if self.pyramid_scale:
            self.pyramid_level = 1 if scale <= 0.5 else 0

    def setPyramidLevel(self, level):
        """The pyramid level of every match (0, or 1: half-resolution match refined at full
        resolution); stored as given, another value fails at match time."""
        self.pyramid_level = int(level)

    def setDisparityRange(self, disparity_range):
        if disparity_range <= 0:
            disparity_range = ((self.image_size[0] // 8) + 15) & -16
        self.disparity_range = disparity_range
        self.params.num_disparities = int(disparity_range)

    def setWindowSize(self, window_size):
        self.window_size = window_size
        self.params.block_size = int(window_size)
        if self.census_window_cfg:
            self.census_window = census_window_from_size(window_size)

    def setCensusWindow(self, taps_x, taps_y, step=1):
        """The census mode's window, stored as given (an invalid one fails at match time)."""
        self.census_window = (int(taps_x), int(taps_y), int(step))

    def setInterpolation(self, enable):
        self.interpolate = bool(enable)

    def setHoleFilling(self, mode, max_gap=16, min_neighbours=2):
        """The hole filter after every match (FILL_OFF / FILL_BACKGROUND / FILL_MEDIAN); stored as
        given, bad values fail at match time."""
        self.fill = FillParams(int(mode), int(max_gap), int(min_neighbours))

    def effective_fill(self):
        """The filter a match runs with: the configured one, or under SGM_HIP_FILL_WHEN=interp the
        one the interp flag selects."""
        if self.fill_when != "interp":
            return self.fill
        if not self.interpolate:
            return FillParams(FILL_OFF, self.fill.max_gap, self.fill.min_neighbours)
        return self.fill.copy(mode=self.fill.mode if self.fill.mode != FILL_OFF else FILL_BACKGROUND)

    def q3(self):
        """interp on and not taken over by the hole filter: the right matcher's image replaces the result."""
        return self.interpolate and self.fill_when != "interp"

    def setMinDisparity(self, min_disparity):
        self.min_disparity = min_disparity
        self.params.min_disparity = int(min_disparity)

    def setUniquenessRatio(self, ratio):
        self.params.uniqueness_ratio = int(ratio)          # Q7: double in cfg -> int

    def setSpeckleFilterWindow(self, window):
        self.params.speckle_window_size = int(window)

    def setSpeckleFilterRange(self, rng):
        self.params.speckle_range = int(rng)

    def setDisp12MaxDiff(self, diff):
        self.params.disp12_max_diff = int(diff)

    def setPreFilterCap(self, cap):
        self.params.prefilter_cap = int(cap)

    def setP1(self, p1):
        self.params.p1 = int(p1)                           # OpenCV setP1(int): truncation

    def setP2(self, p2):
        self.params.p2 = int(p2)

    def setTextureThreshold(self, threshold):              # BM mode only; not used by SGBM
        if self.mode == MODE_OCV_BM:
            self.bm_params.texture_threshold = int(threshold)

    def setPreFilterSize(self, size):                      # BM mode only; not used by SGBM
        if self.mode == MODE_OCV_BM:
            self.bm_params.prefilter_size = int(size)

    def setOcclusionDetection(self, enable):               # not used by SGBM
        pass

    def _engine_for(self):
        if self._engine is None:
            self._engine = Engine(self.device)
        return self._engine

    def _run(self, params, a, b, f32=False, bm=None):
        eng = self._engine_for()
        eng.set_params(params)
        eng.set_census_paths(self.census_paths)
        eng.set_census_window(*self.census_window)
        eng.set_fill_params(self.effective_fill())
        eng.set_pyramid_params(default_pyramid_params(level=self.pyramid_level))
        # colour frames: COLOR_BGR2GRAY on the device, with the grey set of the OpenCV release the
        # compat bits name (COL0_LEGACY marks 3.x: Y14; otherwise 4.x: Y15)
        eng.set_raw_format(3 if np.ndim(a) == 3 else 1,
                           GRAY_Y14 if (params.ocv_compat & OCV_COL0_LEGACY) else GRAY_Y15)
        if params.mode == MODE_OCV_BM:
            eng.set_bm_params(bm if bm is not None else self.bm_params)
        return eng.match_f32(a, b) if f32 else eng.match(a, b)

    def forwardMatch(self):
        try:
            if self.q3():
                # Q3: the WLS output is discarded and disparity_rl (CV_16S) replaces disparity_lr
                self.backwardMatch()
                self.disparity_lr = self.disparity_rl.astype(np.float32)
            else:
                # CV_32FC1 converted on the device (sgm_match_f32)
                self.disparity_lr = self._run(self.params, self.left, self.right, f32=True)
            return 0
        except Exception as e:  # mirrors the catch(cv::Exception&) -> -1
            # matcherOpenCVSGBM.cpp:40 / matcherOpenCVBlock.cpp:40 style
            what = "HIP StereoBM" if self.mode == MODE_OCV_BM else "HIP SGM"
            sys.stderr.write("Error in %s parameters\n%s\n" % (what, e))
            return -1

    def backwardMatch(self):
        self.disparity_rl = self._run(right_matcher_params(self.params), self.right, self.left,
                                      bm=right_matcher_bm_params(self.bm_params))
        return 0

    def match(self):
        code = self.forwardMatch()
        if code == 0:
            self.disparity_lr = self.disparity_lr.astype(np.float32)
        return code

    def getDisparity(self):
        return None if self.disparity_lr is None else self.disparity_lr.copy()

    def getBackDisparity(self):
        return None if self.disparity_rl is None else self.disparity_rl.copy()

    def getLeftImage(self):
        return self.left

    def getRighttImage(self):  # (sic) reference spelling, abstractStereoMatcher.h:71
        return self.right


# ---------------------------------------------------------------- node-level plumbing
NODE_DEFAULTS = dict(stereo_algorithm=CV_StereoBM, min_disparity=9, disparity_range=64,
                     correlation_window_size=15, uniqueness_ratio=15, texture_threshold=10,
                     speckle_size=100, speckle_range=4, disp12MaxDiff=0, p1=200.0, p2=400.0,
                     interp=False, prefilter_cap=31, prefilter_size=9)  # generate_disparity.cpp:90-112


def update_matcher(matcher, cfg):
    """updateMatcher() — generate_disparity.cpp:241-261 (disp12MaxDiff is NOT forwarded, Q1)."""
    matcher.setDisparityRange(cfg["disparity_range"])
    matcher.setWindowSize(cfg["correlation_window_size"])
    matcher.setMinDisparity(cfg["min_disparity"])
    matcher.setUniquenessRatio(int(cfg["uniqueness_ratio"]))
    matcher.setSpeckleFilterRange(cfg["speckle_range"])
    matcher.setSpeckleFilterWindow(cfg["speckle_size"])
    matcher.setPreFilterCap(cfg["prefilter_cap"])
    matcher.setP1(cfg["p1"])
    matcher.setP2(cfg["p2"])
    matcher.setTextureThreshold(cfg["texture_threshold"])
    matcher.setPreFilterSize(cfg["prefilter_size"])
    matcher.setInterpolation(cfg["interp"])


def parameter_callback(config, state):
    """parameterCallback() sanitising (generate_disparity.cpp:735-845) for the HIP entry.

    `state` holds `first` (bool) and the node globals; returns the (possibly rewritten)
    config like dynamic_reconfigure does."""
    config = dict(config)
    if state.get("first", True):
        for k in NODE_DEFAULTS:
            config[k] = state.get(k, NODE_DEFAULTS[k])
        state["first"] = False
        return config
    config["prefilter_size"] |= 1
    if config["stereo_algorithm"] in (CV_StereoBM, CV_StereoSGBM, CV_StereoBMCuda, CV_StereoBPCuda,
                                      CV_StereoCSBPCuda, HIP_StereoSGM, HIP_StereoBM):
        config["correlation_window_size"] |= 1
        config["disparity_range"] = (config["disparity_range"] // 16) * 16
    if config["stereo_algorithm"] == I3DR_StereoSGM and config["correlation_window_size"] > 17:
        config["correlation_window_size"] = 17
    for k in NODE_DEFAULTS:
        state[k] = config[k]
    return config


def bgr2gray(img, gray_set=GRAY_Y14):
    """cv::cvtColor(COLOR_BGR2GRAY) for 8U on the host: fixed-point coefficients over the bytes in
    memory order, round half up. GRAY_Y14 (the default): OpenCV 3.x's 14-bit set; GRAY_Y15: 4.x's
    15-bit set. `Engine.bgr2gray` is the device form."""
    img = np.asarray(img)
    if img.ndim == 2:
        return img.astype(np.uint8, copy=True)
    k0, k1, k2, bits = GRAY_COEFFS[gray_set]
    b, g, r = (img[..., i].astype(np.int32) for i in range(3))
    return ((b * k0 + g * k1 + r * k2 + (1 << (bits - 1))) >> bits).astype(np.uint8)


def stereo_match(matcher, left_mono, right_mono):
    """stereo_match() — generate_disparity.cpp:334-368: empty result on failure."""
    matcher.setDownsampleScale(1)
    matcher.setImages(left_mono, right_mono)
    code = matcher.match()
    if code == 0:
        return matcher.getDisparity()
    sys.stderr.write(f"Exit code:{code}\nFailed to compute stereo match\nPlease check parameters are valid.\n")
    return np.empty((0, 0), np.float32)


def process_disparity(matcher, left_rect, right_rect, f, T, depth_min=0.0, depth_max=10.0, gray_on_device=False):
    """processDisparity() — generate_disparity.cpp:398-456. Returns the DisparityImage fields
    or None when the match failed (the node returns -1 and publishes nothing).
    gray_on_device: colour images go to the matcher as they are and the engine converts them
    (MatcherHIPSGM.setImages: GRAY_Y14 for a 3.x compat setting, GRAY_Y15 otherwise); the default
    keeps the host bgr2gray(), which is GRAY_Y14 whatever the matcher's compat bits."""
    if gray_on_device:
        disp = stereo_match(matcher, left_rect, right_rect)
    else:
        disp = stereo_match(matcher, bgr2gray(left_rect), bgr2gray(right_rect))
    if disp.size == 0:
        return None
    dmat = (disp.astype(np.float32) * np.float32(1.0 / 16)).astype(np.float32)
    min_disp = np.float32(T * f / depth_max)
    with np.errstate(divide="ignore"):
        max_disp = np.float32(T * f / depth_min) if depth_min != 0 else np.float32(np.inf)  # Q8
    dmat[dmat < min_disp] = MISSING_Z
    dmat[dmat > max_disp] = MISSING_Z
    return dict(image=dmat, f=f, T=T, min_disparity=float(min_disp), max_disparity=float(max_disp),
                delta_d=1.0 / 16, height=dmat.shape[0], width=dmat.shape[1], encoding="32FC1",
                step=dmat.shape[1] * 4)


def _camera_info(info):
    """(K, D, R, P) float64 arrays of a CameraInfo given as a mapping, an object with those
    attributes or a 4-tuple (R None: identity)."""
    if isinstance(info, dict):
        info = tuple(info.get(k) for k in "KDRP")
    elif not isinstance(info, (tuple, list)):
        info = tuple(getattr(info, k) for k in "KDRP")
    K, D, R, P = info
    return (np.asarray(K, np.float64).reshape(3, 3), np.asarray([] if D is None else D, np.float64).ravel(),
            None if R is None else np.asarray(R, np.float64).reshape(3, 3), np.asarray(P, np.float64).reshape(3, 4))


def image_cb(matcher, left_raw, right_raw, info_left, info_right, f, T, depth_min=0.0, depth_max=10.0, state=None):
    """imageCb() — generate_disparity.cpp:635-713 with everything on the device: rectify() of both
    raw images, COLOR_BGR2GRAY of colour ones, the match and processDisparity() in one
    match_device_batch_rect call on the raw frames (mono H x W or colour H x W x 3) plus one
    disparity_to_msg.

    info_left / info_right: the cameras' K, D, R, P (mapping, object or 4-tuple). The node
    rectifies at the input size, so the maps have the raw frames' size; they are computed once per
    calibration and kept in `state` (a dict the caller owns; recomputed when K, D, R, P or the size
    change). The raw format and grey set follow MatcherHIPSGM._run. With the matcher's interpolation
    on, the right matcher's parameters run on (right, left) as in forwardMatch (Q3), so the map
    pairs swap sides too.

    Returns (left_rect, right_rect, msg): the two rectified images the node publishes and the
    DisparityImage fields of process_disparity(); None when the match failed (this mirror produces
    the rectified images in the same call as the match, so then it has nothing to publish).
    Rectification is switched off on the matcher's engine again before returning."""
    import torch
    if state is None:
        state = {}
    left_raw = np.ascontiguousarray(left_raw, np.uint8)
    right_raw = np.ascontiguousarray(right_raw, np.uint8)
    if left_raw.shape != right_raw.shape or left_raw.ndim not in (2, 3) or (left_raw.ndim == 3 and left_raw.shape[2] != 3):
        sys.stderr.write("Images MUST be the same resolution\n")
        return None
    h, w = left_raw.shape[:2]
    ch = 3 if left_raw.ndim == 3 else 1
    eng = matcher._engine_for()
    cams = [_camera_info(info_left), _camera_info(info_right)]
    key = (h, w) + tuple(None if a is None else a.tobytes() for c in cams for a in c)
    try:
        if state.get("key") != key:
            maps = torch.empty((4, h, w), dtype=torch.float32, device="cuda")
            stream = _side_stream(torch)
            for i, (K, D, R, P) in enumerate(cams):
                eng.rectify_map(K, D, R, P, w, h, maps[2 * i].data_ptr(), maps[2 * i + 1].data_ptr(), w,
                                stream.cuda_stream)
            stream.synchronize()
            state["key"], state["maps"] = key, maps
            state["map_builds"] = state.get("map_builds", 0) + 1
        maps = state["maps"]
        params, bm = matcher.params, matcher.bm_params
        dl, dr = torch.as_tensor(left_raw).cuda(), torch.as_tensor(right_raw).cuda()
        ml, mr = (maps[0].data_ptr(), maps[1].data_ptr()), (maps[2].data_ptr(), maps[3].data_ptr())
        rect = torch.empty((2,) + left_raw.shape, dtype=torch.uint8, device="cuda")
        first, second, rl, rr = dl, dr, rect[0], rect[1]
        if matcher.q3():
            params, bm = right_matcher_params(params), right_matcher_bm_params(bm)
            first, second, rl, rr, ml, mr = dr, dl, rect[1], rect[0], mr, ml
        eng.set_params(params)
        eng.set_census_paths(matcher.census_paths)
        eng.set_census_window(*matcher.census_window)
        eng.set_fill_params(matcher.effective_fill())
        eng.set_pyramid_params(default_pyramid_params(level=matcher.pyramid_level))
        eng.set_raw_format(ch, GRAY_Y14 if (params.ocv_compat & OCV_COL0_LEGACY) else GRAY_Y15)
        if params.mode == MODE_OCV_BM:
            eng.set_bm_params(bm)
        disp = torch.empty((h, w), dtype=torch.int16, device="cuda")
        msg = torch.empty((h, w), dtype=torch.float32, device="cuda")
        min_disp = np.float32(T * f / depth_max)
        with np.errstate(divide="ignore"):
            max_disp = np.float32(T * f / depth_min) if depth_min != 0 else np.float32(np.inf)  # Q8
        stream = _side_stream(torch)
        eng.set_rectification(ml, mr, w, w, h)
        try:
            eng.match_device_batch_rect([first.data_ptr()], [second.data_ptr()], w, h, w * ch, [rl.data_ptr()],
                                        [rr.data_ptr()], w * ch, [disp.data_ptr()], w, stream.cuda_stream)
            eng.disparity_to_msg(disp.data_ptr(), w, w, h, min_disp, max_disp, msg.data_ptr(), w, stream.cuda_stream)
            stream.synchronize()
        finally:
            eng.set_rectification()
    except SGMError as e:      # the matcher wrappers' catch -> -1, then "Failed to compute stereo match"
        what = "HIP StereoBM" if matcher.mode == MODE_OCV_BM else "HIP SGM"
        sys.stderr.write("Error in %s parameters\n%s\nFailed to compute stereo match\n" % (what, e))
        return None
    dmat = msg.cpu().numpy()
    out = dict(image=dmat, f=f, T=T, min_disparity=float(min_disp), max_disparity=float(max_disp),
               delta_d=1.0 / 16, height=h, width=w, encoding="32FC1", step=w * 4)
    return rect[0].cpu().numpy(), rect[1].cpu().numpy(), out


def image_cb_host(matcher, left_raw, right_raw, info_left, info_right, f, T, depth_min=0.0, depth_max=10.0, state=None):
    """image_cb through the host-buffer entry point: the same arguments and return value, computed
    by one sgm_node_frame call on the numpy arrays (Engine.node_frame), without torch. The maps are
    cached on the matcher's engine (sgm_node_frame rebuilds them when the size or a calibration
    changes); `state`, when given, receives the engine's build count as state["map_builds"]. The
    engine's own rectification setting is not touched."""
    left_raw = np.ascontiguousarray(left_raw, np.uint8)
    right_raw = np.ascontiguousarray(right_raw, np.uint8)
    if left_raw.shape != right_raw.shape or left_raw.ndim not in (2, 3) or (left_raw.ndim == 3 and left_raw.shape[2] != 3):
        sys.stderr.write("Images MUST be the same resolution\n")
        return None
    h, w = left_raw.shape[:2]
    ch = 3 if left_raw.ndim == 3 else 1
    eng = matcher._engine_for()
    params, bm = matcher.params, matcher.bm_params
    first, second, il, ir = left_raw, right_raw, info_left, info_right
    if matcher.q3():              # Q3: the right matcher on (right, left), infos and rectified outputs swapped
        params, bm = right_matcher_params(params), right_matcher_bm_params(bm)
        first, second, il, ir = right_raw, left_raw, info_right, info_left
    min_disp = np.float32(T * f / depth_max)
    with np.errstate(divide="ignore"):
        max_disp = np.float32(T * f / depth_min) if depth_min != 0 else np.float32(np.inf)  # Q8
    try:
        eng.set_params(params)
        eng.set_census_paths(matcher.census_paths)
        eng.set_census_window(*matcher.census_window)
        eng.set_fill_params(matcher.effective_fill())
        eng.set_pyramid_params(default_pyramid_params(level=matcher.pyramid_level))
        eng.set_raw_format(ch, GRAY_Y14 if (params.ocv_compat & OCV_COL0_LEGACY) else GRAY_Y15)
        if params.mode == MODE_OCV_BM:
            eng.set_bm_params(bm)
        ra, rb, dmat, _ = eng.node_frame(first, second, il, ir, min_disp, max_disp)
    except SGMError as e:      # the matcher wrappers' catch -> -1, then "Failed to compute stereo match"
        what = "HIP StereoBM" if matcher.mode == MODE_OCV_BM else "HIP SGM"
        sys.stderr.write("Error in %s parameters\n%s\nFailed to compute stereo match\n" % (what, e))
        return None
    finally:
        if state is not None:
            state["map_builds"] = eng.node_frame_map_builds()
    if matcher.q3():
        ra, rb = rb, ra
    out = dict(image=dmat, f=f, T=T, min_disparity=float(min_disp), max_disparity=float(max_disp),
               delta_d=1.0 / 16, height=h, width=w, encoding="32FC1", step=w * 4)
    return ra, rb, out
