"""ctypes binding of the HIP C-ABI (``include/lgs.h`` -> ``lgs_amd/_lib/liblgs_hip.so``).

This is the only way the package computes anything: there is no CPU fallback.
If the library is missing, or no HIP device is visible, constructing a
``Context`` raises ``LgsError`` immediately.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LGS_LIB") or os.path.join(_HERE, "_lib", "liblgs_hip.so")
# the same sources built with -DLGS_TEST_HOOKS (the environment's test / A/B switches):
# only tests that perturb the certificate on purpose use it (Context(hooks=True))
HOOKS_LIB_PATH = os.path.join(_HERE, "_lib", "liblgs_hip_hooks.so")

LGS_OK = 0
LGS_ERR_INVALID = -1
LGS_ERR_HIP = -2
LGS_ERR_NOMEM = -3
LGS_ERR_OVERFLOW = -4
LGS_ERR_NONFINITE = -5
LGS_ERR_STATE = -6

LGS_BASIS_LINEAR_PROBS = 0x1
LGS_DEVICE_PTRS = 0x1
LGS_EXACT_ORDER = 0x2
LGS_WANG_LING = 0x4
LGS_Z64 = 0x8
LGS_COORD_MAJOR = 0x10
LGS_SAMPLEZ_TABLE = 0x20
LGS_SAMPLEZ_DECISION = 0x40
LGS_SAMPLEZ_LIBM = 0x80
LGS_LOGW_BOUND = 0x400
LGS_TARGETS_QFRAME = 0x800

LGS_X_I32 = 0x100
LGS_X_I64 = 0x200

# lgs_create_ex ctx_flags (include/lgs.h)
LGS_CTX_NO_PIPELINE = 0x1
LGS_CTX_NO_LOOKAHEAD = 0x2
LGS_CTX_SAMPLEZ_LIBM = 0x4
LGS_CTX_PANEL16 = 0x8
LGS_CTX_FAR_FP64 = 0x10
LGS_CTX_STORE32 = 0x20
LGS_CTX_NO_QSKIP = 0x40
LGS_CTX_NO_CU_SPLIT = 0x80

KERNEL_KLEIN, KERNEL_BZ, KERNEL_ACCEPT, KERNEL_MOMENTS = 0, 1, 2, 3
KERNEL_GRAM, KERNEL_SERIES, KERNEL_KLEIN_INIT = 4, 5, 6
KERNEL_CPRIME = 7  # lgs_klein_targets: the c' = Q^T t stage (transposes + GEMM)
KERNEL_DECODE_SELECT = 8  # lgs_klein_decode: the select and gather launches; lgs_imhk_targets: scan and gather
KERNEL_CVP_ENUM = 9  # lgs_closest_vector: the enumeration launches
LGS_CVP_MAX_D = 64
LGS_CVPB_MAX_T = 64          # lgs_closest_vector_bases: targets per basis
LGS_KLEINB_MAX_T = 64        # lgs_klein_bases: targets per basis
LGS_MASS_MAX_D = 64          # lgs_gaussian_mass
LGS_MASS_MOMENTS_MAX_D = 40  # ... with sum_z
LGS_LLL_MAX_D = 64           # lgs_lll_reduce (its launches are timer KERNEL_CVP_ENUM too)
LGS_BKZ_MAX_BLOCK = 32       # lgs_bkz_reduce (timer KERNEL_CVP_ENUM as well)
LGS_COUNTER_RESOLVED = 0
LGS_COUNTER_FALLBACK = 1
LGS_COUNTER_ACCEPT_RESOLVED = 2
LGS_COUNTER_WL_MISMATCH = 3
LGS_COUNTER_QSKIP = 4
LGS_COUNTER_KLEIN_CUS = 5
LGS_COUNTER_DECODE_RESOLVED = 6
# Klein launches by the kernel run_klein chose (exact order, VALU, MFMA fp64 / int8-digit far field)
LGS_COUNTER_LAUNCH_EXACT = 7
LGS_COUNTER_LAUNCH_VALU = 8
LGS_COUNTER_LAUNCH_MFMA_FP64 = 9
LGS_COUNTER_LAUNCH_MFMA_I8 = 10

# every symbol include/lgs.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = ("lgs_version", "lgs_last_error", "lgs_create", "lgs_create_ex", "lgs_destroy", "lgs_set_stream",
           "lgs_set_basis", "lgs_klein", "lgs_imhk", "lgs_imhk_trace", "lgs_imhk_ex", "lgs_lattice_points", "lgs_log_density", "lgs_sample_z", "lgs_timing_enable",
           "lgs_timing_get", "lgs_device_info", "lgs_series_stats", "lgs_gram",
           "lgs_jump_distance", "lgs_marginal_tvd", "lgs_column_range", "lgs_histogram", "lgs_set_decoder", "lgs_nearest_plane",
           "lgs_round_decode", "lgs_counter", "lgs_qskip_elided", "lgs_bz_tiles", "lgs_klein_targets", "lgs_klein_decode",
           "lgs_imhk_targets", "lgs_closest_vector", "lgs_gaussian_mass", "lgs_ball_points", "lgs_exact_table",
           "lgs_exact_sample", "lgs_lll_reduce", "lgs_bkz_reduce", "lgs_closest_vector_bases", "lgs_klein_bases",
           "lgs_imhk_bases")


class ImhkOutputs(ctypes.Structure):
    """struct lgs_imhk_outputs (include/lgs.h)."""
    _fields_ = [("logw_samples", ctypes.c_void_p), ("accepted", ctypes.c_void_p),
                ("vnorm2_samples", ctypes.c_void_p), ("zk_samples", ctypes.c_void_p),
                ("zk_index", ctypes.c_int64), ("fn_chains", ctypes.c_int64),
                ("lag_L", ctypes.c_int64), ("lag_z_ring", ctypes.c_void_p), ("lag_z_sums", ctypes.c_void_p),
                ("lag_v_ring", ctypes.c_void_p), ("lag_v_sums", ctypes.c_void_p), ("lag_v_scale", ctypes.c_double)]


class DecodeOutputs(ctypes.Structure):
    """struct lgs_decode_outputs (include/lgs.h)."""
    _fields_ = [("best_draw", ctypes.c_void_p), ("dist2", ctypes.c_void_p),
                ("dist2_draws", ctypes.c_void_p), ("bound_draws", ctypes.c_void_p)]


class ImhkTargetsOutputs(ctypes.Structure):
    """struct lgs_imhk_targets_outputs (include/lgs.h)."""
    _fields_ = [("logw", ctypes.c_void_p), ("accepts", ctypes.c_void_p), ("final_step", ctypes.c_void_p),
                ("accepted", ctypes.c_void_p), ("logw_draws", ctypes.c_void_p), ("bound_draws", ctypes.c_void_p)]


class CvpOutputs(ctypes.Structure):
    """struct lgs_cvp_outputs (include/lgs.h)."""
    _fields_ = [("dist2", ctypes.c_void_p), ("nodes", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class CvpBasesOutputs(ctypes.Structure):
    """struct lgs_cvp_bases_outputs (include/lgs.h)."""
    _fields_ = [("dist2", ctypes.c_void_p), ("nodes", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("qr_status", ctypes.c_void_p), ("R", ctypes.c_void_p), ("cprime", ctypes.c_void_p)]


class KleinBasesOutputs(ctypes.Structure):
    """struct lgs_klein_bases_outputs (include/lgs.h)."""
    _fields_ = [("best_draw", ctypes.c_void_p), ("dist2", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("qr_status", ctypes.c_void_p), ("R", ctypes.c_void_p), ("cprime", ctypes.c_void_p),
                ("z_draws", ctypes.c_void_p), ("dist2_draws", ctypes.c_void_p)]


class ImhkBasesOutputs(ctypes.Structure):
    """struct lgs_imhk_bases_outputs (include/lgs.h)."""
    _fields_ = [("logw", ctypes.c_void_p), ("accepts", ctypes.c_void_p), ("final_step", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("qr_status", ctypes.c_void_p), ("R", ctypes.c_void_p),
                ("cprime", ctypes.c_void_p), ("accepted", ctypes.c_void_p), ("logw_draws", ctypes.c_void_p),
                ("z_draws", ctypes.c_void_p), ("z_samples", ctypes.c_void_p)]


class MassOutputs(ctypes.Structure):
    """struct lgs_mass_outputs (include/lgs.h)."""
    _fields_ = [("mass", ctypes.c_void_p), ("energy", ctypes.c_void_p), ("points", ctypes.c_void_p),
                ("dist2_min", ctypes.c_void_p), ("sum_z", ctypes.c_void_p), ("nodes", ctypes.c_void_p),
                ("status", ctypes.c_void_p)]


class BallOutputs(ctypes.Structure):
    """struct lgs_ball_outputs (include/lgs.h)."""
    _fields_ = [("offsets", ctypes.c_void_p), ("nodes", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class ExactTableOutputs(ctypes.Structure):
    """struct lgs_exact_table_outputs (include/lgs.h)."""
    _fields_ = [("offsets", ctypes.c_void_p), ("nodes", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("mass", ctypes.c_void_p), ("weights", ctypes.c_void_p), ("cum", ctypes.c_void_p)]


class ExactSampleOutputs(ctypes.Structure):
    """struct lgs_exact_sample_outputs (include/lgs.h)."""
    _fields_ = [("index", ctypes.c_void_p), ("dist2", ctypes.c_void_p)]


class LllOutputs(ctypes.Structure):
    """struct lgs_lll_outputs (include/lgs.h)."""
    _fields_ = [("swaps", ctypes.c_void_p), ("iters", ctypes.c_void_p), ("passes", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("gs_norm2", ctypes.c_void_p)]


class BkzOutputs(ctypes.Structure):
    """struct lgs_bkz_outputs (include/lgs.h)."""
    _fields_ = [("swaps", ctypes.c_void_p), ("iters", ctypes.c_void_p), ("passes", ctypes.c_void_p),
                ("tours", ctypes.c_void_p), ("blocks", ctypes.c_void_p), ("insertions", ctypes.c_void_p),
                ("nodes", ctypes.c_void_p), ("truncated", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("gs_norm2", ctypes.c_void_p)]


class LgsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lgs error {code}: {msg}")
        self.code = code


_lib = None   # the library at LIB_PATH (the product unless LGS_LIB names a variant)
_libs = {}    # every library loaded, by path
_vp = ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)


def load_library(path: str = LIB_PATH):
    """Load liblgs_hip.so (raises if it has not been built)."""
    global _lib
    if path in _libs:
        return _libs[path]
    # One HIP runtime per process: PyTorch ships its own libamdhip64 (soname
    # libamdhip64.so.7) and binds it by the unversioned name, so it must be
    # loaded first; liblgs_hip.so's NEEDED libamdhip64.so.7 then resolves to the
    # same runtime and device pointers / streams are shared with torch.
    if os.environ.get("LGS_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise LgsError(LGS_ERR_STATE, f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(path)
    L.lgs_version.restype = ctypes.c_int
    L.lgs_last_error.restype = ctypes.c_char_p
    L.lgs_create.argtypes = [ctypes.POINTER(_vp), ctypes.c_int]
    if hasattr(L, "lgs_create_ex"):  # (round 6; older A/B baselines lack it)
        L.lgs_create_ex.argtypes = [ctypes.POINTER(_vp), ctypes.c_int, ctypes.c_int64, ctypes.c_uint32]
    L.lgs_destroy.argtypes = [_vp]
    L.lgs_set_stream.argtypes = [_vp, _vp]
    L.lgs_set_basis.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, ctypes.c_double, ctypes.c_int32,
                                ctypes.c_uint32]
    L.lgs_klein.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, _vp, _vp, _vp,
                            ctypes.c_uint32]
    L.lgs_imhk.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint64,
                           ctypes.c_int64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                           ctypes.c_uint32]
    L.lgs_imhk_trace.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint64,
                                 ctypes.c_int64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _vp, ctypes.c_uint32]
    if hasattr(L, "lgs_imhk_ex"):  # (round 4; older builds, e.g. A/B baselines, lack it)
        L.lgs_imhk_ex.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint64,
                                  ctypes.c_int64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  ctypes.POINTER(ImhkOutputs), ctypes.c_uint32]
    L.lgs_lattice_points.argtypes = [_vp, ctypes.c_int64, _vp, _vp, ctypes.c_uint32]
    L.lgs_log_density.argtypes = [_vp, ctypes.c_int64, _vp, _vp, ctypes.c_uint32]
    L.lgs_sample_z.argtypes = [_vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp,
                               ctypes.c_uint32]
    L.lgs_timing_enable.argtypes = [_vp, ctypes.c_int]
    L.lgs_timing_get.argtypes = [_vp, ctypes.c_int, _dp, _i64p]
    L.lgs_counter.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    L.lgs_qskip_elided.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    L.lgs_bz_tiles.argtypes = [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.lgs_device_info.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                  _i64p]
    _i64 = ctypes.c_int64
    L.lgs_series_stats.argtypes = [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                   ctypes.c_double, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint32]
    L.lgs_gram.argtypes = [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, ctypes.c_uint32]
    L.lgs_jump_distance.argtypes = [_vp, _i64, _i64, _vp, _i64, _vp, ctypes.c_uint32]
    L.lgs_marginal_tvd.argtypes = [_vp, _i64, _vp, _i64, _vp, _i64, _vp, ctypes.c_uint32]
    L.lgs_column_range.argtypes = [_vp, _i64, _vp, _i64, _vp, _vp, ctypes.c_uint32]
    L.lgs_histogram.argtypes = [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, ctypes.c_uint32]
    L.lgs_set_decoder.argtypes = [_vp, _vp, _vp]
    L.lgs_nearest_plane.argtypes = [_vp, _i64, _vp, _vp, _vp, ctypes.c_uint32]
    L.lgs_round_decode.argtypes = [_vp, _i64, _vp, _vp, _vp, ctypes.c_uint32]
    if hasattr(L, "lgs_klein_targets"):  # (older A/B baselines lack it)
        L.lgs_klein_targets.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, _i64, _vp, _vp, _vp, _vp,
                                        ctypes.c_uint32]
    if hasattr(L, "lgs_klein_decode"):  # (older A/B baselines lack it)
        L.lgs_klein_decode.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, _i64, _i64, _vp, _vp, _vp, _vp,
                                       ctypes.POINTER(DecodeOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_imhk_targets"):  # (older A/B baselines lack it)
        L.lgs_imhk_targets.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, _i64, _i64, _vp, _vp, _vp, _vp,
                                       ctypes.POINTER(ImhkTargetsOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_closest_vector"):  # (older A/B baselines lack it)
        L.lgs_closest_vector.argtypes = [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, ctypes.POINTER(CvpOutputs),
                                         ctypes.c_uint32]
    if hasattr(L, "lgs_gaussian_mass"):  # (older A/B baselines lack it)
        L.lgs_gaussian_mass.argtypes = [_vp, _i64, _vp, ctypes.c_double, _vp, _vp, _i64, _vp,
                                        ctypes.POINTER(MassOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_ball_points"):  # (older A/B baselines lack them)
        L.lgs_ball_points.argtypes = [_vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, ctypes.POINTER(BallOutputs),
                                      ctypes.c_uint32]
        L.lgs_exact_table.argtypes = [_vp, _i64, _vp, ctypes.c_double, _vp, _vp, _i64, _i64,
                                      ctypes.POINTER(ExactTableOutputs), ctypes.c_uint32]
        L.lgs_exact_sample.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, _i64, _vp, _vp,
                                       ctypes.POINTER(ExactSampleOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_lll_reduce"):  # (older A/B baselines lack it)
        L.lgs_lll_reduce.argtypes = [_vp, _i64, _i64, _vp, ctypes.c_double, ctypes.c_double, _i64, _vp, _vp,
                                     ctypes.POINTER(LllOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_bkz_reduce"):  # (older A/B baselines lack it)
        L.lgs_bkz_reduce.argtypes = [_vp, _i64, _i64, _vp, _i64, ctypes.c_double, ctypes.c_double, _i64, _i64, _i64,
                                     _vp, _vp, ctypes.POINTER(BkzOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_closest_vector_bases"):  # (older A/B baselines lack it)
        L.lgs_closest_vector_bases.argtypes = [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp,
                                               ctypes.POINTER(CvpBasesOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_klein_bases"):  # (older A/B baselines lack it)
        L.lgs_klein_bases.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, _i64, _i64, _i64, _i64, _vp, _vp, _vp,
                                      ctypes.c_int32, _vp, _vp, ctypes.POINTER(KleinBasesOutputs), ctypes.c_uint32]
    if hasattr(L, "lgs_imhk_bases"):  # (older A/B baselines lack it)
        L.lgs_imhk_bases.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint64, _i64, _i64, _i64, _i64, _i64, ctypes.c_int32,
                                     _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, ctypes.POINTER(ImhkBasesOutputs),
                                     ctypes.c_uint32]
    for name in EXPORTS:
        if name not in ("lgs_version", "lgs_last_error") and hasattr(L, name):
            getattr(L, name).restype = ctypes.c_int
    _libs[path] = L
    if path == LIB_PATH:
        _lib = L
    return L


def _check(rc, L=None):
    if rc != LGS_OK:
        msg = (L or _lib or load_library()).lgs_last_error().decode(errors="replace")
        raise LgsError(rc, msg)


def _ptr(a):
    """Host numpy array or device tensor (anything with data_ptr()) -> void*."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags.c_contiguous:
            raise ValueError("arrays must be C-contiguous")
        return ctypes.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        if hasattr(a, "is_contiguous") and not a.is_contiguous():
            raise ValueError("tensors must be contiguous")
        return ctypes.c_void_p(a.data_ptr())
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    raise TypeError(f"unsupported buffer {type(a)}")


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def _check_bufs(flags, device, bufs):
    """Caller buffers must match the call's flags: element type (LGS_Z64 selects
    int64 coefficients), and host vs device memory (LGS_DEVICE_PTRS, on the
    context's device) -- a mismatch would be silently misread by the library."""
    dev_flag = bool(flags & LGS_DEVICE_PTRS)
    for a, want, name in bufs:
        if a is None or isinstance(a, int):  # raw addresses are opaque: the caller vouches for them
            continue
        got = _dtype_name(a)
        if got != want:
            raise ValueError(f"{name}: expected {want}, got {got}")
        is_dev = bool(getattr(a, "is_cuda", False))
        if is_dev != dev_flag:
            raise ValueError(f"{name}: {'device' if is_dev else 'host'} buffer with LGS_DEVICE_PTRS "
                             f"{'set' if dev_flag else 'unset'}")
        if is_dev and a.device.index is not None and a.device.index != device:
            raise ValueError(f"{name}: on cuda:{a.device.index}, context on cuda:{device}")


def _check_padded(x, shape, ld):
    """x must hold the logical `shape` (rows, cols) at row pitch ld: the library reads
    (rows - 1) * ld + cols elements from its pointer."""
    rows, cols = shape
    have = 1
    for s in x.shape:
        have *= int(s)
    if ld < cols or (rows > 0 and have < (rows - 1) * ld + cols):
        raise ValueError(f"buffer of {have} elements does not hold shape {shape} at leading dimension {ld}")


def _outputs(struct, *arrays):
    """ctypes.byref of `struct` filled with the arrays' addresses in field order, or None when
    every one is None (the library takes a null outputs pointer)."""
    if all(a is None for a in arrays):
        return None
    return ctypes.byref(struct(*(None if a is None else _ptr(a).value for a in arrays)))


def _host_retry(flags, call):
    """The *_host methods' width loop: call(flags, z_dtype) with int32 coefficients (int64 at
    once with LGS_Z64 in flags), and once more with LGS_Z64 after LGS_ERR_OVERFLOW."""
    for z64 in (bool(flags & LGS_Z64), True):
        try:
            return call(flags | (LGS_Z64 if z64 else 0), np.int64 if z64 else np.int32)
        except LgsError as e:
            if e.code != LGS_ERR_OVERFLOW or z64:
                raise
    raise AssertionError("unreachable")


def _z64(z):
    return None if z is None else z.astype(np.int64, copy=False)


def x_flags(a) -> int:
    """LGS_X_* element-type flag of a host array / device tensor (fp64, int32, int64)."""
    t = _dtype_name(a)
    if t == "float64":
        return 0
    if t == "int32":
        return LGS_X_I32
    if t == "int64":
        return LGS_X_I64
    raise TypeError(f"diagnostics take float64 / int32 / int64 data, got {t}")


class Context:
    """One HIP device context (stream + device-resident basis + scratch)."""

    def __init__(self, device: int = 0, *, max_proposals: int = 0, pipeline: bool = True,
                 lookahead: bool = True, samplez_libm: bool = False, panel: int = 32, far: str = "int8",
                 store32: bool = False, qskip: bool = True, cu_split: bool = True,
                 hooks: bool = False):
        """lgs_create_ex: max_proposals (0 = the library's default) and the LGS_CTX_*
        options; hooks=True loads liblgs_hip_hooks.so (the environment's test switches)."""
        L = load_library(HOOKS_LIB_PATH if hooks else LIB_PATH)
        self._L = L
        flags = ((0 if pipeline else LGS_CTX_NO_PIPELINE) | (0 if lookahead else LGS_CTX_NO_LOOKAHEAD) |
                 (LGS_CTX_SAMPLEZ_LIBM if samplez_libm else 0) | (LGS_CTX_PANEL16 if panel == 16 else 0) |
                 (LGS_CTX_FAR_FP64 if far == "fp64" else 0) | (LGS_CTX_STORE32 if store32 else 0) |
                 (0 if qskip else LGS_CTX_NO_QSKIP) | (0 if cu_split else LGS_CTX_NO_CU_SPLIT))
        if panel not in (16, 32) or far not in ("int8", "fp64"):
            raise ValueError("panel is 16 or 32, far is 'int8' or 'fp64'")
        h = _vp()
        if hasattr(L, "lgs_create_ex"):
            _check(L.lgs_create_ex(ctypes.byref(h), int(device), int(max_proposals), flags), L)
        elif flags or max_proposals:
            raise LgsError(LGS_ERR_INVALID, "this library build has no lgs_create_ex")
        else:
            _check(L.lgs_create(ctypes.byref(h), int(device)), L)
        self._h = h
        self.device = device
        self.d = 0

    def _ck(self, rc):
        _check(rc, self._L)

    def close(self):
        if getattr(self, "_h", None) and getattr(self, "_L", None) is not None:
            self._L.lgs_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # ---------------------------------------------------------------- setup
    def set_stream(self, stream_handle):
        self._ck(self._L.lgs_set_stream(self._h, _vp(stream_handle) if stream_handle else None))

    def set_basis(self, R, cprime, B, sigma, precision=10, linear_probs=False):
        R = np.ascontiguousarray(R, dtype=np.float64)
        cp = np.ascontiguousarray(cprime, dtype=np.float64)
        Bc = None if B is None else np.ascontiguousarray(B, dtype=np.float64)
        d = R.shape[0]
        if R.shape != (d, d) or cp.shape != (d,) or (Bc is not None and Bc.shape != (d, d)):
            raise ValueError("shape mismatch between R, cprime and B")
        flags = LGS_BASIS_LINEAR_PROBS if linear_probs else 0
        self._ck(self._L.lgs_set_basis(self._h, d, R.ctypes.data_as(_dp), cp.ctypes.data_as(_dp),
                                  None if Bc is None else Bc.ctypes.data_as(_dp), float(sigma),
                                  int(precision), flags))
        self.d = d
        self._keep = (R, cp, Bc)

    # ---------------------------------------------------------------- compute
    def klein(self, seed, first, n, z_out=None, v_out=None, logw_out=None, flags=0):
        """Raw lgs_klein on caller-provided buffers (numpy host or device tensors)."""
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((z_out, zt, "z_out"), (v_out, "float64", "v_out"),
                                         (logw_out, "float64", "logw_out")))
        self._ck(self._L.lgs_klein(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(n),
                              _ptr(z_out), _ptr(v_out), _ptr(logw_out), int(flags)))

    def klein_host(self, seed, first, n, *, want_z=True, want_v=True, want_logw=False, flags=0):
        """Klein samples into fresh host arrays; int32 first, int64 on overflow."""
        d = self.d
        for z64 in (False, True):
            f = flags | (LGS_Z64 if z64 else 0)
            z = np.empty((n, d), dtype=np.int64 if z64 else np.int32) if want_z else None
            v = np.empty((n, d)) if want_v else None
            lw = np.empty(n) if want_logw else None
            try:
                self.klein(seed, first, n, z, v, lw, f)
            except LgsError as e:
                if e.code == LGS_ERR_OVERFLOW and not z64:
                    continue
                raise
            return {"z": None if z is None else z.astype(np.int64, copy=False), "v": v, "logw": lw}
        raise AssertionError("unreachable")

    def imhk(self, seed, first_chain, n_chains, first_step, n_steps, thin, z_state, logw_state,
             state_init, accepts, z_samples=None, v_samples=None, moments=None, flags=0,
             logw_samples=None, accepted=None, vnorm2_samples=None, zk_samples=None, zk_index=0,
             fn_chains=0, lag=None):
        """lgs_imhk; with logw_samples (n_chains x n_steps/thin float64) or accepted
        (n_chains x n_steps uint8) lgs_imhk_trace, which also records each kept
        state's log weight and each step's accept decision; with vnorm2_samples /
        zk_samples (n_chains x n_steps/thin float64 / int64, device) lgs_imhk_ex, which
        also gives ||v||^2 and coefficient zk_index of each kept state (fn_chains > 0:
        of the leading fn_chains chains only, arrays fn_chains x n_steps/thin); lag =
        (L, z_ring, z_sums, v_ring, v_sums, v_scale): device buffers whose lag-0..L sums
        of both series the call continues (include/lgs.h lgs_imhk_outputs.lag_L)."""
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((z_state, zt, "z_state"), (logw_state, "float64", "logw_state"),
                                         (state_init, "int32", "state_init"), (accepts, "int64", "accepts"),
                                         (z_samples, zt, "z_samples"), (v_samples, "float64", "v_samples"),
                                         (moments, "int64", "moments"), (logw_samples, "float64", "logw_samples"),
                                         (accepted, "uint8", "accepted")))
        args = (self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_chain), int(n_chains), int(first_step),
                int(n_steps), int(thin), _ptr(z_state), _ptr(logw_state), _ptr(state_init), _ptr(accepts),
                _ptr(z_samples), _ptr(v_samples), _ptr(moments))
        if vnorm2_samples is not None or zk_samples is not None:
            _check_bufs(flags, self.device, ((vnorm2_samples, "float64", "vnorm2_samples"),
                                             (zk_samples, "int64", "zk_samples")))
            def v(a):
                q = _ptr(a)
                return None if q is None else q.value
            lg = (0, None, None, None, None, 0.0) if lag is None else lag
            if lag is not None:
                _check_bufs(flags, self.device, ((lg[1], "int64", "lag z ring"), (lg[2], "int64", "lag z sums"),
                                                 (lg[3], "float64", "lag v ring"), (lg[4], "float64", "lag v sums")))
            out = ImhkOutputs(v(logw_samples), v(accepted), v(vnorm2_samples), v(zk_samples), int(zk_index),
                              int(fn_chains), int(lg[0]), v(lg[1]), v(lg[2]), v(lg[3]), v(lg[4]), float(lg[5]))
            self._ck(self._L.lgs_imhk_ex(*args, ctypes.byref(out), int(flags)))
        elif logw_samples is None and accepted is None:
            self._ck(self._L.lgs_imhk(*args, int(flags)))
        else:
            self._ck(self._L.lgs_imhk_trace(*args, _ptr(logw_samples), _ptr(accepted), int(flags)))

    def lattice_points(self, z, v_out=None, flags=0):
        if isinstance(z, np.ndarray):
            z64 = z.dtype == np.int64
            zz = np.ascontiguousarray(z, dtype=np.int64 if z64 else np.int32)
            n = zz.shape[0]
            v = np.empty((n, self.d)) if v_out is None else v_out
            self._ck(self._L.lgs_lattice_points(self._h, n, _ptr(zz), _ptr(v),
                                           int(flags | (LGS_Z64 if z64 else 0))))
            return v
        n = z.shape[0] if not (flags & LGS_COORD_MAJOR) else z.shape[1]
        self._ck(self._L.lgs_lattice_points(self._h, n, _ptr(z), _ptr(v_out), int(flags)))
        return v_out

    def log_density(self, z):
        zz = np.ascontiguousarray(z)
        z64 = zz.dtype == np.int64
        if not z64:
            zz = zz.astype(np.int32)
        out = np.empty(zz.shape[0])
        self._ck(self._L.lgs_log_density(self._h, zz.shape[0], _ptr(zz), _ptr(out),
                                    LGS_Z64 if z64 else 0))
        return out

    def sample_z(self, mu, sigma, u, precision=10, table=False, linear_probs=False, mode=None):
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        sg = np.ascontiguousarray(np.broadcast_to(sigma, mu.shape), dtype=np.float64)
        uu = np.ascontiguousarray(u, dtype=np.float64)
        z = np.empty(mu.shape, dtype=np.int64)
        ln = np.empty(mu.shape)
        f = (LGS_SAMPLEZ_TABLE if table else 0) | (LGS_BASIS_LINEAR_PROBS if linear_probs else 0)
        f |= {None: 0, "decision": LGS_SAMPLEZ_DECISION, "libm": LGS_SAMPLEZ_LIBM,
              "libm_decision": LGS_SAMPLEZ_LIBM | LGS_SAMPLEZ_DECISION}[mode]
        self._ck(self._L.lgs_sample_z(self._h, mu.size, _ptr(mu), _ptr(sg), _ptr(uu), int(precision),
                                 _ptr(z), _ptr(ln), f))
        return z, ln

    # ---------------------------------------------------------------- decoding
    def set_decoder(self, Q=None, Binv=None):
        Qc = None if Q is None else np.ascontiguousarray(Q, dtype=np.float64)
        Bi = None if Binv is None else np.ascontiguousarray(Binv, dtype=np.float64)
        for M in (Qc, Bi):
            if M is not None and M.shape != (self.d, self.d):
                raise ValueError("decoder matrices must be d x d")
        self._ck(self._L.lgs_set_decoder(self._h, _ptr(Qc), _ptr(Bi)))
        self._keep_dec = (Qc, Bi)

    def _n_targets(self, targets, flags):
        """n of targets (n, d), or (d, n) with LGS_COORD_MAJOR; no library call."""
        cm = bool(flags & LGS_COORD_MAJOR)
        if len(targets.shape) != 2 or targets.shape[0 if cm else 1] != self.d:
            raise ValueError(f"targets must be (n, {self.d}), or ({self.d}, n) with LGS_COORD_MAJOR")
        return int(targets.shape[1] if cm else targets.shape[0])

    def _check_target_bufs(self, flags, targets, z_out, v_out, cprime_out, *more):
        """_check_bufs of the buffers every per-target call has, and of `more`."""
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((targets, "float64", "targets"), (z_out, zt, "z_out"),
                                         (v_out, "float64", "v_out"), (cprime_out, "float64", "cprime_out")) + more)

    def _host_targets(self, targets, flags, name):
        """Row-major host targets (n, d) of a *_host method."""
        if flags & (LGS_DEVICE_PTRS | LGS_COORD_MAJOR):
            raise ValueError(f"{name} takes row-major host targets")
        t = np.ascontiguousarray(targets, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != self.d:
            raise ValueError(f"targets must be (n, {self.d})")
        return t

    def _host_zvc(self, n, zdt, want_z, want_v, want_cprime):
        """Fresh z / v / c' arrays of a *_host method (None where not wanted)."""
        return (np.empty((n, self.d), dtype=zdt) if want_z else None, np.empty((n, self.d)) if want_v else None,
                np.empty((n, self.d)) if want_cprime else None)

    def decode(self, targets, method="plane", z_out=None, v_out=None, flags=0):
        """Raw lgs_nearest_plane / lgs_round_decode on caller buffers (numpy host or device
        tensors).  targets is float64 (n, d), or (d, n) with LGS_COORD_MAJOR; z_out has the
        same layout, int32 or int64 per LGS_Z64; v_out is float64 (n, d)."""
        if method not in ("plane", "round"):
            raise ValueError("method is 'plane' or 'round'")
        n = self._n_targets(targets, flags)
        cm = bool(flags & LGS_COORD_MAJOR)
        self._check_target_bufs(flags, targets, z_out, v_out, None)
        for a, want, name in ((z_out, (self.d, n) if cm else (n, self.d), "z_out"), (v_out, (n, self.d), "v_out")):
            if a is not None and not isinstance(a, int) and tuple(a.shape) != want:
                raise ValueError(f"{name}: expected shape {want}, got {tuple(a.shape)}")
        fn = self._L.lgs_nearest_plane if method == "plane" else self._L.lgs_round_decode
        self._ck(fn(self._h, n, _ptr(targets), _ptr(z_out), _ptr(v_out), int(flags)))

    def decode_host(self, targets, method="plane", want_v=True):
        """Decode host targets (n x d); int32 coefficients first, int64 on overflow."""
        t = np.ascontiguousarray(targets, dtype=np.float64)

        def call(f, zdt):
            z, v, _ = self._host_zvc(t.shape[0], zdt, True, want_v, False)
            self.decode(t, method, z, v, f)
            return _z64(z), v
        return _host_retry(0, call)

    # ---------------------------------------------------------------- per-sample centres
    def klein_targets(self, seed, first, targets, z_out=None, v_out=None, cprime_out=None, flags=0):
        """Raw lgs_klein_targets on caller buffers (numpy host or device tensors): one Klein
        draw around each target, sample k on the counters of Klein sample first + k.
        targets is (n, d), or (d, n) with LGS_COORD_MAJOR; with LGS_TARGETS_QFRAME it holds
        c' = Q^T t already."""
        n = self._n_targets(targets, flags)
        self._check_target_bufs(flags, targets, z_out, v_out, cprime_out)
        self._ck(self._L.lgs_klein_targets(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), n,
                                           _ptr(targets), _ptr(z_out), _ptr(v_out), _ptr(cprime_out),
                                           int(flags)))

    def klein_targets_host(self, seed, first, targets, *, want_z=True, want_v=True, want_cprime=False,
                           flags=0):
        """Klein draws around host targets (n, d) into fresh host arrays {"z", "v", "cprime"};
        int32 coefficients first, int64 on overflow (same draws: fixed counters)."""
        t = self._host_targets(targets, flags, "klein_targets_host")

        def call(f, zdt):
            z, v, cp = self._host_zvc(t.shape[0], zdt, want_z, want_v, want_cprime)
            self.klein_targets(seed, first, t, z, v, cp, f)
            return {"z": _z64(z), "v": v, "cprime": cp}
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- decoding by sampling
    def klein_decode(self, seed, first, targets, n_draws, z_out=None, v_out=None, cprime_out=None,
                     best_draw=None, dist2=None, dist2_draws=None, bound_draws=None, flags=0):
        """Raw lgs_klein_decode on caller buffers (numpy host or device tensors): the closest
        of n_draws Klein draws around each target; draw k of target t is on the counters of
        Klein sample first + t * n_draws + k.  targets as in klein_targets; best_draw (n,)
        int64, dist2 (n,), dist2_draws / bound_draws (n, n_draws) float64, all optional."""
        n = self._n_targets(targets, flags)
        self._check_target_bufs(flags, targets, z_out, v_out, cprime_out,
                                (best_draw, "int64", "best_draw"), (dist2, "float64", "dist2"),
                                (dist2_draws, "float64", "dist2_draws"), (bound_draws, "float64", "bound_draws"))
        self._ck(self._L.lgs_klein_decode(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), n, int(n_draws),
                                          _ptr(targets), _ptr(z_out), _ptr(v_out), _ptr(cprime_out),
                                          _outputs(DecodeOutputs, best_draw, dist2, dist2_draws, bound_draws),
                                          int(flags)))

    def klein_decode_host(self, seed, first, targets, n_draws, *, want_z=True, want_v=True, want_cprime=False,
                          want_draws=False, flags=0):
        """Decoding by sampling on host targets (n, d) into fresh host arrays {"z", "v",
        "cprime", "best_draw", "dist2"} (and "dist2_draws", "bound_draws" with want_draws);
        int32 coefficients first, int64 on overflow (same draws: fixed counters)."""
        t = self._host_targets(targets, flags, "klein_decode_host")
        K = int(n_draws)
        if K < 1:
            raise ValueError("n_draws must be >= 1")
        n = t.shape[0]

        def call(f, zdt):
            z, v, cp = self._host_zvc(n, zdt, want_z, want_v, want_cprime)
            best, d2 = np.empty(n, dtype=np.int64), np.empty(n)
            dd = np.empty((n, K)) if want_draws else None
            bd = np.empty((n, K)) if want_draws else None
            self.klein_decode(seed, first, t, K, z, v, cp, best, d2, dd, bd, f)
            r = {"z": _z64(z), "v": v, "cprime": cp, "best_draw": best, "dist2": d2}
            if want_draws:
                r["dist2_draws"], r["bound_draws"] = dd, bd
            return r
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- IMHK around per-target centres
    def imhk_targets(self, seed, first_chain, targets, n_steps, z_out=None, v_out=None, cprime_out=None,
                     logw=None, accepts=None, final_step=None, accepted=None, logw_draws=None,
                     bound_draws=None, flags=0):
        """Raw lgs_imhk_targets on caller buffers (numpy host or device tensors): one IMHK chain
        of n_steps steps with Wang-Ling weights around each target; target k is chain
        first_chain + k, its draw t on the counters (chain, step t).  targets as in
        klein_targets; logw (n,) float64, accepts / final_step (n,) int64, accepted
        (n, n_steps) uint8, logw_draws / bound_draws (n, n_steps + 1) float64, all optional."""
        n = self._n_targets(targets, flags)
        self._check_target_bufs(flags, targets, z_out, v_out, cprime_out,
                                (logw, "float64", "logw"), (accepts, "int64", "accepts"),
                                (final_step, "int64", "final_step"), (accepted, "uint8", "accepted"),
                                (logw_draws, "float64", "logw_draws"), (bound_draws, "float64", "bound_draws"))
        self._ck(self._L.lgs_imhk_targets(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_chain), n, int(n_steps),
                                          _ptr(targets), _ptr(z_out), _ptr(v_out), _ptr(cprime_out),
                                          _outputs(ImhkTargetsOutputs, logw, accepts, final_step, accepted,
                                                   logw_draws, bound_draws),
                                          int(flags)))

    def imhk_targets_host(self, seed, first_chain, targets, n_steps, *, want_z=True, want_v=True,
                          want_cprime=False, want_trace=False, flags=0):
        """IMHK chains around host targets (n, d) into fresh host arrays {"z", "v", "cprime",
        "logw", "accepts", "final_step"} (and "accepted", "logw_draws", "bound_draws" with
        want_trace); int32 coefficients first, int64 on overflow (same draws: fixed counters)."""
        t = self._host_targets(targets, flags, "imhk_targets_host")
        T = int(n_steps)
        if T < 0:
            raise ValueError("n_steps must be >= 0")
        n = t.shape[0]

        def call(f, zdt):
            z, v, cp = self._host_zvc(n, zdt, want_z, want_v, want_cprime)
            lw, acc, fs = np.empty(n), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
            tr = np.empty((n, T), dtype=np.uint8) if want_trace else None
            ld = np.empty((n, T + 1)) if want_trace else None
            bd = np.empty((n, T + 1)) if want_trace else None
            self.imhk_targets(seed, first_chain, t, T, z, v, cp, lw, acc, fs, tr, ld, bd, f)
            r = {"z": _z64(z), "v": v, "cprime": cp, "logw": lw, "accepts": acc, "final_step": fs}
            if want_trace:
                r["accepted"], r["logw_draws"], r["bound_draws"] = tr, ld, bd
            return r
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- exact closest vector
    _CVP_FLAGS = LGS_DEVICE_PTRS | LGS_Z64 | LGS_COORD_MAJOR | LGS_TARGETS_QFRAME

    def _cvp_args(self, targets, max_nodes, flags):
        """Argument checks of closest_vector / closest_vector_host, before any library call."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~self._CVP_FLAGS:
            raise ValueError(f"closest_vector: unsupported flags {flags!r}")
        if self.d > LGS_CVP_MAX_D:
            raise ValueError(f"closest_vector supports d <= {LGS_CVP_MAX_D}, the loaded basis has d = {self.d}")
        if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or \
                not 1 <= max_nodes <= 1 << 40:
            raise ValueError(f"max_nodes must be an integer in 1..2^40, got {max_nodes!r}")
        return self._n_targets(targets, flags)

    def closest_vector(self, targets, max_nodes, radius2=None, z_out=None, v_out=None, cprime_out=None,
                       dist2=None, nodes=None, status=None, flags=0):
        """Raw lgs_closest_vector on caller buffers (numpy host or device tensors): the
        closest lattice point of each target by Schnorr-Euchner enumeration, at most
        max_nodes tree nodes per target.  targets as in klein_targets; radius2 (n,) float64
        (only points with squared distance below it), dist2 (n,) float64, nodes (n,) int64,
        status (n,) int32, all optional."""
        n = self._cvp_args(targets, max_nodes, flags)
        cm = bool(flags & LGS_COORD_MAJOR)
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((targets, "float64", "targets"), (radius2, "float64", "radius2"),
                                         (z_out, zt, "z_out"), (v_out, "float64", "v_out"),
                                         (cprime_out, "float64", "cprime_out"), (dist2, "float64", "dist2"),
                                         (nodes, "int64", "nodes"), (status, "int32", "status")))
        for a, want, name in ((z_out, (self.d, n) if cm else (n, self.d), "z_out"), (v_out, (n, self.d), "v_out"),
                              (cprime_out, (n, self.d), "cprime_out"), (radius2, (n,), "radius2"),
                              (dist2, (n,), "dist2"), (nodes, (n,), "nodes"), (status, (n,), "status")):
            if a is not None and not isinstance(a, int) and tuple(a.shape) != want:
                raise ValueError(f"{name}: expected shape {want}, got {tuple(a.shape)}")
        self._ck(self._L.lgs_closest_vector(self._h, n, _ptr(targets), _ptr(radius2), int(max_nodes), _ptr(z_out),
                                            _ptr(v_out), _ptr(cprime_out),
                                            _outputs(CvpOutputs, dist2, nodes, status), int(flags)))

    def closest_vector_host(self, targets, max_nodes, radius2=None, *, want_z=True, want_v=True,
                            want_cprime=False, flags=0):
        """Exact closest vectors of host targets (n, d) into fresh host arrays {"z", "v",
        "cprime", "dist2", "nodes", "status"}; int32 coefficients first, int64 on overflow
        (the same search: it does not depend on the output width)."""
        if isinstance(flags, (int, np.integer)) and flags & (LGS_DEVICE_PTRS | LGS_COORD_MAJOR):
            raise ValueError("closest_vector_host takes row-major host targets")
        t = np.ascontiguousarray(targets, dtype=np.float64)
        n = self._cvp_args(t, max_nodes, flags)
        r2 = None
        if radius2 is not None:
            r2 = np.ascontiguousarray(radius2, dtype=np.float64)
            if r2.shape != (n,) or not np.all(r2 >= 0):
                raise ValueError(f"radius2 must hold {n} non-negative values")

        def call(f, zdt):
            z, v, cp = self._host_zvc(n, zdt, want_z, want_v, want_cprime)
            d2, nd, st = np.empty(n), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32)
            self.closest_vector(t, max_nodes, r2, z, v, cp, d2, nd, st, f)
            return {"z": _z64(z), "v": v, "cprime": cp, "dist2": d2, "nodes": nd, "status": st}
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- exact closest vector, a batch of bases
    @staticmethod
    def _cvpb_args(bases, targets, max_nodes, flags):
        """Argument checks of closest_vector_bases / closest_vector_bases_host, before any library
        call; returns (n, d, T)."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~(LGS_DEVICE_PTRS | LGS_Z64):
            raise ValueError(f"closest_vector_bases: unsupported flags {flags!r}")
        shape, tshape = tuple(bases.shape), tuple(targets.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError(f"bases must have shape (n, d, d), got {shape}")
        n, d = int(shape[0]), int(shape[1])
        if not 2 <= d <= LGS_CVP_MAX_D:
            raise ValueError(f"closest_vector_bases supports 2 <= d <= {LGS_CVP_MAX_D}, got d = {d}")
        if len(tshape) != 3 or tshape[0] != n or tshape[2] != d:
            raise ValueError(f"targets must have shape ({n}, T, {d}), got {tshape}")
        T = int(tshape[1])
        if not 1 <= T <= LGS_CVPB_MAX_T:
            raise ValueError(f"closest_vector_bases supports 1 <= T <= {LGS_CVPB_MAX_T} targets per basis, got {T}")
        if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or \
                not 1 <= max_nodes <= 1 << 40:
            raise ValueError(f"max_nodes must be an integer in 1..2^40, got {max_nodes!r}")
        return n, d, T

    def closest_vector_bases(self, bases, targets, max_nodes, radius2=None, z_out=None, v_out=None, dist2=None,
                             nodes=None, status=None, qr_status=None, R=None, cprime=None, flags=0):
        """Raw lgs_closest_vector_bases on caller buffers (numpy host arrays, or device tensors
        with LGS_DEVICE_PTRS): bases (n, d, d) float64 whose COLUMNS generate lattice p, targets
        (n, T, d) float64, problem (p, k) = target k of basis p.  radius2, dist2 (n, T) float64,
        z_out (n, T, d) int32 (int64 with LGS_Z64), v_out, cprime (n, T, d) float64, nodes (n, T)
        int64, status (n, T) int32, qr_status (n,) int32, R (n, d, d) float64; all outputs
        optional.  Needs no loaded basis."""
        n, d, T = self._cvpb_args(bases, targets, max_nodes, flags)
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((bases, "float64", "bases"), (targets, "float64", "targets"),
                                         (radius2, "float64", "radius2"), (z_out, zt, "z_out"),
                                         (v_out, "float64", "v_out"), (dist2, "float64", "dist2"),
                                         (nodes, "int64", "nodes"), (status, "int32", "status"),
                                         (qr_status, "int32", "qr_status"), (R, "float64", "R"),
                                         (cprime, "float64", "cprime")))
        self._check_shapes(((radius2, (n, T), "radius2"), (z_out, (n, T, d), "z_out"), (v_out, (n, T, d), "v_out"),
                            (dist2, (n, T), "dist2"), (nodes, (n, T), "nodes"), (status, (n, T), "status"),
                            (qr_status, (n,), "qr_status"), (R, (n, d, d), "R"), (cprime, (n, T, d), "cprime")))
        self._ck(self._L.lgs_closest_vector_bases(
            self._h, n, d, T, _ptr(bases), _ptr(targets), _ptr(radius2), int(max_nodes), _ptr(z_out), _ptr(v_out),
            _outputs(CvpBasesOutputs, dist2, nodes, status, qr_status, R, cprime), int(flags)))

    def closest_vector_bases_host(self, bases, targets, max_nodes, radius2=None, *, want_z=True, want_v=True,
                                  want_R=True, want_cprime=False, flags=0):
        """Exact closest vectors of host targets (n, T, d) in the lattices of host bases (n, d, d)
        into fresh host arrays {"z", "v", "dist2", "nodes", "status", "qr_status", "R", "cprime"};
        int32 coefficients first, int64 on overflow (the same search)."""
        if isinstance(flags, (int, np.integer)) and not isinstance(flags, bool) and flags & LGS_DEVICE_PTRS:
            raise ValueError("closest_vector_bases_host takes host arrays")
        b = np.ascontiguousarray(bases, dtype=np.float64)
        t = np.ascontiguousarray(targets, dtype=np.float64)
        n, d, T = self._cvpb_args(b, t, max_nodes, flags)
        r2 = None
        if radius2 is not None:
            r2 = np.ascontiguousarray(radius2, dtype=np.float64)
            if r2.shape != (n, T) or not np.all(r2 >= 0):
                raise ValueError(f"radius2 must hold ({n}, {T}) non-negative values")

        def call(f, zdt):
            z = np.empty((n, T, d), dtype=zdt) if want_z else None
            v = np.empty((n, T, d)) if want_v else None
            out = {"dist2": np.empty((n, T)), "nodes": np.empty((n, T), dtype=np.int64),
                   "status": np.empty((n, T), dtype=np.int32), "qr_status": np.empty(n, dtype=np.int32),
                   "R": np.empty((n, d, d)) if want_R else None, "cprime": np.empty((n, T, d)) if want_cprime else None}
            self.closest_vector_bases(b, t, max_nodes, r2, z, v, flags=f, **out)
            return {"z": _z64(z), "v": v, **out}
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- Klein draws, a batch of bases
    @staticmethod
    def _kleinb_args(bases, targets, sigma, n_draws, precision, flags):
        """Argument checks of klein_bases / klein_bases_host, before any library call; returns
        (n, d, T, K)."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~(LGS_DEVICE_PTRS | LGS_Z64):
            raise ValueError(f"klein_bases: unsupported flags {flags!r}")
        shape, tshape = tuple(bases.shape), tuple(targets.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError(f"bases must have shape (n, d, d), got {shape}")
        n, d = int(shape[0]), int(shape[1])
        if not 2 <= d <= LGS_CVP_MAX_D:
            raise ValueError(f"klein_bases supports 2 <= d <= {LGS_CVP_MAX_D}, got d = {d}")
        if len(tshape) != 3 or tshape[0] != n or tshape[2] != d:
            raise ValueError(f"targets must have shape ({n}, T, {d}), got {tshape}")
        T = int(tshape[1])
        if not 1 <= T <= LGS_KLEINB_MAX_T:
            raise ValueError(f"klein_bases supports 1 <= T <= {LGS_KLEINB_MAX_T} targets per basis, got {T}")
        if isinstance(n_draws, bool) or not isinstance(n_draws, (int, np.integer)) or n_draws < 1 or \
                T * int(n_draws) > 1 << 22:
            raise ValueError(f"n_draws must be a positive integer with T * n_draws <= 2^22, got {n_draws!r}")
        if isinstance(precision, bool) or not isinstance(precision, (int, np.integer)) or precision < 1:
            raise ValueError(f"precision must be a positive integer, got {precision!r}")
        if tuple(sigma.shape) != (n,):
            raise ValueError(f"sigma must have shape ({n},), got {tuple(sigma.shape)}")
        return n, d, T, int(n_draws)

    def klein_bases(self, seed, first_sample, bases, targets, sigma, n_draws, precision=10, z_out=None, v_out=None,
                    best_draw=None, dist2=None, status=None, qr_status=None, R=None, cprime=None, z_draws=None,
                    dist2_draws=None, flags=0):
        """Raw lgs_klein_bases on caller buffers (numpy host arrays, or device tensors with
        LGS_DEVICE_PTRS): bases (n, d, d) float64 whose COLUMNS generate lattice p, targets
        (n, T, d) float64, sigma (n,) float64; n_draws = K Klein draws around every target.
        z_out (n, T, d) int32 (int64 with LGS_Z64) and v_out (n, T, d) float64: the closest draw
        of each target and its lattice point; best_draw (n, T) int64, dist2 (n, T) float64,
        status (n, T) int32, qr_status (n,) int32, R (n, d, d), cprime (n, T, d), z_draws
        (n, T, K, d) and dist2_draws (n, T, K); all outputs optional.  Needs no loaded basis."""
        n, d, T, K = self._kleinb_args(bases, targets, sigma, n_draws, precision, flags)
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((bases, "float64", "bases"), (targets, "float64", "targets"),
                                         (sigma, "float64", "sigma"), (z_out, zt, "z_out"),
                                         (v_out, "float64", "v_out"), (best_draw, "int64", "best_draw"),
                                         (dist2, "float64", "dist2"), (status, "int32", "status"),
                                         (qr_status, "int32", "qr_status"), (R, "float64", "R"),
                                         (cprime, "float64", "cprime"), (z_draws, zt, "z_draws"),
                                         (dist2_draws, "float64", "dist2_draws")))
        self._check_shapes(((z_out, (n, T, d), "z_out"), (v_out, (n, T, d), "v_out"), (best_draw, (n, T), "best_draw"),
                            (dist2, (n, T), "dist2"), (status, (n, T), "status"), (qr_status, (n,), "qr_status"),
                            (R, (n, d, d), "R"), (cprime, (n, T, d), "cprime"), (z_draws, (n, T, K, d), "z_draws"),
                            (dist2_draws, (n, T, K), "dist2_draws")))
        self._ck(self._L.lgs_klein_bases(
            self._h, int(seed) & (2 ** 64 - 1), int(first_sample) & (2 ** 64 - 1), n, d, T, K, _ptr(bases),
            _ptr(targets), _ptr(sigma), int(precision), _ptr(z_out), _ptr(v_out),
            _outputs(KleinBasesOutputs, best_draw, dist2, status, qr_status, R, cprime, z_draws, dist2_draws),
            int(flags)))

    def klein_bases_host(self, seed, first_sample, bases, targets, sigma, n_draws, precision=10, *, want_z=True,
                         want_v=True, want_R=True, want_cprime=False, want_draws=False, flags=0):
        """K Klein draws around each host target (n, T, d) in the lattices of host bases (n, d, d),
        widths sigma (n,), into fresh host arrays {"z", "v", "best_draw", "dist2", "status",
        "qr_status", "R", "cprime", "z_draws", "dist2_draws"}; int32 coefficients first, int64 on
        overflow (the same draws)."""
        if isinstance(flags, (int, np.integer)) and not isinstance(flags, bool) and flags & LGS_DEVICE_PTRS:
            raise ValueError("klein_bases_host takes host arrays")
        b = np.ascontiguousarray(bases, dtype=np.float64)
        t = np.ascontiguousarray(targets, dtype=np.float64)
        s = np.ascontiguousarray(sigma, dtype=np.float64)
        n, d, T, K = self._kleinb_args(b, t, s, n_draws, precision, flags)
        if not np.all((s > 0) & np.isfinite(s)):
            raise ValueError("sigma must be positive and finite")

        def call(f, zdt):
            z = np.empty((n, T, d), dtype=zdt) if want_z else None
            v = np.empty((n, T, d)) if want_v else None
            out = {"best_draw": np.empty((n, T), dtype=np.int64), "dist2": np.empty((n, T)),
                   "status": np.empty((n, T), dtype=np.int32), "qr_status": np.empty(n, dtype=np.int32),
                   "R": np.empty((n, d, d)) if want_R else None, "cprime": np.empty((n, T, d)) if want_cprime else None,
                   "z_draws": np.empty((n, T, K, d), dtype=zdt) if want_draws else None,
                   "dist2_draws": np.empty((n, T, K)) if want_draws else None}
            self.klein_bases(seed, first_sample, b, t, s, K, precision, z, v, flags=f, **out)
            out["z_draws"] = _z64(out["z_draws"])
            return {"z": _z64(z), "v": v, **out}
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- IMHK chains, a batch of bases
    @staticmethod
    def _imhkb_args(bases, targets, sigma, n_chains, n_steps, thin, precision, flags):
        """Argument checks of imhk_bases / imhk_bases_host, before any library call; returns
        (n, d, T, C, S, n_keep)."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~(LGS_DEVICE_PTRS | LGS_Z64):
            raise ValueError(f"imhk_bases: unsupported flags {flags!r}")
        shape, tshape = tuple(bases.shape), tuple(targets.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError(f"bases must have shape (n, d, d), got {shape}")
        n, d = int(shape[0]), int(shape[1])
        if not 2 <= d <= LGS_CVP_MAX_D:
            raise ValueError(f"imhk_bases supports 2 <= d <= {LGS_CVP_MAX_D}, got d = {d}")
        if len(tshape) != 3 or tshape[0] != n or tshape[2] != d:
            raise ValueError(f"targets must have shape ({n}, T, {d}), got {tshape}")
        T = int(tshape[1])
        if not 1 <= T <= LGS_KLEINB_MAX_T:
            raise ValueError(f"imhk_bases supports 1 <= T <= {LGS_KLEINB_MAX_T} targets per basis, got {T}")
        if isinstance(n_chains, bool) or not isinstance(n_chains, (int, np.integer)) or n_chains < 1:
            raise ValueError(f"n_chains must be a positive integer, got {n_chains!r}")
        if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 0:
            raise ValueError(f"n_steps must be a non-negative integer, got {n_steps!r}")
        C, S = int(n_chains), int(n_steps)
        if T * C * (S + 1) > 1 << 22:
            raise ValueError(f"imhk_bases needs T * n_chains * (n_steps + 1) <= 2^22, got {T} * {C} * {S + 1}")
        if isinstance(thin, bool) or not isinstance(thin, (int, np.integer)) or not 1 <= thin < 1 << 31:
            raise ValueError(f"thin must be a positive integer, got {thin!r}")
        if isinstance(precision, bool) or not isinstance(precision, (int, np.integer)) or precision < 1:
            raise ValueError(f"precision must be a positive integer, got {precision!r}")
        if tuple(sigma.shape) != (n,):
            raise ValueError(f"sigma must have shape ({n},), got {tuple(sigma.shape)}")
        return n, d, T, C, S, S // int(thin)

    @staticmethod
    def _imhkb_chains(first_chain, n, T, C):
        if isinstance(first_chain, bool) or not isinstance(first_chain, (int, np.integer)) or first_chain < 0 or \
                int(first_chain) + n * T * C > 1 << 32:
            raise ValueError(f"first_chain must be a non-negative integer with first_chain + n * T * n_chains <= 2^32, "
                             f"got {first_chain!r}")

    def imhk_bases(self, seed, first_chain, bases, targets, sigma, n_chains, n_steps, thin=1, precision=10, z_out=None,
                   v_out=None, logw=None, accepts=None, final_step=None, status=None, qr_status=None, R=None,
                   cprime=None, accepted=None, logw_draws=None, z_draws=None, z_samples=None, flags=0):
        """Raw lgs_imhk_bases on caller buffers (numpy host arrays, or device tensors with
        LGS_DEVICE_PTRS): bases (n, d, d) float64 whose COLUMNS generate lattice p, targets
        (n, T, d) float64, sigma (n,) float64; C = n_chains IMHK chains of S = n_steps steps with
        Wang-Ling weights around every target, chain j of target k of basis p being chain
        first_chain + (p T + k) C + j.  z_out (n, T, C, d) int32 (int64 with LGS_Z64) and v_out
        (n, T, C, d) float64: the final states and their lattice points; logw (n, T, C) float64,
        accepts / final_step (n, T, C) int64, status (n, T) int32, qr_status (n,) int32, R
        (n, d, d), cprime (n, T, d), accepted (n, T, C, S) uint8, logw_draws (n, T, C, S + 1),
        z_draws (n, T, C, S + 1, d) and z_samples (n, T, C, S // thin, d): the state after steps
        thin, 2 thin, ..; all outputs optional.  Needs no loaded basis."""
        n, d, T, C, S, nk = self._imhkb_args(bases, targets, sigma, n_chains, n_steps, thin, precision, flags)
        self._imhkb_chains(first_chain, n, T, C)
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((bases, "float64", "bases"), (targets, "float64", "targets"),
                                         (sigma, "float64", "sigma"), (z_out, zt, "z_out"),
                                         (v_out, "float64", "v_out"), (logw, "float64", "logw"),
                                         (accepts, "int64", "accepts"), (final_step, "int64", "final_step"),
                                         (status, "int32", "status"), (qr_status, "int32", "qr_status"),
                                         (R, "float64", "R"), (cprime, "float64", "cprime"),
                                         (accepted, "uint8", "accepted"), (logw_draws, "float64", "logw_draws"),
                                         (z_draws, zt, "z_draws"), (z_samples, zt, "z_samples")))
        self._check_shapes(((z_out, (n, T, C, d), "z_out"), (v_out, (n, T, C, d), "v_out"), (logw, (n, T, C), "logw"),
                            (accepts, (n, T, C), "accepts"), (final_step, (n, T, C), "final_step"),
                            (status, (n, T), "status"), (qr_status, (n,), "qr_status"), (R, (n, d, d), "R"),
                            (cprime, (n, T, d), "cprime"), (accepted, (n, T, C, S), "accepted"),
                            (logw_draws, (n, T, C, S + 1), "logw_draws"), (z_draws, (n, T, C, S + 1, d), "z_draws"),
                            (z_samples, (n, T, C, nk, d), "z_samples")))
        self._ck(self._L.lgs_imhk_bases(
            self._h, int(seed) & (2 ** 64 - 1), int(first_chain), n, d, T, C, S, int(thin), _ptr(bases), _ptr(targets),
            _ptr(sigma), int(precision), _ptr(z_out), _ptr(v_out),
            _outputs(ImhkBasesOutputs, logw, accepts, final_step, status, qr_status, R, cprime, accepted, logw_draws,
                     z_draws, z_samples), int(flags)))

    def imhk_bases_host(self, seed, first_chain, bases, targets, sigma, n_chains, n_steps, thin=1, precision=10, *,
                        want_z=True, want_v=True, want_R=True, want_cprime=False, want_trace=False,
                        want_samples=False, flags=0):
        """C IMHK chains of S steps around each host target (n, T, d) in the lattices of host bases
        (n, d, d), widths sigma (n,), into fresh host arrays {"z", "v", "logw", "accepts",
        "final_step", "status", "qr_status", "R", "cprime"}, with want_trace also "accepted",
        "logw_draws" and "z_draws", with want_samples "z_samples"; int32 coefficients first,
        int64 on overflow (the same chains)."""
        if isinstance(flags, (int, np.integer)) and not isinstance(flags, bool) and flags & LGS_DEVICE_PTRS:
            raise ValueError("imhk_bases_host takes host arrays")
        b = np.ascontiguousarray(bases, dtype=np.float64)
        t = np.ascontiguousarray(targets, dtype=np.float64)
        s = np.ascontiguousarray(sigma, dtype=np.float64)
        n, d, T, C, S, nk = self._imhkb_args(b, t, s, n_chains, n_steps, thin, precision, flags)
        self._imhkb_chains(first_chain, n, T, C)
        if not np.all((s > 0) & np.isfinite(s)):
            raise ValueError("sigma must be positive and finite")

        def call(f, zdt):
            z = np.empty((n, T, C, d), dtype=zdt) if want_z else None
            v = np.empty((n, T, C, d)) if want_v else None
            out = {"logw": np.empty((n, T, C)), "accepts": np.empty((n, T, C), dtype=np.int64),
                   "final_step": np.empty((n, T, C), dtype=np.int64), "status": np.empty((n, T), dtype=np.int32),
                   "qr_status": np.empty(n, dtype=np.int32), "R": np.empty((n, d, d)) if want_R else None,
                   "cprime": np.empty((n, T, d)) if want_cprime else None,
                   "accepted": np.empty((n, T, C, S), dtype=np.uint8) if want_trace else None,
                   "logw_draws": np.empty((n, T, C, S + 1)) if want_trace else None,
                   "z_draws": np.empty((n, T, C, S + 1, d), dtype=zdt) if want_trace else None,
                   "z_samples": np.empty((n, T, C, nk, d), dtype=zdt) if want_samples else None}
            self.imhk_bases(seed, first_chain, b, t, s, C, S, int(thin), precision, z, v, flags=f, **out)
            out["z_draws"], out["z_samples"] = _z64(out["z_draws"]), _z64(out["z_samples"])
            return {"z": _z64(z), "v": v, **out}
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- exact Gaussian mass
    _MASS_FLAGS = LGS_DEVICE_PTRS | LGS_COORD_MAJOR | LGS_TARGETS_QFRAME

    def _mass_args(self, targets, sigma, max_nodes, flags, moments):
        """Argument checks of gaussian_mass / gaussian_mass_host, before any library call."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~self._MASS_FLAGS:
            raise ValueError(f"gaussian_mass: unsupported flags {flags!r}")
        if self.d > LGS_MASS_MAX_D:
            raise ValueError(f"gaussian_mass supports d <= {LGS_MASS_MAX_D}, the loaded basis has d = {self.d}")
        if moments and self.d > LGS_MASS_MOMENTS_MAX_D:
            raise ValueError(f"gaussian_mass: sum_z supports d <= {LGS_MASS_MOMENTS_MAX_D}, "
                             f"the loaded basis has d = {self.d}")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or \
                not (sigma > 0 and np.isfinite(sigma)):
            raise ValueError(f"sigma must be a positive finite number, got {sigma!r}")
        if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or \
                not 1 <= max_nodes <= 1 << 40:
            raise ValueError(f"max_nodes must be an integer in 1..2^40, got {max_nodes!r}")
        return self._n_targets(targets, flags)

    def gaussian_mass(self, targets, sigma, radius2, shift=None, max_nodes=1 << 26, cprime_out=None, mass=None,
                      energy=None, points=None, dist2_min=None, sum_z=None, nodes=None, status=None, flags=0):
        """Raw lgs_gaussian_mass on caller buffers (numpy host or device tensors): the Gaussian
        weight, at width sigma, of the lattice points with squared distance below radius2 of
        each target, by fixed-radius enumeration.  targets as in closest_vector; radius2 (n,)
        float64, required; shift (n,) float64 (subtracted from the squared distance inside the
        exponential); mass / energy / dist2_min (n,) float64, points / nodes (n,) int64, status
        (n,) int32, sum_z (n, d) float64, all optional."""
        n = self._mass_args(targets, sigma, max_nodes, flags, sum_z is not None)
        if radius2 is None:
            raise ValueError("radius2 is required: the ball of gaussian_mass is finite")
        _check_bufs(flags, self.device, ((targets, "float64", "targets"), (radius2, "float64", "radius2"),
                                         (shift, "float64", "shift"), (cprime_out, "float64", "cprime_out"),
                                         (mass, "float64", "mass"), (energy, "float64", "energy"),
                                         (points, "int64", "points"), (dist2_min, "float64", "dist2_min"),
                                         (sum_z, "float64", "sum_z"), (nodes, "int64", "nodes"),
                                         (status, "int32", "status")))
        for a, want, name in ((cprime_out, (n, self.d), "cprime_out"), (radius2, (n,), "radius2"),
                              (shift, (n,), "shift"), (mass, (n,), "mass"), (energy, (n,), "energy"),
                              (points, (n,), "points"), (dist2_min, (n,), "dist2_min"), (sum_z, (n, self.d), "sum_z"),
                              (nodes, (n,), "nodes"), (status, (n,), "status")):
            if a is not None and not isinstance(a, int) and tuple(a.shape) != want:
                raise ValueError(f"{name}: expected shape {want}, got {tuple(a.shape)}")
        self._ck(self._L.lgs_gaussian_mass(self._h, n, _ptr(targets), float(sigma), _ptr(radius2), _ptr(shift),
                                           int(max_nodes), _ptr(cprime_out),
                                           _outputs(MassOutputs, mass, energy, points, dist2_min, sum_z, nodes,
                                                    status), int(flags)))

    def gaussian_mass_host(self, targets, sigma, radius2, shift=None, max_nodes=1 << 26, *, moments=False,
                           want_cprime=False, flags=0):
        """lgs_gaussian_mass of host targets (n, d) into fresh host arrays {"mass", "energy",
        "points", "dist2_min", "sum_z" (None without moments), "nodes", "status", "cprime"}."""
        if isinstance(flags, (int, np.integer)) and flags & (LGS_DEVICE_PTRS | LGS_COORD_MAJOR):
            raise ValueError("gaussian_mass_host takes row-major host targets")
        t = np.ascontiguousarray(targets, dtype=np.float64)
        n = self._mass_args(t, sigma, max_nodes, flags, moments)
        if radius2 is None:
            raise ValueError("radius2 is required: the ball of gaussian_mass is finite")
        r2 = np.ascontiguousarray(radius2, dtype=np.float64)
        if r2.shape != (n,) or not np.all((r2 >= 0) & np.isfinite(r2)):
            raise ValueError(f"radius2 must hold {n} finite non-negative values")
        sh = None
        if shift is not None:
            sh = np.ascontiguousarray(shift, dtype=np.float64)
            if sh.shape != (n,) or not np.all(np.isfinite(sh)):
                raise ValueError(f"shift must hold {n} finite values")
        r = {"mass": np.empty(n), "energy": np.empty(n), "points": np.empty(n, dtype=np.int64),
             "dist2_min": np.empty(n), "sum_z": np.empty((n, self.d)) if moments else None,
             "nodes": np.empty(n, dtype=np.int64), "status": np.empty(n, dtype=np.int32),
             "cprime": np.empty((n, self.d)) if want_cprime else None}
        self.gaussian_mass(t, sigma, r2, sh, max_nodes, r["cprime"], r["mass"], r["energy"], r["points"],
                           r["dist2_min"], r["sum_z"], r["nodes"], r["status"], flags)
        return r

    # ---------------------------------------------------------------- the ball's points, the exact sampler
    _BALL_FLAGS = LGS_DEVICE_PTRS | LGS_COORD_MAJOR | LGS_TARGETS_QFRAME | LGS_Z64

    def _ball_args(self, name, targets, max_nodes, rows, rows_name, flags):
        """Argument checks of ball_points / exact_table, before any library call."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~self._BALL_FLAGS:
            raise ValueError(f"{name}: unsupported flags {flags!r}")
        if self.d > LGS_MASS_MAX_D:
            raise ValueError(f"{name} supports d <= {LGS_MASS_MAX_D}, the loaded basis has d = {self.d}")
        if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or \
                not 1 <= max_nodes <= 1 << 40:
            raise ValueError(f"max_nodes must be an integer in 1..2^40, got {max_nodes!r}")
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or rows < 0:
            raise ValueError(f"{rows_name} must be a non-negative integer, got {rows!r}")
        return self._n_targets(targets, flags)

    @staticmethod
    def _check_shapes(specs):
        for a, want, name in specs:
            if a is not None and not isinstance(a, int) and tuple(a.shape) != want:
                raise ValueError(f"{name}: expected shape {want}, got {tuple(a.shape)}")

    def ball_points(self, targets, radius2, max_nodes=1 << 26, capacity=0, z_out=None, dist2_out=None,
                    cprime_out=None, offsets=None, nodes=None, status=None, flags=0):
        """Raw lgs_ball_points on caller buffers (numpy host or device tensors): the lattice
        points with squared distance below radius2 of each target, in traversal order.
        targets as in gaussian_mass; radius2 (n,) float64, required; z_out (capacity, d) int32
        (int64 with LGS_Z64) and dist2_out (capacity,) float64, both None with capacity 0 (the
        size query); offsets (n + 1,) int64, nodes (n,) int64, status (n,) int32, optional.
        Rows are written only when offsets[n] <= capacity."""
        n = self._ball_args("ball_points", targets, max_nodes, capacity, "capacity", flags)
        if radius2 is None:
            raise ValueError("radius2 is required: the ball of ball_points is finite")
        if capacity > 0 and (z_out is None or dist2_out is None):
            raise ValueError("capacity > 0 needs z_out and dist2_out")
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((targets, "float64", "targets"), (radius2, "float64", "radius2"),
                                         (z_out, zt, "z_out"), (dist2_out, "float64", "dist2_out"),
                                         (cprime_out, "float64", "cprime_out"), (offsets, "int64", "offsets"),
                                         (nodes, "int64", "nodes"), (status, "int32", "status")))
        self._check_shapes(((radius2, (n,), "radius2"), (z_out, (capacity, self.d), "z_out"),
                            (dist2_out, (capacity,), "dist2_out"), (cprime_out, (n, self.d), "cprime_out"),
                            (offsets, (n + 1,), "offsets"), (nodes, (n,), "nodes"), (status, (n,), "status")))
        self._ck(self._L.lgs_ball_points(self._h, n, _ptr(targets), _ptr(radius2), int(max_nodes), int(capacity),
                                         _ptr(z_out) if capacity else None, _ptr(dist2_out) if capacity else None,
                                         _ptr(cprime_out), _outputs(BallOutputs, offsets, nodes, status), int(flags)))

    def _host_radius(self, n, radius2, name):
        if radius2 is None:
            raise ValueError(f"radius2 is required: the ball of {name} is finite")
        r2 = np.ascontiguousarray(radius2, dtype=np.float64)
        if r2.shape != (n,) or not np.all((r2 >= 0) & np.isfinite(r2)):
            raise ValueError(f"radius2 must hold {n} finite non-negative values")
        return r2

    def ball_points_host(self, targets, radius2, max_nodes=1 << 26, max_points=1 << 24, *, want_cprime=False,
                         flags=0):
        """The balls of host targets (n, d) into fresh host arrays {"z" (N, d) int64, "dist2"
        (N,), "offsets" (n + 1,), "nodes", "status", "cprime"}: a size query, then the listing
        call (int32 coefficients first, int64 on overflow).  More than max_points points in
        all is a ValueError."""
        if isinstance(flags, (int, np.integer)) and not isinstance(flags, bool) and \
                flags & (LGS_DEVICE_PTRS | LGS_COORD_MAJOR):
            raise ValueError("ball_points_host takes row-major host targets")
        t = np.ascontiguousarray(targets, dtype=np.float64)
        n = self._ball_args("ball_points", t, max_nodes, max_points, "max_points", flags)
        r2 = self._host_radius(n, radius2, "ball_points")
        off = np.zeros(n + 1, dtype=np.int64)
        nd, st = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32)
        cp = np.empty((n, self.d)) if want_cprime else None
        self.ball_points(t, r2, max_nodes, 0, None, None, cp, off, nd, st, flags)
        total = int(off[n])
        if total > max_points:
            raise ValueError(f"the balls hold {total} points > max_points = {max_points}")

        def call(f, zdt):
            z, d2 = np.empty((total, self.d), dtype=zdt), np.empty(total)
            if total:
                self.ball_points(t, r2, max_nodes, total, z, d2, None, off, nd, st, f)
            return {"z": _z64(z), "dist2": d2, "offsets": off, "nodes": nd, "status": st, "cprime": cp}
        return _host_retry(flags, call)

    def exact_table(self, targets, sigma, radius2, shift=None, max_nodes=1 << 26, max_points=1 << 24, offsets=None,
                    nodes=None, status=None, mass=None, weights=None, cum=None, flags=0):
        """Raw lgs_exact_table on caller buffers: lists the balls of the targets and keeps
        them in the context, with weights exp((shift - D) / 2 sigma^2) and their blocked
        running sums, for exact_sample.  offsets (n + 1,) int64, nodes (n,) int64, status (n,)
        int32, mass (n,) float64, weights / cum (max_points,) float64, all optional.  A target
        over max_nodes, an empty ball or more than max_points points: LgsError (INVALID) after
        offsets, nodes and status are filled, and no table is kept."""
        n = self._ball_args("exact_table", targets, max_nodes, max_points, "max_points", flags)
        if n < 1:
            raise ValueError("exact_table needs at least one target")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or \
                not (sigma > 0 and np.isfinite(sigma)):
            raise ValueError(f"sigma must be a positive finite number, got {sigma!r}")
        if radius2 is None:
            raise ValueError("radius2 is required: the ball of exact_table is finite")
        _check_bufs(flags & ~LGS_Z64, self.device,
                    ((targets, "float64", "targets"), (radius2, "float64", "radius2"), (shift, "float64", "shift"),
                     (offsets, "int64", "offsets"), (nodes, "int64", "nodes"), (status, "int32", "status"),
                     (mass, "float64", "mass"), (weights, "float64", "weights"), (cum, "float64", "cum")))
        self._check_shapes(((radius2, (n,), "radius2"), (shift, (n,), "shift"), (offsets, (n + 1,), "offsets"),
                            (nodes, (n,), "nodes"), (status, (n,), "status"), (mass, (n,), "mass"),
                            (weights, (max_points,), "weights"), (cum, (max_points,), "cum")))
        self._table_n = 0
        self._ck(self._L.lgs_exact_table(self._h, n, _ptr(targets), float(sigma), _ptr(radius2), _ptr(shift),
                                         int(max_nodes), int(max_points),
                                         _outputs(ExactTableOutputs, offsets, nodes, status, mass, weights, cum),
                                         int(flags)))
        self._table_n = n

    def exact_table_host(self, targets, sigma, radius2, shift=None, max_nodes=1 << 26, max_points=1 << 24, *,
                         want_weights=False, flags=0):
        """exact_table of host targets (n, d) into fresh host arrays {"offsets", "nodes",
        "status", "mass", "weights", "cum"} (the last two None without want_weights; with it a
        size query by ball_points comes first, so that they hold offsets[n] values)."""
        if isinstance(flags, (int, np.integer)) and not isinstance(flags, bool) and \
                flags & (LGS_DEVICE_PTRS | LGS_COORD_MAJOR):
            raise ValueError("exact_table_host takes row-major host targets")
        t = np.ascontiguousarray(targets, dtype=np.float64)
        n = self._ball_args("exact_table", t, max_nodes, max_points, "max_points", flags)
        r2 = self._host_radius(n, radius2, "exact_table")
        sh = None
        if shift is not None:
            sh = np.ascontiguousarray(shift, dtype=np.float64)
            if sh.shape != (n,) or not np.all(np.isfinite(sh)):
                raise ValueError(f"shift must hold {n} finite values")
        r = {"offsets": np.zeros(n + 1, dtype=np.int64), "nodes": np.empty(n, dtype=np.int64),
             "status": np.empty(n, dtype=np.int32), "mass": np.empty(n), "weights": None, "cum": None}
        cap = max_points
        if want_weights:
            self.ball_points(t, r2, max_nodes, 0, offsets=r["offsets"], flags=flags)
            cap = min(max_points, int(r["offsets"][n]))
            r["weights"], r["cum"] = np.empty(cap), np.empty(cap)
        self.exact_table(t, sigma, r2, sh, max_nodes, cap, r["offsets"], r["nodes"], r["status"], r["mass"],
                         r["weights"], r["cum"], flags)
        return r

    def exact_sample(self, seed, first_sample, n_draws, n_targets, z_out=None, v_out=None, index=None, dist2=None,
                     flags=0):
        """Raw lgs_exact_sample on caller buffers: n_draws rows per target of the table, by
        inverse CDF.  n_targets is the table's target count (the buffers' shapes are checked
        against it); z_out (n_targets * n_draws, d) int32 / int64, v_out likewise float64, index
        (n_targets * n_draws,) int64, dist2 likewise float64."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or \
                flags & ~(LGS_DEVICE_PTRS | LGS_Z64):
            raise ValueError(f"exact_sample: unsupported flags {flags!r}")
        for v, name in ((n_draws, "n_draws"), (n_targets, "n_targets")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
        for v, name in ((seed, "seed"), (first_sample, "first_sample")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 1 << 64:
                raise ValueError(f"{name} must be an integer in 0..2^64-1, got {v!r}")
        total = int(n_targets) * int(n_draws)
        zt = "int64" if flags & LGS_Z64 else "int32"
        _check_bufs(flags, self.device, ((z_out, zt, "z_out"), (v_out, "float64", "v_out"),
                                         (index, "int64", "index"), (dist2, "float64", "dist2")))
        self._check_shapes(((z_out, (total, self.d), "z_out"), (v_out, (total, self.d), "v_out"),
                            (index, (total,), "index"), (dist2, (total,), "dist2")))
        if getattr(self, "_table_n", None) not in (None, 0) and self._table_n != n_targets:
            raise ValueError(f"the table holds {self._table_n} targets, n_targets = {n_targets}")
        self._ck(self._L.lgs_exact_sample(self._h, int(seed), int(first_sample), int(n_draws), _ptr(z_out),
                                          _ptr(v_out), _outputs(ExactSampleOutputs, index, dist2), int(flags)))

    def exact_sample_host(self, seed, first_sample, n_draws, n_targets, *, want_z=True, want_v=True, flags=0):
        """exact_sample into fresh host arrays {"z", "v", "index", "dist2"} (int32 coefficients
        first, int64 on overflow: the draws do not depend on the output width)."""
        if isinstance(flags, (int, np.integer)) and not isinstance(flags, bool) and flags & LGS_DEVICE_PTRS:
            raise ValueError("exact_sample_host returns host arrays")

        def call(f, zdt):
            total = int(n_targets) * int(n_draws)
            z, v, _ = self._host_zvc(total, zdt, want_z, want_v, False)
            ix, d2 = np.empty(total, dtype=np.int64), np.empty(total)
            self.exact_sample(seed, first_sample, n_draws, n_targets, z, v, ix, d2, f)
            return {"z": _z64(z), "v": v, "index": ix, "dist2": d2}
        return _host_retry(flags, call)

    # ---------------------------------------------------------------- LLL reduction
    @staticmethod
    def _lll_args(basis, delta, eta, max_iters, flags):
        """Argument checks of lll_reduce / lll_reduce_host, before any library call; returns (n, d)."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~LGS_DEVICE_PTRS:
            raise ValueError(f"lll_reduce: unsupported flags {flags!r}")
        shape = tuple(basis.shape)
        if len(shape) != 3 or shape[1] != shape[2]:
            raise ValueError(f"basis must have shape (n, d, d), got {shape}")
        n, d = int(shape[0]), int(shape[1])
        if not 2 <= d <= LGS_LLL_MAX_D:
            raise ValueError(f"lll_reduce supports 2 <= d <= {LGS_LLL_MAX_D}, got d = {d}")
        for name, v, lo, hi in (("delta", delta, 0.25, 1.0), ("eta", eta, 0.5, 1.0)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo < v < hi:
                raise ValueError(f"{name} must lie in ({lo}, {hi}), got {v!r}")
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or \
                not 1 <= max_iters <= 1 << 40:
            raise ValueError(f"max_iters must be an integer in 1..2^40, got {max_iters!r}")
        return n, d

    def lll_reduce(self, basis, basis_out, U_out, delta=0.99, eta=0.51, max_iters=1 << 40, swaps=None, iters=None,
                   passes=None, status=None, gs_norm2=None, flags=0):
        """Raw lgs_lll_reduce on caller buffers (numpy host arrays, or device tensors with
        LGS_DEVICE_PTRS): basis, basis_out, U_out (n, d, d) int64 with vector i in COLUMN i
        (basis_out = basis @ U_out); swaps, iters, passes (n,) int64, status (n,) int32,
        gs_norm2 (n, d) float64, all optional.  Needs no loaded basis."""
        n, d = self._lll_args(basis, delta, eta, max_iters, flags)
        _check_bufs(flags, self.device, ((basis, "int64", "basis"), (basis_out, "int64", "basis_out"),
                                         (U_out, "int64", "U_out"), (swaps, "int64", "swaps"),
                                         (iters, "int64", "iters"), (passes, "int64", "passes"),
                                         (status, "int32", "status"), (gs_norm2, "float64", "gs_norm2")))
        if basis_out is None or U_out is None:
            raise ValueError("basis_out and U_out are required")
        self._check_shapes(((basis_out, (n, d, d), "basis_out"), (U_out, (n, d, d), "U_out"), (swaps, (n,), "swaps"),
                            (iters, (n,), "iters"), (passes, (n,), "passes"), (status, (n,), "status"),
                            (gs_norm2, (n, d), "gs_norm2")))
        self._ck(self._L.lgs_lll_reduce(self._h, n, d, _ptr(basis), float(delta), float(eta), int(max_iters),
                                        _ptr(basis_out), _ptr(U_out),
                                        _outputs(LllOutputs, swaps, iters, passes, status, gs_norm2), int(flags)))

    def lll_reduce_host(self, basis, delta=0.99, eta=0.51, max_iters=1 << 40):
        """LLL of host bases (n, d, d) int64, vectors in columns, into fresh host arrays
        {"basis", "U", "swaps", "iters", "passes", "status", "gs_norm2"}."""
        b = np.ascontiguousarray(basis)
        if b.dtype != np.int64:
            raise ValueError(f"basis: expected int64, got {b.dtype}")
        n, d = self._lll_args(b, delta, eta, max_iters, 0)
        if np.any(np.abs(b) >= 1 << 28):
            raise ValueError("basis entries must be below 2^28 in magnitude")
        out = {"basis": np.empty((n, d, d), dtype=np.int64), "U": np.empty((n, d, d), dtype=np.int64),
               "swaps": np.empty(n, dtype=np.int64), "iters": np.empty(n, dtype=np.int64),
               "passes": np.empty(n, dtype=np.int64), "status": np.empty(n, dtype=np.int32),
               "gs_norm2": np.empty((n, d))}
        self.lll_reduce(b, out["basis"], out["U"], delta, eta, max_iters, out["swaps"], out["iters"], out["passes"],
                        out["status"], out["gs_norm2"])
        return out

    # ---------------------------------------------------------------- BKZ reduction
    _BKZ_COUNTERS = ("swaps", "iters", "passes", "tours", "blocks", "insertions", "nodes", "truncated")

    @classmethod
    def _bkz_args(cls, basis, block_size, delta, eta, max_tours, max_iters, enum_nodes, flags):
        """Argument checks of bkz_reduce / bkz_reduce_host, before any library call; returns (n, d)."""
        if isinstance(flags, bool) or not isinstance(flags, (int, np.integer)) or flags & ~LGS_DEVICE_PTRS:
            raise ValueError(f"bkz_reduce: unsupported flags {flags!r}")
        n, d = cls._lll_args(basis, delta, eta, max_iters, flags)
        for name, v, lo, hi in (("block_size", block_size, 2, LGS_BKZ_MAX_BLOCK), ("max_tours", max_tours, 1, 1 << 40),
                                ("enum_nodes", enum_nodes, 1, 1 << 40)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
        return n, d

    def bkz_reduce(self, basis, basis_out, U_out, block_size, delta=0.99, eta=0.51, max_tours=1 << 40,
                   max_iters=1 << 40, enum_nodes=1 << 40, swaps=None, iters=None, passes=None, tours=None,
                   blocks=None, insertions=None, nodes=None, truncated=None, status=None, gs_norm2=None, flags=0):
        """Raw lgs_bkz_reduce on caller buffers (numpy host arrays, or device tensors with
        LGS_DEVICE_PTRS): basis, basis_out, U_out (n, d, d) int64 with vector i in COLUMN i
        (basis_out = basis @ U_out); the eight counters (n,) int64, status (n,) int32, gs_norm2
        (n, d) float64, all optional.  Needs no loaded basis."""
        n, d = self._bkz_args(basis, block_size, delta, eta, max_tours, max_iters, enum_nodes, flags)
        ctr = (swaps, iters, passes, tours, blocks, insertions, nodes, truncated)
        _check_bufs(flags, self.device, ((basis, "int64", "basis"), (basis_out, "int64", "basis_out"),
                                         (U_out, "int64", "U_out"), (status, "int32", "status"),
                                         (gs_norm2, "float64", "gs_norm2")) +
                    tuple((b, "int64", nm) for b, nm in zip(ctr, self._BKZ_COUNTERS)))
        if basis_out is None or U_out is None:
            raise ValueError("basis_out and U_out are required")
        self._check_shapes(((basis_out, (n, d, d), "basis_out"), (U_out, (n, d, d), "U_out"), (status, (n,), "status"),
                            (gs_norm2, (n, d), "gs_norm2")) +
                           tuple((b, (n,), nm) for b, nm in zip(ctr, self._BKZ_COUNTERS)))
        self._ck(self._L.lgs_bkz_reduce(self._h, n, d, _ptr(basis), int(block_size), float(delta), float(eta),
                                        int(max_tours), int(max_iters), int(enum_nodes), _ptr(basis_out), _ptr(U_out),
                                        _outputs(BkzOutputs, *ctr, status, gs_norm2), int(flags)))

    def bkz_reduce_host(self, basis, block_size, delta=0.99, eta=0.51, max_tours=1 << 40, max_iters=1 << 40,
                        enum_nodes=1 << 40):
        """BKZ of host bases (n, d, d) int64, vectors in columns, into fresh host arrays {"basis",
        "U", the eight counters, "status", "gs_norm2"}."""
        b = np.ascontiguousarray(basis)
        if b.dtype != np.int64:
            raise ValueError(f"basis: expected int64, got {b.dtype}")
        n, d = self._bkz_args(b, block_size, delta, eta, max_tours, max_iters, enum_nodes, 0)
        if np.any(np.abs(b) >= 1 << 28):
            raise ValueError("basis entries must be below 2^28 in magnitude")
        out = {"basis": np.empty((n, d, d), dtype=np.int64), "U": np.empty((n, d, d), dtype=np.int64),
               "status": np.empty(n, dtype=np.int32), "gs_norm2": np.empty((n, d))}
        out.update({nm: np.empty(n, dtype=np.int64) for nm in self._BKZ_COUNTERS})
        self.bkz_reduce(b, out["basis"], out["U"], block_size, delta, eta, max_tours, max_iters, enum_nodes,
                        *(out[nm] for nm in self._BKZ_COUNTERS), out["status"], out["gs_norm2"])
        return out

    # ---------------------------------------------------------------- diagnostics
    def series_stats(self, x, n_series, n, group_size, group_stride, series_stride, time_stride,
                     max_lag=-1, window_c=5.0, batch_size=0, mean=None, c0=None, acf=None,
                     tau=None, batch_means=None, flags=0):
        """Raw lgs_series_stats; x / outputs are host arrays or device tensors
        (flags must then carry LGS_DEVICE_PTRS); element type via x_flags(x)."""
        self._ck(self._L.lgs_series_stats(self._h, _ptr(x), int(n_series), int(n), int(group_size),
                                     int(group_stride), int(series_stride), int(time_stride),
                                     int(max_lag), float(window_c), int(batch_size), _ptr(mean),
                                     _ptr(c0), _ptr(acf), _ptr(tau), _ptr(batch_means),
                                     int(flags | x_flags(x))))

    def gram(self, x, shift=None, sum_out=None, gram_out=None, coord_major=False, flags=0, ldx=None,
             shape=None):
        """sum y and sum y y^T, y = x - shift, ADDED to sum_out (d) / gram_out (d x d):
        int64 (exact) for int32 / int64 x, fp64 for float64 x.  ldx (default: the row
        length of x) is the leading dimension in elements; x is then the padded 2-D
        buffer and shape its logical shape, (d, n) coordinate-major or (n, d)."""
        f = flags | (LGS_COORD_MAJOR if coord_major else 0) | x_flags(x)
        shape = tuple(x.shape) if shape is None else tuple(shape)
        if coord_major:
            d, n = shape
        else:
            n, d = shape
        if ldx is None:
            ldx = n if coord_major else d
        _check_padded(x, shape, int(ldx))
        self._ck(self._L.lgs_gram(self._h, int(d), int(n), _ptr(x), int(ldx),
                             _ptr(shift), _ptr(sum_out), _ptr(gram_out), int(f)))

    def jump_distance(self, x, out, flags=0, ld=None, shape=None):
        """||x[t+1] - x[t]||_2 of the rows of x (n x d) into out (n - 1).  ld (default d)
        is the row pitch in elements; x is then the padded buffer, shape the logical (n, d)."""
        n, d = tuple(x.shape) if shape is None else tuple(shape)
        if ld is None:
            ld = d
        _check_padded(x, (n, d), int(ld))
        self._ck(self._L.lgs_jump_distance(self._h, int(n), int(d), _ptr(x), int(ld), _ptr(out),
                                      int(flags | x_flags(x))))

    def marginal_tvd(self, x1, x2, out, flags=0):
        if _dtype_name(x1) != _dtype_name(x2):
            raise TypeError("both sample sets must have the same dtype")
        d = x1.shape[1]
        self._ck(self._L.lgs_marginal_tvd(self._h, int(d), _ptr(x1), int(x1.shape[0]), _ptr(x2),
                                     int(x2.shape[0]), _ptr(out), int(flags | x_flags(x1))))

    def column_range(self, x, lo, hi, flags=0):
        """Per-column min / max (fp64) of row-major (n, d) samples into lo / hi (d)."""
        n, d = x.shape
        self._ck(self._L.lgs_column_range(self._h, int(d), _ptr(x), int(n), _ptr(lo), _ptr(hi),
                                     int(flags | x_flags(x))))

    def histogram(self, x, edges, first_denom, counts, flags=0):
        """np.histogram counts per column: x (n, d), edges (d, bins+1), first_denom
        (d, 2), counts (d, bins) int64 -- all host or all device (LGS_DEVICE_PTRS)."""
        n, d = x.shape
        bins = edges.shape[1] - 1
        if tuple(edges.shape) != (d, bins + 1) or tuple(first_denom.shape) != (d, 2) or \
                tuple(counts.shape) != (d, bins):
            raise ValueError("histogram: edges (d, bins+1), first_denom (d, 2), counts (d, bins)")
        _check_bufs(flags, self.device, ((edges, "float64", "edges"), (first_denom, "float64", "first_denom"),
                                         (counts, "int64", "counts")))
        self._ck(self._L.lgs_histogram(self._h, int(d), _ptr(x), int(n), int(bins), _ptr(edges),
                                  _ptr(first_denom), _ptr(counts), int(flags | x_flags(x))))

    # ---------------------------------------------------------------- timing / info
    def timing_enable(self, on=True):
        self._ck(self._L.lgs_timing_enable(self._h, 1 if on else 0))

    def timing_get(self, kernel):
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        self._ck(self._L.lgs_timing_get(self._h, int(kernel), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def resolved(self, reset=False):
        """Decisions the certificate did not cover and that were redone at the
        reference-order mean (LGS_COUNTER_RESOLVED), since creation / the last reset."""
        v = ctypes.c_uint64(0)
        self._ck(self._L.lgs_counter(self._h, LGS_COUNTER_RESOLVED, 1 if reset else 0, ctypes.byref(v)))
        return v.value

    def fallbacks(self, reset=False):
        """Klein launches redone with a wider store / the fp64 far field (LGS_COUNTER_FALLBACK)."""
        v = ctypes.c_uint64(0)
        self._ck(self._L.lgs_counter(self._h, LGS_COUNTER_FALLBACK, 1 if reset else 0, ctypes.byref(v)))
        return v.value

    def counter(self, which, reset=False):
        """lgs_counter: one of the LGS_COUNTER_* event counts since creation / the last reset."""
        v = ctypes.c_uint64(0)
        self._ck(self._L.lgs_counter(self._h, int(which), 1 if reset else 0, ctypes.byref(v)))
        return v.value

    def qskip_elided(self, reset=False):
        """lgs_qskip_elided: the q-panel skips (LGS_COUNTER_QSKIP) that found their panel clean
        and stored nothing."""
        v = ctypes.c_uint64(0)
        self._ck(self._L.lgs_qskip_elided(self._h, 1 if reset else 0, ctypes.byref(v)))
        return v.value

    def bz_tiles(self, reset=False):
        """lgs_bz_tiles: (lean, gemm) -- the 64 x 128 tiles of the int8-digit lattice points
        computed without the digit GEMM (diagonal-only blocks of B) and with it."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._ck(self._L.lgs_bz_tiles(self._h, 1 if reset else 0, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def device_info(self):
        buf = ctypes.create_string_buffer(256)
        ncu = ctypes.c_int(0)
        mem = ctypes.c_int64(0)
        self._ck(self._L.lgs_device_info(self._h, buf, 256, ctypes.byref(ncu), ctypes.byref(mem)))
        return {"name": buf.value.decode(), "n_cu": ncu.value, "hbm_bytes": mem.value}


def version() -> int:
    return load_library().lgs_version()
