"""ctypes binding of libfigh.so (include/figh.h).  No torch, no fallback.

``load()`` raises if the shared library is missing; every compute call raises
``FighError`` when the library reports a failure (no HIP device, bad
arguments ...).  Nothing in this package computes on the CPU instead.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FIGH_LIB_PATH: another build of the same ABI (same-box A/B of kernel variants); default is the in-tree library
LIB_PATH = os.environ.get("FIGH_LIB_PATH") or os.path.join(_HERE, "libfigh.so")

ABI_VERSION = 117  # include/figh.h FIGH_ABI_VERSION: load() refuses a library of another ABI

FIGH_OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_ALLOC, ERR_UNSUPPORTED, ERR_COMM = -1, -2, -3, -4, -5

MODE_JOINT_TORQUE, MODE_EXT_WRENCH = 0, 1
FLAG_FRICTION, FLAG_ACT_INERTIA, FLAG_OFFSET, FLAG_TX40, FLAG_GENERIC, FLAG_BLOCKED_INPUTS = 1, 2, 4, 8, 256, 512
FLAG_COMPACT_BLOCKS = 2048  # figh_regressor_build_padded writes the block-compact W (figh.h)
FLAG_FORCE_COMPACT = 8192  # figh_regressor_build_padded, external wrench: force rows in their own region, a line per 4 links
FLAG_LINK_COMPACT = 4096  # figh_regressor_build_padded, external wrench on a free-flyer root: links without entries dropped
FLAG_ZEROS_PRESENT = 1024  # opt-in of figh_regressor_build_padded: structural zeros of W are already there (figh.h)

_c_double_p = C.POINTER(C.c_double)
_c_int32_p = C.POINTER(C.c_int32)

# symbol -> (restype, argtypes); exactly the declarations of include/figh.h
SIGNATURES = {
    "figh_version": (C.c_int, []),
    "figh_last_error": (C.c_char_p, []),
    "figh_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "figh_device_set": (C.c_int, [C.c_int]),
    "figh_host_wait_mode": (C.c_int, [C.c_int]),
    "figh_tsqr_null_pivot_tol": (C.c_int, [C.c_double]),
    "figh_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "figh_device_info": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "figh_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "figh_free": (C.c_int, [C.c_void_p]),
    "figh_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "figh_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "figh_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "figh_host_free": (C.c_int, [C.c_void_p]),
    "figh_memcpy_d2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "figh_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t]),
    "figh_synchronize": (C.c_int, []),
    "figh_profile_enable": (C.c_int, [C.c_int]),
    "figh_profile_reset": (C.c_int, []),
    "figh_profile_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), _c_double_p]),
    "figh_model_create": (C.c_int, [C.c_int, _c_int32_p, _c_int32_p, _c_double_p, _c_double_p, _c_int32_p,
                                    _c_int32_p, _c_double_p, _c_int32_p, C.POINTER(C.c_void_p)]),
    "figh_model_destroy": (C.c_int, [C.c_void_p]),
    "figh_regressor_shape": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "figh_regressor_build": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "figh_regressor_build_padded": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "figh_regressor_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "figh_repack_samples": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "figh_coupling_tx40": (C.c_int, [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "figh_colsq": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p]),
    "figh_gather_cols": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "figh_place_block": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_int64]),
    "figh_matvec": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "figh_block_sqnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "figh_tsqr": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, _c_double_p, C.c_int,
                            C.c_void_p]),
    "figh_tsqr_structured": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, _c_double_p,
                                       C.c_int, _c_int32_p, C.c_int, C.c_void_p]),
    "figh_tsqr_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "figh_select_columns": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "figh_tsqr_selected_wrench": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int64]),
    "figh_regressor_force_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "figh_model_set_active_rows": (C.c_int, [C.c_void_p, _c_int32_p, C.c_int]),
    "figh_regressor_link_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _c_int32_p, C.POINTER(C.c_int)]),
    "figh_tsqr_selected_blocks": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "figh_block_rows_residuals": (C.c_int, [C.c_void_p, C.c_int, _c_int32_p, C.c_int, C.c_void_p, C.c_void_p]),
    "figh_tsqr_selected": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int,
                                     C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "figh_regressor_tsqr_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double,
                                            C.c_void_p]),
    "figh_chain_host_tail": (C.c_int, [C.c_void_p]),
    "figh_chain_pass_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "figh_tsqr_merge_base": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]),
    "figh_tsqr_merge_base_norms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int,
                                             C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "figh_compact_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                    C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    "figh_base_permutation": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]),
    "figh_regressor_colsq": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_void_p]),
    "figh_regressor_tsqr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, _c_double_p, C.c_int, C.c_int64,
                                      C.c_void_p]),
    "figh_regressor_tsqr_norms": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, _c_double_p, C.c_int, C.c_int64,
                                            C.c_void_p, C.c_void_p]),
    "figh_regressor_tsqr_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "figh_regressor_tsqr_batch_fused": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "figh_regressor_gram": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, _c_double_p, _c_double_p,
                                      _c_double_p]),
    "figh_filtfilt_cols": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, _c_double_p, _c_double_p,
                                     C.c_int, C.c_int, _c_double_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int64)]),
    "figh_medfilt_cols": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "figh_joint_difference": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "figh_gradient_cols": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_int64]),
    "figh_quat_log": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]),
    "figh_rotvec_to_quat": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "figh_wrench_transport": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_int]),
    "figh_spline_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_double, _c_int32_p, _c_int32_p,
                                     _c_double_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    "figh_excitation_constraints": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, _c_int32_p, _c_int32_p, C.c_int,
                                              _c_int32_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_int64]),
    "figh_collision_distances": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, _c_int32_p, C.c_void_p, C.c_int64, C.c_int,
                                           _c_int32_p, _c_int32_p, _c_double_p, _c_double_p, C.c_int, _c_int32_p, C.c_double,
                                           C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "figh_difference_quotients": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int64]),
    "figh_singular_values_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                             C.c_void_p]),
    "figh_kinematic_regressor": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, _c_double_p, C.c_int,
                                           _c_double_p, _c_int32_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p]),
    "figh_calib_fkm_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int, _c_int32_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _c_double_p, C.c_int, _c_double_p,
                                       C.c_int, C.c_void_p, C.c_int64]),
    "figh_gather_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "figh_design_gram": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, _c_double_p]),
    "figh_design_scores": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, _c_double_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "figh_comm_available": (C.c_int, []),
    "figh_comm_unique_id": (C.c_int, [C.c_void_p]),
    "figh_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "figh_comm_destroy": (C.c_int, []),
    "figh_comm_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "figh_comm_allreduce_sum": (C.c_int, [C.c_void_p, C.c_int64]),
}


class FighError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libfigh error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load():
    """Load libfigh.so (built by ``__graft_entry__.build()`` / ``make -C figaroh_plus_amd/csrc``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libfigh.so not found at %s -- build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        have = lib.figh_version()
        if have != ABI_VERSION:
            raise ImportError("%s implements ABI %d, this package is written against %d (include/figh.h FIGH_ABI_VERSION): "
                              "rebuild it (make -C figaroh_plus_amd/csrc)" % (LIB_PATH, have, ABI_VERSION))
        _lib = lib
    return _lib


def check(rc):
    if rc != FIGH_OK:
        msg = load().figh_last_error()
        raise FighError(rc, msg.decode() if msg else "")
    return rc


def device_count():
    n = C.c_int(0)
    check(load().figh_device_count(C.byref(n)))
    return n.value


def device_info():
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    mem = C.c_size_t(0)
    check(load().figh_device_info(name, 256, C.byref(cus), C.byref(mem)))
    return {"name": name.value.decode(), "cu_count": cus.value, "hbm_bytes": mem.value}


def synchronize():
    check(load().figh_synchronize())


class DeviceArray:
    """A float64 / int32 buffer in HBM owned by this object (hipMalloc through the C-ABI)."""

    def __init__(self, shape, dtype=np.float64):
        self.shape = (shape,) if np.isscalar(shape) else tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.size = int(np.prod(self.shape)) if len(self.shape) else 1
        self.nbytes = self.size * self.dtype.itemsize
        p = C.c_void_p()
        check(load().figh_malloc(C.byref(p), max(self.nbytes, 8)))
        self.ptr = p.value

    @classmethod
    def from_host(cls, arr, dtype=None):
        arr = np.ascontiguousarray(arr, dtype=dtype if dtype is not None else arr.dtype)
        d = cls(arr.shape, arr.dtype)
        if arr.nbytes:
            check(load().figh_memcpy_h2d(d.ptr, arr.ctypes.data, arr.nbytes))
        return d

    def to_host(self, out=None):
        if out is None:
            out = np.empty(self.shape, dtype=self.dtype)
        assert out.nbytes == self.nbytes and out.flags["C_CONTIGUOUS"]
        if self.nbytes:
            check(load().figh_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes))
        return out

    def zero_(self):
        check(load().figh_memset(self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if getattr(self, "ptr", None):
            load().figh_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_null_tol = 0.0


def tsqr_null_pivot_tol(tol):
    """Threshold of the null-pivot rule of the TSQR kernels (include/figh.h); 0 = exact zeros only.  Returns the previous one."""
    global _null_tol
    check(load().figh_tsqr_null_pivot_tol(float(tol)))
    prev, _null_tol = _null_tol, float(tol)
    return prev


class null_pivots:
    """``with null_pivots(tol_qr): ...`` -- the TSQR launches inside run with the null-pivot rule at tol_qr / 64: a column
    that is going to be classified as dependent (|R_kk| <= tol_qr, qrdecomposition.py:215-221) by a margin of 64 costs a
    norm per tile instead of a column step."""

    def __init__(self, tol_qr):  # None: leave the process-wide setting alone
        self.tol = None if tol_qr is None else max(float(tol_qr), 0.0) / 64.0

    def __enter__(self):
        self.prev = None if self.tol is None else tsqr_null_pivot_tol(self.tol)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            tsqr_null_pivot_tol(self.prev)
        return False


def profile_enable(on=True, level=2):
    """level 1: dominant kernels only (cheap, usable inside a timed region); level 2: every launch."""
    check(load().figh_profile_enable(int(level) if on else 0))


def profile_reset():
    check(load().figh_profile_reset())


def profile_get(name):
    n = C.c_int(0)
    ms = C.c_double(0.0)
    check(load().figh_profile_get(name.encode(), C.byref(n), C.byref(ms)))
    return n.value, ms.value


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class ModelHandle:
    """figh_model_t for a flattened tree (``Model.to_flat()``)."""

    def __init__(self, flat):
        n = int(flat["njoints"])
        self.njoints, self.nq, self.nv = n, int(flat["nq"]), int(flat["nv"])
        parents, jtype = _i32(flat["parents"]), _i32(flat["jtype"])
        idx_q, idx_v = _i32(flat["idx_q"]), _i32(flat["idx_v"])
        axis, placement, gravity = _f64(flat["axis"]), _f64(flat["placement"]), _f64(flat["gravity"])
        body_mask = _i32(np.asarray(flat["mass"], dtype=float) != 0.0)
        h = C.c_void_p()
        check(load().figh_model_create(
            n, parents.ctypes.data_as(_c_int32_p), jtype.ctypes.data_as(_c_int32_p),
            axis.ctypes.data_as(_c_double_p), placement.ctypes.data_as(_c_double_p),
            idx_q.ctypes.data_as(_c_int32_p), idx_v.ctypes.data_as(_c_int32_p),
            gravity.ctypes.data_as(_c_double_p), body_mask.ctypes.data_as(_c_int32_p), C.byref(h)))
        self.handle = h.value
        # the library's own criterion (figh_model_create): fixed-base serial chain of <= 8 revolute joints
        self._chain = n - 1 <= 8 and all(int(jtype[i]) == 0 and int(parents[i]) == i - 1 for i in range(1, n))

    def is_chain(self):
        """True when the joint-torque regressor of this model is built by the chain kernel (dense row tiles)."""
        return self._chain

    def set_active_rows(self, rows=None):
        """figh_model_set_active_rows: the dof indices whose row blocks regressor_build_padded stores (None: all).  Changes
        what THIS handle writes: take a private handle (``ModelHandle(model.to_flat())``), not a shared one."""
        if rows is None or len(rows) == 0:
            check(load().figh_model_set_active_rows(self.handle, None, 0))
        else:
            arr = np.ascontiguousarray(rows, dtype=np.int32)
            check(load().figh_model_set_active_rows(self.handle, arr.ctypes.data_as(_c_int32_p), len(arr)))

    def shape(self, mode, flags):
        r, c = C.c_int(0), C.c_int(0)
        check(load().figh_regressor_shape(self.handle, mode, flags, C.byref(r), C.byref(c)))
        return r.value, c.value

    def destroy(self):
        if getattr(self, "handle", None):
            load().figh_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ------------------------------------------------------------------ thin typed wrappers (device pointers)
def regressor_build(model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_W, ldw, d_colsq=None):
    check(load().figh_regressor_build(model.handle, mode, flags, ft_mask, N, d_q.ptr, d_v.ptr, d_a.ptr, d_W.ptr, ldw,
                                      d_colsq.ptr if d_colsq is not None else None))


def regressor_build_padded(model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_W, ldw, d_colsq=None):
    """Link-padded W (16 columns per link) for device-resident use; ``d_W`` may be None (column norms only)."""
    check(load().figh_regressor_build_padded(model.handle, mode, flags, ft_mask, N, d_q.ptr, d_v.ptr, d_a.ptr,
                                             d_W.ptr if d_W is not None else None, ldw,
                                             d_colsq.ptr if d_colsq is not None else None))


APPLY_WAVES_PER_CU = 8  # csrc/figh_dynamics.hip kDynWavesPerCu


def regressor_apply_waves(N):
    """Waves (one per workgroup) of a figh_regressor_apply launch over N samples: one per tile of 64 samples, at most
    APPLY_WAVES_PER_CU per compute unit, each looping over the tiles (the launch rule of csrc/figh_dynamics.hip)."""
    return max(1, min((int(N) + 63) // 64, APPLY_WAVES_PER_CU * device_info()["cu_count"]))


def regressor_apply(model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_phi, d_tau):
    """d_tau = W(q, v, a) . phi without W (figh_regressor_apply).  Returns False -- nothing launched, d_tau untouched -- when
    the library does not serve (model, mode, flags); raises on any other error."""
    rc = load().figh_regressor_apply(model.handle if model is not None else None, mode, flags, ft_mask, N, d_q.ptr, d_v.ptr,
                                     d_a.ptr, d_phi.ptr, d_tau.ptr)
    if rc == ERR_UNSUPPORTED:
        return False
    check(rc)
    return True


def coupling_tx40(N, nv, d_v, d_a, d_out):
    check(load().figh_coupling_tx40(N, nv, d_v.ptr, d_a.ptr, d_out.ptr))


def colsq(d_W, rows, cols, ldw, d_out):
    check(load().figh_colsq(d_W.ptr, rows, cols, ldw, d_out.ptr))


def gather_cols(d_W, rows, ldw, d_idx, n, d_out, ldo):
    check(load().figh_gather_cols(d_W.ptr, rows, ldw, d_idx.ptr, n, d_out.ptr, ldo))


def place_block(src_ptr, ld_src, rows, cols, scale, dst_ptr, ld_dst):
    """Raw device addresses (``DeviceArray.ptr`` + a byte offset): the blocks are sub-matrices."""
    check(load().figh_place_block(src_ptr, ld_src, rows, cols, scale, dst_ptr, ld_dst))


def matvec(d_W, rows, ldw, d_idx, n, d_x, d_y):
    check(load().figh_matvec(d_W.ptr, rows, ldw, d_idx.ptr if d_idx is not None else None, n, d_x.ptr, d_y.ptr))


def block_sqnorm(d_a, d_b, rows, nblocks, d_out):
    check(load().figh_block_sqnorm(d_a.ptr, d_b.ptr if d_b is not None else None, rows, nblocks, d_out.ptr))


def tsqr(d_W, rows, ldw, d_idx, n, d_tau, block_weight, d_R, first_cols=None):
    """``first_cols``: structure hint (figh_tsqr_structured): per row block, the first gathered column that can be
    non-zero."""
    bw = None
    nb = 0
    if block_weight is not None:
        bwa = _f64(block_weight)
        bw = bwa.ctypes.data_as(_c_double_p)
        nb = len(bwa)
    if first_cols is not None:
        fc = _i32(first_cols)
        check(load().figh_tsqr_structured(d_W.ptr, rows, ldw, d_idx.ptr if d_idx is not None else None, n,
                                          d_tau.ptr if d_tau is not None else None, bw, nb,
                                          fc.ctypes.data_as(_c_int32_p), len(fc), d_R.ptr))
        return
    check(load().figh_tsqr(d_W.ptr, rows, ldw, d_idx.ptr if d_idx is not None else None, n,
                           d_tau.ptr if d_tau is not None else None, bw, nb, d_R.ptr))


def regressor_colsq(model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_colsq, chunk_samples=0):
    check(load().figh_regressor_colsq(model.handle, mode, flags, ft_mask, N, d_q.ptr, d_v.ptr, d_a.ptr, chunk_samples,
                                      d_colsq.ptr))


def regressor_tsqr(model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_idx, n, d_tau, block_weight, d_R, chunk_samples=0,
                   d_colsq=None):
    """``d_colsq`` (ncols doubles): also diag(W^T W) of all columns from the same pass (figh_regressor_tsqr_norms)."""
    bw, nb = None, 0
    if block_weight is not None:
        bwa = _f64(block_weight)
        bw, nb = bwa.ctypes.data_as(_c_double_p), len(bwa)
    args = (model.handle, mode, flags, ft_mask, N, d_q.ptr, d_v.ptr, d_a.ptr, d_idx.ptr if d_idx is not None else None, n,
            d_tau.ptr if d_tau is not None else None, bw, nb, chunk_samples, d_R.ptr)
    if d_colsq is not None:
        check(load().figh_regressor_tsqr_norms(*args, d_colsq.ptr))
    else:
        check(load().figh_regressor_tsqr(*args))


class PinnedArray:
    """float64 vector in page-locked host memory (figh_host_alloc); ``.array`` is a NumPy view, valid until ``free``."""

    def __init__(self, n):
        self._ptr = C.c_void_p()
        check(load().figh_host_alloc(C.byref(self._ptr), 8 * int(n)))
        self.size = int(n)
        self.array = np.ctypeslib.as_array(C.cast(self._ptr, C.POINTER(C.c_double)), shape=(self.size,))

    def free(self):
        if self._ptr:
            self.array = None
            check(load().figh_host_free(self._ptr))
            self._ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def regressor_tsqr_batch(model, mode, flags, ft_mask, B, n_per, d_q, d_v, d_a, d_idx, n, d_R_stack, d_R):
    """B trajectories of n_per samples (back to back in d_q, d_v, d_a) -> B n x n triangles in d_R."""
    check(load().figh_regressor_tsqr_batch(model.handle, mode, flags, ft_mask, B, n_per, d_q.ptr, d_v.ptr, d_a.ptr,
                                           d_idx.ptr if d_idx is not None else None, n,
                                           d_R_stack.ptr if d_R_stack is not None else None, d_R.ptr))


def regressor_tsqr_batch_fused(model, flags, B, n_per, d_q, d_v, d_a, d_idx, n, d_R_stack, d_R):
    """regressor_tsqr_batch in one W-free launch + the merge levels (serial chains in joint-torque mode, figh.h).  Returns
    False -- nothing launched -- when the shape is not supported; raises on any other error."""
    rc = load().figh_regressor_tsqr_batch_fused(model.handle, flags, B, n_per, d_q.ptr, d_v.ptr, d_a.ptr, d_idx.ptr, n,
                                                d_R_stack.ptr if d_R_stack is not None else None, d_R.ptr)
    if rc == ERR_UNSUPPORTED:
        return False
    check(rc)
    return True


def regressor_gram(model, mode, flags, ft_mask, N, d_q, d_v, d_a, d_idx, n, d_tau=None, chunk_samples=0):
    """(G, g, tau_sq): W_e^T W_e, W_e^T tau, tau^T tau (g, tau_sq None without tau)."""
    G = np.empty((n, n))
    g = np.empty(n) if d_tau is not None else None
    tt = C.c_double(0.0)
    check(load().figh_regressor_gram(model.handle, mode, flags, ft_mask, N, d_q.ptr, d_v.ptr, d_a.ptr,
                                     d_idx.ptr if d_idx is not None else None, n,
                                     d_tau.ptr if d_tau is not None else None, chunk_samples,
                                     G.ctypes.data_as(_c_double_p),
                                     g.ctypes.data_as(_c_double_p) if g is not None else None,
                                     C.byref(tt) if d_tau is not None else None))
    return G, g, (tt.value if d_tau is not None else None)


def filtfilt_cols(d_X, rows, cols, ldx, nblocks, form, b, a, zi, padlen, q, d_Y, ldy):
    """Zero-phase filter + keep every q-th sample of every (row block, column) sequence; returns the output rows."""
    b, a, zi = _f64(b), _f64(a), _f64(zi)
    nsec = b.shape[0] if form == 0 else 1
    order = 2 if form == 0 else b.size - 1
    out = C.c_int64(0)
    check(load().figh_filtfilt_cols(d_X.ptr, rows, cols, ldx, nblocks, form, b.ctypes.data_as(_c_double_p),
                                    a.ctypes.data_as(_c_double_p), nsec, order, zi.ctypes.data_as(_c_double_p), padlen, q,
                                    d_Y.ptr, ldy, C.byref(out)))
    return out.value


def medfilt_cols(X_ptr, rows, cols, ldx, nblocks, kernel_size, Y_ptr, ldy):
    """scipy.signal.medfilt of every (row block, column) sequence (figh_medfilt_cols), on raw device addresses."""
    check(load().figh_medfilt_cols(X_ptr, rows, cols, ldx, nblocks, kernel_size, Y_ptr, ldy))


def joint_difference_tile(nq, nv):
    """Sample pairs per LDS tile of figh_joint_difference (the rule of csrc/figh_differentiate.hip difference_tile)."""
    per_row = 8 * ((nq | 1) + (nv | 1))
    return 64 * min(4, (65536 - 8 * (nq | 1)) // (64 * per_row))


def joint_difference(model, N, q_ptr, ts, dt_ptr, dq_ptr):
    """dq[i] = difference(model, q[i], q[i + 1]) / (dt[i] or ts), i < N - 1 (figh_joint_difference); ``dt_ptr`` None or the
    address of N - 1 doubles."""
    check(load().figh_joint_difference(model.handle, N, q_ptr, float(ts), dt_ptr, dq_ptr))


def gradient_cols(F_ptr, rows, cols, ld, ncols_active, h, h_ptr, G_ptr, ldg):
    """np.gradient(F[:, c], edge_order=1) / (h_ptr[row] or h) for c < ncols_active, +0.0 behind (figh_gradient_cols)."""
    check(load().figh_gradient_cols(F_ptr, rows, cols, ld, ncols_active, float(h), h_ptr, G_ptr, ldg))


WRENCH_LAYOUTS = {"sample": 0, "stacked": 1}  # include/figh.h FIGH_WRENCH_SAMPLE / FIGH_WRENCH_STACKED


def quat_log(quat_ptr, N, ld_quat, rotvec_ptr, ld_rotvec):
    """rotvec[i] = log3 of the quaternion (x y z w) at quat_ptr + 8 i ld_quat (figh_quat_log), on raw device addresses."""
    check(load().figh_quat_log(quat_ptr, N, ld_quat, rotvec_ptr, ld_rotvec))


def rotvec_to_quat(rotvec_ptr, N, ld_rotvec, ref_ptr, ld_ref, out_ptr, ld_out):
    """out[i] = +-quaternion of exp3(rotvec[i]), the sign chosen against ref[i] (figh_rotvec_to_quat); ``out_ptr`` may be
    ``ref_ptr`` with the same leading dimension."""
    check(load().figh_rotvec_to_quat(rotvec_ptr, N, ld_rotvec, ref_ptr, ld_ref, out_ptr, ld_out))


def wrench_transport(model, joint, N, q_ptr, ldq, F_ptr, layout_in, inverse, out_ptr, layout_out):
    """N wrenches through oMi[joint](q_i) (figh_wrench_transport); the layouts are keys of WRENCH_LAYOUTS."""
    check(load().figh_wrench_transport(model.handle, int(joint), N, q_ptr, ldq, F_ptr, WRENCH_LAYOUTS[layout_in],
                                       1 if inverse else 0, out_ptr, WRENCH_LAYOUTS[layout_out]))


def spline_sample(model, B, n_wps, n_per, freq, act_idxq, act_idxv, tps, d_wps, d_vel_wps, vel_stride, d_acc_wps, acc_stride,
                  d_q0, q_ptr, ldq, v_ptr, a_ptr, ldv):
    """B waypoint sets -> full-configuration samples back to back (figh_spline_sample); the outputs are raw device addresses
    (windows of padded buffers), ``vel_stride`` / ``acc_stride`` 0 for one set of velocity / acceleration waypoints."""
    iq, iv, tps = _i32(act_idxq), _i32(act_idxv), _f64(tps).reshape(-1)
    if len(tps) != n_wps or len(iv) != len(iq) or d_wps.size < B * len(iq) * n_wps or d_q0.size < model.nq:
        raise ValueError("spline_sample: %d time points, %d / %d active indices and %d waypoint entries for B = %d, n_wps = %d"
                         % (len(tps), len(iq), len(iv), d_wps.size, B, n_wps))
    for d, stride in ((d_vel_wps, vel_stride), (d_acc_wps, acc_stride)):
        if d.size < (B - 1) * stride + len(iq) * n_wps:
            raise ValueError("spline_sample: a velocity / acceleration waypoint buffer is shorter than its stride asks for")
    check(load().figh_spline_sample(model.handle, B, n_wps, len(iq), n_per, float(freq), iq.ctypes.data_as(_c_int32_p),
                                    iv.ctypes.data_as(_c_int32_p), tps.ctypes.data_as(_c_double_p), d_wps.ptr, d_vel_wps.ptr,
                                    vel_stride, d_acc_wps.ptr, acc_stride, d_q0.ptr, q_ptr, ldq, v_ptr, a_ptr, ldv))


def excitation_constraints(model, B, n_per, act_idxq, act_idxv, idx_waypoints, q_ptr, ldq, v_ptr, ldv, d_tau, out_ptr, ld_out):
    """Row b of out = concatenate((q_wp, v_act, tau_act), axis=None) of trajectory b (figh_excitation_constraints)."""
    iq, iv, iw = _i32(act_idxq), _i32(act_idxv), _i32(idx_waypoints).reshape(-1)
    if len(iv) != len(iq) or d_tau.size < model.nv * B * n_per:
        raise ValueError("excitation_constraints: %d / %d active indices, tau of %d entries for %d x %d samples of %d efforts"
                         % (len(iq), len(iv), d_tau.size, B, n_per, model.nv))
    check(load().figh_excitation_constraints(model.handle, B, n_per, len(iq), iq.ctypes.data_as(_c_int32_p),
                                             iv.ctypes.data_as(_c_int32_p), len(iw), iw.ctypes.data_as(_c_int32_p), q_ptr, ldq,
                                             v_ptr, ldv, d_tau.ptr, out_ptr, ld_out))


def _ptr(x):
    return x.ptr if hasattr(x, "ptr") else x


def collision_distances(model, B, n_per, idx, q_ptr, ldq, kind, parent, placement, dims, pairs, tol, max_iter, out_ptr, ld_b,
                        witness_ptr=None, status_ptr=None):
    """figh_collision_distances on raw device addresses: out[b ld_b + i n_pairs + p] for the samples ``idx`` (None: every
    sample) of B trajectories of n_per configurations; the geometry table and the pair list are host arrays (figh.h)."""
    kind, parent, pairs = _i32(kind).reshape(-1), _i32(parent).reshape(-1), _i32(pairs).reshape(-1)
    placement, dims = _f64(placement).reshape(-1), _f64(dims).reshape(-1)
    n_geom = len(kind)
    if len(parent) != n_geom or len(placement) != 12 * n_geom or len(dims) != 3 * n_geom or len(pairs) % 2:
        raise ValueError("collision_distances: %d kinds, %d parents, %d placement and %d dimension entries, %d pair entries"
                         % (n_geom, len(parent), len(placement), len(dims), len(pairs)))
    iw = _i32(idx).reshape(-1) if idx is not None else None
    check(load().figh_collision_distances(model.handle if model is not None else None, B, n_per,
                                          len(iw) if iw is not None else 0,
                                          iw.ctypes.data_as(_c_int32_p) if iw is not None else None, _ptr(q_ptr), ldq, n_geom,
                                          kind.ctypes.data_as(_c_int32_p), parent.ctypes.data_as(_c_int32_p),
                                          placement.ctypes.data_as(_c_double_p), dims.ctypes.data_as(_c_double_p),
                                          len(pairs) // 2, pairs.ctypes.data_as(_c_int32_p), float(tol), int(max_iter),
                                          _ptr(out_ptr), ld_b, _ptr(witness_ptr), _ptr(status_ptr)))


def difference_quotients(C_ptr, ldc, n_con, n_var, scheme, dx_ptr, J_ptr, ldj):
    """figh_difference_quotients on raw device addresses: J[i, j] = (C[1 + j, i] - C[0 or 1 + n_var + j, i]) / dx[j]."""
    check(load().figh_difference_quotients(_ptr(C_ptr), ldc, n_con, n_var, scheme, _ptr(dx_ptr), _ptr(J_ptr), ldj))


SINGULAR_VALUES_MAX_R = 128  # csrc/figh_singular.hip kMaxR: above it figh_singular_values_batch answers ERR_UNSUPPORTED
SINGULAR_VALUES_WGS_PER_CU = 8  # csrc/figh_singular.hip kMaxWgsPerCu: its grid has at most that many workgroups per CU


def singular_values_batch(R_ptr, B, r, stride, max_sweeps, sigma_ptr, ld_sigma, status_ptr):
    """figh_singular_values_batch on raw device addresses: sigma[b, :r] unordered, status[b] = (sweeps, converged)."""
    check(load().figh_singular_values_batch(_ptr(R_ptr), B, r, stride, max_sweeps, _ptr(sigma_ptr), ld_sigma,
                                            _ptr(status_ptr)))


def kinematic_regressor(model, N, q_ptr, ldq, end_joint, end_placement, start_joint, start_placement, support, meas_mask,
                        R_ptr, ldr, J_ptr, ldj, rowsq_R_ptr=None, rowsq_J_ptr=None):
    """figh_kinematic_regressor on raw device addresses: the measured row blocks of the kinematic regressor R and / or of
    the frame Jacobian J (either may be None), and their rows' sums of squares.  Placements are 12 doubles (R, p)."""
    ep = _f64(end_placement).reshape(-1)
    sp = _f64(start_placement).reshape(-1) if start_placement is not None else None
    sup = _i32(support).reshape(-1)
    if ep.size != 12 or (sp is not None and sp.size != 12):
        raise ValueError("kinematic_regressor: a placement is 12 doubles (rotation row-major, translation)")
    check(load().figh_kinematic_regressor(model.handle, N, _ptr(q_ptr), ldq, int(end_joint), ep.ctypes.data_as(_c_double_p),
                                          int(start_joint), sp.ctypes.data_as(_c_double_p) if sp is not None else None,
                                          sup.ctypes.data_as(_c_int32_p), len(sup), int(meas_mask), _ptr(R_ptr), ldr,
                                          _ptr(J_ptr), ldj, _ptr(rowsq_R_ptr), _ptr(rowsq_J_ptr)))


def calib_fkm_batch(model, B, N, q_ptr, ldq, chain, d_placements, d_wMo, d_eeMf, end_joint, end_placement, start_joint,
                    start_placement, meas_mask, out_ptr, ld_out):
    """figh_calib_fkm_batch: the measured pose components of B parameter vectors x N poses, out[b ld_out + k N + i]."""
    ep = _f64(end_placement).reshape(-1)
    sp = _f64(start_placement).reshape(-1) if start_placement is not None else None
    ch = _i32(chain).reshape(-1)
    if ep.size != 12 or (sp is not None and sp.size != 12):
        raise ValueError("calib_fkm_batch: a placement is 12 doubles (rotation row-major, translation)")
    if d_placements.size < B * len(ch) * 12 or d_wMo.size < 12 * B or d_eeMf.size < 12 * B:
        raise ValueError("calib_fkm_batch: placements / wMo / eeMf hold fewer than B x n_chain x 12 / B x 12 doubles")
    check(load().figh_calib_fkm_batch(model.handle, B, N, _ptr(q_ptr), ldq, len(ch), ch.ctypes.data_as(_c_int32_p),
                                      d_placements.ptr, d_wMo.ptr, d_eeMf.ptr, int(end_joint),
                                      ep.ctypes.data_as(_c_double_p), int(start_joint),
                                      sp.ctypes.data_as(_c_double_p) if sp is not None else None, int(meas_mask),
                                      _ptr(out_ptr), ld_out))


def gather_rows(W_ptr, ldw, cols, d_idx, n, out_ptr, ld_out):
    """figh_gather_rows: out[r, :] = W[idx[r], :], order kept (d_idx: int32 DeviceArray of at least n entries)."""
    if d_idx.size < n:
        raise ValueError("gather_rows: %d indices for n = %d" % (d_idx.size, n))
    check(load().figh_gather_rows(_ptr(W_ptr), ldw, cols, d_idx.ptr, n, _ptr(out_ptr), ld_out))


def design_gram(R_ptr, ldr, N, c, n, w_ptr=None):
    """figh_design_gram: M = sum_i w_i sum_k r_{k,i} r_{k,i}^T over the resident pool, as an (n, n) host array (w_ptr: N
    device doubles, None = all ones)."""
    M = np.empty((max(int(n), 0), max(int(n), 0)))
    check(load().figh_design_gram(_ptr(R_ptr), ldr, N, c, n, _ptr(w_ptr), M.ctypes.data_as(_c_double_p)))
    return M


def design_scores(R_ptr, ldr, N, c, n, L, trace_ptr, det_add_ptr, det_rm_ptr):
    """figh_design_scores: tr G_i, det(I + G_i), det(I - G_i) of G_i = R_i M^-1 R_i^T for every candidate, from the host
    Cholesky factor L of M (n x n, lower triangle read); each output (N device doubles) may be None, not all three."""
    L = _f64(L)
    if L.shape != (n, n):
        raise ValueError("design_scores: L is %r, expected (%d, %d)" % (L.shape, n, n))
    check(load().figh_design_scores(_ptr(R_ptr), ldr, N, c, n, L.ctypes.data_as(_c_double_p), _ptr(trace_ptr),
                                    _ptr(det_add_ptr), _ptr(det_rm_ptr)))


def compact_rows(W_ptr, rows, cols, ldw, tau_ptr, key_col, threshold, Wout_ptr, ld_out, tauout_ptr):
    """figh_compact_rows on raw device addresses (views into larger buffers); returns the number of kept rows."""
    out = C.c_int64(0)
    check(load().figh_compact_rows(W_ptr, rows, cols, ldw, tau_ptr, key_col, threshold, Wout_ptr, ld_out, tauout_ptr,
                                   C.byref(out)))
    return out.value


def base_permutation(d_R, nc, n, tol_qr, d_perm):
    check(load().figh_base_permutation(d_R.ptr, nc, n, tol_qr, d_perm.ptr))


def tsqr_merge(d_Rs, count, nc, d_R):
    check(load().figh_tsqr_merge(d_Rs.ptr, count, nc, d_R.ptr))


def select_columns(d_colsq, ncols, tol_e, link_stride, d_sel):
    check(load().figh_select_columns(d_colsq.ptr, ncols, tol_e, link_stride, d_sel.ptr))


def tsqr_selected(d_W, rows, ldw, d_colsq, ncols, tol_e, link_stride, nblocks, n_expected, d_tau, tol_qr, d_sel, d_R):
    """Elimination + TSQR of the kept columns back to back on the device (``n_expected`` <= 0: selection only);
    ``tol_qr`` >= 0 folds the rank decision and the regrouped factorisation into the last merge level (figh.h)."""
    check(load().figh_tsqr_selected(d_W.ptr, rows, ldw, d_colsq.ptr, ncols, tol_e, link_stride, nblocks, n_expected,
                                    d_tau.ptr if d_tau is not None else None, tol_qr, d_sel.ptr,
                                    d_R.ptr if d_R is not None else None))


def tsqr_selected_wrench(d_W, rows, ldw, d_colsq, ncols, tol_e, link_stride, n_expected, nf_expected, d_tau, tol_qr, d_sel,
                         d_R, d_link_pos=None, ld_force=0):
    """tsqr_selected for the external-wrench regressor of a free-flyer model: force rows over the ``nf_expected`` kept
    columns that can be non-zero there, torque rows chained onto their triangle (figh.h).  ``d_link_pos``: the device copy
    of :func:`regressor_link_layout`'s map when W is link-compact."""
    check(load().figh_tsqr_selected_wrench(d_W.ptr, rows, ldw, d_colsq.ptr, ncols, tol_e, link_stride, n_expected,
                                           nf_expected, d_tau.ptr if d_tau is not None else None, tol_qr, d_sel.ptr,
                                           d_R.ptr if d_R is not None else None,
                                           d_link_pos.ptr if d_link_pos is not None else None, int(ld_force)))


def regressor_force_layout(model, mode, flags, ft_mask):
    """Leading dimension of the force region of the force-compact layout (FLAG_FORCE_COMPACT, figh.h), 0 when it does not
    apply."""
    ldf = C.c_int64(0)
    rc = load().figh_regressor_force_layout(model.handle, mode, flags, ft_mask, C.byref(ldf))
    if rc == ERR_UNSUPPORTED:
        return 0
    check(rc)
    return int(ldf.value)


def regressor_link_layout(model, mode, flags, ft_mask):
    """(link_pos, nlive) of the link-compact layout (FLAG_LINK_COMPACT, figh.h) or None when it does not apply."""
    nlinks = model.njoints - 1
    pos = np.zeros(nlinks, dtype=np.int32)
    nlive = C.c_int(0)
    rc = load().figh_regressor_link_layout(model.handle, mode, flags, ft_mask, pos.ctypes.data_as(_c_int32_p), C.byref(nlive))
    if rc == ERR_UNSUPPORTED:
        return None
    check(rc)
    return pos, int(nlive.value)


def tsqr_selected_blocks(d_W, rows, ldw, d_colsq, ncols, tol_e, link_stride, n_expected, counts, d_cols, d_pos, d_tau,
                         tol_qr, d_sel, d_R, block_off=None, block_ld=None, d_block_tri=None):
    """tsqr_selected with one column list per row block (joint-torque regressor of a tree, figh.h); ``counts``: int32
    host array, one entry per row block; ``block_off`` / ``block_ld``: the block-compact W (element offsets, int64, and
    leading dimensions, int32, per row block); ``d_block_tri`` (optional) receives the compact stack of the embedded
    per-row-block triangles (figh.h)."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    off = ld = None
    if block_off is not None:
        off = np.ascontiguousarray(block_off, dtype=np.int64)
        ld = np.ascontiguousarray(block_ld, dtype=np.int32)
    check(load().figh_tsqr_selected_blocks(d_W.ptr, rows, ldw, d_colsq.ptr, ncols, tol_e, link_stride, n_expected,
                                           len(counts), counts.ctypes.data, d_cols.ptr, d_pos.ptr,
                                           off.ctypes.data if off is not None else None,
                                           ld.ctypes.data if ld is not None else None,
                                           d_tau.ptr if d_tau is not None else None, tol_qr, d_sel.ptr, d_R.ptr,
                                           d_block_tri.ptr if d_block_tri is not None else None))


def block_rows_residuals(d_rows, row_off, nc, d_v, d_r2):
    """d_r2[b] = sum over rows [row_off[b], row_off[b+1]) of (row . v)^2 (figh.h); ``row_off``: nblocks + 1 ints."""
    ro = _i32(row_off)
    check(load().figh_block_rows_residuals(d_rows.ptr, len(ro) - 1, ro.ctypes.data_as(_c_int32_p), nc, d_v.ptr, d_r2.ptr))


def regressor_tsqr_fused(model, flags, N, d_q, d_v, d_a, d_W, ldw, d_colsq, d_kept, n, d_tau, tol_qr, d_R):
    """K1 + level-0 TSQR over the caller's kept-column list in one launch (serial chains, figh.h).  Returns False -- nothing
    launched -- when the shape is not supported; raises on any other error."""
    rc = load().figh_regressor_tsqr_fused(model.handle, flags, N, d_q.ptr, d_v.ptr, d_a.ptr, d_W.ptr, ldw, d_colsq.ptr,
                                          d_kept.ptr, n, d_tau.ptr if d_tau is not None else None, tol_qr, d_R.ptr)
    if rc == ERR_UNSUPPORTED:
        return False
    check(rc)
    return True


TAIL_OK, TAIL_SINGULAR = 0, 1


class _HostTailStruct(C.Structure):
    """figh_host_tail_t of include/figh.h"""
    _fields_ = [("rows_k", C.c_void_p), ("n", C.c_int32), ("with_tau", C.c_int32), ("tol_qr", C.c_double),
                ("total_rows", C.c_int64), ("pieces", C.c_int64), ("null_rule", C.c_int32), ("n_cached_base", C.c_int32),
                ("cached_base", C.c_void_p), ("bounds", C.c_void_p), ("idx", C.c_void_p), ("absdiag", C.c_void_p),
                ("beta", C.c_void_p), ("phi_ls", C.c_void_p), ("phi_b", C.c_void_p), ("residual_norm", C.c_double),
                ("n_base", C.c_int32), ("status", C.c_int32), ("certified", C.c_int32), ("bounds_recomputed", C.c_int32)]


class HostTail:
    """The argument block of figh_chain_host_tail / figh_chain_pass_fused for problems of ``n`` columns (+ tau) with the
    output arrays it points to, allocated once and overwritten by every call: copy what is to outlive the next one.
    ``cache_of`` is whatever object the caller ties the validity of ``bounds`` / ``cached_base`` to (the pipeline: its
    ``_cert_cache`` tuple)."""

    def __init__(self, n, with_tau):
        self.n, self.with_tau = int(n), bool(with_tau)
        self.idx = np.zeros(self.n, dtype=np.int32)
        self.cached_base = np.zeros(self.n, dtype=np.int32)
        self.absdiag, self.phi_ls, self.phi_b = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        self.beta = np.zeros(self.n * self.n)
        self.bounds = np.zeros(self.n + 2)
        self.cache_of = None
        s = self.s = _HostTailStruct()
        s.n, s.with_tau, s.n_cached_base = self.n, int(self.with_tau), -1
        for name in ("cached_base", "bounds", "idx", "absdiag", "beta", "phi_ls", "phi_b"):
            setattr(s, name, getattr(self, name).ctypes.data)
        self.ref = C.addressof(s)

    def keep_bounds(self, owner):
        """The bounds just computed belong to this call's base columns and stay valid while ``cache_of is owner``."""
        r = self.s.n_base
        self.cached_base[:r] = self.idx[:r]
        self.s.n_cached_base = r
        self.cache_of = owner

    def bounds_tuple(self):
        """(A_base, A_dep, |R1^-1|_inf) as _host.null_rule_bounds returns them, None when they are not valid."""
        if self.bounds[self.n + 1] == 0.0:
            return None
        r = self.s.n_base
        return self.bounds[:r].copy(), self.bounds[r:self.n].copy(), float(self.bounds[self.n])


def chain_host_tail(tail, rows_k):
    """figh_chain_host_tail on ``rows_k`` ((nc + 1) x nc, C-contiguous float64): results in ``tail``'s arrays and ``tail.s``."""
    tail.s.rows_k = rows_k.ctypes.data
    check(load().figh_chain_host_tail(tail.ref))


def chain_pass_fused(model, flags, N, d_q, d_v, d_a, d_W, ldw, d_kept, n, d_tau, tol_qr, tol_e, d_pack, h_pack, pack_bytes,
                     kept_mask_u8, tail):
    """One fused pass in one call (figh.h): None when the shape does not fuse (nothing launched), False when the device
    selected other columns than ``kept_mask_u8`` (the pack is on the host, the tail was not run), True with the results in
    ``tail``."""
    changed = C.c_int(0)
    rc = load().figh_chain_pass_fused(model.handle, flags, N, d_q.ptr, d_v.ptr, d_a.ptr, d_W.ptr, ldw, d_kept.ptr, n,
                                      d_tau.ptr if d_tau is not None else None, tol_qr, tol_e, d_pack.ptr, h_pack, pack_bytes,
                                      kept_mask_u8.ctypes.data, C.byref(changed), tail.ref)
    if rc == ERR_UNSUPPORTED:
        return None
    check(rc)
    return not changed.value


def tsqr_merge_base(d_Rs, count, nc, n_free, tol_qr, d_Rk):
    check(load().figh_tsqr_merge_base(d_Rs.ptr, count, nc, n_free, tol_qr, d_Rk.ptr))


def tsqr_merge_base_norms(d_Rs, count, nc, n_free, tol_qr, d_part, nblocks, ncols, tol_e, d_colsq, d_sel, d_Rk):
    """tsqr_merge_base + the sum of the norm partials + select_columns, in one launch where the merge tree allows it."""
    check(load().figh_tsqr_merge_base_norms(d_Rs.ptr, count, nc, n_free, tol_qr, d_part.ptr, nblocks, ncols, tol_e,
                                            d_colsq.ptr, d_sel.ptr, d_Rk.ptr))


def repack_samples(d_src, N, width):
    """Tile-blocked copy of a sample-major N x width device array (figh_repack_samples): a new DeviceArray."""
    d_dst = DeviceArray((((N + 63) // 64) * 64 * width,), np.float64)
    check(load().figh_repack_samples(d_src.ptr, N, width, d_dst.ptr))
    return d_dst
