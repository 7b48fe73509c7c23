"""ctypes binding of librl_mincurv.so (include/rl_mincurv.h).

The HIP library is the product; there is no CPU fallback anywhere in this package.  If the shared
object is missing, or no MI355X/HIP device is usable, every compute entry point raises.
"""
import contextlib
import ctypes
import os
import threading

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RL_LIB_PATH") or os.path.join(_PKG, "librl_mincurv.so")  # RL_LIB_PATH: dev hook for A/B builds

NCOL = 19
WEIGHT_MIN, WEIGHT_MAX = 2.0 ** -30, 2.0 ** 30   # include/rl_mincurv.h: the allowed weights of the weighted entries
MAX_ITER = 32
BOUNDS_SHARED_RINGS, BOUNDS_WIDTHS, BOUNDS_POINTS = 0, 1, 2
SEARCH_BRUTE, SEARCH_CULLED, SEARCH_WINDOWED = 0, 1, 2
POSE_FRENET, POSE_GLOBAL = 0, 1   # include/rl_mincurv.h: RL_POSE_*
ARITH_DEFAULT, ARITH_FAST, ARITH_REFERENCE, ARITH_BRANCH = -1, 0, 1, 2   # include/rl_mincurv.h: RL_ARITH_*

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_vp = ctypes.c_void_p


class Stats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_float), ("lds_bytes", ctypes.c_int),
                ("block_threads", ctypes.c_int), ("rings_in_lds", ctypes.c_int),
                ("reserved", ctypes.c_int * 4)]


class RlError(RuntimeError):
    pass


_i, _d = ctypes.c_int, ctypes.c_double
_st = ctypes.POINTER(Stats)
_D, _I = object(), object()   # an argument in the entry's memory space: double* / int* of a _host entry, void* of its _dev twin


def _host(args):
    return _i, [_dp if a is _D else _ip if a is _I else a for a in args]


def _dev(args):
    return _i, [_vp if a is _D or a is _I else a for a in args]


# the argument list of each _host / _dev pair, once; plain _dp / _ip is a host pointer in both (model vector, models table,
# shared i_start, region tables, the QSS lookup tables of rl_qss_sim_dev)
_SOLVE_BATCH = [_vp, _vp, _i, _D, _i, _ip, _i, _i, _D, _D, _I, _I, _st]
_SOLVE_BATCH_FROM = [_vp, _vp, _i, _D, _i, _D, _I, _i, _i, _i, _D, _D, _I, _I, _st]   # and _joint_
_SPLINE_FIT = [_vp, _vp, _D, _i, _i, _i, _D, _i, _D, _D]
_DT_EVAL = [_vp, _dp, _i, _i, _dp, _dp, _dp, _dp, _d, _d, _dp, _dp, _dp, _dp, _dp, _dp]
_MINTIME_SOLVE = [_vp, _dp, _i, _i, _D, _D, _D, _D, _i, _d, _d, _d, _d, _D, _D, _D, _i, _d, _D]   # and _vehicles
_MINTIME_TRACKS = [_vp, _dp, _i, _i, _i, _i, _ip, _D, _D, _D, _D, _d, _dp, _dp, _dp, _D, _D, _D, _i, _d, _D]
_BICYCLE_SOLVE = [_vp, _dp, _i, _i, _D, _D, _D, _D, _i, _D, _D, _D, _i, _d, _D]
_BICYCLE_LINES = [_vp, _dp, _i, _i, _i, _D, _D, _i, _D, _D, _i, _D, _D, _D, _i, _d, _D]
_QSS_SIM = [_vp, _D, _i, _i, _dp, _dp, _i, _dp, _dp, _i, _dp, _I]
_QSS_SIM_VEHICLES = [_vp, _D, _i, _i, _D, _D, _i, _D, _D, _i, _D, _I]
_GLOBAL = [_vp, _vp, _D, _i, _d, _i, _D, _D, _D, _D, _st]
_GLOBAL_WEIGHTED = [_vp, _vp, _D, _D, _i, _d, _i, _D, _D, _D, _D, _st]
_GLOBAL_XY = [_vp, _vp, _D, _i, _d, _d, _i, _D, _D, _D, _D, _st]
_TABLES = [_vp, _vp, _D, _i, _i, _D, _d, _D, _i, _D]
_POSE_TABLES = [_vp, _vp, _i, _D, _i, _i, _D, _D, _D, _i, _i, _D, _D, _i, _D, _D]
_FRENET = [_vp, _D, _i, _i, _i, _D, _D, _D, _D, _i, _D, _I, _D]
_FRENET_RESAMPLE = [_vp, _D, _D, _i, _i, _i, _D, _i, _d, _D, _I]
_TABLE_SUMMARY = [_vp, _D, _i, _i, _I, _D]
_SWEEP = [_vp, _vp, _ip, _i, _dp, _dp, _dp, _ip, _st]

# every symbol include/rl_mincurv.h declares: (restype, argtypes)
_SIGNATURES = {
    "rl_version": (_i, []),
    "rl_last_error": (ctypes.c_char_p, []),
    "rl_debug_dump_enable": (_i, [_i]),
    "rl_debug_read": (_i, [_dp, ctypes.c_longlong]),
    "rl_ctx_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "rl_ctx_destroy": (None, [_vp]),
    "rl_ctx_set_stream": (_i, [_vp, _vp]),
    "rl_ctx_synchronize": (_i, [_vp]),
    "rl_ctx_set_arith": (_i, [_vp, _i]),
    "rl_ctx_get_arith": (_i, [_vp]),
    "rl_ctx_set_numpy_raise": (_i, [_vp, _i]),
    "rl_ctx_set_option": (_i, [_vp, ctypes.c_char_p, _i]),
    "rl_debug_cr_heading": (_i, [_vp, _dp, _dp, _i, _dp]),
    "rl_spline_eval": (_i, [_vp, _dp, _i, _dp, _dp, _i, _dp, _i, _i, _dp]),
    "rl_sample_along": (_i, [_vp, _dp, _i, _dp, _dp, _i, _d, _dp, _i, _dp]),
    "rl_fill_bounds": (_i, [_vp, _dp, _i, _dp, _i, _dp, _i, _d]),
    "rl_fill_region": (_i, [_vp, _dp, _i, _i, _dp, _ip, _i, _ip]),
    "rl_region_index_dev": (_i, [_vp, _vp, _i, _i, _i, _dp, _ip, _i, _vp]),
    "rl_track_create": (_i, [_vp, _dp, _i, _dp, _dp, _i, _i, ctypes.POINTER(_vp)]),
    "rl_track_destroy": (None, [_vp]),
    "rl_track_set_rings": (_i, [_vp, _dp, _i, _dp, _i]),
    "rl_track_set_control_points": (_i, [_vp, _dp, _dp]),
    "rl_track_set_length": (_i, [_vp, _d]),
    "rl_mincurv_cost": (_i, [_vp, _vp, _ip, _i, _dp, _dp, _dp, _ip]),
    "rl_mincurv_cost_weighted": (_i, [_vp, _vp, _ip, _i, _dp, _dp, _dp, _dp, _ip]),
    "rl_track_constraint": (_i, [_vp, _vp, _dp, _i, _dp, _dp, _dp, _ip]),
    "rl_mincurv_sweep": (_i, _SWEEP),
    "rl_mincurv_sweep_joint": (_i, _SWEEP),
    "rl_mincurv_solve_batch_dev": _dev(_SOLVE_BATCH),
    "rl_mincurv_solve_batch_host": _host(_SOLVE_BATCH),
    "rl_mincurv_solve_batch_from_dev": _dev(_SOLVE_BATCH_FROM),
    "rl_mincurv_solve_batch_from_host": _host(_SOLVE_BATCH_FROM),
    "rl_mincurv_solve_batch_joint_dev": _dev(_SOLVE_BATCH_FROM),
    "rl_mincurv_solve_batch_joint_host": _host(_SOLVE_BATCH_FROM),
    "rl_spline_fit_batch_dev": _dev(_SPLINE_FIT),
    "rl_spline_fit_batch_host": _host(_SPLINE_FIT),
    "rl_dt_eval_nodes": (_i, _DT_EVAL),
    "rl_dt_eval_jac": (_i, _DT_EVAL),
    "rl_mintime_solve_batch": _host(_MINTIME_SOLVE),
    "rl_mintime_solve_batch_dev": _dev(_MINTIME_SOLVE),
    "rl_mintime_solve_vehicles": _host(_MINTIME_SOLVE),
    "rl_mintime_solve_vehicles_dev": _dev(_MINTIME_SOLVE),
    "rl_mintime_solve_tracks": _host(_MINTIME_TRACKS),
    "rl_mintime_solve_tracks_dev": _dev(_MINTIME_TRACKS),
    "rl_debug_mt_rows": (_i, [_dp, _i, _i, _i, _ip, _dp, _dp, _dp, _dp]),
    "rl_bicycle_eval_nodes": (_i, [_vp, _dp, _i, _i, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "rl_bicycle_solve_batch": _host(_BICYCLE_SOLVE),
    "rl_bicycle_solve_batch_dev": _dev(_BICYCLE_SOLVE),
    "rl_bicycle_solve_lines": _host(_BICYCLE_LINES),
    "rl_bicycle_solve_lines_dev": _dev(_BICYCLE_LINES),
    "rl_bicycle_eval_nodes_lines": (_i, [_vp, _dp, _i, _i, _i, _dp, _dp, _i, _dp, _dp, _dp, _dp, _dp, _dp]),
    "rl_qss_sim_dev": _dev(_QSS_SIM),
    "rl_mincurv_global_batch_dev": _dev(_GLOBAL),
    "rl_mincurv_global_batch_host": _host(_GLOBAL),
    "rl_mincurv_global_weighted_batch_dev": _dev(_GLOBAL_WEIGHTED),
    "rl_mincurv_global_weighted_batch_host": _host(_GLOBAL_WEIGHTED),
    "rl_qss_sim": _host(_QSS_SIM),
    "rl_qss_sim_vehicles_dev": _dev(_QSS_SIM_VEHICLES),
    "rl_qss_sim_vehicles_host": _host(_QSS_SIM_VEHICLES),
    "rl_mincurv_global_xy_batch_dev": _dev(_GLOBAL_XY),
    "rl_mincurv_global_xy_batch_host": _host(_GLOBAL_XY),
    "rl_tables_batch_dev": _dev(_TABLES),
    "rl_tables_batch_host": _host(_TABLES),
    "rl_pose_tables_batch_dev": _dev(_POSE_TABLES),
    "rl_pose_tables_batch_host": _host(_POSE_TABLES),
    "rl_frenet_batch_dev": _dev(_FRENET),
    "rl_frenet_batch_host": _host(_FRENET),
    "rl_frenet_resample_dev": _dev(_FRENET_RESAMPLE),
    "rl_frenet_resample_host": _host(_FRENET_RESAMPLE),
    "rl_table_summary_dev": _dev(_TABLE_SUMMARY),
    "rl_table_summary_host": _host(_TABLE_SUMMARY),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None
_lock = threading.Lock()


def load():
    """Load librl_mincurv.so (no GPU needed just to load and resolve symbols)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RlError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        if os.environ.get("RL_NO_TORCH", "0") != "1":
            try:  # share ONE HIP runtime with torch when both live in the process
                import torch  # noqa: F401
            except Exception:
                pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc):
    if rc != 0:
        raise RlError(f"librl_mincurv error {rc}: {load().rl_last_error().decode()}")


def as_d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def as_i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


_default_device = 0


def set_default_device(device):
    """Device used by the mirror classes / ops when none is given (one process per GPU: LOCAL_RANK)."""
    global _default_device
    _default_device = int(device)


class Context:
    """rl_ctx wrapper: one per (process, device).  Raises if no HIP device is usable."""

    _cache = {}

    def __init__(self, device=0):
        self.lib = load()
        h = _vp()
        check(self.lib.rl_ctx_create(int(device), ctypes.byref(h)))
        self.h = h
        self.device = device

    @classmethod
    def get(cls, device=None):
        if device is None:
            device = _default_device
        ctx = cls._cache.get(device)
        if ctx is None:
            ctx = cls(device)
            cls._cache[device] = ctx
        return ctx

    def set_stream(self, stream_handle):
        check(self.lib.rl_ctx_set_stream(self.h, _vp(stream_handle or 0)))

    def synchronize(self):
        check(self.lib.rl_ctx_synchronize(self.h))

    def set_arith(self, arith):
        """ARITH_DEFAULT (nothing chosen: the reference-order arithmetic wherever it exists, the fast one elsewhere), ARITH_FAST,
        ARITH_REFERENCE (the reference's operations in the reference's order) or ARITH_BRANCH (include/rl_mincurv.h).
        Returns the previous setting (ARITH_DEFAULT while nothing was chosen)."""
        old = self.lib.rl_ctx_get_arith(self.h)
        check(self.lib.rl_ctx_set_arith(self.h, int(arith)))
        return old

    def set_option(self, name, value):
        """Test hooks (include/rl_mincurv.h: rl_ctx_set_option): "qss_kernel", "qss_df_waves", "qss_df_bail_at", "qss_df_redo",
        "tables_search", "tables_rings", "frenet_search", "sweep_bracket", "global_last_as_mid" (1: the last linearisation of the
        global QPs leaves at the intermediate tolerance -- it changes what the call returns; tests/global_kkt_cases.py)."""
        check(self.lib.rl_ctx_set_option(self.h, name.encode(), int(value)))

    def set_numpy_raise(self, on):
        """Reference-order sweep: np.seterr(all='raise') is already in effect when the driver starts
        (include/rl_mincurv.h: rl_ctx_set_numpy_raise)."""
        check(self.lib.rl_ctx_set_numpy_raise(self.h, 1 if on else 0))

    @contextlib.contextmanager
    def arith(self, arith):
        """with ctx.arith(ARITH_REFERENCE): ...  -- the sweep calls inside run in that arithmetic."""
        old = self.set_arith(arith)
        try:
            yield self
        finally:
            self.set_arith(old)


class Track:
    """rl_track wrapper: device tables for one (knots, degree, sample count, control points)."""

    def __init__(self, ctx, t, cx, cy, k, N):
        self.ctx = ctx
        self.t, tp = as_d(t)
        cx, xp = as_d(cx)
        cy, yp = as_d(cy)
        self.k, self.N = int(k), int(N)
        self.n = len(self.t) - self.k - 1
        assert len(cx) == self.n and len(cy) == self.n
        h = _vp()
        check(ctx.lib.rl_track_create(ctx.h, tp, len(self.t), xp, yp, self.k, self.N, ctypes.byref(h)))
        self.h = h

    def set_rings(self, ringL, ringR):
        ringL, lp = as_d(ringL)
        ringR, rp = as_d(ringR)
        check(self.ctx.lib.rl_track_set_rings(self.h, lp, len(ringL), rp, len(ringR)))

    def set_length(self, length):
        check(self.ctx.lib.rl_track_set_length(self.h, float(length)))

    def set_control_points(self, cx, cy):
        cx, xp = as_d(cx)
        cy, yp = as_d(cy)
        check(self.ctx.lib.rl_track_set_control_points(self.h, xp, yp))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.ctx.lib.rl_track_destroy(self.h)
                self.h = None
        except Exception:
            pass
