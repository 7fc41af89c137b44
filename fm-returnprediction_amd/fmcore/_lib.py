"""ctypes binding of libfm_hip.so (include/fm_hip.h).

The shared library is built in-tree (``fm-returnprediction_amd/lib/libfm_hip.so``, see
``csrc/Makefile`` / ``__graft_entry__.build()``).  There is no fallback: if the library is
missing, or no HIP device is present when a compute entry point is used, this module
raises.  All pointer arguments are device pointers taken from torch tensors.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("FM_HIP_LIB", os.path.join(_PKG_DIR, "lib", "libfm_hip.so"))

FM_ST_FITTED = 0x1
FM_ST_SKIPPED = 0x2
FM_ST_INF_IN_X = 0x4
FM_ST_INF_IN_Y = 0x8
FM_ST_CONST_SUSPECT = 0x10
FM_ST_CONST_COL = 0x20
FM_ST_RANK_DEF = 0x40
FM_ST_REFIT = 0x80
FM_ST_NEG_VAR = 0x100

FM_MAX_COLS = 31
FM_MAX_MODELS = 6
FM_MAX_LEVELS = 3
FM_MAX_PORTS = 20
FM_MAX_SORTS = 16
FM_MAX_SORT_K = 30
FM_MAX_DIST_Q = 8
FM_MAX_PAIRS = 16
FM_FCMP_NREC = 7
FM_FHOR_NREC = 6
FM_TS_FUSED_MAX_LDS = 128 * 1024
FM_RANK_AVERAGE, FM_RANK_MIN, FM_RANK_MAX = 0, 1, 2
FM_RANK_RAW, FM_RANK_PCT, FM_RANK_UNIFORM = 0, 1, 2

_p = C.c_void_p
_i32 = C.c_int32
_i64 = C.c_int64
_f64 = C.c_double


class GramArgs(C.Structure):
    _fields_ = [
        ("cols", _p), ("col_stride", _i64), ("ncols", _i32), ("nseg", _i32),
        ("seg_off", _p), ("chunk_seg", _p), ("chunk_row", _p), ("nchunks", _i32),
        ("lo", _p), ("hi", _p), ("shift", _p), ("inv_scale", _p),
        ("level", _p), ("nlevels", _i32),
        ("model_mask", _p), ("model_ymask", _p), ("nmodels", _i32),
        ("pattern_id", _p), ("npatterns", _i32),
        ("partial", _p), ("flags", _p), ("chunk_order", _p),
        ("hi_plane", _p), ("lo_plane", _p), ("plane_stride", _i64),
        ("wg_chunk_off", _p), ("nwg", _i32),
    ]


class SelectArgs(C.Structure):
    _fields_ = [
        ("cols", _p), ("col_stride", _i64), ("ncols", _i32), ("seg_off", _p), ("nseg", _i32),
        ("max_seg_len", _i32), ("row_mask", _p), ("q_lo", _f64), ("q_hi", _f64),
        ("min_count", _i32), ("lerp_mode", _i32), ("lo", _p), ("hi", _p), ("nvalid", _p),
        ("mean", _p), ("sd", _p), ("center", _p), ("level", _p), ("ws", _p),
        ("hi_plane", _p), ("plane_stride", _i64), ("lo_plane", _p),
    ]


class UniverseArgs(C.Structure):
    _fields_ = [
        ("me", _p), ("nyse", _p), ("q_a", _f64), ("q_b", _f64), ("cut_a", _p), ("cut_b", _p),
        ("level", _p),
    ]


class TsArgs(C.Structure):
    _fields_ = [
        ("rec", _p), ("r_seg", _i64), ("r_prob", _i64), ("status", _p), ("s_seg", _i64),
        ("s_prob", _i64), ("nseg", _i32), ("nprob", _i32), ("kmax", _i32), ("nw_lags", _i32),
        ("idx", _p), ("count", _p), ("mean", _p), ("se", _p), ("tstat", _p), ("nobs", _p),
        ("work", _p), ("window", _i32), ("min_periods", _i32), ("pmax", _i32), ("roll", _p),
        ("moments", _p), ("mom_stride", _i32), ("prob_k", _p), ("lag", _i32), ("seg_lo", _i32),
        ("seg_hi", _i32), ("pred", _p), ("pred_status", _p),
        # month-sharded runs: problem range of the summaries, own-rows rolling (0 = off)
        ("sum_p_lo", _i32), ("sum_p_hi", _i32), ("roll_own", _i32), ("pad_ts", _i32),
    ]


class SolveArgs(C.Structure):
    _fields_ = [
        ("partial", _p), ("seg_chunk_off", _p), ("nseg", _i32), ("zw", _i32),
        ("nlevels", _i32), ("npatterns", _i32), ("pattern_models", _p),
        ("nprob", _i32), ("prob_model", _p), ("prob_level", _p), ("prob_z", _p),
        ("prob_nz", _p), ("prob_flags", _p), ("add_back", _p), ("gram_flags", _p),
        ("nmodels", _i32), ("pmax", _i32), ("rec", _p), ("status", _p),
        ("moments", _p), ("mom_stride", _i32), ("ab_ncols", _i32),
        # what the statsmodels fix-ups read: set for fm_solve (inline) or, after it, for fm_solve_fixup
        ("fix_cols", _p), ("fix_stride", _i64), ("fix_seg_off", _p), ("fix_lo", _p), ("fix_hi", _p),
        ("fix_shift", _p), ("fix_inv_scale", _p), ("fix_level", _p), ("fix_check_const", _i32),
        ("fix_pad", _i32),
        # a planes-only panel's fix-up rows (fix_cols None; stride = fix_stride)
        ("fix_hi_plane", _p), ("fix_lo_plane", _p),
    ]


FM_NFIELDS = 12
FM_NCHARS = 12


class CharsArgs(C.Structure):
    _fields_ = [("ids", _p), ("n", _i64), ("field", _p * FM_NFIELDS), ("out", _p * FM_NCHARS)]


class PortArgs(C.Structure):
    _fields_ = [
        ("forecast", _p), ("ret", _p), ("weight", _p), ("level", _p), ("nyse", _p), ("seg_off", _p),
        ("nseg", _i32), ("max_seg_len", _i32), ("nport", _i32), ("min_level", _i32),
        ("nyse_breakpoints", _i32), ("min_count", _i32), ("q", _f64 * (FM_MAX_PORTS - 1)),
        ("bp", _p), ("port", _p), ("rec", _p), ("cnt", _p), ("status", _p),
    ]


class ForecastSrc(C.Structure):
    """fm_forecast_src: the fused forecast FPortArgs, FDistArgs, FCmpArgs and FHorArgs embed as ``src``."""
    _fields_ = [
        ("cols", _p), ("col_stride", _i64), ("hi_plane", _p), ("lo_plane", _p), ("plane_stride", _i64),
        ("lo", _p), ("hi", _p), ("coef", _p), ("forecast_out", _p), ("nrows", _i64),
        ("ncols", _i32), ("coef_stride", _i32), ("nsel", _i32), ("pad_src", _i32),
        ("sel_k", _i32 * FM_MAX_SORTS), ("sel_level", _i32 * FM_MAX_SORTS),
        ("sel_cols", (_i32 * FM_MAX_SORT_K) * FM_MAX_SORTS),
    ]


class FPortArgs(C.Structure):
    _fields_ = [
        ("src", ForecastSrc), ("ret_col", _i32), ("nseg", _i32), ("max_seg_len", _i32), ("nport", _i32),
        ("nyse_breakpoints", _i32), ("min_count", _i32), ("weight", _p), ("level", _p), ("nyse", _p),
        ("seg_off", _p), ("q", _f64 * (FM_MAX_PORTS - 1)), ("bp", _p), ("port", _p), ("rec", _p),
        ("cnt", _p), ("status", _p),
    ]


class FDistArgs(C.Structure):
    _fields_ = [
        ("src", ForecastSrc), ("forecast", _p), ("level", _p), ("seg_off", _p), ("nseg", _i32),
        ("max_seg_len", _i32), ("min_count", _i32), ("nq", _i32), ("q", _f64 * FM_MAX_DIST_Q),
        ("rec", _p), ("cnt", _p), ("status", _p),
    ]


class FCmpArgs(C.Structure):
    _fields_ = [
        ("src", ForecastSrc), ("forecast", _p), ("ret", _p), ("level", _p), ("seg_off", _p),
        ("ret_col", _i32), ("nseg", _i32), ("max_seg_len", _i32), ("min_count", _i32), ("npair", _i32),
        ("pad_fcmp", _i32), ("pair_a", _i32 * FM_MAX_PAIRS), ("pair_b", _i32 * FM_MAX_PAIRS),
        ("pair_level", _i32 * FM_MAX_PAIRS), ("rec", _p), ("cnt", _p), ("status", _p),
    ]


class FHorArgs(C.Structure):
    _fields_ = [
        ("src", ForecastSrc), ("forecast", _p), ("ret", _p), ("level", _p), ("seg_off", _p), ("nseg", _i32),
        ("max_seg_len", _i32), ("min_count", _i32), ("nq", _i32), ("q", _f64 * FM_MAX_DIST_Q),
        ("level_mult", _f64), ("gain", _f64), ("scaled_out", _p), ("rec", _p), ("cnt", _p), ("status", _p),
    ]


class RankArgs(C.Structure):
    _fields_ = [
        ("src", _p), ("src_stride", _i64), ("dst", _p), ("dst_stride", _i64), ("ncols", _i32),
        ("nseg", _i32), ("seg_off", _p), ("max_seg_len", _i32), ("min_level", _i32), ("level", _p),
        ("method", _i32), ("scale", _i32), ("nvalid", _p),
    ]


FM_MAX_HORIZON = 60
FM_MAX_FACTORS = 6
FM_MAX_ALPHA_MODELS = 4
FM_ALPHA_MAX_LAGS = 64
FM_ALPHA_MAX_MONTHS = 4096
FM_ALPHA_NSTAT = 4


class LinksArgs(C.Structure):
    _fields_ = [
        ("ids", _p), ("seg_off", _p), ("month_index", _p), ("nrows", _i64), ("nseg", _i32), ("step", _i32),
        ("link", _p), ("bad", _p),
    ]


class HorizonArgs(C.Structure):
    _fields_ = [
        ("ret", _p), ("link", _p), ("seg_off", _p), ("nrows", _i64), ("nseg", _i32), ("horizon", _i32),
        ("out", _p),
    ]


class AlphaArgs(C.Structure):
    _fields_ = [
        ("rec", _p), ("rec_month", _i64), ("rec_sort", _i64), ("rec_row", _i64), ("rec_col", _i64),
        ("status", _p), ("st_month", _i64), ("st_sort", _i64), ("nsel", _i32), ("nrow", _i32), ("T", _i32),
        ("K", _i32), ("M", _i32), ("nw_lags", _i32), ("factors", _p), ("rf", _p),
        ("model_mask", C.c_uint32 * FM_MAX_ALPHA_MODELS), ("spread_row", _i32), ("pad_alpha", _i32),
        ("coef", _p), ("se", _p), ("se_hac", _p), ("stat", _p), ("nobs", _p),
    ]


FM_MAX_HOLD = 36


class HoldArgs(C.Structure):
    _fields_ = [
        ("seg_off", _p), ("month_index", _p), ("link_prev", _p), ("port", _p), ("status", _p), ("ret", _p),
        ("weight", _p), ("sort_rec", _p), ("nrows", _i64), ("nseg", _i32), ("nsel", _i32), ("nport", _i32),
        ("hold", _i32), ("members", _p), ("stay", _p), ("cohort_n", _p), ("cohort", _p), ("status_out", _p),
        ("rec", _p), ("turnover", _p),
    ]


FM_MAX_GROUPS = 256
FM_GADJ_DEMEAN, FM_GADJ_MEAN, FM_GADJ_ZSCORE = 0, 1, 2


class GroupAdjArgs(C.Structure):
    _fields_ = [
        ("src", _p), ("src_stride", _i64), ("dst", _p), ("dst_stride", _i64), ("seg_off", _p), ("group", _p),
        ("level", _p), ("nrows", _i64), ("ncols", _i32), ("nseg", _i32), ("ngroups", _i32), ("mode", _i32),
        ("min_count", _i32), ("min_level", _i32), ("gcount", _p), ("gmean", _p), ("gsd", _p),
    ]


FM_MAX_DSORT = 10


class DsortArgs(C.Structure):
    _fields_ = [
        ("a", _p), ("b", _p), ("a_sort_stride", _i64), ("b_sort_stride", _i64), ("ret", _p), ("weight", _p),
        ("level", _p), ("nyse", _p), ("seg_off", _p), ("nrows", _i64), ("nseg", _i32), ("nsel", _i32),
        ("max_seg_len", _i32), ("na", _i32), ("nb", _i32), ("conditional", _i32), ("min_level", _i32),
        ("nyse_breakpoints", _i32), ("min_count", _i32), ("min_count_bin", _i32),
        ("qa", _f64 * (FM_MAX_DSORT - 1)), ("qb", _f64 * (FM_MAX_DSORT - 1)), ("rec_b", _p), ("rec_a", _p),
        ("cnt", _p), ("cell", _p), ("bpa", _p), ("bpb", _p), ("status", _p),
    ]


FM_WLS_MAX_COLS = 15


class WlsArgs(C.Structure):
    _fields_ = [
        ("cols", _p), ("col_stride", _i64), ("nrows", _i64), ("ncols", _i32), ("nseg", _i32), ("seg_off", _p),
        ("lo", _p), ("hi", _p), ("shift", _p), ("level", _p), ("weight", _p), ("nprob", _i32), ("pmax", _i32),
        ("prob_level", _p), ("prob_z", _p), ("prob_nz", _p), ("rec", _p), ("status", _p), ("moments", _p),
        ("mom_stride", _i32), ("pad_wls", _i32),
    ]


FM_POOL_MAX_K = 14
FM_POOL_FIRM_BLOCK = 256
FM_POOL_SE_CLASSICAL, FM_POOL_SE_WHITE, FM_POOL_SE_MONTH, FM_POOL_SE_FIRM, FM_POOL_SE_TWOWAY = range(5)
FM_POOL_SE_NAMES = ("classical", "white", "month", "firm", "twoway")


class PoolArgs(C.Structure):
    _fields_ = [
        ("cols", _p), ("col_stride", _i64), ("nrows", _i64), ("ncols", _i32), ("nseg", _i32), ("seg_off", _p),
        ("lo", _p), ("hi", _p), ("shift", _p), ("level", _p), ("firm", _p), ("nfirms", _i32), ("seg_lo", _i32),
        ("seg_hi", _i32), ("month_fe", _i32), ("small_sample", _i32), ("nprob", _i32), ("pmax", _i32),
        ("stage", _i32), ("prob_level", _p), ("prob_z", _p), ("prob_nz", _p), ("coef", _p), ("se", _p),
        ("cov", _p), ("stat", _p), ("status", _p), ("resid", _p), ("bad", _p), ("ws", _p), ("ws_bytes", _i64),
    ]


# name -> (restype, argtypes)
_SIGS = {
    "fm_version": (C.c_char_p, []),
    "fm_last_error": (C.c_char_p, []),
    "fm_device_arch": (_i32, [C.c_char_p, _i32]),
    "fm_struct_size": (_i64, [C.c_char_p]),
    "fm_select_cuts": (_i32, [_p, _i64, _i32, _p, _i32, _i32, _p, _f64, _f64, _i32, _i32,
                              _p, _p, _p, _p, _p, _p, _p]),
    "fm_select_ws_bytes": (_i64, [_i32, _i32, _i32]),
    "fm_split_planes": (_i32, [_p, _i64, _i32, _i64, _p, _p, _i64, _p]),
    "fm_select": (_i32, [C.POINTER(SelectArgs), _p]),
    "fm_select_universe": (_i32, [C.POINTER(SelectArgs), C.POINTER(UniverseArgs), _p]),
    "fm_clip": (_i32, [_p, _p, _i64, _i32, _p, _i32, _i64, _p, _p, _p]),
    "fm_standardize": (_i32, [_p, _p, _i64, _i32, _p, _i32, _i64, _p, _p, _p]),
    "fm_universe_level": (_i32, [_p, _p, _i32, _i64, _p, _p, _p, _p]),
    "fm_universe": (_i32, [_p, _p, _p, _i32, _i32, _f64, _f64, _p, _p, _p, _p]),
    "fm_sorted_join": (_i32, [_p, _p, _i64, _p, _p, _i64, _p, _p, _p]),
    "fm_ffill_expand": (_i32, [_p, _p, _p, _i32, _i64, _p, _i64, _i32, _p, _i64, _p, _p, _p]),
    "fm_pilot_shift": (_i32, [_p, _i64, _i32, _p, _i32, _p, _p]),
    "fm_gram": (_i32, [C.POINTER(GramArgs), _p]),
    "fm_solve": (_i32, [C.POINTER(SolveArgs), _p]),
    "fm_solve_fixup": (_i32, [C.POINTER(SolveArgs), _p]),
    "fm_ts_compact": (_i32, [_p, _i64, _i64, _i32, _i32, _p, _p, _p]),
    "fm_ts_summary": (_i32, [_p, _i64, _i64, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p,
                             _p, _p]),
    "fm_rolling_mean": (_i32, [_p, _i64, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p]),
    "fm_rolling_mean_own": (_i32, [_p, _i64, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                   _p, _p]),
    "fm_predictive": (_i32, [_p, _i32, _i32, _i32, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p,
                             _p]),
    "fm_ts_fused": (_i32, [C.POINTER(TsArgs), _p]),
    "fm_ts_fused_lds_bytes": (C.c_size_t, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "fm_forecast": (_i32, [_p, _i64, _i32, _p, _i32, _i64, _p, _i32, _p, _p]),
    "fm_portfolio_sort": (_i32, [C.POINTER(PortArgs), _p]),
    "fm_forecast_portfolio_sort": (_i32, [C.POINTER(FPortArgs), _p]),
    "fm_lagged_coef": (_i32, [_p, _p, _p, _i32, _i32, _i32, _p, _i32, _i32, _p, _p]),
    "fm_forecast_dist": (_i32, [C.POINTER(FDistArgs), _p]),
    "fm_forecast_compare": (_i32, [C.POINTER(FCmpArgs), _p]),
    "fm_forecast_horizon": (_i32, [C.POINTER(FHorArgs), _p]),
    "fm_rank_transform": (_i32, [C.POINTER(RankArgs), _p]),
    "fm_month_links": (_i32, [C.POINTER(LinksArgs), _p]),
    "fm_horizon_return": (_i32, [C.POINTER(HorizonArgs), _p]),
    "fm_portfolio_alpha": (_i32, [C.POINTER(AlphaArgs), _p]),
    "fm_portfolio_hold": (_i32, [C.POINTER(HoldArgs), _p]),
    "fm_group_adjust": (_i32, [C.POINTER(GroupAdjArgs), _p]),
    "fm_group_adjust_batch": (_i32, [_i32]),
    "fm_portfolio_double_sort": (_i32, [C.POINTER(DsortArgs), _p]),
    "fm_wls": (_i32, [C.POINTER(WlsArgs), _p]),
    "fm_pool": (_i32, [C.POINTER(PoolArgs), _p]),
    "fm_pool_ws_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "fm_segment_moments": (_i32, [_p, _i64, _i32, _p, _i32, _p, _i32, _i32, _p, _p, _p, _p]),
    "fm_distinct_count": (_i32, [_p, _i64, _p, _i64, _i32, _p, _i32, _i32, _i64, _i64, _p, _p, _p]),
    "fm_firm_chars": (_i32, [C.POINTER(CharsArgs), _p]),
    "fm_rolling_std": (_i32, [_p, _p, _i64, _i32, _i32, _f64, _p, _p]),
    "fm_rolling_beta": (_i32, [_p, _p, _p, _i64, _p, _i32, _i32, _p, _p, _p, _i32, _p, _p, _p]),
    "fm_gen_panel": (_i32, [C.c_uint64, _i64, _i32, _i32, _f64, _f64, _p, _i64, _p, _p, _p]),
    "fm_gen_panel_planes": (_i32, [C.c_uint64, _i64, _i32, _i32, _f64, _f64, _p, _i64, _p, _p, _i64, _p, _p, _p]),
    "fm_merge_planes": (_i32, [_p, _p, _i64, _i32, _i64, _p, _i64, _p]),
    "fm_stream_probe": (_i32, [_p, _i64, _p, _p]),
    "fm_stream_copy_probe": (_i32, [_p, _p, _i64, _p]),
}

EXPORTED = tuple(_SIGS)
_STRUCTS = {"fm_gram_args": GramArgs, "fm_solve_args": SolveArgs, "fm_select_args": SelectArgs,
            "fm_universe_args": UniverseArgs, "fm_ts_args": TsArgs, "fm_chars_args": CharsArgs,
            "fm_port_args": PortArgs, "fm_rank_args": RankArgs, "fm_forecast_src": ForecastSrc,
            "fm_fport_args": FPortArgs, "fm_fdist_args": FDistArgs,
            "fm_fcmp_args": FCmpArgs, "fm_links_args": LinksArgs, "fm_horizon_args": HorizonArgs,
            "fm_fhor_args": FHorArgs, "fm_alpha_args": AlphaArgs,
            "fm_hold_args": HoldArgs, "fm_gadj_args": GroupAdjArgs,
            "fm_dsort_args": DsortArgs, "fm_wls_args": WlsArgs,
            "fm_pool_args": PoolArgs}

_lib = None


class FMError(RuntimeError):
    """A libfm_hip entry point returned an error code."""


def load():
    """Load libfm_hip.so (once).  Raises ImportError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libfm_hip.so not found at {LIB_PATH}; build it with "
            "`make -C fm-returnprediction_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # the argument structs must match the library's layouts byte for byte (a struct shorter
    # than the C one leaves the library reading past it)
    for cname, cls in _STRUCTS.items():
        want = lib.fm_struct_size(cname.encode())
        if want != C.sizeof(cls):
            raise ImportError(f"ABI mismatch: {cname} is {want} bytes in libfm_hip.so, "
                              f"{C.sizeof(cls)} in fmcore._lib.{cls.__name__}")
    _lib = lib
    return lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.fm_last_error().decode(errors="replace")
        raise FMError(f"{name} failed ({rc}): {msg}")
    return rc


def version():
    return load().fm_version().decode()
