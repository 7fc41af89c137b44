"""CPU tests of fm_forecast_horizon (extension A17): the binding, the argument checks that return
before any launch, the exact numpy restatement (tests/fhor_oracle.py) against the plain numpy
chain, the extrapolation gain, and the signatures and rules of the Python layers."""
import ctypes
import dataclasses
import inspect

import numpy as np
import pytest

import fhor_oracle as HO
from fmtol import assert_series_close

FAKE = 4096   # a device pointer that is never dereferenced: every call below is refused first


def _args(L, **kw):
    """A call with null pointers everywhere: one month, one sort, q = (0.1, 0.9), a = 3, g = 2.71.
    A keyword names a field of the struct or of its embedded fm_forecast_src."""
    a = L.FHorArgs()
    a.nseg, a.src.nsel, a.src.nrows, a.max_seg_len, a.min_count, a.nq = 1, 1, 10, 10, 1, 2
    a.q[0], a.q[1] = 0.1, 0.9
    a.level_mult, a.gain = 3.0, 2.71
    own = {f[0] for f in L.FHorArgs._fields_}
    for k, v in kw.items():
        if k == "q":
            a.nq = len(v)
            for i, x in enumerate(v[:L.FM_MAX_DIST_Q]):
                a.q[i] = x
        else:
            assert k in own or hasattr(a.src, k), k
            setattr(a if k in own else a.src, k, v)
    return a


def _rc(L, a):
    lib = L.load()
    rc = lib.fm_forecast_horizon(ctypes.byref(a), None)
    return rc, lib.fm_last_error().decode()


def test_binding_and_zeroed_struct():
    from fmcore import _lib as L
    lib = L.load()
    assert "fm_forecast_horizon" in L.EXPORTED and hasattr(lib, "fm_forecast_horizon")
    assert lib.fm_struct_size(b"fm_fhor_args") == ctypes.sizeof(L.FHorArgs)
    assert L._STRUCTS["fm_fhor_args"] is L.FHorArgs and L.FM_FHOR_NREC == 6
    names = [f[0] for f in L.FHorArgs._fields_]
    assert names[0] == "src" and names[-4:] == ["scaled_out", "rec", "cnt", "status"]
    assert {"forecast", "ret", "level", "seg_off", "nseg", "max_seg_len", "min_count", "nq", "q", "level_mult",
            "gain"} <= set(names)
    # a zeroed struct names no source, no gain and no min_count: refused, not read
    rc, msg = _rc(L, L.FHorArgs())
    assert rc == -1 and msg.startswith("fm_forecast_horizon: ")


def test_argument_checks_return_before_any_launch():
    """Every pointer is null or never read: each call is refused on its arguments alone."""
    from fmcore import _lib as L
    rc, msg = _rc(L, _args(L))                                   # no source
    assert rc == -1 and "exactly one" in msg
    for two in (dict(forecast=FAKE, cols=FAKE), dict(forecast=FAKE, hi_plane=FAKE, lo_plane=FAKE),
                dict(cols=FAKE, hi_plane=FAKE, lo_plane=FAKE)):
        rc, msg = _rc(L, _args(L, **two))
        assert rc == -1 and "exactly one" in msg, two
    rc, msg = _rc(L, _args(L, forecast=FAKE, forecast_out=FAKE))
    assert rc == -1 and "forecast_out goes with a panel source" in msg
    rc, msg = _rc(L, _args(L, q=[0.1 * i for i in range(1, 10)]))   # nq = 9
    assert rc == -1 and "nq" in msg
    for q in ([0.9, 0.1], [0.5, 0.5], [0.0, 0.5], [0.5, 1.0], [float("nan"), 0.5], [0.5, float("nan")]):
        rc, msg = _rc(L, _args(L, q=q))
        assert rc == -1 and "ascending" in msg, q
    rc, msg = _rc(L, _args(L, min_count=0))
    assert rc == -1 and "min_count" in msg
    for g in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = _rc(L, _args(L, forecast=FAKE, ret=FAKE, gain=g))
        assert rc == -1 and "gain must be finite and > 0" in msg, g
    for a in (float("inf"), -float("inf"), float("nan")):
        rc, msg = _rc(L, _args(L, forecast=FAKE, ret=FAKE, level_mult=a))
        assert rc == -1 and "level_mult must be finite" in msg, a
    rc, msg = _rc(L, _args(L, nsel=L.FM_MAX_SORTS + 1))
    assert rc == -1 and "nsel" in msg
    rc, msg = _rc(L, _args(L, forecast=FAKE, sel_level=(ctypes.c_int32 * L.FM_MAX_SORTS)(256)))
    assert rc == -1 and "sel_level" in msg
    rc, msg = _rc(L, _args(L, forecast=FAKE))                    # a good source, no return vector
    assert rc == -1 and "ret is needed" in msg
    rc, msg = _rc(L, _args(L, forecast=FAKE, ret=FAKE))          # ... and no outputs
    assert rc == -1 and msg == "fm_forecast_horizon: null pointer"
    rc, msg = _rc(L, _args(L, max_seg_len=16385))
    assert rc == -3 and "16384" in msg
    assert _rc(L, _args(L, max_seg_len=16384))[0] == -1          # the limit itself: refused for its source only
    # level_mult may be zero or negative; only the gain is signed
    assert "null pointer" in _rc(L, _args(L, forecast=FAKE, ret=FAKE, level_mult=0.0))[1]
    assert "null pointer" in _rc(L, _args(L, forecast=FAKE, ret=FAKE, level_mult=-2.0))[1]


def test_empty_calls_are_valid_with_host_pointers():
    """nsel == 0 or nseg == 0 returns before anything is read, pointers and all."""
    from fmcore import _lib as L
    assert _rc(L, _args(L, nsel=0))[0] == 0 and _rc(L, _args(L, nseg=0))[0] == 0
    assert _rc(L, _args(L, nsel=0, q=[]))[0] == 0
    buf = (ctypes.c_double * 8)(*([7.0] * 8))
    p = ctypes.cast(buf, ctypes.c_void_p).value                  # host memory: an empty call never touches it
    for kw in (dict(nsel=0), dict(nseg=0)):
        assert _rc(L, _args(L, forecast=p, ret=p, rec=p, cnt=p, status=p, seg_off=p, scaled_out=p, **kw))[0] == 0
    assert list(buf) == [7.0] * 8
    # the argument rules still hold on an empty call
    assert _rc(L, _args(L, nsel=0, gain=0.0))[0] == -1 and _rc(L, _args(L, nseg=0, min_count=0))[0] == -1


def _good_src(f):
    """A panel source that passes every check: 3 FP64 columns of 10 rows, one sort of K = 2."""
    f.cols, f.col_stride, f.ncols, f.nrows, f.nsel = FAKE, 10, 3, 10, 1
    f.sel_k[0], f.sel_cols[0][0], f.sel_cols[0][1] = 2, 1, 2
    f.coef, f.coef_stride = FAKE, 3


def _set(**kw):
    return lambda f: [setattr(f, k, v) for k, v in kw.items()]


def _sel(field, value):
    def edit(f):
        if field == "col":
            f.sel_cols[0][1] = value
        else:
            getattr(f, field)[0] = value
    return edit


BAD_SOURCES = [
    ("cols and planes together", _set(hi_plane=FAKE, lo_plane=FAKE, plane_stride=10), "exactly one"),
    ("one plane only", _set(cols=None, hi_plane=FAKE, plane_stride=10), "both planes"),
    ("the other plane only", _set(cols=None, lo_plane=FAKE, plane_stride=10), "both planes"),
    ("stride below nrows", _set(col_stride=9), "stride below"),
    ("plane stride below nrows", _set(cols=None, hi_plane=FAKE, lo_plane=FAKE, plane_stride=9), "stride below"),
    ("K = 0", _sel("sel_k", 0), "K = 0"),
    ("K = 31", _sel("sel_k", 31), "K = 31"),
    ("coef_stride below K + 1", _set(coef_stride=2), "coef_stride 2 below K + 1 = 3"),
    ("column -1", _sel("col", -1), "column -1 outside"),
    ("column ncols", _sel("col", 3), "column 3 outside"),
    ("sel_level 256", _sel("sel_level", 256), "sel_level"),
    ("lo without hi", _set(lo=FAKE), "lo and hi"),
    ("hi without lo", _set(hi=FAKE), "lo and hi"),
    ("coef NULL", _set(coef=None), "null pointer"),
]


@pytest.mark.parametrize("what,edit,text", BAD_SOURCES, ids=[b[0] for b in BAD_SOURCES])
def test_a_bad_panel_source_is_refused_as_fm_forecast_dist_refuses_it(what, edit, text):
    """fm_forecast_horizon checks its fm_forecast_src with its sibling's helper: the same bad source
    gets FM_EINVAL from both, in the same words after the prefix."""
    from fmcore import _lib as L
    lib = L.load()
    d = L.FDistArgs()
    d.nseg, d.max_seg_len, d.min_count = 1, 10, 1
    h = _args(L, ret=FAKE)
    msgs = []
    for a, fn, who in ((d, lib.fm_forecast_dist, "fm_forecast_dist"), (h, lib.fm_forecast_horizon, "fm_forecast_horizon")):
        _good_src(a.src)
        assert fn(ctypes.byref(a), None) == -1 and lib.fm_last_error().decode() == who + ": null pointer"   # the outputs
        edit(a.src)
        assert fn(ctypes.byref(a), None) == -1, (what, who)
        msg = lib.fm_last_error().decode()
        assert msg.startswith(who + ": ") and text in msg, (what, msg)
        msgs.append(msg[len(who) + 2:])
    assert msgs[0] == msgs[1], (what, msgs)


def _ragged(seed=5):
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, 2, 3, 40, 1, 17, 2, 300, 64, 65, 5, 4200])
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    F = rng.standard_t(3, n) * 0.02 + 0.01
    F[rng.random(n) < 0.1] = np.nan
    F[int(seg_off[8]) + 3], F[int(seg_off[8]) + 4] = np.inf, -np.inf
    F[int(seg_off[4]):int(seg_off[5])] = np.nan          # a month without an eligible row
    ret = 0.5 * F + rng.normal(0.0, 0.1, n)
    ret[rng.random(n) < 0.05] = np.nan
    ret[int(seg_off[9]):int(seg_off[10])] = np.nan       # a month without a return
    level = rng.integers(0, 3, n).astype(np.uint8)
    return seg_off, F, ret, level


def test_exact_restatement_vs_plain_chain():
    """(a), the fixed summation order written out, against (b), np.mean / np.std / np.quantile /
    np.polyfit, on a random ragged panel: counts, status and the scaled forecasts' NaN masks equal,
    every rec column and the scaled forecasts at RTOL under the series rule."""
    seg_off, F, ret, level = _ragged()
    q = (0.1, 0.5, 0.9)
    g = 1.0 + 0.9 + 0.9 * 0.9
    for min_level, min_count in ((0, 1), (1, 1), (0, 3)):
        a = HO.forecast_horizon_exact(seg_off, F, ret, 3.0, g, level, min_level, q, min_count)
        b = HO.forecast_horizon(seg_off, F, ret, 3.0, g, level, min_level, q, min_count)
        assert np.array_equal(a["cnt"], b["cnt"]) and np.array_equal(a["status"], b["status"])
        assert np.array_equal(a["status"], (a["cnt"][:, 0] >= min_count).astype(np.int32))
        assert {0, 1, 2} <= set(a["cnt"][:, 0].tolist()) and a["cnt"][9, 1] == 0 and a["status"][9] == 1
        assert np.isnan(a["rec"][a["status"] == 0]).all()
        for c in range(a["rec"].shape[1]):
            assert_series_close(a["rec"][:, c], b["rec"][:, c], f"rec[:, {c}] level>={min_level} min_count={min_count}")
        assert_series_close(a["scaled"], b["scaled"], "scaled")
        assert np.isfinite(a["rec"][a["cnt"][:, 1] >= 3][:, 2:5]).all()
        assert np.isnan(a["rec"][a["cnt"][:, 1] < 2][:, 2:5]).all()
    # a = 1, g = 1 leaves the forecasts as they are, up to the rounding of m + (F - m)
    one = HO.forecast_horizon_exact(seg_off, F, ret, 1.0, 1.0, level, 0, q)
    ok = np.isfinite(F)
    assert np.array_equal(np.isnan(one["scaled"]), ~ok) and np.allclose(one["scaled"][ok], F[ok], rtol=0, atol=1e-15)


def test_tile_sum_order():
    """The written-out order: a month of one tile is the butterfly alone; tiles l and l + 64 meet in
    lane l before the second butterfly."""
    x = np.zeros(64)
    x[0], x[32], x[1] = 1.0, 2.0 ** -53, 2.0 ** -53     # lane 0 adds lane 32 first: 1 + 2^-53 rounds to 1
    assert HO.tile_sum(x) == 1.0
    x = np.zeros(65 * 64)
    x[0], x[64 * 64] = 1.0, -1.0                         # tiles 0 and 64: lane 0's two terms
    x[64] = 2.0 ** -60                                   # tile 1: lane 1
    assert HO.tile_sum(x) == 2.0 ** -60
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 4095, 4096, 4097, 16384):
        v = rng.normal(size=n)
        assert abs(HO.tile_sum(v) - np.sum(v)) <= 1e-12 * np.sum(np.abs(v))


def test_extrapolation_gain():
    from fmcore import engine as E
    assert abs(E.extrapolation_gain(12, 0.9) - sum(0.9 ** j for j in range(12))) <= 1e-15 * sum(0.9 ** j for j in range(12))
    for k in (1, 2, 3, 6, 12, 60):
        assert E.extrapolation_gain(k, 1.0) == k
    assert E.extrapolation_gain(1, 0.9) == 1.0 and E.extrapolation_gain(2, 0.9) == 1.9
    assert E.extrapolation_gain(3, 0.9) == 1.0 + 0.9 + 0.9 * 0.9


def test_python_signatures():
    from fmcore import engine as E, lewellen as LW
    from fmdrop import bind, calc_Lewellen_2014 as CL

    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}

    assert list(inspect.signature(E.forecast_horizon).parameters) == \
        ["panel", "coef", "sel", "ret", "level_mult", "gain", "cuts", "level", "q", "min_count", "scaled_out",
         "forecast_out", "out"]
    assert defaults(E.forecast_horizon) == dict(cuts=None, level=None, q=(0.1, 0.9), min_count=1, scaled_out=False,
                                                forecast_out=False, out=None)
    assert list(inspect.signature(E.forecast_horizon_vector).parameters)[:10] == \
        ["seg_off", "forecast", "ret", "level_mult", "gain", "level", "min_level", "q", "min_count", "max_seg_len"]
    assert defaults(E.forecast_horizon_vector) == dict(level=None, min_level=0, q=(0.1, 0.9), min_count=1,
                                                       max_seg_len=None, scaled_out=False)
    assert list(inspect.signature(E.forecast_horizon_summary).parameters) == ["h", "nw_lags"]
    assert list(inspect.signature(E.extrapolation_gain).parameters) == ["k", "decay"]
    assert [f.name for f in dataclasses.fields(E.ForecastHorizon)] == ["rec", "cnt", "status", "scaled", "forecast"]
    fields = dataclasses.fields(LW.PipelineConfig)
    names = [f.name for f in fields]
    assert names[-3:] == ["horizon", "forecast_compare", "rank"]
    assert names[-7:-3] == ["extrapolate", "extrapolate_decay", "extrapolate_q", "extrapolate_nw_lags"]
    assert all(f.kw_only for f in fields[-7:-3])
    c = LW.PipelineConfig()
    assert (c.extrapolate, c.extrapolate_decay, c.extrapolate_q, c.extrapolate_nw_lags) == (None, 0.9, (0.1, 0.9), None)
    res = {f.name: f for f in dataclasses.fields(LW.PipelineResult)}
    for name in ("extrapolated", "extrapolated_summary", "extrapolated_problems"):
        assert res[name].default is None
    p = inspect.signature(CL.build_table_3_extrapolated).parameters
    assert list(p) == ["crsp_comp", "horizon", "variables_dict", "decay", "q", "cfg"]
    assert p["decay"].default == 0.9 and p["q"].default == (0.1, 0.9)
    p = inspect.signature(CL.forecast_extrapolation).parameters
    assert list(p)[:7] == ["df", "forecast", "horizon", "decay", "return_col", "universe", "q"]
    assert (p["decay"].default, p["return_col"].default, p["universe"].default, p["q"].default) == (0.9, "retx", None, (0.1, 0.9))
    src = inspect.getsource(bind)   # extensions, like Tables 3 to 5: not bound into the reference's namespace
    assert "build_table_3_extrapolated" not in src and "forecast_extrapolation" not in src


def test_pipeline_config_rules_need_no_device():
    from fmcore import lewellen as LW
    from fmcore import step as ST
    for k in (0, 1, -3, 61, 2.5, True, "3"):
        with pytest.raises(ValueError, match="extrapolate must be an integer in 2..60"):
            LW.run_pipeline(None, LW.PipelineConfig(extrapolate=k))
    for rho in (0.0, -0.5, 1.0000001, float("nan"), float("inf"), "0.9", True):
        with pytest.raises(ValueError, match=r"extrapolate_decay must lie in \(0, 1\]"):
            LW.run_pipeline(None, LW.PipelineConfig(extrapolate=3, extrapolate_decay=rho))
    with pytest.raises(ValueError, match="extrapolate=3 excludes horizon=3"):
        LW.run_pipeline(None, LW.PipelineConfig(extrapolate=3, horizon=3, lag=3))
    with pytest.raises(ValueError, match="extrapolate excludes standardize"):
        LW.run_pipeline(None, LW.PipelineConfig(extrapolate=3, standardize=True))
    with pytest.raises(ValueError, match="extrapolate needs forecasts"):
        LW.run_pipeline(None, LW.PipelineConfig(extrapolate=3, forecasts=False))
    LW.check_extrapolate(LW.PipelineConfig())
    LW.check_extrapolate(LW.PipelineConfig(extrapolate=2, extrapolate_decay=1.0))
    LW.check_extrapolate(LW.PipelineConfig(extrapolate=60, extrapolate_decay=1e-3, lag=5))
    with pytest.raises(ValueError, match="ShardedStep: cfg.extrapolate must be None"):
        ST.ShardedStep(None, LW.PipelineConfig(extrapolate=3), None)
