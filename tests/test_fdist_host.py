"""CPU tests of fm_forecast_dist (extension A14): the binding, the argument checks that return
before any launch, the numpy restatement (tests/fdist_oracle.py) against the pandas chain, and the
signatures of the Python layers."""
import ctypes
import dataclasses
import inspect

import numpy as np
import pandas as pd
import pytest

import fdist_oracle as FO


def _args(L, **kw):
    """A call with null pointers everywhere: one month, one sort, q = (0.1, 0.9).  A keyword names
    a field of the struct or of its embedded fm_forecast_src."""
    a = L.FDistArgs()
    a.nseg, a.src.nsel, a.src.nrows, a.max_seg_len, a.min_count, a.nq = 1, 1, 10, 10, 1, 2
    a.q[0], a.q[1] = 0.1, 0.9
    own = {f[0] for f in L.FDistArgs._fields_}
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
    rc = lib.fm_forecast_dist(ctypes.byref(a), None)
    return rc, lib.fm_last_error().decode()


def test_binding():
    from fmcore import _lib as L
    lib = L.load()
    assert "fm_forecast_dist" in L.EXPORTED and hasattr(lib, "fm_forecast_dist")
    assert lib.fm_struct_size(b"fm_fdist_args") == ctypes.sizeof(L.FDistArgs)
    assert L.FM_MAX_DIST_Q == 8


def test_argument_checks_return_before_any_launch():
    """Every pointer is null or never read: each call is refused on its arguments alone."""
    from fmcore import _lib as L
    rc, msg = _rc(L, _args(L))                                   # no source
    assert rc == -1 and "exactly one" in msg
    fake = 4096                                                  # never dereferenced: the call is refused first
    for two in (dict(forecast=fake, cols=fake), dict(forecast=fake, hi_plane=fake, lo_plane=fake),
                dict(cols=fake, hi_plane=fake, lo_plane=fake)):
        rc, msg = _rc(L, _args(L, **two))
        assert rc == -1 and "exactly one" in msg, two
    rc, msg = _rc(L, _args(L, q=[0.1 * i for i in range(1, 10)]))   # nq = 9
    assert rc == -1 and "nq" in msg
    for q in ([0.9, 0.1], [0.5, 0.5], [0.0, 0.5], [0.5, 1.0], [float("nan"), 0.5], [0.5, float("nan")]):
        rc, msg = _rc(L, _args(L, q=q))
        assert rc == -1 and "ascending" in msg, q
    rc, msg = _rc(L, _args(L, min_count=0))
    assert rc == -1 and "min_count" in msg
    rc, msg = _rc(L, _args(L, nsel=L.FM_MAX_SORTS + 1))
    assert rc == -1 and "nsel" in msg
    rc, msg = _rc(L, _args(L, max_seg_len=16385))
    assert rc == -3 and "16384" in msg
    assert _rc(L, _args(L, max_seg_len=16384))[0] == -1          # the limit itself: refused for its source only
    # the empty calls are valid, pointers and all
    assert _rc(L, _args(L, nsel=0))[0] == 0 and _rc(L, _args(L, nseg=0))[0] == 0
    assert _rc(L, _args(L, nsel=0, q=[]))[0] == 0


FAKE = 4096   # a device pointer that is never dereferenced: every call below is refused first


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
def test_both_fused_entry_points_refuse_a_bad_source_alike(what, edit, text):
    """fm_forecast_portfolio_sort and fm_forecast_dist embed one fm_forecast_src and check it with
    one helper: the same bad source gets FM_EINVAL from both, in the same words after the prefix.
    The outputs and seg_off stay NULL, so even the good source is refused before any launch."""
    from fmcore import _lib as L
    lib = L.load()
    p = L.FPortArgs()
    p.nseg, p.max_seg_len, p.nport, p.min_count, p.ret_col = 1, 10, 10, 1, 0
    for j in range(9):
        p.q[j] = (j + 1) / 10
    d = _args(L)
    msgs = []
    for a, fn, who in ((p, lib.fm_forecast_portfolio_sort, "fm_forecast_portfolio_sort"), (d, lib.fm_forecast_dist, "fm_forecast_dist")):
        _good_src(a.src)
        assert fn(ctypes.byref(a), None) == -1 and lib.fm_last_error().decode() == who + ": null pointer"   # the outputs
        edit(a.src)
        assert fn(ctypes.byref(a), None) == -1, (what, who)
        msg = lib.fm_last_error().decode()
        assert msg.startswith(who + ": ") and text in msg, (what, msg)
        msgs.append(msg[len(who) + 2:])
    assert msgs[0] == msgs[1], (what, msgs)


def test_restatement_vs_pandas_chain():
    """groupby(month)[F].mean() / .std() / .quantile(q) on the eligible rows, ragged months with
    n = 0, 1 and 2 eligible rows among them, at 1e-12."""
    rng = np.random.default_rng(5)
    lens = np.array([0, 1, 2, 3, 40, 1, 17, 2, 300, 64, 5])
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    F = rng.standard_t(3, n) * 0.02 + 0.01
    F[rng.random(n) < 0.1] = np.nan
    F[int(seg_off[8]) + 3] = np.inf
    F[int(seg_off[8]) + 4] = -np.inf
    F[int(seg_off[4]):int(seg_off[5])] = np.nan          # a month without an eligible row
    level = rng.integers(0, 3, n).astype(np.uint8)
    month = np.repeat(np.arange(len(lens)), lens)
    q = (0.1, 0.5, 0.9)
    for min_level in (0, 1):
        got = FO.forecast_dist(seg_off, F, level, min_level, q)
        d = pd.DataFrame({"m": month, "F": F})[np.isfinite(F) & (level >= min_level)]
        g = d.groupby("m")["F"]
        exp = pd.DataFrame({"mean": g.mean(), "std": g.std()})
        for lv in q:
            exp[lv] = g.quantile(lv)
        cnt = g.size().reindex(range(len(lens)), fill_value=0).to_numpy()
        assert np.array_equal(got["cnt"], cnt) and np.array_equal(got["status"], (cnt >= 1).astype(np.int32))
        assert {0, 1, 2} <= set(cnt.tolist())
        for t in range(len(lens)):
            if cnt[t] == 0:
                assert np.isnan(got["rec"][t]).all()
                continue
            e = exp.loc[t].to_numpy()
            assert np.isnan(got["rec"][t, 1]) == (cnt[t] == 1) == bool(np.isnan(e[1]))
            fin = np.isfinite(e)
            assert np.all(np.abs(got["rec"][t][fin] - e[fin]) <= 1e-12 * np.maximum(np.abs(e[fin]), 1.0)), (min_level, t)
    # min_count above a month's count
    got = FO.forecast_dist(seg_off, F, None, 0, q, min_count=3)
    assert np.array_equal(got["status"], (got["cnt"] >= 3).astype(np.int32))
    assert np.isnan(got["rec"][got["status"] == 0]).all()


def test_python_signatures():
    from fmcore import engine as E, lewellen as LW
    from fmdrop import bind, calc_Lewellen_2014 as CL

    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}

    assert list(inspect.signature(E.forecast_dist).parameters) == \
        ["panel", "coef", "sel", "cuts", "level", "q", "min_count", "forecast_out", "out"]
    assert defaults(E.forecast_dist) == dict(cuts=None, level=None, q=(0.1, 0.9), min_count=1, forecast_out=False, out=None)
    assert list(inspect.signature(E.forecast_dist_vector).parameters) == \
        ["seg_off", "forecast", "level", "min_level", "q", "min_count", "max_seg_len"]
    assert defaults(E.forecast_dist_vector) == dict(level=None, min_level=0, q=(0.1, 0.9), min_count=1, max_seg_len=None)
    assert defaults(E.forecast_dist_summary) == dict(nw_lags=4)
    assert [f.name for f in dataclasses.fields(E.ForecastDist)] == ["rec", "cnt", "status", "forecast"]
    fields = dataclasses.fields(LW.PipelineConfig)
    assert fields[-1].name == "rank"
    byname = {f.name: f for f in fields}
    assert byname["forecast_dist"].default is False and byname["forecast_dist"].kw_only
    assert byname["forecast_dist_q"].default == (0.1, 0.9) and byname["forecast_dist_q"].kw_only
    assert LW.PipelineConfig().forecast_dist is False
    for name in ("forecast_dist", "forecast_dist_summary", "forecast_dist_problems"):
        assert name in {f.name for f in dataclasses.fields(LW.PipelineResult)}
    p = inspect.signature(CL.forecast_distribution).parameters
    assert list(p)[:5] == ["df", "forecast", "universe", "q", "date_col"]
    assert p["universe"].default is None and p["q"].default == (0.1, 0.9) and p["date_col"].default == "mthcaldt"
    p = inspect.signature(CL.build_table_3).parameters
    assert list(p) == ["crsp_comp", "variables_dict", "q", "cfg"] and p["q"].default == (0.1, 0.9)
    # extensions, like Table 5: not bound into the reference's namespace
    src = inspect.getsource(bind)
    assert "build_table_3" not in src and "forecast_distribution" not in src


def test_pipeline_config_rules_need_no_device():
    """forecast_dist needs forecasts=True and excludes standardize=True: refused before any work."""
    from fmcore import lewellen as LW
    with pytest.raises(ValueError, match="standardize"):
        LW.run_pipeline(None, LW.PipelineConfig(forecast_dist=True, standardize=True))
    with pytest.raises(ValueError, match="forecasts"):
        LW.run_pipeline(None, LW.PipelineConfig(forecast_dist=True, forecasts=False))
