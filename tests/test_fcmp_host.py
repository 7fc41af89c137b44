"""CPU tests of fm_forecast_compare (extension A15; paper Table 4): the binding, the argument checks
that return before any HIP call, the numpy restatement (tests/fcmp_oracle.py) against an
independent numpy chain, and the signatures of the Python layers."""
import ctypes
import dataclasses
import inspect

import numpy as np
import pytest

import fcmp_oracle as CO
from fmtol import assert_series_close

FAKE = 4096   # a device pointer that is never dereferenced: every call below returns first


def _args(L, source="vec", **kw):
    """One month of 10 rows, two forecasts, the pair (0, 1): a call that passes every check, every
    pointer FAKE (``source``: "vec" the caller's vectors, "f64" / "planes" a 3-column panel, None
    no source).  A keyword names a field of the struct or of its embedded fm_forecast_src; pairs =
    [(a, b, level), ...] sets the pair table."""
    a = L.FCmpArgs()
    a.nseg, a.max_seg_len, a.min_count, a.npair = 1, 10, 1, 1
    a.src.nsel, a.src.nrows = 2, 10
    a.pair_a[0], a.pair_b[0] = 0, 1
    a.seg_off = a.rec = a.cnt = a.status = FAKE
    if source == "vec":
        a.forecast = a.ret = FAKE
    elif source is not None:
        f = a.src
        if source == "f64":
            f.cols, f.col_stride = FAKE, 10
        else:
            f.hi_plane, f.lo_plane, f.plane_stride = FAKE, FAKE, 10
        f.ncols, f.coef, f.coef_stride = 3, FAKE, 3
        for j in range(2):
            f.sel_k[j], f.sel_cols[j][0], f.sel_cols[j][1] = 2, 1, 2
    own = {f[0] for f in L.FCmpArgs._fields_}
    for k, v in kw.items():
        if k == "pairs":
            a.npair = len(v)
            for i, (pa, pb, lv) in enumerate(v[:L.FM_MAX_PAIRS]):
                a.pair_a[i], a.pair_b[i], a.pair_level[i] = pa, pb, lv
        else:
            assert k in own or hasattr(a.src, k), k
            setattr(a if k in own else a.src, k, v)
    return a


def _rc(L, a):
    lib = L.load()
    rc = lib.fm_forecast_compare(ctypes.byref(a), None)
    return rc, lib.fm_last_error().decode()


def test_binding():
    from fmcore import _lib as L
    lib = L.load()
    assert "fm_forecast_compare" in L.EXPORTED and hasattr(lib, "fm_forecast_compare")
    assert lib.fm_struct_size(b"fm_fcmp_args") == ctypes.sizeof(L.FCmpArgs)
    assert L._STRUCTS["fm_fcmp_args"] is L.FCmpArgs
    assert L.FM_MAX_PAIRS == 16 and L.FM_FCMP_NREC == 7
    # zero-initialised, the embedded source first, the outputs last
    names = [f[0] for f in L.FCmpArgs._fields_]
    assert names[0] == "src" and names[-3:] == ["rec", "cnt", "status"]
    assert bytes(L.FCmpArgs()) == bytes(ctypes.sizeof(L.FCmpArgs))


REFUSED = [
    ("npair 17", "vec", dict(npair=17), -1, "npair"),
    ("npair -1", "vec", dict(npair=-1), -1, "npair"),
    ("pair a = -1", "vec", dict(pairs=[(-1, 1, 0)]), -1, "outside the 2 forecasts"),
    ("pair a = nsel", "vec", dict(pairs=[(2, 1, 0)]), -1, "outside the 2 forecasts"),
    ("pair b = -1", "vec", dict(pairs=[(0, -1, 0)]), -1, "outside the 2 forecasts"),
    ("pair b = nsel", "vec", dict(pairs=[(0, 1, 0), (0, 2, 0)]), -1, "pair 1 (0, 2)"),
    ("pairs without forecasts", "vec", dict(nsel=0), -1, "outside the 0 forecasts"),
    ("pair_level 256", "vec", dict(pairs=[(0, 1, 256)]), -1, "pair_level"),
    ("pair_level -1", "vec", dict(pairs=[(0, 1, -1)]), -1, "pair_level"),
    ("min_count 0", "vec", dict(min_count=0), -1, "min_count"),
    ("no source", None, dict(), -1, "exactly one"),
    ("vectors and columns", "vec", dict(cols=FAKE), -1, "exactly one"),
    ("vectors and planes", "vec", dict(hi_plane=FAKE, lo_plane=FAKE), -1, "exactly one"),
    ("columns and planes", "f64", dict(hi_plane=FAKE, lo_plane=FAKE, plane_stride=10), -1, "exactly one"),
    ("one plane only", "planes", dict(lo_plane=None), -1, "both planes"),
    ("vectors without ret", "vec", dict(ret=None), -1, "need ret"),
    ("vectors with forecast_out", "vec", dict(forecast_out=FAKE), -1, "forecast_out"),
    ("panel with ret", "f64", dict(ret=FAKE), -1, "ret goes with forecast vectors"),
    ("ret_col -1", "f64", dict(ret_col=-1), -1, "ret_col"),
    ("ret_col ncols", "planes", dict(ret_col=3), -1, "ret_col"),
    ("column outside the panel", "f64", dict(ncols=2), -1, "outside the panel's 2"),
    ("nsel 17", "vec", dict(nsel=17), -1, "nsel"),
    ("seg_off NULL", "vec", dict(seg_off=None), -1, "null pointer"),
    ("rec NULL", "f64", dict(rec=None), -1, "null pointer"),
    ("cnt NULL", "planes", dict(cnt=None), -1, "null pointer"),
    ("status NULL", "vec", dict(status=None), -1, "null pointer"),
    ("16,385-row months, vectors", "vec", dict(max_seg_len=16385), -3, "16384"),
    ("16,385-row months, panel", "f64", dict(max_seg_len=16385), -3, "16384"),
    ("16,385-row months, no source", None, dict(max_seg_len=16385), -3, "16384"),
]


@pytest.mark.parametrize("what,source,kw,code,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_before_any_hip_call(what, source, kw, code, text):
    """No pointer is ever read and no device is present: each call is refused on its arguments alone."""
    from fmcore import _lib as L
    rc, msg = _rc(L, _args(L, source, **kw))
    assert rc == code and msg.startswith("fm_forecast_compare: ") and text in msg, (what, rc, msg)


def test_limit_itself_and_empty_calls():
    from fmcore import _lib as L
    assert _rc(L, _args(L, None, max_seg_len=16384))[0] == -1     # the limit itself: refused for its source only
    for source in ("vec", "f64", "planes"):
        assert _rc(L, _args(L, source, pairs=[]))[0] == 0, source
        assert _rc(L, _args(L, source, nseg=0))[0] == 0, source
    # the empty calls have no pointers
    a = L.FCmpArgs()
    a.min_count = 1
    assert _rc(L, a)[0] == 0
    a.nseg, a.src.nrows = 5, 100
    assert _rc(L, a)[0] == 0
    assert ctypes.cdll.LoadLibrary(L.LIB_PATH).fm_forecast_compare(None, None) == -1


def _chain_months():
    rng = np.random.default_rng(7)
    lens = np.array([0, 1, 2, 3, 40, 5, 17, 300, 64, 9])
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    Fa = rng.normal(0.01, 0.02, n)
    Fb = 0.6 * Fa + rng.normal(0.0, 0.02, n)
    ret = 2.0 * (Fb - 0.6 * Fa) + rng.normal(0.0, 0.1, n)
    first = int(seg_off[4])                                   # the 1-, 2- and 3-row months stay whole
    Fa[first:][rng.random(n - first) < 0.05] = np.nan
    Fb[first:][rng.random(n - first) < 0.05] = np.nan
    ret[first:][rng.random(n - first) < 0.1] = np.nan
    Fa[int(seg_off[7]) + 3] = np.inf
    ret[int(seg_off[7]) + 5] = -np.inf
    ret[int(seg_off[5]):int(seg_off[6])] = np.nan             # a month without returns
    level = rng.integers(0, 3, n).astype(np.uint8)
    level[:first] = 2
    return seg_off, Fa, Fb, ret, level


def test_restatement_vs_independent_chain():
    """np.corrcoef, np.polyfit and np.linalg.lstsq month by month, under the project's 1e-9 series
    rule; counts, status and the NaN pattern exact."""
    seg_off, Fa, Fb, ret, level = _chain_months()
    T = len(seg_off) - 1
    for min_level in (0, 1):
        got = CO.forecast_compare(seg_off, Fa, Fb, ret, level, min_level)
        exp = np.full((T, 7), np.nan)
        cnt = np.zeros((T, 2), dtype=np.int32)
        for t in range(T):
            s = slice(int(seg_off[t]), int(seg_off[t + 1]))
            ok = np.isfinite(Fa[s]) & np.isfinite(Fb[s]) & (level[s] >= min_level)
            fa, fb, r = Fa[s][ok], Fb[s][ok], ret[s][ok]
            fin = np.isfinite(r)
            cnt[t] = ok.sum(), fin.sum()
            if ok.sum() < 2:
                continue
            slope, icept = np.polyfit(fa, fb, 1)
            e = fb - (icept + slope * fa)
            exp[t, :4] = np.corrcoef(fa, fb)[0, 1], slope, icept, np.std(e, ddof=1)
            if fin.sum() < 2:
                continue
            X = np.column_stack([np.ones(fin.sum()), e[fin]])
            (c0, c1), res, _, _ = np.linalg.lstsq(X, r[fin], rcond=None)
            fit = X @ np.array([c0, c1])
            exp[t, 4:] = c1, c0, 1.0 - np.sum((r[fin] - fit) ** 2) / np.sum((r[fin] - r[fin].mean()) ** 2)
        assert np.array_equal(got["cnt"], cnt) and np.array_equal(got["status"], (cnt[:, 0] >= 2).astype(np.int32))
        assert {0, 1, 2} <= set(cnt[:, 0].tolist()) and (cnt[:, 1] < 2).any() and (cnt[:, 1] < cnt[:, 0]).any()
        two = cnt[:, 0] == 2                                  # two rows: a perfect fit, the chain's residual is noise
        assert two.any() and np.all(np.abs(np.abs(got["rec"][two, 0]) - 1.0) <= 1e-15) and np.all(got["rec"][two, 3] <= 1e-17)
        for c in range(7):
            sel = ~two if c >= 3 else np.ones(T, dtype=bool)
            assert_series_close(got["rec"][sel, c], exp[sel, c], f"level >= {min_level}, rec[:, {c}]")
    got = CO.forecast_compare(seg_off, Fa, Fb, ret, None, 0, min_count=10)
    assert np.array_equal(got["status"], (got["cnt"][:, 0] >= 10).astype(np.int32))
    assert np.isnan(got["rec"][got["status"] == 0]).all() and (got["cnt"][got["status"] == 0, 0] > 0).any()


def test_restatement_degenerate_months():
    """IEEE arithmetic decides: identical forecasts give slope 1.0 and residual sd 0.0 exactly and a NaN
    predictive slope; a constant F_a gives NaN from the slope on, with status 1."""
    rng = np.random.default_rng(8)
    F = rng.normal(size=50)
    r = rng.normal(size=50)
    seg_off = np.array([0, 50])
    same = CO.forecast_compare(seg_off, F, F, r)
    assert same["rec"][0, 1] == 1.0 and same["rec"][0, 3] == 0.0 and same["rec"][0, 0] == 1.0
    assert np.isnan(same["rec"][0, 4:]).all() and same["status"][0] == 1
    const = CO.forecast_compare(seg_off, np.full(50, 0.25), F, r)
    assert np.isnan(const["rec"][0]).all() and const["status"][0] == 1 and list(const["cnt"][0]) == [50, 50]


def test_python_signatures():
    from fmcore import engine as E, lewellen as LW
    from fmdrop import bind, calc_Lewellen_2014 as CL

    def defaults(f):
        return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}

    assert list(inspect.signature(E.forecast_compare).parameters) == \
        ["panel", "coef", "sel", "pairs", "cuts", "ret", "level", "min_count", "forecast_out", "out"]
    assert defaults(E.forecast_compare) == dict(cuts=None, ret="retx", level=None, min_count=1, forecast_out=False, out=None)
    assert list(inspect.signature(E.forecast_compare_vector).parameters) == \
        ["seg_off", "forecast", "ret", "pairs", "level", "min_count", "max_seg_len"]
    assert defaults(E.forecast_compare_vector) == dict(level=None, min_count=1, max_seg_len=None)
    assert defaults(E.forecast_compare_summary) == dict(nw_lags=4)
    assert [f.name for f in dataclasses.fields(E.ForecastCompare)] == ["rec", "cnt", "status", "forecast"]
    fields = dataclasses.fields(LW.PipelineConfig)
    assert fields[-1].name == "rank" and fields[-2].name == "forecast_compare"
    assert fields[-2].default is False and fields[-2].kw_only and LW.PipelineConfig().forecast_compare is False
    assert [f.name for f in dataclasses.fields(LW.PipelineResult)][-3:] == \
        ["forecast_compare", "forecast_compare_summary", "forecast_compare_pairs"]
    p = inspect.signature(CL.forecast_comparison).parameters
    assert list(p) == ["df", "forecast_a", "forecast_b", "return_col", "universe", "date_col", "nw_lags"]
    assert p["return_col"].default == "retx" and p["universe"].default is None and p["nw_lags"].default == 4
    assert list(inspect.signature(CL.build_table_4).parameters) == ["crsp_comp", "variables_dict", "cfg"]
    src = inspect.getsource(bind)   # extensions, like Tables 3 and 5: not bound into the reference's namespace
    assert "build_table_4" not in src and "forecast_comparison" not in src


def test_pair_batches():
    """At most FM_MAX_PAIRS pairs over at most FM_MAX_SORTS distinct forecasts per launch, cut
    greedily in the pairs' order, indices local to the launch's ascending forecast list."""
    from fmcore import engine as E
    pairs = [(2 * i, 2 * i + 1, i % 3) for i in range(12)] + [(0, 1, 0)] * 20
    got, batches = E._pair_batches("t", pairs, 24)
    assert got == pairs and [p0 for p0, _, _ in batches] == [0, 8, 24]
    assert batches[0][2] == list(range(16)) and batches[1][2] == [0, 1] + list(range(16, 24))
    assert len(batches[1][1]) == 16 and batches[2][2] == [0, 1] and len(batches[2][1]) == 8
    for p0, part, js in batches:
        assert [(js[a], js[b], lv) for a, b, lv in part] == pairs[p0:p0 + len(part)]
    assert E._pair_batches("t", [], 3)[1] == [(0, [], [])]
    with pytest.raises(ValueError, match="outside the 3 forecasts"):
        E._pair_batches("t", [(0, 3, 0)], 3)


def test_pipeline_config_rules_need_no_device():
    """forecast_compare needs forecasts=True and excludes standardize=True: refused before any work,
    naming the field."""
    from fmcore import lewellen as LW
    with pytest.raises(ValueError, match="forecast_compare excludes standardize"):
        LW.run_pipeline(None, LW.PipelineConfig(forecast_compare=True, standardize=True))
    with pytest.raises(ValueError, match="forecast_compare needs forecasts"):
        LW.run_pipeline(None, LW.PipelineConfig(forecast_compare=True, forecasts=False))
