"""Host-side checks of the weighted cross-sections (A22): the binding and fm_wls's argument refusals
(each returns before any launch), the numpy restatement (tests/wls_oracle.py) against an independent
longdouble computation and against numpy's lstsq on sqrt(w)-scaled rows, the input conditions the
GPU tests rely on (no compared month is ill-conditioned; the cancellation case defeats a float64
raw-moment fit), and the rules of the Python layers that need no device."""
import ctypes
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import wls_oracle as WO
from fmtol import RTOL, assert_series_close, series_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the ABI
def test_binding_and_header():
    from fmcore import _lib as L
    lib = L.load()
    assert "fm_wls" in L.EXPORTED and hasattr(lib, "fm_wls")
    assert lib.fm_struct_size(b"fm_wls_args") == ctypes.sizeof(L.WlsArgs) == 144
    assert L._STRUCTS["fm_wls_args"] is L.WlsArgs
    with open(os.path.join(ROOT, "include", "fm_hip.h")) as f:
        header = f.read()
    assert "fm_wls          <- build-defined extension A22; no reference line" in header
    assert "X(fm_wls_args)" in header
    assert "#define FM_WLS_MAX_COLS 15\n" in header and L.FM_WLS_MAX_COLS == 15
    body = header[header.index("typedef struct fm_wls_args {"):header.index("} fm_wls_args;")]
    fields = re.findall(r"^\s+(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
    assert fields == [n for n, _ in L.WlsArgs._fields_] and len(fields) == 21


FAKE = 1 << 24   # never dereferenced: every call below returns before a launch
POINTERS = ("cols", "seg_off", "weight", "prob_level", "prob_z", "prob_nz", "rec", "status")


def _args(L, **kw):
    a = L.WlsArgs(col_stride=100, nrows=100, ncols=15, nseg=4, nprob=3, pmax=15, mom_stride=0)
    for i, name in enumerate(POINTERS):
        setattr(a, name, FAKE * (i + 1))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refuses_bad_arguments_before_any_launch():
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_wls(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    cases = [(None, "null args")]
    cases += [(_args(L, ncols=v), "ncols must be 1..15") for v in (0, -1, 16, 31)]     # more than 15 columns
    cases += [(_args(L, pmax=v), "pmax must be 1..15") for v in (0, 16)]
    cases += [(_args(L, nseg=-1), "negative"), (_args(L, nprob=-1), "negative"), (_args(L, nrows=-1), "negative")]
    cases += [(_args(L, nprob=65536), "65,535")]
    cases += [(_args(L, **{name: None}), "null pointer") for name in POINTERS]       # cols NULL: a planes-only panel
    cases += [(_args(L, col_stride=99), "col_stride")]
    cases += [(_args(L, lo=FAKE), "lo and hi"), (_args(L, hi=FAKE), "lo and hi")]
    cases += [(_args(L, moments=FAKE, mom_stride=1 + 16 + 256 - 1), "mom_stride")]
    for a, text in cases:
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_wls: ") and text in msg, (text, r, msg)
    for kw in (dict(nseg=0), dict(nprob=0), dict(nseg=0, cols=None, weight=None, rec=None)):
        assert rc(_args(L, **kw))[0] == 0, kw


# ---------------------------------------------------------------- the restatement
def _months(d, models, level=None):
    """Every (month, problem) of a panel whose restatement is fitted: (X, y, w) of the used rows."""
    for mi, (y, xs, levels) in enumerate(models):
        for u in levels:
            for t in range(len(d["seg_off"]) - 1):
                s = slice(int(d["seg_off"][t]), int(d["seg_off"][t + 1]))
                use = WO.used_rows(d["cols"], xs, y, d["w"], level, u, s)
                if use.sum() >= len(xs) + 1:
                    yield (mi, u, t), np.column_stack([d["cols"][c][s][use] for c in xs]), d["cols"][y][s][use], \
                        d["w"][s][use]


@pytest.fixture(scope="module")
def parity_ref():
    d = WO.parity_panel()
    return d, WO.fm_wls(d["cols"], d["seg_off"], WO.MODELS, d["w"], d["level"], moments=True)


def test_parity_panel_is_what_the_gpu_tests_need(parity_ref):
    from fmcore import _lib as L
    d, ref = parity_ref
    WO.assert_well_conditioned(ref)     # zero months left out for their conditioning
    lens = np.diff(d["seg_off"])
    assert list(lens[:8]) == WO.EDGE_LENS and lens.max() <= 300 and len(lens) == 24
    pmax, st = ref["pmax"], ref["status"]
    assert pmax == 15 and len(ref["problems"]) == 11
    wide = [k for k, (_, _, K) in enumerate(ref["problems"]) if K == 14]
    assert (st[:2] == L.FM_ST_SKIPPED).all() and (st[2, wide] == L.FM_ST_SKIPPED).all()      # 0, 3 and K rows
    assert (st[3, wide] == L.FM_ST_FITTED).all() and (ref["rec"][3, wide, pmax + 1] == 15).all()   # N == K + 1
    assert [int(ref["rec"][t, 0, pmax + 1]) for t in range(8)] == WO.EDGE_LENS   # the used rows' tile edges
    assert (st[8:] == L.FM_ST_FITTED).all()
    assert np.isnan(np.concatenate(d["cols"])).mean() > 0.01


def test_long_panel_wraps_the_ring():
    """The input conditions of the long-month GPU tests: used-row counts past the kernel's 320-row
    ring (so its indices wrap, more than three times over), every solved month well-conditioned."""
    from fmcore import _lib as L
    d = WO.long_panel()
    ref = WO.fm_wls(d["cols"], d["seg_off"], WO.LONG_MODELS, d["w"], d["level"], moments=True)
    WO.assert_well_conditioned(ref)
    assert (ref["status"][[0, 1, 2, 3, 5]] == L.FM_ST_FITTED).all()
    N = ref["rec"][:, :, ref["pmax"] + 1]
    assert list(np.diff(d["seg_off"])) == WO.LONG_LENS
    assert N[:, 0].max() > 3 * WO.RING_ROWS and (N[[1, 2, 3, 5], 0] > WO.RING_ROWS).all()   # K = 3, level 0
    wide = [k for k, (_, _, K) in enumerate(ref["problems"]) if K == 14]
    assert (N[[2, 3], wide[0]] > 2 * WO.RING_ROWS).all()                                     # the 16-wide rows too
    assert N[0, 0] < WO.RING_ROWS < WO.LONG_LENS[0] and N[4].max() < 64                      # and months that do not
    assert ref["status"][4, wide[1]] == L.FM_ST_SKIPPED and ref["status"][4, wide[0]] == L.FM_ST_FITTED
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(d["w"]) & (d["w"] > 0))
    assert 0.05 < bad.mean() < 0.15 and np.isnan(np.concatenate(d["cols"])).mean() > 0.01


def test_restatement_matches_longdouble_and_lstsq(parity_ref):
    d, ref = parity_ref
    pmax = ref["pmax"]
    at = {(mi, u): k for k, (mi, u, _) in enumerate(ref["problems"])}
    T = len(d["seg_off"]) - 1
    ld = np.full_like(ref["rec"], np.nan)
    ls = np.full_like(ref["rec"], np.nan)
    for (mi, u, t), X, yv, w in _months(d, WO.MODELS, d["level"]):
        k, K = at[mi, u], X.shape[1]
        ld[t, k, :K + 1], ld[t, k, pmax] = WO.wls_longdouble(X, yv, w)
        r = np.sqrt(w)
        ls[t, k, :K + 1] = np.linalg.lstsq(r[:, None] * np.column_stack([np.ones(len(yv)), X]), r * yv, rcond=None)[0]
    for k, (_, _, K) in enumerate(ref["problems"]):
        for c in range(K + 1):
            assert_series_close(ref["rec"][:, k, c], ld[:, k, c], f"longdouble rec[:, {k}, {c}]", RTOL)
            assert_series_close(ref["rec"][:, k, c], ls[:, k, c], f"lstsq rec[:, {k}, {c}]", RTOL)
        assert_series_close(ref["rec"][:, k, pmax], ld[:, k, pmax], f"longdouble R2[{k}]", RTOL)
    assert np.isfinite(ld[3:, :, 0]).all() and T == 24


def test_restatement_semantics():
    """The rules one by one on a small month: bad weights drop rows, the skip rule, the inf bits, the
    three degenerate designs, the moment block's scaling, and the weights' scale invariance."""
    from fmcore import _lib as L
    rng = np.random.default_rng(2)
    n = 40
    X = rng.normal(size=(n, 3))
    yv = 0.1 + X @ [0.5, -0.2, 0.3] + 0.05 * rng.normal(size=n)
    w = np.exp(rng.normal(size=n))
    o = WO.wls_month(X, yv, w)
    assert o["status"] == L.FM_ST_FITTED and o["N"] == n
    D = np.column_stack([X, yv]) - o["mean"]
    assert np.allclose(o["S"], (w[:, None] * D).T @ D * n / w.sum(), rtol=1e-12, atol=0)
    o2 = WO.wls_month(X, yv, w * 2.0 ** -7)
    assert o2["coef"].tobytes() == o["coef"].tobytes() and o2["S"].tobytes() == o["S"].tobytes()
    assert WO.wls_month(X[:3], yv[:3], w[:3])["status"] == L.FM_ST_SKIPPED
    assert WO.wls_month(X[:4], yv[:4], w[:4])["status"] == L.FM_ST_FITTED      # N == K + 1 is kept
    Xi = X.copy()
    Xi[5, 1] = np.inf
    assert WO.wls_month(Xi, yv, w)["status"] == L.FM_ST_INF_IN_X
    yi = yv.copy()
    yi[7] = -np.inf
    assert WO.wls_month(X, yi, w)["status"] == L.FM_ST_INF_IN_Y
    for bad in (np.column_stack([X[:, 0], 2 * X[:, 0], X[:, 2]]), np.column_stack([X[:, 0], np.zeros(n), X[:, 2]]),
                np.column_stack([X[:, 0], np.full(n, 3.7), X[:, 2]])):
        r = WO.wls_month(bad, yv, w)
        assert r["status"] == L.FM_ST_RANK_DEF and np.isnan(r["coef"]).all() and np.isnan(r["r2"])
    cols = [yv] + [X[:, j] for j in range(3)]
    wb = w.copy()
    wb[[0, 3, 9, 11]] = [np.nan, np.inf, 0.0, -1.0]
    use = WO.used_rows(cols, [1, 2, 3], 0, wb, None, 0, slice(0, n))
    assert use.sum() == n - 4 and not use[[0, 3, 9, 11]].any()


def test_cancellation_case_has_teeth():
    """Predictors with mean 1e4 times their standard deviation: the restatement (centred, as the
    kernel's two passes) meets RTOL against the longdouble check, a float64 raw-moment fit does not."""
    d = WO.cancel_panel()
    assert WO.CANCEL_OFFSET == 1e4
    T = len(d["seg_off"]) - 1
    for y, xs, _ in WO.CANCEL_MODELS:
        A, B, C = (np.zeros((T, len(xs) + 1)) for _ in range(3))
        for t in range(T):
            X, yv, w = WO.month_design(d, xs, y, t)
            assert np.all(np.abs(X.mean(axis=0)) > 0.9e4 * X.std(axis=0))   # the sample figures scatter about 1e4
            o = WO.wls_month(X, yv, w)
            A[t], B[t], C[t] = o["coef"], WO.wls_longdouble(X, yv, w)[0], WO.wls_raw_moments_f64(X, yv, w)
        for c in range(len(xs) + 1):
            assert_series_close(A[:, c], B[:, c], f"restatement coef {c}", RTOL)
        assert not any(series_close(C[:, c], B[:, c], RTOL) for c in range(1, len(xs) + 1))


# ---------------------------------------------------------------- the Python layers
def test_config_rules_and_signatures():
    from fmcore import engine as E
    from fmcore import lewellen as LW
    from fmcore import step as ST
    from fmdrop import calc_Lewellen_2014 as CL
    from fmdrop import regressions as RG
    fields = dataclasses.fields(LW.PipelineConfig)
    names = [f.name for f in fields]
    f = {x.name: x for x in fields}["wls_weights"]
    assert f.kw_only and f.default is None and LW.PipelineConfig().wls_weights is None
    assert names[-1] == "rank"                                                   # rank is still the trailing field
    assert names.index("wls_weights") == names.index("double_sort_conditional") + 1
    assert names.index("wls_weights") < names.index("forecast_dist")
    with pytest.raises(ValueError, match="wls_weights excludes standardize"):
        LW.run_pipeline(None, LW.PipelineConfig(wls_weights="me", standardize=True))
    with pytest.raises(ValueError, match="ShardedStep: cfg.wls_weights must be None"):
        ST.ShardedStep(None, LW.PipelineConfig(wls_weights="me"), None)
    # a planes-only panel is refused before any device work
    planes_only = E.DevicePanel(cols=None, names=["a"], seg_off=None, seg_off_h=np.zeros(1, dtype=np.int64), planes=object())
    with pytest.raises(ValueError, match="planes-only"):
        LW.check_wls(LW.PipelineConfig(wls_weights="me"), planes_only)
    with pytest.raises(ValueError, match="planes-only"):
        E.fm_pass_wls(planes_only, [])
    # the 15-column limit is the panel's, checked before any device work; horizon > 1 adds a column
    def fake(ncols):
        return E.DevicePanel(cols=np.zeros((ncols, 0)), names=[f"c{i}" for i in range(ncols - 1)] + ["retx"],
                             seg_off=None, seg_off_h=np.zeros(1, dtype=np.int64))
    LW.check_wls(LW.PipelineConfig(wls_weights="me"), fake(15))
    LW.check_wls(LW.PipelineConfig(wls_weights="me", horizon=3, lag=3), fake(14))
    with pytest.raises(ValueError, match="at most 15 columns, this one has 16"):
        LW.check_wls(LW.PipelineConfig(wls_weights="me"), fake(16))
    with pytest.raises(ValueError, match="horizon=3 adds the k-month return"):
        LW.check_wls(LW.PipelineConfig(wls_weights="me", horizon=3, lag=3), fake(15))
    LW.check_wls(LW.PipelineConfig(horizon=3, lag=3), fake(16))            # off: no rule
    p = inspect.signature(E.fm_pass_wls).parameters
    assert list(p) == ["panel", "models", "weight", "level", "nlevels", "cuts", "shift", "moments"]
    assert (p["weight"].default, p["level"].default, p["nlevels"].default, p["moments"].default) == (None, None, 1, False)
    # the drop-in: one more keyword at the end, off by default
    p = inspect.signature(RG.run_monthly_cs_regressions).parameters
    assert list(p) == ["df", "return_col", "predictor_cols", "date_col", "weight_col"] and p["weight_col"].default is None
    p = inspect.signature(CL.build_table_2).parameters
    assert list(p) == ["subsets_comp_crsp", "variables_dict", "weight_col"] and p["weight_col"].default is None
    assert LW.PipelineConfig(**dict(wls_weights="me", portfolios=5)).wls_weights == "me"   # what a **cfg passes on


def test_inf_months_raise_like_the_ols_path():
    from fmcore import _lib as L
    from fmcore import api
    api.raise_like_reference_wls(np.array([L.FM_ST_FITTED, L.FM_ST_SKIPPED, L.FM_ST_RANK_DEF, L.FM_ST_INF_IN_Y]))
    with pytest.raises(api.MissingDataError, match="exog contains inf or nans"):
        api.raise_like_reference_wls(np.array([L.FM_ST_FITTED, L.FM_ST_INF_IN_X]))
    # months that are not fitted (RANK_DEF among them) are absent from the frame
    rec = np.arange(3 * 5, dtype=np.float64).reshape(3, 5)
    frame = api.cs_frame(np.array([10, 11, 12]), rec, np.array([L.FM_ST_FITTED, L.FM_ST_RANK_DEF, L.FM_ST_FITTED]), 3,
                         ["a", "b"], "m")
    assert list(frame["m"]) == [10, 12] and list(frame.columns) == ["m", "N", "R2", "slope_a", "slope_b"]
