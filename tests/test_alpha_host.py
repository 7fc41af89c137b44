"""Host-side checks of the portfolio alphas (A18): the binding, fm_portfolio_alpha's argument
refusals (each returns before any launch), the numpy restatement (tests/alpha_oracle.py) against an
independent longdouble computation from the centred normal equations, the Python layers'
signatures and field order, and the PipelineConfig rules."""
import ctypes
import dataclasses
import inspect
import os

import numpy as np
import pytest

import alpha_oracle as AO
from fmtol import series_close


# ---------------------------------------------------------------- binding
def test_binding_has_the_alpha_entry_point():
    from fmcore import _lib as L
    lib = L.load()
    assert "fm_portfolio_alpha" in L.EXPORTED and hasattr(lib, "fm_portfolio_alpha")
    assert lib.fm_struct_size(b"fm_alpha_args") == ctypes.sizeof(L.AlphaArgs) == 168
    assert (L.FM_MAX_FACTORS, L.FM_MAX_ALPHA_MODELS, L.FM_ALPHA_MAX_LAGS, L.FM_ALPHA_MAX_MONTHS, L.FM_ALPHA_NSTAT) == \
        (6, 4, 64, 4096, 4)
    assert L._STRUCTS["fm_alpha_args"] is L.AlphaArgs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fm_hip.h")) as f:
        hdr = f.read()
    assert "fm_portfolio_alpha <- build-defined extension A18" in hdr and "X(fm_alpha_args)" in hdr


FAKE = 4096   # never dereferenced: every call below returns before a launch


def _args(L, **kw):
    a = L.AlphaArgs(rec=FAKE, rec_month=44, rec_sort=44 * 100, rec_row=4, rec_col=1, status=FAKE, st_month=1,
                    st_sort=100, nsel=2, nrow=11, T=100, K=3, M=2, nw_lags=4, factors=FAKE, rf=None, spread_row=10,
                    coef=FAKE, se=FAKE, se_hac=FAKE, stat=FAKE, nobs=FAKE)
    a.model_mask[0], a.model_mask[1] = 0b001, 0b111
    for k, v in kw.items():
        if k == "masks":
            for m, x in enumerate(v):
                a.model_mask[m] = x
        else:
            setattr(a, k, v)
    return a


def test_portfolio_alpha_refuses_bad_arguments_before_any_launch():
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_portfolio_alpha(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    cases = [(None, "null args"), (_args(L, rec=None), "rec"), (_args(L, status=None), "status"),
             (_args(L, factors=None), "factors"), (_args(L, coef=None), "coef"), (_args(L, se=None), "se is"),
             (_args(L, se_hac=None), "se_hac"), (_args(L, stat=None), "stat is"), (_args(L, nobs=None), "nobs"),
             (_args(L, K=0), "K must be 1..6"), (_args(L, K=7, masks=(1, 1)), "K must be 1..6"),
             (_args(L, M=0), "M must be 1..4"), (_args(L, M=5), "M must be 1..4"),
             (_args(L, nw_lags=-1), "nw_lags must be 0..64"), (_args(L, nw_lags=65), "nw_lags must be 0..64"),
             (_args(L, masks=(1, 0)), "model_mask[1] is empty"), (_args(L, masks=(0, 1)), "model_mask[0] is empty"),
             (_args(L, masks=(1, 0b1000)), "model_mask[1]"), (_args(L, K=1, M=1, masks=(0b10,)), "model_mask[0]"),
             (_args(L, nsel=-1), "nsel"), (_args(L, nrow=-1), "nrow"), (_args(L, T=-1), "T must"),
             (_args(L, spread_row=-2), "spread_row")]
    for a, text in cases:
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_portfolio_alpha: ") and text in msg, (text, r, msg)
    # rf is optional, and a mask of all K = 6 factors is in range
    r, msg = rc(_args(L, T=4097))
    assert r == -3 and "4096" in msg, (r, msg)
    assert rc(_args(L, T=4097, rec=None, coef=None))[0] == -3      # the limit comes before the pointers
    assert rc(_args(L, T=4097, K=9))[0] == -1                      # ... and after the ranges
    # empty calls are valid and launch nothing
    for kw in (dict(T=0), dict(nsel=0), dict(nrow=0), dict(T=0, rec=None, status=None, factors=None, coef=None)):
        assert rc(_args(L, **kw))[0] == 0, kw


# ---------------------------------------------------------------- the oracle against longdouble
LD = np.longdouble


def _ld_solve_spd(A, B):
    """Solve A X = B for a symmetric positive definite longdouble A by Cholesky."""
    k = A.shape[0]
    G = np.zeros((k, k), dtype=LD)
    for j in range(k):
        G[j, j] = np.sqrt(A[j, j] - np.sum(G[j, :j] ** 2))
        for i in range(j + 1, k):
            G[i, j] = (A[i, j] - np.sum(G[i, :j] * G[j, :j])) / G[j, j]
    Y = np.zeros(B.shape, dtype=LD)
    for i in range(k):
        Y[i] = (B[i] - G[i, :i] @ Y[:i]) / G[i, i]
    X = np.zeros(B.shape, dtype=LD)
    for i in range(k - 1, -1, -1):
        X[i] = (Y[i] - G[i + 1:, i] @ X[i + 1:]) / G[i, i]
    return X


def longdouble_alpha(d, F, nw_lags):
    """All months used, full rank: the regression from the centred normal equations in longdouble,
    with the sandwich evaluated in the centred basis and mapped back (alpha = dbar - beta'fbar)."""
    d, F = d.astype(LD), F.astype(LD)
    n, k = F.shape
    fbar, dbar = F.sum(axis=0) / n, d.sum() / n
    fc, dc = F - fbar, d - dbar
    A = fc.T @ fc
    Ai = _ld_solve_spd(A, np.eye(k, dtype=LD))
    beta = Ai @ (fc.T @ dc)
    e = dc - fc @ beta
    ee, syy = e @ e, dc @ dc
    s2 = ee / (n - k - 1)
    Xc = np.column_stack([np.ones(n, dtype=LD), fc])
    U = Xc * e[:, None]
    S = U.T @ U
    for l in range(1, min(nw_lags, n - 1) + 1):
        G = U[l:].T @ U[:-l]
        S = S + (LD(1) - LD(l) / LD(nw_lags + 1)) * (G + G.T)
    B = np.zeros((k + 1, k + 1), dtype=LD)
    B[0, 0] = LD(1) / n
    B[1:, 1:] = Ai
    C = np.eye(k + 1, dtype=LD)      # theta = C theta_centred
    C[0, 1:] = -fbar
    V = C @ (B @ S @ B) @ C.T
    Vc = C @ (s2 * B) @ C.T
    coef = np.concatenate([[dbar - beta @ fbar], beta])
    return dict(coef=coef.astype(np.float64), se=np.sqrt(np.diag(Vc)).astype(np.float64),
                se_hac=np.sqrt(np.maximum(np.diag(V), 0)).astype(np.float64),
                stat=np.array([1 - ee / syy, np.sqrt(s2), dbar, np.sqrt(syy / (n - 1))], dtype=np.float64))


def _design(seed, T, K):
    rng = np.random.default_rng(seed)
    F = rng.normal(0.005, 0.04, (T, K))
    d = 0.002 + F @ rng.normal(0.6, 0.4, K) + 0.02 * rng.standard_t(4, T)
    return d, F


@pytest.mark.parametrize("K", [1, 3, 6])
@pytest.mark.parametrize("T", [5, 8, 9, 12, 16, 63, 64, 65, 130, 600, 4096])
def test_oracle_matches_longdouble(T, K):
    """Agreement to 1e-12 under fmtol's rule, except se_hac at n == k + 2: one residual degree of
    freedom, where the meat cancels to rounding (the two differ by about 1e-9 there), so se_hac is
    held to the oracle only from n >= k + 3 on -- in every test of the feature."""
    d, F = _design(T * 10 + K, T, K)
    status = np.ones(T, dtype=np.int32)
    if T < K + 2:
        o = AO.alpha_series(d, status, F, range(K), 4)
        assert o["nobs"] == T and all(np.isnan(o[k]).all() for k in ("coef", "se", "se_hac", "stat"))
        return
    for lags in (0, 4, 12):
        o = AO.alpha_series(d, status, F, range(K), lags)
        x = longdouble_alpha(d, F, lags)
        assert o["nobs"] == T
        for key in ("coef", "se", "stat"):
            assert series_close(o[key], x[key], 1e-12), (key, lags, o[key], x[key])
        if T >= K + 3:
            assert series_close(o["se_hac"], x["se_hac"], 1e-12), (lags, o["se_hac"], x["se_hac"])
        else:
            assert np.all(np.isfinite(o["se_hac"]) & (o["se_hac"] >= 0))


def test_oracle_rules():
    """The valid-month rule, the rank rule and the clamp, on inputs made for each."""
    d, F = _design(1, 40, 3)
    status = np.ones(40, dtype=np.int32)
    status[[3, 4]] = 0
    d[7], d[8], F[9, 1], F[10, 2] = np.nan, np.inf, np.nan, -np.inf
    assert AO.alpha_series(d, status, F, [0], 0)["nobs"] == 36
    assert AO.alpha_series(d, status, F, [0, 1], 0)["nobs"] == 35
    o = AO.alpha_series(d, status, F, [0, 2], 0)
    assert o["nobs"] == 35 and np.isnan(o["coef"][2]) and np.isfinite(o["coef"][[0, 1, 3]]).all()
    # the months used are what a plain regression on the kept rows uses
    keep = np.setdiff1d(np.arange(40), [3, 4, 7, 8, 10])
    o2 = AO.alpha_series(d[keep], np.ones(len(keep), dtype=np.int32), F[keep], [0, 2], 0)
    assert all(np.array_equal(o[k], o2[k], equal_nan=True) for k in ("coef", "se", "se_hac", "stat"))
    # rank: a duplicated and a constant factor refuse the coefficients, not the mean and sd
    for G in (np.column_stack([F[:, 0], F[:, 0]]), np.column_stack([F[:, 0], np.full(40, 0.25)])):
        r = AO.alpha_series(d, status, G, [0, 1], 4)
        assert r["nobs"] == 36 and np.isnan(r["coef"]).all() and np.isnan(r["se"]).all() and np.isnan(r["se_hac"]).all()
        assert np.isnan(r["stat"][:2]).all() and np.isfinite(r["stat"][2:]).all()
        assert np.isfinite(AO.alpha_series(d, status, G, [0], 4)["coef"][:2]).all()
    # n < k + 2: NaN but nobs; a constant dependent series: R2 NaN
    st3 = np.zeros(40, dtype=np.int32)
    st3[[20, 21, 22]] = 1
    r = AO.alpha_series(d, st3, F, [0, 1], 0)
    assert r["nobs"] == 3 and all(np.isnan(r[k]).all() for k in ("coef", "se", "se_hac", "stat"))
    assert np.isfinite(AO.alpha_series(d, st3, F, [0], 0)["coef"][:2]).all()
    r = AO.alpha_series(np.full(40, 0.25), np.ones(40, dtype=np.int32), F[:, :1], [0], 2)
    assert np.isnan(r["stat"][0]) and r["stat"][2] == 0.25 and r["stat"][3] == 0.0 and np.isfinite(r["coef"]).all()
    # the clamp: a negative variance is written as se 0
    assert np.sqrt(np.maximum(np.array([-1e-30, 4.0]), 0.0)).tolist() == [0.0, 2.0]
    # HAC with L = 0 is White's estimator; the lag count is capped at n - 1
    X = np.column_stack([np.ones(36), np.cos(np.arange(36.0))])
    e = np.linspace(-1, 1, 36)
    assert np.allclose(AO.hac_meat(X, e, 0), (X * e[:, None] ** 2).T @ X, rtol=1e-14)
    S64 = AO.hac_meat(X[:5], e[:5], 64)
    S4 = (X[:5] * e[:5, None]).T @ (X[:5] * e[:5, None])
    for l in range(1, 5):
        G = (X[l:5] * e[l:5, None]).T @ (X[:5 - l] * e[:5 - l, None])
        S4 = S4 + (1 - l / 65.0) * (G + G.T)
    assert np.allclose(S64, S4, rtol=1e-14)


# ---------------------------------------------------------------- the Python layers
def test_signatures_and_field_order():
    from fmcore import engine as E
    from fmcore import lewellen as LW
    from fmdrop import bind
    from fmdrop import calc_Lewellen_2014 as CL
    assert [f.name for f in dataclasses.fields(E.PortfolioAlphas)] == ["coef", "se", "se_hac", "stat", "nobs"]
    assert isinstance(E.PortfolioAlphas.tstat, property) and isinstance(E.PortfolioAlphas.tstat_hac, property)
    p = inspect.signature(E.portfolio_alphas).parameters
    assert list(p) == ["ports", "factors", "models", "rf", "nw_lags"]
    assert (p["models"].default, p["rf"].default, p["nw_lags"].default) == (None, None, 0)
    assert E.alpha_model_masks(None, 1) == [1] and E.alpha_model_masks(None, 3) == [1, 7]
    assert E.alpha_model_masks([[2], [0, 2]], 3) == [4, 5]
    for bad, K in (([[]], 3), ([[3]], 3), ([[0, 0]], 3), ([[-1]], 3), ([], 3), ([[0]] * 5, 3)):
        with pytest.raises(ValueError, match="portfolio_alphas"):
            E.alpha_model_masks(bad, K)
    fields = dataclasses.fields(LW.PipelineConfig)
    names = [f.name for f in fields]
    i = names.index("alpha_factors")
    assert names[i:i + 4] == ["alpha_factors", "alpha_models", "alpha_rf", "alpha_nw_lags"]
    assert i + 4 <= names.index("horizon") and names[-1] == "rank"          # in front of horizon
    assert all(f.kw_only and f.default is None for f in fields[i:i + 4])
    rn = [f.name for f in dataclasses.fields(LW.PipelineResult)]
    assert rn.index("portfolio_alphas") + 1 == rn.index("extrapolated")
    assert {f.name: f for f in dataclasses.fields(LW.PipelineResult)}["portfolio_alphas"].default is None
    p = inspect.signature(CL.build_table_alphas).parameters
    assert list(p) == ["crsp_comp", "factors", "rf", "models", "nport", "cfg"]
    assert (p["rf"].default, p["models"].default, p["nport"].default) == (None, None, 10)
    assert CL.ALPHA_COLUMNS == ["alpha", "t", "t_hac", "R2", "nobs"]
    assert "build_table_alphas" not in inspect.getsource(bind)   # an extension, like Tables 3 to 5: not bound


def test_pipeline_config_rules_need_no_device():
    from fmcore import lewellen as LW
    from fmcore import step as ST
    F = np.zeros((30, 3))
    with pytest.raises(ValueError, match="alpha_factors needs portfolios"):
        LW.run_pipeline(None, LW.PipelineConfig(alpha_factors=F))
    with pytest.raises(ValueError, match="alpha_factors excludes horizon=3"):
        LW.run_pipeline(None, LW.PipelineConfig(alpha_factors=F, portfolios=10, horizon=3, lag=3))
    with pytest.raises(ValueError, match="alpha_factors has 30 rows, the panel has 31 months"):
        LW.check_alphas(LW.PipelineConfig(alpha_factors=F, portfolios=10), 31)
    with pytest.raises(ValueError, match="alpha_rf has 29 rows"):
        LW.check_alphas(LW.PipelineConfig(alpha_factors=F, portfolios=10, alpha_rf=np.zeros(29)), 30)
    for bad in (np.zeros(30), np.zeros((30, 7)), np.zeros((30, 0)), np.zeros((30, 2, 2))):
        with pytest.raises(ValueError, match="alpha_factors must be"):
            LW.check_alphas(LW.PipelineConfig(alpha_factors=bad, portfolios=10), 30)
    with pytest.raises(ValueError, match="a model must name distinct factor columns in 0..2"):
        LW.check_alphas(LW.PipelineConfig(alpha_factors=F, portfolios=10, alpha_models=[[0], [3]]), 30)
    for name, v in (("alpha_models", [[0]]), ("alpha_rf", np.zeros(30)), ("alpha_nw_lags", 4)):
        with pytest.raises(ValueError, match=f"{name} needs alpha_factors"):
            LW.check_alphas(LW.PipelineConfig(**{name: v}))
    LW.check_alphas(LW.PipelineConfig())
    LW.check_alphas(LW.PipelineConfig(alpha_factors=F, portfolios=10, alpha_rf=np.zeros(30), alpha_models=[[1, 2]]), 30)
    with pytest.raises(ValueError, match="ShardedStep: cfg.alpha_factors must be None"):
        ST.ShardedStep(None, LW.PipelineConfig(alpha_factors=F, portfolios=10), None)
