"""numpy restatement of fm_portfolio_alpha (include/fm_hip.h, build-defined extension A18): the
time-series regression of each forecast-sorted portfolio's monthly return on factor returns, in
float64 with numpy's lstsq on the uncentred design [1, f] and the HAC sum written lag by lag as the
definition states it.  The valid-month rule, the rank rule (Cholesky pivots of the centred
cross-products against 1e-10 of the diagonal) and the clamp of a negative HAC variance are stated
as the header states them.  The reference has no such table, so this restatement is what the
device is pinned to; tests/test_alpha_host.py holds it against an independent longdouble
computation."""
import numpy as np

from fmcore import _lib as L
from fmtol import RTOL, assert_series_close

NSTAT = L.FM_ALPHA_NSTAT     # R2, s, mean, sd
PIVOT_TOL = 1e-10
OUTS = ("coef", "se", "se_hac", "stat", "nobs")


def used_months(d, status, F, cols):
    return (np.asarray(status) == 1) & np.isfinite(d) & np.isfinite(F[:, cols]).all(axis=1)


def min_pivot_ratio(f):
    """Cholesky of the centred cross-products A in ascending factor order: the smallest pivot (A_jj
    minus the squares of its row of the factor so far) over A_jj met up to the first one the rank
    rule refuses; 0.0 for a diagonal entry that is 0."""
    fc = f - f.sum(axis=0) / len(f)
    A = fc.T @ fc
    k = A.shape[0]
    Lc = np.zeros((k, k))
    worst = np.inf
    for j in range(k):
        if A[j, j] == 0.0:
            return 0.0
        piv = A[j, j] - np.sum(Lc[j, :j] ** 2)
        worst = min(worst, piv / A[j, j])
        if not piv > PIVOT_TOL * A[j, j]:
            return worst
        Lc[j, j] = np.sqrt(piv)
        for i in range(j + 1, k):
            Lc[i, j] = (A[i, j] - np.sum(Lc[i, :j] * Lc[j, :j])) / Lc[j, j]
    return worst


def full_rank(f):
    """The rank rule: refused when a diagonal entry A_jj is 0 or a pivot is <= 1e-10 * A_jj."""
    return min_pivot_ratio(f) > PIVOT_TOL


def hac_meat(X, e, nw_lags):
    """S = sum e_t^2 x_t x_t' + sum_{l=1..min(L, n-1)} (1 - l/(L+1)) sum_t e_t e_{t-l} (x_t x_{t-l}' + x_{t-l} x_t')."""
    n = len(e)
    U = X * e[:, None]
    S = U.T @ U
    for l in range(1, min(int(nw_lags), n - 1) + 1):
        G = U[l:].T @ U[:-l]
        S = S + (1.0 - l / (nw_lags + 1.0)) * (G + G.T)
    return S


def alpha_series(d, status, F, cols, nw_lags):
    """One series, one model (``cols``: its factor columns, ascending) -> dict of coef / se / se_hac
    [K+1], stat [4] and nobs."""
    K = F.shape[1]
    cols = sorted(int(c) for c in cols)
    k = len(cols)
    out = dict(coef=np.full(K + 1, np.nan), se=np.full(K + 1, np.nan), se_hac=np.full(K + 1, np.nan),
               stat=np.full(NSTAT, np.nan), nobs=0, pivot=np.nan)
    with np.errstate(invalid="ignore"):
        use = used_months(d, status, F, cols)
    n = int(use.sum())
    out["nobs"] = n
    if n < k + 2:
        return out
    dd, f = d[use], F[use][:, cols]
    dbar = dd.sum() / n
    syy = float(np.sum((dd - dbar) ** 2))
    out["stat"][2] = dbar
    out["stat"][3] = np.sqrt(syy / (n - 1))
    out["pivot"] = min_pivot_ratio(f)     # for the tests' input conditions
    if not out["pivot"] > PIVOT_TOL:
        return out
    X = np.column_stack([np.ones(n), f])
    theta = np.linalg.lstsq(X, dd, rcond=None)[0]
    e = dd - X @ theta
    ee = float(e @ e)
    s2 = ee / (n - k - 1)
    XtXi = np.linalg.inv(X.T @ X)
    slots = [0] + [1 + c for c in cols]
    out["coef"][slots] = theta
    out["se"][slots] = np.sqrt(s2 * np.diag(XtXi))
    v = np.diag(XtXi @ hac_meat(X, e, nw_lags) @ XtXi)
    out["se_hac"][slots] = np.sqrt(np.maximum(v, 0.0))
    out["stat"][0] = np.nan if syy == 0.0 else 1.0 - ee / syy
    out["stat"][1] = np.sqrt(s2)
    return out


def portfolio_alphas(rec, status, F, models, rf=None, nw_lags=0):
    """``rec`` [S, T, nrow, 4] (or [T, nrow, 4]), ``status`` [S, T] (or [T]), ``F`` [T, K], ``models``
    a list of factor-column lists, ``rf`` [T] or None (not subtracted from the last row, the spread)
    -> dict of arrays with the leading dimensions [S, nrow, 2, M] (or [nrow, 2, M])."""
    single = rec.ndim == 3
    if single:
        rec, status = rec[None], np.asarray(status)[None]
    S, T, nrow, _ = rec.shape
    K, M = F.shape[1], len(models)
    out = dict(coef=np.full((S, nrow, 2, M, K + 1), np.nan), se=np.full((S, nrow, 2, M, K + 1), np.nan),
               se_hac=np.full((S, nrow, 2, M, K + 1), np.nan), stat=np.full((S, nrow, 2, M, NSTAT), np.nan),
               nobs=np.zeros((S, nrow, 2, M), dtype=np.int32), pivot=np.full((S, nrow, 2, M), np.nan))
    for j in range(S):
        for p in range(nrow):
            for w in range(2):
                d = np.array(rec[j, :, p, 2 * w], dtype=np.float64)
                if rf is not None and p != nrow - 1:
                    with np.errstate(invalid="ignore"):
                        d = d - rf
                for m, cols in enumerate(models):
                    o = alpha_series(d, status[j], F, cols, nw_lags)
                    for key in out:
                        out[key][j, p, w, m] = o[key]
    if single:
        out = {key: v[0] for key, v in out.items()}
    return out


def assert_alphas_close(got, exp, models, what=""):
    """NaN patterns and nobs exact; numbers under fmtol's rule at RTOL with the RMS of the compared
    array as the scale.  se_hac is compared where n >= k + 3; at n == k + 2 (one residual degree of
    freedom, where the meat cancels to rounding) it only has to be finite and >= 0."""
    assert np.array_equal(got["nobs"], exp["nobs"]), f"{what}: nobs"
    for key in ("coef", "se"):   # the alphas and the loadings differ in size: each under its own scale
        assert_series_close(got[key][..., 0], exp[key][..., 0], f"{what}: {key}[alpha]", RTOL)
        assert_series_close(got[key][..., 1:], exp[key][..., 1:], f"{what}: {key}[factors]", RTOL)
    for c in range(NSTAT):
        assert_series_close(got["stat"][..., c], exp["stat"][..., c], f"{what}: stat[{c}]", RTOL)
    ks = np.array([len(c) for c in models])
    thin = exp["nobs"] == ks + 2                       # [..., M] by broadcasting over the last axis
    g, e = got["se_hac"].copy(), exp["se_hac"].copy()
    assert np.array_equal(np.isnan(g), np.isnan(e)), f"{what}: se_hac NaN pattern"
    gt = g[thin]
    assert np.all(np.isnan(gt) | (np.isfinite(gt) & (gt >= 0.0))), f"{what}: se_hac at n == k + 2"
    g[thin], e[thin] = 0.0, 0.0
    assert_series_close(g[..., 0], e[..., 0], f"{what}: se_hac[alpha]", RTOL)
    assert_series_close(g[..., 1:], e[..., 1:], f"{what}: se_hac[factors]", RTOL)
