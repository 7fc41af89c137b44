"""numpy restatement of fm_wls (include/fm_hip.h, build-defined extension A22): the weighted monthly
cross-sections, per month and problem, in float64 and in the kernel's documented semantics -- the row
rule, the clip, the skip rule, the inf bits, the weighted means, the centred moments of the weights
scaled to sum to N, the constant-column rule, the Cholesky pivot rule, b = Sxx^-1 Sxy and the
weighted R2.  Beside it an independent np.longdouble computation from the uncentred normal equations
of [1, x] (tests/test_wls_host.py holds the two together), the parity panels of the GPU tests, and
the chain through the time-series oracles of oracle.fm_oracle.  The reference has no WLS, so this
restatement is what the device is pinned to."""
import functools

import numpy as np

from fmcore import _lib as L
from fmtol import RTOL, assert_series_close
from oracle import fm_oracle as O

REFIT_REL = 1e-6     # fm_solve's: a pivot at or below this part of its diagonal entry is refused
CONST_REL = 1e-20    # S_kk at or below this part of S_kk + N m_k^2: a constant column
# A month counts as ill-conditioned for the comparisons when a pivot falls below this part of its
# diagonal entry: a hundred times the kernel's own limit, so that no compared month sits near the
# decision, and a condition number the RTOL of the comparisons can carry.
WELL_REL = 1e-4
LD = np.longdouble


def clip_month(x, lo, hi):
    """fm_gram's clip: max with lo, then min with hi; a NaN bound is ignored, a NaN x stays NaN."""
    x = np.array(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if lo is not None and not np.isnan(lo):
            x = np.where(x < lo, lo, x)
        if hi is not None and not np.isnan(hi):
            x = np.where(x > hi, hi, x)
    return x


def used_rows(cols, xs, y, w, level, u, s):
    """The rows of slice ``s`` that take part: every column of the model non-NaN, level >= u, the
    weight finite and > 0."""
    ok = np.ones(s.stop - s.start, dtype=bool)
    for c in list(xs) + [y]:
        ok &= ~np.isnan(cols[c][s])
    if level is not None:
        ok &= level[s] >= u
    with np.errstate(invalid="ignore"):
        ok &= np.isfinite(w[s]) & (w[s] > 0)
    return ok


def wls_month(X, yv, w):
    """One month's used rows (already clipped) -> dict(status, N, coef [K+1], r2, mean [K+1], S
    [K+1, K+1], pivot: the smallest Cholesky pivot over its diagonal entry, or NaN)."""
    N, K = X.shape
    K1 = K + 1
    out = dict(status=0, N=N, coef=np.full(K1, np.nan), r2=np.nan, mean=np.full(K1, np.nan),
               S=np.full((K1, K1), np.nan), pivot=np.nan)
    if N < K1:
        out["status"] = L.FM_ST_SKIPPED
        return out
    st = (L.FM_ST_INF_IN_X if np.isinf(X).any() else 0) | (L.FM_ST_INF_IN_Y if np.isinf(yv).any() else 0)
    if st:
        out["status"] = st
        return out
    Z = np.column_stack([X, yv])
    W = w.sum()
    m = (w[:, None] * Z).sum(axis=0) / W
    wt = w * (N / W)
    D = Z - m
    S = (wt[:, None] * D).T @ D
    out["mean"], out["S"] = m, S
    d = np.diag(S)[:K]
    bad = not np.all(d > CONST_REL * (d + N * m[:K] ** 2))
    worst = np.inf
    Lc = np.zeros((K, K))
    for j in range(K):
        if bad:
            break
        piv = S[j, j] - np.sum(Lc[j, :j] ** 2)
        if not S[j, j] > 0.0 or not piv > REFIT_REL * S[j, j]:
            bad = True
            worst = min(worst, piv / S[j, j] if S[j, j] > 0.0 else 0.0)
            break
        worst = min(worst, piv / S[j, j])
        Lc[j, j] = np.sqrt(piv)
        for i in range(j + 1, K):
            Lc[i, j] = (S[i, j] - np.sum(Lc[i, :j] * Lc[j, :j])) / Lc[j, j]
    out["pivot"] = 0.0 if bad and not np.isfinite(worst) else worst
    if bad:
        out["status"] = L.FM_ST_RANK_DEF
        return out
    b = np.linalg.solve(S[:K, :K], S[:K, K])
    out["coef"] = np.concatenate([[m[K] - b @ m[:K]], b])
    out["r2"] = 1.0 - (S[K, K] - b @ S[:K, K]) / S[K, K]
    out["status"] = L.FM_ST_FITTED
    return out


def _ld_solve_spd(A, B):
    k = A.shape[0]
    G = np.zeros((k, k), dtype=LD)
    for j in range(k):
        G[j, j] = np.sqrt(A[j, j] - np.sum(G[j, :j] ** 2))
        for i in range(j + 1, k):
            G[i, j] = (A[i, j] - np.sum(G[i, :j] * G[j, :j])) / G[j, j]
    Y = np.zeros(B.shape, dtype=LD)
    for i in range(k):
        Y[i] = (B[i] - G[i, :i] @ Y[:i]) / G[i, i]
    Xs = np.zeros(B.shape, dtype=LD)
    for i in range(k - 1, -1, -1):
        Xs[i] = (Y[i] - G[i + 1:, i] @ Xs[i + 1:]) / G[i, i]
    return Xs


def wls_longdouble(X, yv, w):
    """The independent check: beta from the weighted normal equations in longdouble, centred at the
    longdouble weighted means (the unscaled weights, no moment block, no pivot rule), the intercept
    mapped back, R2 = 1 - SSR_w / sum(w (y - ybar_w)^2) from the residuals.  -> (coef [K+1], r2)."""
    X, yv, w = X.astype(LD), yv.astype(LD), w.astype(LD)
    W = w.sum()
    xbar, ybar = (w @ X) / W, (w @ yv) / W
    Xc, yc = X - xbar, yv - ybar
    b = _ld_solve_spd((w[:, None] * Xc).T @ Xc, (w[:, None] * Xc).T @ yc)
    e = yc - Xc @ b
    r2 = 1 - (w @ (e * e)) / (w @ (yc * yc))
    return np.concatenate([[ybar - b @ xbar], b]).astype(np.float64), float(r2)


def wls_raw_moments_f64(X, yv, w):
    """What the two passes are for: the same fit from float64 RAW moments (sum w z z' minus the
    product of the first moments).  Loses (mean / sd)^2 of its digits; used only to show that the
    cancellation case has teeth."""
    Z = np.column_stack([X, yv])
    K = X.shape[1]
    W = w.sum()
    g = (w[:, None] * Z).sum(axis=0)
    S = (w[:, None] * Z).T @ Z - np.outer(g, g) / W
    b = np.linalg.solve(S[:K, :K], S[:K, K])
    m = g / W
    return np.concatenate([[m[K] - b @ m[:K]], b])


def fm_wls(cols, seg_off, models, w, level=None, lo=None, hi=None, moments=False):
    """``models`` = [(y, xs, levels), ...] over the panel columns ``cols`` (month-sorted arrays) ->
    dict(problems [(model, level, K)], rec [T, P, pmax+2], status [T, P], moments [T, P, stride] or
    None, pivot [T, P]) laid out as engine.fm_pass_wls lays out its FMResult."""
    T = len(seg_off) - 1
    problems = [(mi, u, len(xs)) for mi, (_, xs, levels) in enumerate(models) for u in levels]
    pmax = max(2, max(K + 1 for _, _, K in problems))
    stride = 1 + (pmax + 1) + (pmax + 1) ** 2
    rec = np.full((T, len(problems), pmax + 2), np.nan)
    status = np.zeros((T, len(problems)), dtype=np.int32)
    mom = np.full((T, len(problems), stride), np.nan) if moments else None
    pivot = np.full((T, len(problems)), np.nan)
    for t in range(T):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        clipped = {}
        for k, (mi, u, K) in enumerate(problems):
            y, xs, _ = models[mi]
            use = used_rows(cols, xs, y, w, level, u, s)
            for c in list(xs) + [y]:
                if c not in clipped:
                    clipped[c] = clip_month(cols[c][s], None if lo is None else lo[c, t], None if hi is None else hi[c, t])
            X = np.column_stack([clipped[c][use] for c in xs]).reshape(int(use.sum()), K)
            o = wls_month(X, clipped[y][use], w[s][use])
            status[t, k] = o["status"]
            pivot[t, k] = o["pivot"]
            rec[t, k, pmax + 1] = o["N"]
            if o["status"] == L.FM_ST_FITTED:
                rec[t, k, :K + 1] = o["coef"]
                rec[t, k, pmax] = o["r2"]
            if moments and o["N"] >= K + 1 and not o["status"] & (L.FM_ST_INF_IN_X | L.FM_ST_INF_IN_Y):
                K1 = K + 1
                mom[t, k, 0] = o["N"]
                mom[t, k, 1:1 + K1] = o["mean"]
                mom[t, k, 1 + K1:1 + K1 + K1 * K1] = o["S"].ravel()
    return dict(problems=problems, rec=rec, status=status, moments=mom, pivot=pivot, pmax=pmax)


def assert_well_conditioned(ref):
    """The input condition of the parity panels, checked on the CPU: every month with N >= K + 1
    and no inf is fitted with every pivot above WELL_REL of its diagonal entry.  So no month is
    left out of a comparison for its conditioning."""
    for k, (_, _, K) in enumerate(ref["problems"]):
        st = ref["status"][:, k]
        solved = (st & (L.FM_ST_SKIPPED | L.FM_ST_INF_IN_X | L.FM_ST_INF_IN_Y)) == 0
        assert (st[solved] == L.FM_ST_FITTED).all(), (k, st)
        assert (ref["pivot"][solved, k] > WELL_REL).all(), (k, ref["pivot"][solved, k].min())


def assert_result_close(got_rec, got_status, got_mom, ref, what=""):
    """N and status exact; every coefficient series, R2 and every moment entry's series within RTOL
    under fmtol's rule."""
    pmax = ref["pmax"]
    assert np.array_equal(got_status, ref["status"]), f"{what}: status"
    assert np.array_equal(got_rec[:, :, pmax + 1], ref["rec"][:, :, pmax + 1]), f"{what}: N"
    for k, (_, _, K) in enumerate(ref["problems"]):
        for c in list(range(K + 1)) + [pmax]:
            assert_series_close(got_rec[:, k, c], ref["rec"][:, k, c], f"{what}: rec[:, {k}, {c}]", RTOL)
        assert np.isnan(got_rec[:, k, K + 1:pmax]).all(), f"{what}: pad of problem {k}"
        if got_mom is not None:
            written = ~np.isnan(ref["moments"][:, k, 0])
            for c in range(1 + (K + 1) + (K + 1) ** 2):
                assert_series_close(got_mom[written, k, c], ref["moments"][written, k, c],
                                    f"{what}: moments[:, {k}, {c}]", RTOL)


# ------------------------------------------------------------------ the parity panels
NCOL = 15                      # column 0 the return, 1 .. 14 the predictors
XS14 = list(range(1, 15))
# the three Table-2 models' sizes (3, 7 and 14 predictors) over three levels, Figure 1's (5) over two
MODELS = [(0, [1, 2, 3], (0, 1, 2)), (0, [1, 2, 3, 4, 5, 6, 7], (0, 1, 2)), (0, XS14, (0, 1, 2)),
          (0, [2, 3, 9, 4, 6], (0, 2))]
EDGE_LENS = [0, 3, 14, 15, 63, 64, 65, 257]   # empty, skipped, K and K + 1 of the widest model, tile edges, several tiles a wave


@functools.lru_cache(maxsize=None)
def parity_panel(seed=11, T=24):
    """About 24 ragged months of up to 300 rows, 15 columns with 2 % NaN, weights like market equity
    (log-normal) and a level byte; the first months have the edge lengths, no NaN and level 2 in every
    row, so the lengths are every problem's N there (the kernel cuts the USED rows into tiles)."""
    rng = np.random.default_rng(seed)
    lens = np.array(EDGE_LENS + list(rng.integers(200, 301, size=T - len(EDGE_LENS))))
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    X = rng.standard_t(5, (NCOL, n)) * (0.5 + 0.1 * np.arange(NCOL))[:, None]
    beta = rng.normal(0.0, 0.02, NCOL - 1)
    X[0] = 0.01 + beta @ X[1:] + 0.1 * rng.standard_t(4, n)
    X[rng.random((NCOL, n)) < 0.02] = np.nan
    for t in range(len(EDGE_LENS)):    # the edge months: no NaN, so the level-0 problems' N is the length
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        X[:, s] = np.where(np.isnan(X[:, s]), 0.25, X[:, s])
    w = np.exp(rng.normal(5.0, 1.5, n))
    level = rng.integers(0, 3, n).astype(np.uint8)
    level[:int(seg_off[len(EDGE_LENS)])] = 2
    return dict(seg_off=seg_off, cols=[np.ascontiguousarray(X[c]) for c in range(NCOL)], w=w, level=level)


# ------------------------------------------------------------------ the long months
# fm_wls stages the used rows in an LDS ring of RING_ROWS rows (five 64-row tiles): a month with more
# used rows than that wraps the ring, gives a wave more than two tiles and keeps the load of one
# 256-row block in flight under the MFMAs of the one before, over many blocks.  Lengths chosen
# around the ring and the blocks: one past the ring, a whole number of blocks, and the 700 / 1,500
# rows of a production-like month, with 2 % NaN, a level byte and a tenth of the weights bad.
RING_ROWS = 320
LONG_LENS = [321, 700, 1536, 1500, 40, 1279]
LONG_MODELS = [(0, [1, 2, 3], (0, 1, 2)), (0, XS14, (0, 2)), (0, [2, 3, 9, 4, 6], (0,))]


@functools.lru_cache(maxsize=None)
def long_panel(seed=23):
    rng = np.random.default_rng(seed)
    seg_off = np.concatenate([[0], np.cumsum(LONG_LENS)]).astype(np.int64)
    n = int(seg_off[-1])
    X = rng.standard_t(5, (NCOL, n)) * (0.5 + 0.1 * np.arange(NCOL))[:, None]
    X[0] = 0.01 + rng.normal(0.0, 0.02, NCOL - 1) @ X[1:] + 0.1 * rng.standard_t(4, n)
    X[rng.random((NCOL, n)) < 0.02] = np.nan
    w = np.exp(rng.normal(5.0, 1.5, n))
    bad = rng.random(n) < 0.1
    w[bad] = rng.choice([np.nan, np.inf, 0.0, -1.0], size=int(bad.sum()))
    level = rng.integers(0, 3, n).astype(np.uint8)
    return dict(seg_off=seg_off, cols=[np.ascontiguousarray(X[c]) for c in range(NCOL)], w=w, level=level)


# ------------------------------------------------------------------ the chain behind the cross-sections
def ts_chain(ref, cols, seg_off, models, w, level, lo, hi, window, min_periods, lag, nw_lags=4):
    """From the restatement's records: per problem the fitted months, the FM summary of every record
    column (mean, NW t-statistic, nobs), the rolling means over the fitted rows and the predictive
    records (weighted slope of y on F = a + b'x with the coefficients of `lag` fitted rows before, its
    weighted R2, N) -- oracle.fm_oracle's rolling_mean and newey_west_mean_se, the weighted fit the
    restatement's own."""
    out = []
    pmax = ref["pmax"]
    for k, (mi, u, K) in enumerate(ref["problems"]):
        y, xs, _ = models[mi]
        months = np.flatnonzero(ref["status"][:, k] & L.FM_ST_FITTED)
        rec = ref["rec"][months, k]
        summ = {}
        for c in list(range(K + 1)) + [pmax, pmax + 1]:
            x = rec[:, c]
            se = O.newey_west_mean_se(x, nw_lags)
            summ[c] = (x.mean(), x.mean() / se, len(x), float(np.sqrt(np.mean(x * x))), se)
        roll = np.column_stack([O.rolling_mean(rec[:, c], window, min_periods) for c in range(K + 1)])
        pred = np.full((len(months), 3), np.nan)
        for i in range(lag, len(months)):
            c = roll[i - lag]
            if np.isnan(c).any():
                continue
            t = months[i]
            s = slice(int(seg_off[t]), int(seg_off[t + 1]))
            use = used_rows(cols, xs, y, w, level, u, s)
            Xc = np.column_stack([clip_month(cols[j][s], lo[j, t], hi[j, t])[use] for j in xs])
            yv = clip_month(cols[y][s], lo[y, t], hi[y, t])[use]
            o = wls_month((c[0] + Xc @ c[1:])[:, None], yv, w[s][use])
            pred[i] = (o["coef"][1], o["r2"], o["N"])
        out.append(dict(months=months, summary=summ, rolling=roll, pred=pred))
    return out


# ------------------------------------------------------------------ the cancellation case
# Predictors whose mean is CANCEL_OFFSET times their standard deviation.  At 1e4 (the issue's figure)
# a float64 raw-moment fit loses about (1e4)^2 * 2^-53 = 1e-8 of its slopes, which already misses
# RTOL = 1e-9 on this panel (tests/test_wls_host.py asserts it), so the offset was not enlarged.
CANCEL_OFFSET = 1e4
CANCEL_MODELS = [(0, [1, 2, 3], (0,)), (0, list(range(1, 8)), (0,))]


@functools.lru_cache(maxsize=None)
def cancel_panel(seed=5, T=6, offset=CANCEL_OFFSET):
    rng = np.random.default_rng(seed)
    lens = rng.integers(250, 301, size=T)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    sd = 0.5 + 0.25 * np.arange(8)
    Z = rng.normal(size=(8, n))
    X = sd[:, None] * (offset + Z)
    X[0] = 0.01 + rng.normal(0.0, 0.05, 7) @ Z[1:] + 0.1 * rng.normal(size=n)
    w = np.exp(rng.normal(5.0, 1.5, n))
    return dict(seg_off=seg_off, cols=[np.ascontiguousarray(X[c]) for c in range(8)], w=w)


def month_design(d, xs, y, t):
    s = slice(int(d["seg_off"][t]), int(d["seg_off"][t + 1]))
    return np.column_stack([d["cols"][c][s] for c in xs]), d["cols"][y][s], d["w"][s]
