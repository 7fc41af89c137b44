"""numpy restatement of fm_portfolio_sort's definition (include/fm_hip.h): a
loop over months with np.quantile, np.searchsorted(side="left") and masked means.  The
reference has no portfolio sort, so this restatement is what the device is pinned to."""
import numpy as np

from oracle import fm_oracle as O


def portfolio_sort(seg_off, F, R, W=None, level=None, nyse=None, nport=10, q=None, min_level=0,
                   nyse_breakpoints=False, min_count=None):
    """-> dict(bp [T, nport-1], port [rows] uint8, rec [T, nport+1, 4], cnt [T, nport] int32,
    status [T] int32)."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    F = np.asarray(F, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    T = len(seg_off) - 1
    q = np.arange(1, nport) / nport if q is None else np.asarray(q, dtype=np.float64)
    min_count = nport if min_count is None else min_count
    bp = np.full((T, nport - 1), np.nan)
    port = np.full(len(F), 255, dtype=np.uint8)
    rec = np.full((T, nport + 1, 4), np.nan)
    cnt = np.zeros((T, nport), dtype=np.int32)
    status = np.zeros(T, dtype=np.int32)
    for t in range(T):
        a, b = int(seg_off[t]), int(seg_off[t + 1])
        f, r = F[a:b], R[a:b]
        elig = np.isfinite(f)
        if level is not None:
            elig &= np.asarray(level[a:b]) >= min_level
        brk = elig & (np.asarray(nyse[a:b]) != 0) if nyse_breakpoints else elig
        if brk.sum() < min_count:
            continue
        status[t] = 1
        bp[t] = np.quantile(f[brk], q)
        p = np.full(b - a, 255, dtype=np.uint8)
        p[elig] = np.searchsorted(bp[t], f[elig], side="left")
        port[a:b] = p
        for k in range(nport):
            m = (p == k) & np.isfinite(r)
            cnt[t, k] = m.sum()
            if m.any():
                rec[t, k, 0] = r[m].mean()
                rec[t, k, 1] = f[m].mean()
            if W is not None:
                w = np.asarray(W[a:b], dtype=np.float64)
                with np.errstate(invalid="ignore"):
                    mw = m & np.isfinite(w) & (w > 0)
                if mw.any():
                    rec[t, k, 2] = np.sum(w[mw] * r[mw]) / np.sum(w[mw])
                    rec[t, k, 3] = np.sum(w[mw] * f[mw]) / np.sum(w[mw])
        rec[t, nport] = rec[t, nport - 1] - rec[t, 0]
    return dict(bp=bp, port=port, rec=rec, cnt=cnt, status=status)


def portfolio_summary(rec, status, nw_lags=4):
    """FM mean, Newey-West s.e. (oracle.fm_oracle.newey_west_mean_se), t and nobs of every
    (portfolio, column) series over the sorted months, NaN entries dropped per series."""
    rec = np.asarray(rec)[np.asarray(status) == 1]
    n1, k = rec.shape[1:]
    mean, se, t = (np.full((n1, k), np.nan) for _ in range(3))
    nobs = np.zeros((n1, k), dtype=np.int32)
    for i in range(n1):
        for c in range(k):
            x = rec[:, i, c]
            x = x[~np.isnan(x)]
            nobs[i, c] = x.size
            if x.size == 0:
                continue
            mean[i, c] = x.mean()
            se[i, c] = O.newey_west_mean_se(x, nw_lags)
            with np.errstate(divide="ignore", invalid="ignore"):
                t[i, c] = mean[i, c] / se[i, c]
    return mean, se, t, nobs


def random_panel(seed=7, T=60, lo=250, hi=300):
    """The random ragged panel of the tests: T months of lo..hi rows."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=T)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    F = rng.normal(0.01, 0.02, n)
    F[rng.random(n) < 0.03] = np.nan
    F[rng.random(n) < 0.002] = np.inf
    R = rng.normal(0.01, 0.15, n)
    R[rng.random(n) < 0.02] = np.nan
    W = np.exp(rng.normal(5.0, 2.0, n))
    W[rng.random(n) < 0.01] = np.nan
    level = rng.integers(0, 3, n).astype(np.uint8)
    nyse = (rng.random(n) < 0.4).astype(np.uint8)
    return dict(seg_off=seg_off, F=F, R=R, W=W, level=level, nyse=nyse)
