"""numpy restatement of fm_forecast_dist (include/fm_hip.h, extension A14): per month the count,
mean, ddof-1 standard deviation and numpy 'linear' quantiles of the eligible forecasts.  The
reference has no such statistics (paper Table 3's univariate properties), so this restatement --
held to the pandas chain by tests/test_fdist_host.py -- is what the device is pinned to."""
import numpy as np


def forecast_dist(seg_off, F, level=None, min_level=0, q=(0.1, 0.9), min_count=1):
    """-> dict(rec [T, 2+nq] float64, cnt [T] int32, status [T] int32) of one forecast vector."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    F = np.asarray(F, dtype=np.float64)
    T, nq = len(seg_off) - 1, len(q)
    rec = np.full((T, 2 + nq), np.nan)
    cnt = np.zeros(T, dtype=np.int32)
    status = np.zeros(T, dtype=np.int32)
    ok = np.isfinite(F)
    if level is not None:
        ok &= np.asarray(level) >= min_level
    for t in range(T):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        f = F[s][ok[s]]
        cnt[t] = f.size
        if f.size < min_count:
            continue
        status[t] = 1
        rec[t, 0] = f.mean()
        if f.size > 1:
            rec[t, 1] = f.std(ddof=1)
        for i, lv in enumerate(q):
            rec[t, 2 + i] = np.quantile(f, lv, method="linear")
    return dict(rec=rec, cnt=cnt, status=status)


def forecast_dist_batch(seg_off, Fs, level=None, min_levels=None, q=(0.1, 0.9), min_count=1):
    """The same for forecasts [nsel, rows] with one min_level each: a leading [nsel] dimension."""
    min_levels = [0] * len(Fs) if min_levels is None else min_levels
    outs = [forecast_dist(seg_off, F, level, lv, q, min_count) for F, lv in zip(Fs, min_levels)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}
