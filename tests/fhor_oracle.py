"""Two numpy restatements of fm_forecast_horizon (include/fm_hip.h, extension A17): per month the
monthly forecast F scaled to G = a m + g (F - m) around its cross-sectional mean m, G's mean,
ddof-1 standard deviation and quantiles, and the realised long-horizon return regressed on G.

(a) ``forecast_horizon_exact`` writes the header's fixed summation order out (64-row tiles, the
    wave butterfly, lane sums over the tiles l, l + 64, ..., the butterfly again) and every other
    step as one numpy operation in the header's order: what the device is pinned to bit for bit.
(b) ``forecast_horizon`` is the plain chain -- np.mean, np.std(ddof=1), np.quantile, np.polyfit --
    and knows nothing of the order.  tests/test_fhor_host.py holds (a) to (b).
The reference has no long-horizon extrapolation (the paper's Section 4, second approach)."""
import numpy as np

NREC = 6
_LANES = np.arange(64)


def _butterfly(x):
    """[..., 64] -> [...]: lane l adds the value of lane l ^ 32, then ^ 16, 8, 4, 2, 1."""
    for s in (32, 16, 8, 4, 2, 1):
        x = x + x[..., _LANES ^ s]
    return x[..., 0]


def tile_sum(x):
    """The fixed-order sum of the month's per-row terms ``x`` (rows that do not count hold +0.0)."""
    x = np.asarray(x, dtype=np.float64)
    ntile = max(1, -(-len(x) // 64))
    pad = np.zeros(ntile * 64)
    pad[:len(x)] = x
    tiles = _butterfly(pad.reshape(ntile, 64))
    lanes = np.zeros(64)
    for t0 in range(0, ntile, 64):          # lane l: tile sums l, l + 64, ... in order, from +0.0
        part = tiles[t0:t0 + 64]
        lanes[:len(part)] = lanes[:len(part)] + part
    return _butterfly(lanes)


def _quantile_linear(srt, q, scale):
    """numpy 'linear' quantile of scale(srt) from the two neighbouring order statistics of srt."""
    n = len(srt)
    vi = np.float64(n - 1) * np.float64(q)
    if vi >= n - 1:
        i = j = n - 1
        g = vi + 1.0
    else:
        f = np.floor(vi)
        i, j, g = int(f), int(f) + 1, vi - f
    a, b = scale(srt[i]), scale(srt[j])
    d = b - a
    return b - d * (1.0 - g) if g >= 0.5 else a + d * g


def forecast_horizon_exact(seg_off, F, ret, level_mult, gain, level=None, min_level=0, q=(0.1, 0.9), min_count=1):
    """-> dict(rec [T, 6+nq] float64, cnt [T, 2] int32, status [T] int32, scaled [rows] float64)."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    F, ret = np.asarray(F, dtype=np.float64), np.asarray(ret, dtype=np.float64)
    a, g = np.float64(level_mult), np.float64(gain)
    T, nq = len(seg_off) - 1, len(q)
    rec = np.full((T, NREC + nq), np.nan)
    cnt = np.zeros((T, 2), dtype=np.int32)
    status = np.zeros(T, dtype=np.int32)
    scaled = np.full(len(F), np.nan)
    inE = np.isfinite(F)
    if level is not None:
        inE &= np.asarray(level) >= min_level
    inR = inE & np.isfinite(ret)
    for t in range(T):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        f, r, e, rr = F[s], ret[s], inE[s], inR[s]
        nE, nR = int(e.sum()), int(rr.sum())
        cnt[t] = nE, nR
        if nE < min_count:
            continue
        status[t] = 1
        with np.errstate(all="ignore"):
            m = tile_sum(np.where(e, f, 0.0)) / np.float64(nE)
            base = a * m

            def scale(x):
                d = x - m
                return base + g * d

            G = np.where(e, scale(f), np.nan)
            scaled[s] = G
            mG = tile_sum(np.where(e, G, 0.0)) / np.float64(nE)
            d = G - mG
            ss = tile_sum(np.where(e, d * d, 0.0))
            rec[t, 0] = mG
            if nE > 1:
                rec[t, 1] = np.sqrt(ss / np.float64(nE - 1))
            rec[t, 5] = m
            srt = np.sort(f[e])
            for i, lv in enumerate(q):
                rec[t, NREC + i] = _quantile_linear(srt, lv, scale)
            if nR < 2:
                continue
            mg = tile_sum(np.where(rr, G, 0.0)) / np.float64(nR)
            mr = tile_sum(np.where(rr, r, 0.0)) / np.float64(nR)
            dg, dr = G - mg, r - mr
            Sgg = tile_sum(np.where(rr, dg * dg, 0.0))
            Sgr = tile_sum(np.where(rr, dg * dr, 0.0))
            Srr = tile_sum(np.where(rr, dr * dr, 0.0))
            rec[t, 2] = Sgr / Sgg
            rec[t, 3] = mr - rec[t, 2] * mg
            rec[t, 4] = (Sgr * Sgr) / (Sgg * Srr)
    return dict(rec=rec, cnt=cnt, status=status, scaled=scaled)


def forecast_horizon(seg_off, F, ret, level_mult, gain, level=None, min_level=0, q=(0.1, 0.9), min_count=1):
    """The same outputs from the plain chain; a constant G or a constant return gives the NaN slope
    (and what follows from it) that 0 / 0 gives the definition."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    F, ret = np.asarray(F, dtype=np.float64), np.asarray(ret, dtype=np.float64)
    T, nq = len(seg_off) - 1, len(q)
    rec = np.full((T, NREC + nq), np.nan)
    cnt = np.zeros((T, 2), dtype=np.int32)
    status = np.zeros(T, dtype=np.int32)
    scaled = np.full(len(F), np.nan)
    inE = np.isfinite(F)
    if level is not None:
        inE &= np.asarray(level) >= min_level
    inR = inE & np.isfinite(ret)
    for t in range(T):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        e, rr = inE[s], inR[s]
        f = F[s][e]
        cnt[t] = f.size, int(rr.sum())
        if f.size < min_count:
            continue
        status[t] = 1
        m = np.mean(f)
        G = level_mult * m + gain * (f - m)
        scaled[np.flatnonzero(e) + s.start] = G
        rec[t, 0], rec[t, 5] = np.mean(G), m
        if f.size > 1:
            rec[t, 1] = np.std(G, ddof=1)
        for i, lv in enumerate(q):
            rec[t, NREC + i] = np.quantile(G, lv, method="linear")
        x, y = G[rr[e]], ret[s][rr]
        if x.size < 2 or np.ptp(x) == 0.0:
            continue
        slope, icept = np.polyfit(x - x.mean(), y, 1)
        rec[t, 2] = slope
        rec[t, 3] = icept - slope * x.mean()
        if np.ptp(y) > 0.0:
            rec[t, 4] = np.corrcoef(x, y)[0, 1] ** 2
    return dict(rec=rec, cnt=cnt, status=status, scaled=scaled)


def batch(fn, seg_off, Fs, ret, level_mult, gain, level=None, min_levels=None, q=(0.1, 0.9), min_count=1):
    """``fn`` (one of the two above) for forecasts [nsel, rows] with one min_level each: a leading
    [nsel] dimension."""
    min_levels = [0] * len(Fs) if min_levels is None else min_levels
    outs = [fn(seg_off, F, ret, level_mult, gain, level, lv, q, min_count) for F, lv in zip(Fs, min_levels)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def same_bits(got, exp):
    """Equal NaN masks and equal bits everywhere else (the sign of zero included)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or not np.array_equal(np.isnan(got), np.isnan(exp)):
        return False
    ok = ~np.isnan(exp)
    return bool(np.array_equal(got[ok].view(np.uint64), exp[ok].view(np.uint64)))
