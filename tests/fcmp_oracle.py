"""numpy restatement of fm_forecast_compare (include/fm_hip.h, extension A15): per month and pair,
forecast b regressed on forecast a over the rows where both are finite, then the realised return
regressed on that regression's residual, with np.mean and np.sum in the header's operation order.
The reference has no model comparison (paper Table 4), so this restatement -- held to
np.corrcoef / np.polyfit / np.linalg.lstsq by tests/test_fcmp_host.py -- is what the device is
pinned to."""
import numpy as np

NREC = 7


def forecast_compare(seg_off, Fa, Fb, ret, level=None, min_level=0, min_count=1):
    """-> dict(rec [T, 7] float64, cnt [T, 2] int32, status [T] int32) of one pair (b on a)."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    Fa, Fb, ret = (np.asarray(v, dtype=np.float64) for v in (Fa, Fb, ret))
    T = len(seg_off) - 1
    rec = np.full((T, NREC), np.nan)
    cnt = np.zeros((T, 2), dtype=np.int32)
    status = np.zeros(T, dtype=np.int32)
    inE = np.isfinite(Fa) & np.isfinite(Fb)
    if level is not None:
        inE &= np.asarray(level) >= min_level
    inR = inE & np.isfinite(ret)
    for t in range(T):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        fa, fb = Fa[s][inE[s]], Fb[s][inE[s]]
        nE, nR = fa.size, int(inR[s].sum())
        cnt[t] = nE, nR
        if nE < max(min_count, 2):
            continue
        status[t] = 1
        with np.errstate(invalid="ignore", divide="ignore"):
            ma, mb = np.mean(fa), np.mean(fb)
            da, db = fa - ma, fb - mb
            Saa, Sbb, Sab = np.sum(da * da), np.sum(db * db), np.sum(da * db)
            beta = Sab / Saa
            e = db - beta * da
            rec[t, 0] = Sab / np.sqrt(Saa * Sbb)
            rec[t, 1] = beta
            rec[t, 2] = mb - beta * ma
            rec[t, 3] = np.sqrt(np.sum(e * e) / (nE - 1))
            if nR < 2:
                continue
            keep = inR[s][inE[s]]
            e, r = e[keep], ret[s][inR[s]]
            me, mr = np.mean(e), np.mean(r)
            de, dr = e - me, r - mr
            See, Ser, Srr = np.sum(de * de), np.sum(de * dr), np.sum(dr * dr)
            rec[t, 4] = Ser / See
            rec[t, 5] = mr - rec[t, 4] * me
            rec[t, 6] = (Ser * Ser) / (See * Srr)
    return dict(rec=rec, cnt=cnt, status=status)


def forecast_compare_batch(seg_off, Fs, ret, pairs, level=None, min_count=1):
    """The same for ``pairs`` = [(a, b, min_level), ...] over the forecasts ``Fs`` [nsel, rows]: a
    leading [npair] dimension."""
    outs = [forecast_compare(seg_off, Fs[a], Fs[b], ret, level, lv, min_count) for a, b, lv in pairs]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}
