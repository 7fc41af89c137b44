"""numpy restatement of fm_forecast_portfolio_sort and fm_lagged_coef (include/fm_hip.h): the
clipped sequential forecast, the lagged coefficient table and the per-sort call into
port_oracle.portfolio_sort -- plus the pipeline fixture of the end-to-end tests and its expected
Table-5 values from oracle.fm_oracle alone.  The reference has no forecast-sorted portfolios, so
this restatement (and, for the chain, the pandas functions of oracle.fm_oracle) is what the
device is pinned to."""
import functools

import numpy as np

import port_oracle as PO
from oracle import fm_oracle as O


def winsor_cuts(cols, seg_off, lower=1, upper=99, min_count=5):
    """The pipeline's cut tables [C, T] (reference :516-527): numpy 'linear' percentiles of each
    month's non-NaN values, NaN (no clipping) below ``min_count`` values."""
    C, T = len(cols), len(seg_off) - 1
    lo, hi = np.full((C, T), np.nan), np.full((C, T), np.nan)
    for c in range(C):
        for t in range(T):
            v = cols[c][seg_off[t]:seg_off[t + 1]]
            v = v[~np.isnan(v)]
            if v.size >= min_count:
                lo[c, t], hi[c, t] = O.percentile_linear(v, lower), O.percentile_linear(v, upper)
    return lo, hi


def clip_column(x, seg_off, lo, hi):
    """fm_clip of one column: x < lo -> lo, x > hi -> hi; a NaN bound is ignored, NaN stays."""
    out = np.array(x, dtype=np.float64)
    for t in range(len(seg_off) - 1):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        v = out[s]
        with np.errstate(invalid="ignore"):
            if not np.isnan(lo[t]):
                v = np.where(v < lo[t], lo[t], v)
            if not np.isnan(hi[t]):
                v = np.where(v > hi[t], hi[t], v)
        out[s] = v
    return out


def forecast(cols, seg_off, coef, xs, lo=None, hi=None):
    """F = c0, then F = F + c_k * clip(x_k) for k = 1..K in order: every product and every sum
    is one rounded numpy operation.  ``coef`` [T, >= K+1], ``xs`` the predictors' columns."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    month = np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))
    F = np.array(coef[month, 0], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, c in enumerate(xs):
            x = np.asarray(cols[c], dtype=np.float64)
            if lo is not None:
                x = clip_column(x, seg_off, lo[c], hi[c])
            F = F + coef[month, 1 + k] * x
    return F


def lagged_coef(roll, idx, count, problems, lag):
    """out[j, idx[p, i]] = roll[p, i - lag] for the fitted rows i in [lag, count[p]), p =
    problems[j]; every other row NaN."""
    P, T, pmax = roll.shape
    out = np.full((len(problems), T, pmax), np.nan)
    for j, p in enumerate(problems):
        for i in range(lag, int(count[p])):
            out[j, idx[p, i]] = roll[p, i - lag]
    return out


def forecast_portfolio_sort(cols, seg_off, coef, sel, lo=None, hi=None, ret=0, W=None, level=None, nyse=None,
                            nport=10, q=None, nyse_breakpoints=False, min_count=None):
    """-> dict of port_oracle.portfolio_sort's outputs with a leading [nsel] dimension, and the
    forecasts ``F`` [nsel, rows].  ``sel`` = [(xs, min_level), ...], ``coef`` [nsel, T, >= K+1]."""
    outs = []
    for j, (xs, min_level) in enumerate(sel):
        F = forecast(cols, seg_off, coef[j], xs, lo, hi)
        o = PO.portfolio_sort(seg_off, F, cols[ret], W, level, nyse, nport=nport, q=q, min_level=min_level,
                              nyse_breakpoints=nyse_breakpoints, min_count=min_count)
        o["F"] = F
        outs.append(o)
    if not outs:
        return {}
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def universe_levels(me, nyse, seg_off):
    """get_subsets' nested levels: (me >= NYSE 20th) + (me >= NYSE 50th), pandas quantiles."""
    level = np.zeros(len(me), dtype=np.uint8)
    for t in range(len(seg_off) - 1):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        ny = me[s][np.asarray(nyse[s], dtype=bool)]
        a, b = O.pandas_quantile(ny, 0.2), O.pandas_quantile(ny, 0.5)
        with np.errstate(invalid="ignore"):
            level[s] = (me[s] >= a).astype(np.uint8) + (me[s] >= b).astype(np.uint8)
    return level


# ------------------------------------------------------------------ the pipeline fixture
PIPE = dict(T=30, N=334, seed=77, nan_rate=0.02, present_rate=0.9, window=12, min_periods=6, lag=1, nport=5)


def pipeline_columns():
    from fmcore import lewellen as LW
    mc = LW.table2_models()
    return list(dict.fromkeys(["retx"] + [c for xs in mc.values() for c in xs] + LW.FIG1_VARS)), mc


@functools.lru_cache(maxsize=None)
def pipeline_fixture():
    """30 ragged months of 280..320 rows, the 15 pipeline columns, me and the NYSE flag; rows
    sorted by (month, permno) as every consumer sorts them."""
    from fmcore import synth
    a = synth.synth_arrays(PIPE["T"], PIPE["N"], PIPE["seed"], nan_rate=PIPE["nan_rate"],
                           present_rate=PIPE["present_rate"])
    names, mc = pipeline_columns()
    uniq, counts = np.unique(a["month"], return_counts=True)
    seg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert len(uniq) == PIPE["T"] and counts.min() >= 280 and counts.max() <= 320, (counts.min(), counts.max())
    return dict(arrays=a, names=names, model_cols=mc, seg_off=seg_off,
                cols=[np.ascontiguousarray(a[c], dtype=np.float64) for c in names])


@functools.lru_cache(maxsize=None)
def pipeline_expected():
    """Table 5 of the fixture from the oracle alone: oracle.fm_oracle.pipeline_arrays' rolling
    coefficients per (model, universe), numpy forecasts on the winsorized columns, port_oracle.
    -> (keys [(model, level)], dict of arrays with a leading [nsort] dimension)."""
    fx = pipeline_fixture()
    a, names, seg_off, cols = fx["arrays"], fx["names"], fx["seg_off"], fx["cols"]
    T = len(seg_off) - 1
    models = {name: ("retx", xs, (0, 1, 2)) for name, xs in fx["model_cols"].items()}
    ref = O.pipeline_arrays({c: a[c] for c in names}, seg_off, a["me"], a["nyse"].astype(bool), models, None,
                            window=PIPE["window"], min_periods=PIPE["min_periods"])
    lo, hi = winsor_cuts(cols, seg_off)
    level = universe_levels(a["me"], a["nyse"], seg_off)
    keys = [(m, u) for m in fx["model_cols"] for u in (0, 1, 2)]
    pmax = 1 + max(len(xs) for xs in fx["model_cols"].values())
    roll = np.full((len(keys), T, pmax), np.nan)
    idx = np.zeros((len(keys), T), dtype=np.int64)
    count = np.zeros(len(keys), dtype=np.int64)
    for j, key in enumerate(keys):
        r = ref[key]
        n = len(r["month"])
        count[j] = n
        idx[j, :n] = r["month"]
        roll[j, :n, :r["rolling"].shape[1]] = r["rolling"]
    coef = lagged_coef(roll, idx, count, list(range(len(keys))), PIPE["lag"])
    sel = [([names.index(c) for c in fx["model_cols"][m]], u) for m, u in keys]
    exp = forecast_portfolio_sort(cols, seg_off, coef, sel, lo, hi, ret=names.index("retx"), W=a["me"],
                                  level=level, nyse=a["nyse"].astype(np.uint8), nport=PIPE["nport"])
    exp["level"] = level
    return keys, exp
