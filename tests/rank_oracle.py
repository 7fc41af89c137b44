"""Expected values of the per-month rank transform (A13; fm_rank_transform), from pandas:
``Series.groupby(codes).rank(method=..., pct=...)`` for the scales raw and pct, and
``rank() / (count + 1) - 0.5`` from pandas' rank and group count for uniform; a ``level``
mask is applied by setting the ineligible values to NaN first.  ``counting_rank`` is a plain
numpy restatement of the definition in include/fm_hip.h (the two counts `less` and `eq` of
every eligible row), checked against pandas bit for bit in tests/test_rank_host.py."""
import numpy as np
import pandas as pd

METHODS = ("average", "min", "max")
SCALES = ("raw", "pct", "uniform")
COMBOS = [(m, s) for m in METHODS for s in SCALES]


def month_codes(seg_off):
    seg_off = np.asarray(seg_off, dtype=np.int64)
    return np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))


def _masked(x, level, min_level):
    x = np.array(x, dtype=np.float64, copy=True)
    if level is not None:
        x[np.asarray(level) < min_level] = np.nan
    return x


def pandas_rank(x, seg_off, method="average", scale="pct", level=None, min_level=0):
    """One column's expected ranks [n] (float64, NaN for ineligible rows)."""
    g = pd.Series(_masked(x, level, min_level)).groupby(month_codes(seg_off))
    if scale == "raw":
        r = g.rank(method=method)
    elif scale == "pct":
        r = g.rank(method=method, pct=True)
    else:
        r = g.rank(method=method) / (g.transform("count") + 1) - 0.5
    return r.to_numpy(dtype=np.float64)


def pandas_nvalid(x, seg_off, level=None, min_level=0):
    """The months' counts of ranked rows [T] (pandas' group counts; 0 for an empty month)."""
    T = len(seg_off) - 1
    c = pd.Series(_masked(x, level, min_level)).groupby(month_codes(seg_off)).count()
    out = np.zeros(T, dtype=np.int32)
    out[c.index.to_numpy()] = c.to_numpy()
    return out


def counting_rank(x, seg_off, method="average", scale="pct", level=None, min_level=0):
    """The definition restated: per month, over the eligible rows (not NaN, level >=
    min_level), less = #{smaller}, eq = #{equal, itself included}; r = less + (eq + 1) / 2
    (average), less + 1 (min), less + eq (max); raw r, pct r / n, uniform r / (n + 1) - 0.5."""
    x = _masked(x, level, min_level)
    out = np.full(len(x), np.nan)
    for t in range(len(seg_off) - 1):
        v = x[seg_off[t]:seg_off[t + 1]]
        ok = ~np.isnan(v)
        e = v[ok]
        n = len(e)
        if n == 0:
            continue
        less = (e[None, :] < e[:, None]).sum(axis=1).astype(np.float64)
        eq = (e[None, :] == e[:, None]).sum(axis=1).astype(np.float64)   # -0.0 == +0.0
        r = {"average": less + (eq + 1.0) / 2.0, "min": less + 1.0, "max": less + eq}[method]
        y = {"raw": r, "pct": r / n, "uniform": r / (n + 1.0) - 0.5}[scale]
        o = np.full(len(v), np.nan)
        o[ok] = y
        out[seg_off[t]:seg_off[t + 1]] = o
    return out


def assert_same_bits(got, exp, what=""):
    """Bit-exact: equal NaN masks and equal int64 views of the non-NaN outputs."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    exp = np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, f"{what}: shapes {got.shape} vs {exp.shape}"
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), f"{what}: {int((gn != en).sum())} NaN mismatches, first at {np.flatnonzero((gn != en).ravel())[:5]}"
    a, b = got[~gn].view(np.int64), exp[~en].view(np.int64)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (f"{what}: {bad.size} of {a.size} values differ, first at {bad[:5]}: "
                           f"{got[~gn][bad[:5]]!r} vs {exp[~en][bad[:5]]!r}")


def tie_heavy(n, rng, nan_rate=0.05):
    """Tie-heavy values with NaN (payload in the low word too), +-inf and both signed zeros."""
    x = rng.integers(-6, 7, n).astype(np.float64) / 4.0
    x[rng.random(n) < 0.08] = -0.0
    x[rng.random(n) < 0.08] = 0.0
    x[rng.random(n) < 0.03] = np.inf
    x[rng.random(n) < 0.03] = -np.inf
    nan = rng.random(n) < nan_rate
    x[nan] = np.nan
    xi = x.view(np.uint64)
    w = np.flatnonzero(nan)
    xi[w[::3]] = np.uint64(0x7FF0000000001234)    # NaNs told apart from +-inf by their low word only
    xi[w[1::3]] = np.uint64(0xFFF0000000000001)
    return x
