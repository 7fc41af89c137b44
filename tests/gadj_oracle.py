"""numpy restatement of fm_group_adjust (build-defined extension A20; the definition is in
include/fm_hip.h), float64 throughout, and the fixtures of its tests.

Per (column, month, group): n = the eligible rows (value not NaN, 0 <= code < ngroups, level >=
min_level), m = float64(math.fsum(x)) / float64(n), d = x - m, sd = sqrt(float64(math.fsum(d * d)) /
float64(n - 1)).  math.fsum is the correctly rounded sum, so the oracle has no summation order of
its own; a group that holds an infinity is summed by numpy instead (fsum refuses inf - inf), which
gives the IEEE result the definition asks for.  ``pandas_adjust`` restates the plain case (no level,
min_count = 1) a second time through groupby([month, code]).transform."""
import functools
import math

import numpy as np

MODES = ("demean", "mean", "zscore")
U = 2.0 ** -53
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


def _sum(v):
    return np.float64(math.fsum(v)) if np.all(np.isfinite(v)) else np.sum(v)


def group_adjust(seg_off, X, group, ngroups, min_count=1, level=None, min_level=0):
    """-> dict: "demean", "mean", "zscore" [C, n] (the three modes' dst), "gcount" int32, "gmean", "gsd"
    and "gabs" (sum |x| / n, for the tests' error bound), each [C, T, ngroups]."""
    X = np.asarray(X, dtype=np.float64)
    C, n = X.shape
    T, G = len(seg_off) - 1, int(ngroups)
    out = {m: np.full((C, n), np.nan) for m in MODES}
    gcount = np.zeros((C, T, G), dtype=np.int32)
    gmean, gsd, gabs = (np.full((C, T, G), np.nan) for _ in range(3))
    code = np.asarray(group).astype(np.int64)
    has = (code >= 0) & (code < G)
    if level is not None:
        has &= np.asarray(level).astype(np.int64) >= min_level
    need = max(1, int(min_count))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(T):
            a, b = int(seg_off[t]), int(seg_off[t + 1])
            rows = a + np.flatnonzero(has[a:b])
            if len(rows) == 0:
                continue
            rows = rows[np.argsort(code[rows], kind="stable")]
            for idx in np.split(rows, np.flatnonzero(np.diff(code[rows])) + 1):
                g = int(code[idx[0]])
                for c in range(C):
                    x = X[c, idx]
                    e = ~np.isnan(x)
                    x, r = x[e], idx[e]
                    k = len(x)
                    gcount[c, t, g] = k
                    if k == 0:
                        continue
                    m = np.float64(_sum(x)) / np.float64(k)
                    d = x - m
                    sd = np.sqrt(np.float64(_sum(d * d)) / np.float64(k - 1)) if k >= 2 else np.float64(np.nan)
                    gabs[c, t, g] = np.float64(_sum(np.abs(x))) / np.float64(k)
                    gsd[c, t, g] = sd
                    if k < need:
                        continue
                    gmean[c, t, g] = m
                    out["demean"][c, r] = d
                    out["mean"][c, r] = m
                    if k >= 2 and np.isfinite(sd) and sd > 0:
                        out["zscore"][c, r] = d / sd
    return dict(out, gcount=gcount, gmean=gmean, gsd=gsd, gabs=gabs)


def pandas_adjust(seg_off, X, group, ngroups, mode):
    """The plain case (no level, min_count = 1) through pandas -> [C, n]."""
    import pandas as pd
    X = np.asarray(X, dtype=np.float64)
    C, n = X.shape
    month = np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))
    code = np.asarray(group).astype(np.int64)
    has = (code >= 0) & (code < ngroups)
    out = np.full((C, n), np.nan)
    for c in range(C):
        df = pd.DataFrame({"month": month[has], "code": code[has], "x": X[c, has]})
        g = df.groupby(["month", "code"])["x"]
        m = g.transform("mean").to_numpy()
        x = df["x"].to_numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            if mode == "mean":
                v = np.where(np.isnan(x), np.nan, m)
            elif mode == "demean":
                v = x - m
            else:
                sd = g.transform("std").to_numpy()
                v = np.where(np.isfinite(sd) & (sd > 0), (x - m) / sd, np.nan)
        out[c, has] = v
    return out


def per_row(seg_off, group, ngroups, table):
    """table [C, T, G] -> [C, n]: each row's own (month, group) entry, NaN for a row without a group."""
    C = table.shape[0]
    n = int(seg_off[-1])
    month = np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))
    code = np.asarray(group).astype(np.int64)
    has = (code >= 0) & (code < ngroups)
    out = np.full((C, n), np.nan)
    out[:, has] = table[:, month[has], code[has]].astype(np.float64)
    return out


def sum_bound(seg_off, group, ngroups, exp, ref):
    """The forward error bound of DEMEAN / MEAN: 1.01 U ((n + 2) A + 2 |ref|) per row, with n and
    A = sum |x| / n of the row's group (an n-term sum in any order, the division and the subtraction on
    either side)."""
    nn = per_row(seg_off, group, ngroups, exp["gcount"])
    A = per_row(seg_off, group, ngroups, exp["gabs"])
    return 1.01 * U * ((nn + 2) * A + 2 * np.abs(ref))


def table_bound(exp):
    """The same bound for the gmean table's entries."""
    return 1.01 * U * ((exp["gcount"] + 2.0) * exp["gabs"] + 2 * np.abs(exp["gmean"]))


def assert_same_bits(got, exp, what):
    """Equal NaN masks, and equal bits everywhere else (infinities and the sign of zero included)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), (what, "NaN masks differ at", np.argwhere(gn != en)[:8])
    a, b = got[~gn].view(np.uint64), exp[~en].view(np.uint64)
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, (what, len(bad), "values differ, first", got[~gn][bad[:4]], exp[~en][bad[:4]])


def assert_within(got, exp, bound, what):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), (what, "NaN masks differ at", np.argwhere(gn != en)[:8])
    inf = np.isinf(exp)
    assert np.array_equal(got[inf], exp[inf]), (what, "infinities differ")
    ok = ~en & ~inf
    with np.errstate(invalid="ignore"):
        err = np.abs(got[ok] - exp[ok])
    worst = float(np.max(err / bound[ok], initial=0.0, where=bound[ok] > 0))
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert np.all(err <= bound[ok]), (what, worst)


# ------------------------------------------------------------------------------------------------
# The fixtures.  Months of 0, 1, 63, 64, 65, 255, 256, 257, 1000 and 5000 rows: an empty month, every
# tile shape of the kernel (a wave takes 64 rows, a workgroup's four waves 256) and a month of many
# rounds.
# ------------------------------------------------------------------------------------------------
LENS = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 5000]
SEG_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
NROWS = int(SEG_OFF[-1])
NGROUPS = (1, 2, 49, 64, 65, 256)
NCOLS = (1, 3, 17)
OFF_1000, OFF_5000 = int(SEG_OFF[8]), int(SEG_OFF[9])
ONE_GROUP_TILE = OFF_5000 + 128      # 64 rows of code 0: the third tile of the longest month
DISTINCT_TILE = OFF_5000 + 192       # 64 rows of codes 0..63 (mod ngroups): the fourth tile
LAST_TILE_1000 = OFF_1000 + 960      # the 1000-row month's last, partial tile (40 rows)
ROW_PINF, ROW_BOTH = OFF_5000 + 1000, (OFF_5000 + 1001, OFF_5000 + 1002)
NAN_COL, INF_COL = 1, 2


@functools.lru_cache(maxsize=None)
def codes(G, foreign=None):
    """The rows' codes at ngroups = G: uniform over 0..G-1, about 2 % of them "no group" in its four
    spellings (-1, ``foreign`` = G unless given, INT32_MIN, INT32_MAX), one tile of one group, one tile of
    min(G, 64) distinct groups, and (G >= 2) group G - 1 present in the 1000-row month's last tile only."""
    rng = np.random.default_rng(1000 + G)
    c = rng.integers(0, G, NROWS).astype(np.int64)
    bad = np.flatnonzero(rng.random(NROWS) < 0.02)
    c[bad] = np.array([-1, G if foreign is None else foreign, I32_MIN, I32_MAX], dtype=np.int64)[np.arange(len(bad)) % 4]
    c[ONE_GROUP_TILE:ONE_GROUP_TILE + 64] = 0
    c[DISTINCT_TILE:DISTINCT_TILE + 64] = np.arange(64) % G
    if G >= 2:
        head = c[OFF_1000:LAST_TILE_1000]
        head[head == G - 1] = G - 2
        c[LAST_TILE_1000 + 10] = c[LAST_TILE_1000 + 20] = G - 1
    c[ROW_PINF] = 1 % G
    c[ROW_BOTH[0]] = c[ROW_BOTH[1]] = 0
    c = c.astype(np.int32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def int_values():
    """[17, NROWS] integers in +-2^20 (every sum exact in any order: n 2^20 < 2^53), 5 % NaN, column
    NAN_COL all NaN, and in column INF_COL of the longest month a +inf in group 1 (mod G) and both
    infinities in group 0."""
    rng = np.random.default_rng(77)
    X = rng.integers(-(2 ** 20), 2 ** 20 + 1, (max(NCOLS), NROWS)).astype(np.float64)
    X[rng.random(X.shape) < 0.05] = np.nan
    X[NAN_COL] = np.nan
    X[INF_COL, ROW_PINF] = np.inf
    X[INF_COL, ROW_BOTH[0]], X[INF_COL, ROW_BOTH[1]] = np.inf, -np.inf
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def int_expected(G, min_count=1, leveled=False, C=None):
    return group_adjust(SEG_OFF, int_values()[:C], codes(G), G, min_count=min_count,
                        level=levels() if leveled else None, min_level=1)


@functools.lru_cache(maxsize=None)
def levels():
    lv = np.random.default_rng(5).integers(0, 3, NROWS).astype(np.uint8)
    lv.setflags(write=False)
    return lv


REAL_G = 49
REAL_SCALES = (1e-3, 1e-2, 1.0, 10.0, 1e3, 1.0)
CONST_GROUP, CONST_VALUE = 3, 7.25


@functools.lru_cache(maxsize=None)
def real_values():
    """[6, NROWS] normal values, column c with scale REAL_SCALES[c] and mean 5 scales (the last column
    centred), 5 % NaN; in column 0 group CONST_GROUP of the 1000-row month is constant."""
    rng = np.random.default_rng(78)
    C = len(REAL_SCALES)
    X = rng.normal(0.0, 1.0, (C, NROWS))
    for c, s in enumerate(REAL_SCALES):
        X[c] = s * (X[c] + (5.0 if c < C - 1 else 0.0))
    X[rng.random(X.shape) < 0.05] = np.nan
    g = codes(REAL_G)
    X[0, OFF_1000 + np.flatnonzero(g[OFF_1000:OFF_5000] == CONST_GROUP)] = CONST_VALUE
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def real_expected():
    return group_adjust(SEG_OFF, real_values(), codes(REAL_G), REAL_G)
