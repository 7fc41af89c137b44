"""Plain references and test inputs for the kernels around the regression core:
fm_segment_moments / fm_distinct_count (Table 1), fm_sorted_join / fm_ffill_expand (panel
ETL) and fm_rolling_beta.  numpy, math.fsum and np.longdouble only -- no torch, no project
code -- with loops where a loop is the clearest statement of the definition in
include/fm_hip.h.  tests/test_side_host.py pins every reference to pandas / numpy and shows
that the inputs built here tell plausible wrong variants apart; tests/test_gpu_side.py
compares the kernels with the references on the same inputs.  Each reference takes its
building blocks (eligibility, week start, window sum, ...) as arguments, so that a wrong
variant is the reference with one block swapped."""
import bisect
import math

import numpy as np

RTOL = 1e-9                      # the project's FP64 contract (tests/fmtol.py)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _seg(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ------------------------------------------------------------------------------------------
# fm_segment_moments / fm_distinct_count
# ------------------------------------------------------------------------------------------
def eligible(v, level=None, min_level=0, finite_only=True):
    """Rows that count: level >= min_level (every row without a level), not NaN, and finite
    under finite_only."""
    v = np.asarray(v, dtype=np.float64)
    ok = ~np.isnan(v)
    if level is not None:
        ok &= np.asarray(level).astype(np.int64) >= min_level
    if finite_only:
        ok &= ~np.isinf(v)
    return ok


def _fsum_ld(a):
    """Sum of long doubles: fsum of their FP64 heads plus fsum of the remainders."""
    hi = a.astype(np.float64)
    lo = (a - hi).astype(np.float64)
    return np.longdouble(math.fsum(hi)) + np.longdouble(math.fsum(lo))


def moments(v):
    """(n, mean, sd) of the eligible values v: mean = fsum / n, sd = sqrt(sum of squared
    long-double deviations / (n - 1)); NaN mean for n == 0, NaN sd for n < 2.  With an inf
    among the values (finite_only off) numpy's IEEE result: mean +-inf or NaN, sd NaN."""
    n = len(v)
    if n == 0:
        return 0, np.nan, np.nan
    if not np.isfinite(v).all():
        with np.errstate(invalid="ignore"):
            return n, float(np.sum(v) / n), np.nan
    mean = np.longdouble(math.fsum(v)) / n
    if n < 2:
        return n, float(mean), np.nan
    d = v.astype(np.longdouble) - mean
    return n, float(mean), float(np.sqrt(_fsum_ld(d * d) / (n - 1)))


def segment_moments(X, seg_off, level=None, min_level=0, finite_only=True, eligible=eligible, moments=moments):
    """count int32 [C, T], mean and sd float64 [C, T] of every (column, segment)."""
    C, T = X.shape[0], len(seg_off) - 1
    cnt = np.zeros((C, T), dtype=np.int32)
    mean, sd = np.full((C, T), np.nan), np.full((C, T), np.nan)
    for c in range(C):
        ok = eligible(X[c], level, min_level, finite_only)
        for s in range(T):
            r0, r1 = seg_off[s], seg_off[s + 1]
            cnt[c, s], mean[c, s], sd[c, s] = moments(X[c, r0:r1][ok[r0:r1]])
    return cnt, mean, sd


def moments_mismatches(got, ref):
    """The (column, segment) cells where (count, mean, sd) `got` misses the reference: counts
    equal, NaN / inf positions equal, |mean - ref| <= 1e-9 max(|ref|, sd_ref) (1e-9 |ref|
    where sd_ref is NaN), |sd - ref| <= 1e-9 ref."""
    (gc, gm, gs), (rc, rm, rs) = got, ref
    bad = []
    for idx in np.ndindex(rc.shape):
        ok = gc[idx] == rc[idx]
        for g, r, scale in ((gm[idx], rm[idx], rs[idx]), (gs[idx], rs[idx], 0.0)):
            if np.isfinite(r):
                s = abs(r) if np.isnan(scale) else max(abs(r), scale)
                ok &= bool(np.isfinite(g) and abs(g - r) <= RTOL * s)
            else:
                ok &= bool((np.isnan(g) and np.isnan(r)) or g == r)
        if not ok:
            bad.append((idx, (int(gc[idx]), float(gm[idx]), float(gs[idx])),
                        (int(rc[idx]), float(rm[idx]), float(rs[idx]))))
    return bad


MOMENT_LENS = (0, 1, 2, 255, 256, 257, 511, 513, 1000, 0)
LEVEL_RUNS = ((False, 0), (True, 0), (True, 1), (True, 2), (True, 3))   # (with level, min_level)


def moments_inputs(seed=11):
    """seg_off, X [3, n], level [n].  Column 0: N(0,1) with 5 % NaN.  Column 1: 1e5 + N(0,1)
    (a one-pass variance is off by ~1e-5 there).  Column 2: +inf (segment 3), -inf (4), both
    signs (5), all NaN (6), NaN but one row (7), +inf on level-0 rows only (8)."""
    rng = np.random.default_rng(seed)
    seg_off = _seg(MOMENT_LENS)
    n = int(seg_off[-1])
    X = np.empty((3, n))
    X[0] = rng.normal(size=n)
    X[0][rng.random(n) < 0.05] = np.nan
    X[1] = 1e5 + rng.normal(size=n)
    X[2] = rng.normal(size=n)
    level = rng.integers(0, 3, n).astype(np.uint8)
    seg = lambda s: np.arange(seg_off[s], seg_off[s + 1])  # noqa: E731
    X[2][rng.choice(seg(3), 6, replace=False)] = np.inf
    X[2][rng.choice(seg(4), 6, replace=False)] = -np.inf
    both = rng.choice(seg(5), 12, replace=False)
    X[2][both[:6]], X[2][both[6:]] = np.inf, -np.inf
    level[both[:3]], level[both[6:9]] = 2, 2          # both signs survive every min_level <= 2
    X[2][seg(6)] = np.nan
    X[2][seg(7)] = np.nan
    X[2][seg_off[7] + 100], level[seg_off[7] + 100] = 0.75, 2
    low = seg(8)[level[seg(8)] == 0]
    X[2][low[:5]] = np.inf
    return seg_off, X, level


def distinct_count(ids, X, level=None, min_level=0, finite_only=True, eligible=eligible):
    """Distinct ids among each column's eligible rows -> int32 [C]."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.array([len(set(ids[eligible(x, level, min_level, finite_only)].tolist())) for x in X], dtype=np.int32)


DISTINCT_ID_SETS = {              # name -> (lowest id, id range)
    "range1": (7, 1),
    "range33": (100, 33),         # the bitmap's last word is partial
    "range64": (-64, 64),         # exactly two words
    "negative": (-1000, 40),
    "above2p32": (5 << 33, 100),
}


def distinct_inputs(name, edges, n=3001, seed=5):
    """ids [n], X [4, n], level [n] for DISTINCT_ID_SETS[name].  Columns: 20 % NaN; NaN and
    +-inf; +-inf only; all NaN.  With `edges`, the ids one below and one above the set are
    added on rows that are NaN in every column, so they widen the id range the kernel is
    given and never count."""
    lo, rng_ = DISTINCT_ID_SETS[name]
    rng = np.random.default_rng(seed + len(name))
    ids = lo + rng.integers(0, rng_, n).astype(np.int64)
    X = rng.normal(size=(4, n))
    X[0][rng.random(n) < 0.2] = np.nan
    X[1][rng.random(n) < 0.3] = np.nan
    X[1][rng.random(n) < 0.3] = np.inf
    X[1][rng.random(n) < 0.1] = -np.inf
    X[2][rng.random(n) < 0.5] = np.inf
    X[2][rng.random(n) < 0.2] = -np.inf
    X[3] = np.nan
    level = rng.integers(0, 3, n).astype(np.uint8)
    if rng_ > 1:
        # ids met only under some settings: on level-0 rows, on inf rows
        only_l0, only_inf = lo + rng_ - 1, lo
        ids[ids == only_l0] = lo + 1
        ids[ids == only_inf] = lo + 1
        w = np.flatnonzero(level == 0)[:3]
        ids[w] = only_l0
        w = np.flatnonzero(np.isinf(X[2]) & ~np.isnan(X[0]))[:3]
        ids[w], X[0][w], X[1][w] = only_inf, np.inf, -np.inf
    if edges:
        w = rng.choice(n, 4, replace=False)
        ids[w] = [lo - 1, lo + rng_, lo - 1, lo + rng_]
        X[:, w] = np.nan
        level[w] = 2
    return ids, X, level


def contention_inputs(seed=6):
    """One id on 5,000 rows beside its 31 neighbours of the same bitmap word."""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([np.full(5000, 1000 + 13), 1000 + np.repeat(np.arange(32), 3)]).astype(np.int64)
    ids = rng.permutation(ids)
    X = rng.normal(size=(2, len(ids)))
    X[1][rng.random(len(ids)) < 0.5] = np.nan
    return ids, X


DISTINCT_BIG_N = 4096 * 256 + 300   # one row per thread of the capped grid, then 300 more


def distinct_big_inputs(seed=7):
    """The capped grid's second trip: the last 300 rows carry ids found nowhere else."""
    rng = np.random.default_rng(seed)
    n = DISTINCT_BIG_N
    ids = rng.integers(0, 50000, n).astype(np.int64)
    ids[-300:] = 100000 + 3 * np.arange(300)
    X = rng.normal(size=(2, n))
    X[1][rng.random(n) < 0.5] = np.nan
    X[1][-300:] = np.nan
    X[1][-300::2] = 1.0
    return ids, X


# ------------------------------------------------------------------------------------------
# fm_sorted_join
# ------------------------------------------------------------------------------------------
def _tuples(keys):
    return list(zip(*[np.asarray(k, dtype=np.int64).tolist() for k in keys]))


def join_bounds(left_keys, right_keys, lower=bisect.bisect_left, upper=bisect.bisect_right):
    """lo[i] = right keys lexicographically below left key i, hi[i] = those below or equal.
    Keys: lists of one or two int64 arrays; the right keys sorted lexicographically."""
    lt, rt = _tuples(left_keys), _tuples(right_keys)
    assert rt == sorted(rt)
    lo = np.array([lower(rt, k) for k in lt], dtype=np.int64)
    hi = np.array([upper(rt, k) for k in lt], dtype=np.int64)
    return lo, hi


def join_pairs(left_keys, right_keys):
    """(li, rj) of an inner equality join, by brute force: left rows in order, each with its
    matches in the right frame's order.  The right keys need not be sorted."""
    lt, rt = _tuples(left_keys), _tuples(right_keys)
    pairs = [(i, j) for i, k in enumerate(lt) for j, r in enumerate(rt) if r == k]
    return (np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64))


JOIN_NL = (1, 255, 256, 257, 3000)
JOIN_NR = (1, 2, 1000)
HEAVY_KEY = 4                     # 500 times on the right of an nr = 1,000 case


def join_inputs(nl, nr, two, seed=9):
    """(left keys, sorted right keys) as lists of one or two int64 arrays.  Right keys from
    the alphabet -3 .. 12 (duplicates are common), 7 + 2^32 and 7 + 2^33 beside 7 (differ
    only above bit 32), HEAVY_KEY 500 times, second parts from {-1, 0, 1, 2^40} (pairs equal
    in part 1 that differ in part 2).  INT64 minimum and maximum are on the right for odd nl
    only, so the left's copies match there and fall below / above every right key for even
    nl; the left also holds alphabet misses in between."""
    rng = np.random.default_rng(seed + 7 * nl + nr + 1000 * two)
    part2 = np.array([-1, 0, 1, 1 << 40], dtype=np.int64)
    if nr <= 2:
        r1 = np.array([5, 5 + (1 << 32)][:nr] if nl % 2 else [5] * nr, dtype=np.int64)
        r2 = np.array([0, 1][:nr], dtype=np.int64)
        special = np.array([4, 5, 6, 5 + (1 << 32), I64_MIN, I64_MAX, -5], dtype=np.int64)
    else:
        r1 = np.concatenate([np.full(500, HEAVY_KEY), rng.integers(-3, 13, nr - 500 - 12),
                             [7, 7 + (1 << 32), 7 + (1 << 33), 7 + (1 << 32), -3, -3, 12, 12],
                             [I64_MIN, I64_MIN, I64_MAX, I64_MAX] if nl % 2 else [-2, -1, 0, 1]]).astype(np.int64)
        r2 = part2[rng.integers(0, 4, nr)]
        special = np.array([I64_MIN, I64_MAX, -4, 13, HEAVY_KEY, 7, 7 + (1 << 32), 7 + (1 << 33), 7 + (1 << 34),
                            (1 << 32), -3, 12, -(1 << 32) - 3], dtype=np.int64)
    o = np.lexsort((r2, r1))
    r1, r2 = r1[o], r2[o]
    l1 = np.concatenate([special, r1[rng.integers(0, nr, nl)]])[:nl]
    l2 = np.concatenate([part2[rng.integers(0, 4, len(special))], r2[rng.integers(0, nr, nl)]])[:nl]
    l2[rng.random(nl) < 0.2] = 2          # a second part no right key has
    p = rng.permutation(nl)
    l1, l2 = l1[p], l2[p]
    return ([l1, l2], [r1, r2]) if two else ([l1], [r1])


# ------------------------------------------------------------------------------------------
# fm_ffill_expand
# ------------------------------------------------------------------------------------------
def last_at_or_before(months, m):
    """Index of the last record with month <= m (months ascending; the first qualifies)."""
    j = 0
    for k, v in enumerate(months):
        if v <= m:
            j = k
    return j


def ffill_expand(rec_off, rec_month, out_off, vals, pick=last_at_or_before):
    """out_month int32 [nout], out_src int64 [nout], out_vals [C, nout]: output row i belongs
    to the group g with out_off[g] <= i < out_off[g+1], is month rec_month[rec_off[g]] +
    (i - out_off[g]) and copies the group's last record at or before that month."""
    nout = int(out_off[-1])
    month = np.zeros(nout, dtype=np.int32)
    src = np.zeros(nout, dtype=np.int64)
    for g in range(len(out_off) - 1):
        r0, r1 = int(rec_off[g]), int(rec_off[g + 1])
        for i in range(int(out_off[g]), int(out_off[g + 1])):
            month[i] = rec_month[r0] + (i - out_off[g])
            src[i] = r0 + pick(rec_month[r0:r1].tolist(), int(month[i]))
    return month, src, np.asarray(vals)[:, src]


FFILL_CASES = {                  # name -> (ngroups, nout or None = as planned)
    "g1_255": (1, 255), "g1_256": (1, 256), "g1_257": (1, 257),
    "g2_255": (2, 255), "g2_256": (2, 256), "g2_257": (2, 257),
    "g700": (700, None), "g700_sparse257": (700, 257),
}


def ffill_inputs(name, seed=13):
    """rec_off, rec_month, out_off, vals [3, nrec] with host-planned offsets.  Groups of 1 to
    5 records (a third of them single records; 4 records in the one- and two-group cases) up to 40 months apart, two records in one
    month now and then; each plans its span, cut short or run up to 12 months past its last
    record.  g700 plans zero months for the groups 0, 350, 351 and 699; g700_sparse257 plans
    one month for 257 groups and none for the other 443 (runs of empty groups)."""
    G, nout = FFILL_CASES[name]
    rng = np.random.default_rng(seed + G + (nout or 0))
    nrec = np.where(rng.random(G) < 0.33, 1, rng.integers(2, 6, G)) if G > 2 else np.full(G, 4)
    rec_off = _seg(nrec)
    rec_month = np.zeros(int(rec_off[-1]), dtype=np.int32)
    counts = np.zeros(G, dtype=np.int64)
    for g in range(G):
        gaps = rng.integers(0, 41, nrec[g])
        gaps[rng.random(nrec[g]) < 0.5] = 12
        gaps[0] = 0
        m = 1960 * 12 + int(rng.integers(0, 480)) + np.cumsum(gaps)
        rec_month[rec_off[g]:rec_off[g + 1]] = m
        counts[g] = max(int(m[-1] - m[0]) + 1 + int(rng.integers(-6, 13)), 1)
    if name == "g700":
        counts[[0, 350, 351, 699]] = 0
    elif name == "g700_sparse257":
        counts[:] = 0
        counts[rng.choice(np.arange(1, G - 1), 257, replace=False)] = 1
    elif G == 1:
        counts[0] = nout
    else:
        counts[:] = (100, nout - 100)
    out_off = _seg(counts)
    vals = rng.normal(size=(3, len(rec_month)))
    vals[0][rng.random(len(rec_month)) < 0.2] = np.nan
    vals[1][rng.random(len(rec_month)) < 0.2] = -0.0
    vals[2][::5] = np.inf
    return rec_off, rec_month, out_off, vals


# ------------------------------------------------------------------------------------------
# fm_rolling_beta
# ------------------------------------------------------------------------------------------
WEEK = 7
PREFIX_ROWS = 128                 # a finite window of more rows is a difference of prefix sums
KAPPA_CAP = 1e4


def week_start(d):
    """The Monday on or before day d (days since 1970-01-01, a Thursday)."""
    return d - (d + 3) % 7        # Python's % is never negative


def beta_class(b):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    b = np.asarray(b, dtype=np.float64)
    return np.where(np.isnan(b), 1, np.where(b == np.inf, 2, np.where(b == -np.inf, 3, 0)))


def rolling_beta(day, ri, rm, seg_off, q_seg, q_day0, q_day1, period_weeks, week_start=week_start,
                 last_first=True, window_sum=math.fsum):
    """Per query (firm, month [q_day0, q_day1]): the last Monday S of the month with
    week_start(firm's first day) <= S <= firm's last day and a row in [S, S + 7 period_weeks)
    gives beta = (Sxy - Sx Sy / N) / (Syy - Sy^2 / N) over the window's x = log(1 + ri),
    y = log(1 + rm); NaN without one.  A finite window's four sums are math.fsum's, any other
    window's numpy's IEEE ones (compare the class only).  Returns a dict of per-query arrays:
    beta, kappa (the formula's condition number; NaN unless the window is finite), rows (0 =
    no window), start (S), first (the window starts at the firm's first row), nonfinite,
    skipped (a later Monday of the month had an empty window)."""
    day = np.asarray(day, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        x, y = np.log(np.asarray(ri) + 1.0), np.log(np.asarray(rm) + 1.0)
    fin = np.isfinite(x) & np.isfinite(y)
    xy, yy = x * y, y * y
    span = WEEK * period_weeks
    nq = len(q_seg)
    out = dict(beta=np.full(nq, np.nan), kappa=np.full(nq, np.nan), rows=np.zeros(nq, dtype=np.int64),
               start=np.zeros(nq, dtype=np.int64), first=np.zeros(nq, dtype=bool),
               nonfinite=np.zeros(nq, dtype=bool), skipped=np.zeros(nq, dtype=bool))
    for q in range(nq):
        a, b = int(seg_off[q_seg[q]]), int(seg_off[q_seg[q] + 1])
        if b <= a:
            continue
        d = day[a:b]
        t0, last = week_start(int(d[0])), int(d[-1])
        mondays = list(range(week_start(int(q_day1[q])), int(q_day0[q]) - 1, -WEEK))
        for S in mondays if last_first else mondays[::-1]:
            if S < t0 or S > last:
                continue
            i0 = a + int(np.searchsorted(d, S, side="left"))
            i1 = a + int(np.searchsorted(d, S + span, side="left"))
            if i1 <= i0:
                out["skipped"][q] = True
                continue
            N = float(i1 - i0)
            w = slice(i0, i1)
            out["rows"][q], out["start"][q], out["first"][q] = i1 - i0, S, i0 == a
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                if fin[w].all():
                    sx, sy, sxy, syy = (np.float64(window_sum(v[w].tolist())) for v in (x, y, xy, yy))
                    num, den = sxy - sx * sy / N, syy - sy * sy / N
                    # the kernel differences prefix sums that run from the firm's first row
                    k0 = a if i1 - i0 > PREFIX_ROWS else i0
                    f = fin[k0:i1]
                    A, B = np.abs(xy[k0:i1][f]).sum(), yy[k0:i1][f].sum()
                    out["kappa"][q] = (A + abs(sx * sy) / N) / abs(num) + (B + sy * sy / N) / abs(den)
                else:
                    out["nonfinite"][q] = True
                    sx, sy, sxy, syy = x[w].sum(), y[w].sum(), xy[w].sum(), yy[w].sum()
                    num, den = sxy - sx * sy / N, syy - sy * sy / N
                out["beta"][q] = num / den
            break
    return out


def beta_compare(got, ref):
    """(bad query indices, share of the finite answers set aside for kappa > KAPPA_CAP).
    NaN / +-inf positions exact; finite answers within 1e-9 max(|ref|, RMS of the run's
    finite reference answers) unless set aside."""
    got = np.asarray(got, dtype=np.float64)
    rb = ref["beta"]
    finite = np.isfinite(rb)
    aside = finite & ~(ref["kappa"] <= KAPPA_CAP)
    rms = float(np.sqrt(np.mean(rb[finite] ** 2))) if finite.any() else 0.0
    with np.errstate(invalid="ignore"):
        ok = beta_class(got) == beta_class(rb)
        ok &= ~finite | aside | (np.abs(got - rb) <= RTOL * np.maximum(np.abs(rb), rms))
    return np.flatnonzero(~ok), float(aside.sum()) / max(int(finite.sum()), 1)


BETA_LENS = (0, 1, 7, 8, 9, 255, 256, 257, 1000, 5000)
BETA_PERIODS = (1, 26, 156)


def _month_of(day):
    return np.asarray(day, dtype="datetime64[D]").astype("datetime64[M]")


def beta_inputs(seed=2):
    """day int32 [n], ri, rm [n], seg_off [nseg+1] and the queries q_seg, q_day0, q_day1.
    Market days: business days from 1962-01-01 (day -2,922) with 1 % removed, market
    returns N(0.0004, 0.01), stock returns beta rm + N(0, 0.015).  Firms: BETA_LENS,
    then a firm with a gap of more than 156 weeks that ends its first block mid-month, one
    with NaN returns, one with a -100 % stock return, one with a -100 % market return on a
    row.  The 1,000-row firm starts in the last week of a month (its first window is that
    month's answer).  Queries: every month from two before a firm's first row to two after
    its last; six months on the empty firm."""
    rng = np.random.default_rng(seed)
    cal = np.arange(np.datetime64("1962-01-01"), np.datetime64("1986-01-01"))
    cal = cal[np.is_busday(cal)]
    cal = cal[rng.random(len(cal)) > 0.01]
    mday = cal.astype(np.int64)
    mret = rng.normal(0.0004, 0.01, len(cal))
    # market days whose week is the last to start in its month / that fall on the 9th-14th
    monday = mday - (mday + 3) % 7
    last_week = np.flatnonzero((_month_of(monday) == _month_of(mday)) & (_month_of(monday + 7) != _month_of(mday)))
    mid_month = np.flatnonzero(np.isin((cal - cal.astype("datetime64[M]")).astype(np.int64), np.arange(8, 14)))
    days, ris, rms, lens = [], [], [], []

    def firm(idx, edit=None):
        b = rng.normal(1.0, 0.4)
        r, m = b * mret[idx] + rng.normal(0, 0.015, len(idx)), mret[idx].copy()
        if edit:
            edit(r, m)
        days.append(mday[idx]), ris.append(r), rms.append(m), lens.append(len(idx))

    for L in BETA_LENS:
        if L == 5000:
            s = 0
        elif L == 1000:
            s = int(last_week[np.searchsorted(last_week, rng.integers(0, 3000))])
        else:
            s = int(rng.integers(0, len(cal) - L))
        firm(np.arange(s, s + L))
    e = int(mid_month[np.searchsorted(mid_month, 1500)])        # the gap firm's first block ends here
    s2 = int(np.searchsorted(mday, mday[e] + 1300))
    firm(np.r_[np.arange(e - 299, e + 1), np.arange(s2, s2 + 600)])

    def nans(r, m):
        r[rng.choice(len(r), 6, replace=False)] = np.nan
    firm(np.arange(700, 1600), nans)

    def stock_wipeout(r, m):
        r[len(r) // 2] = -1.0
    firm(np.arange(2000, 2800), stock_wipeout)

    def market_wipeout(r, m):
        m[len(m) // 3] = -1.0
    firm(np.arange(3000, 3700), market_wipeout)

    seg_off = _seg(lens)
    q_seg, q0, q1 = [], [], []
    for f, L in enumerate(lens):
        if L:
            m0, m1 = _month_of(days[f][0]) - 2, _month_of(days[f][-1]) + 2
        else:
            m0, m1 = np.datetime64("1969-10"), np.datetime64("1970-03")
        months = np.arange(m0, m1 + 1)
        q_seg.append(np.full(len(months), f))
        q0.append(months.astype("datetime64[D]").astype(np.int64))
        q1.append((months + 1).astype("datetime64[D]").astype(np.int64) - 1)
    i32 = lambda parts: np.concatenate(parts).astype(np.int32)  # noqa: E731
    return dict(day=i32(days), ri=np.concatenate(ris), rm=np.concatenate(rms), seg_off=seg_off,
                q_seg=i32(q_seg), q_day0=i32(q0), q_day1=i32(q1), gap_firm=len(BETA_LENS))


def beta_reference(inp, period_weeks, **kw):
    return rolling_beta(inp["day"], inp["ri"], inp["rm"], inp["seg_off"], inp["q_seg"], inp["q_day0"],
                        inp["q_day1"], period_weeks, **kw)


def beta_conditions(refs):
    """What the device test needs of its inputs so that it cannot pass by missing the code,
    from the references {period_weeks: dict}: every summation path and the 128 | 129 boundary
    at 26 weeks, one-row and 2..5-row windows at 1 week, prefix-path windows (one at a firm's
    first row) and a long non-finite window at 156 weeks, a month whose last Monday has an
    empty window, a window starting before 1970, unanswered queries.  Raises AssertionError
    naming the first that fails; returns the kappa-exclusion shares."""
    r1, r26, r156 = refs[1], refs[26], refs[156]
    rows = r26["rows"][r26["rows"] > 0]
    assert 128 in rows and 129 in rows, "26 weeks: no 128- or 129-row window"
    assert (rows <= 128).sum() >= 20 and (rows > 128).sum() >= 20, "26 weeks: < 20 windows on a side of 128 | 129"
    assert (rows[(rows >= 8) & (rows <= 128)] % 8 != 0).any(), "26 weeks: every leaf window is a multiple of 8"
    assert (r1["rows"] == 1).any() and np.isnan(r1["beta"][r1["rows"] == 1]).all(), "1 week: one-row windows"
    assert all((r1["rows"] == k).any() for k in (2, 3, 4, 5)), "1 week: windows of 2 to 5 rows"
    long_ = r156["rows"] > PREFIX_ROWS
    assert (long_ & r156["nonfinite"]).any(), "156 weeks: no long window with a non-finite row"
    prefix = long_ & ~r156["nonfinite"]
    assert prefix.sum() >= 200, "156 weeks: < 200 prefix-path windows"
    assert (prefix & r156["first"]).any(), "156 weeks: no prefix-path window at a firm's first row"
    for p, r in refs.items():
        assert (r["skipped"] & (r["rows"] > 0)).any(), f"{p} weeks: no month whose last Monday has an empty window"
        assert ((r["rows"] > 0) & (r["start"] < 0)).any(), f"{p} weeks: no window starting on a negative day"
        assert (r["rows"] == 0).any() and np.isnan(r["beta"][r["rows"] == 0]).all()
    shares = {}
    for p, r in refs.items():
        finite = np.isfinite(r["beta"])
        shares[p] = float((finite & ~(r["kappa"] <= KAPPA_CAP)).sum()) / int(finite.sum())
    return shares
