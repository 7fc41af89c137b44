"""Host-side checks of the Table-1, ETL and rolling-beta tests (no device needed):
(a) the plain references of tests/side_oracle.py agree with pandas / numpy on the inputs
    the device tests use;
(b) those inputs have power: each plausible wrong variant of a reference -- the reference
    with one building block swapped -- misses the device tests' own comparison on them;
(c) the argument checks that run before any HIP call return the documented codes."""
import bisect
import ctypes
import math

import numpy as np
import pandas as pd
import pytest

import side_oracle as SO


def _codes(seg_off):
    return np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))


def _runs(level):
    for with_level, min_level in SO.LEVEL_RUNS:
        for finite_only in (True, False):
            yield (level if with_level else None), min_level, finite_only


@pytest.fixture(scope="module")
def mom():
    return SO.moments_inputs()


@pytest.fixture(scope="module")
def beta():
    inp = SO.beta_inputs()
    return inp, {p: SO.beta_reference(inp, p) for p in SO.BETA_PERIODS}


# ---------------------------------------------------------------- (a) references vs pandas / numpy
def test_moments_reference_equals_pandas(mom):
    seg_off, X, level = mom
    T = len(seg_off) - 1
    assert tuple(np.diff(seg_off)) == SO.MOMENT_LENS
    for lv, ml, fo in _runs(level):
        ref = SO.segment_moments(X, seg_off, lv, ml, fo)
        V = np.where(np.stack([SO.eligible(x, lv, ml, fo) for x in X]), X, np.nan)
        cnt, mean, sd = (np.zeros((3, T), np.int32), np.full((3, T), np.nan), np.full((3, T), np.nan))
        with np.errstate(invalid="ignore"):
            for c in range(3):
                g = pd.Series(V[c]).groupby(_codes(seg_off))
                a = g.agg(["count", "mean"])
                cnt[c, a.index], mean[c, a.index] = a["count"], a["mean"]
                # pandas' groupby std is undefined with an inf in the group: numpy's two-pass one
                for s in range(T):
                    v = V[c, seg_off[s]:seg_off[s + 1]]
                    v = v[~np.isnan(v)]
                    sd[c, s] = np.std(v, ddof=1) if len(v) > 1 else np.nan
        assert SO.moments_mismatches((cnt, mean, sd), ref) == [], (ml, fo)
    # the edge outputs are in the panel: cnt 0 and 1, +inf, -inf and NaN means without finite_only
    c0, m0, s0 = SO.segment_moments(X, seg_off, None, 0, False)
    assert (c0 == 0).any() and (c0 == 1).any() and np.isnan(s0[c0 == 1]).all() and np.isnan(m0[c0 == 0]).all()
    assert m0[2, 3] == np.inf and m0[2, 4] == -np.inf and np.isnan(m0[2, 5]) and c0[2, 5] == 257
    c3, _, _ = SO.segment_moments(X, seg_off, level, 3, True)
    assert not c3.any()


def test_two_pass_fp64_is_within_the_tolerance():
    """Column 1's mean / sd ratio: a two-pass FP64 sum is far inside 1e-9 of the long-double
    value, a one-pass one far outside (what makes the 1e-9 comparison a test)."""
    rng = np.random.default_rng(1)
    for n in (257, 1000):
        v = 1e5 + rng.normal(size=n)
        _, _, ref = SO.moments(v)
        two = math.sqrt(((v - v.mean()) ** 2).sum() / (n - 1))
        assert abs(two - ref) <= 1e-14 * ref
        assert abs(_one_pass(v)[2] - ref) > 1e-7 * ref


def test_distinct_reference_equals_pandas():
    for name in SO.DISTINCT_ID_SETS:
        for edges in (False, True):
            ids, X, level = SO.distinct_inputs(name, edges)
            lo, rng_ = SO.DISTINCT_ID_SETS[name]
            assert ids.min() == lo - edges and ids.max() == lo + rng_ - 1 + edges
            for lv, ml, fo in _runs(level):
                ref = SO.distinct_count(ids, X, lv, ml, fo)
                exp = [pd.Series(ids[SO.eligible(x, lv, ml, fo)]).nunique() for x in X]
                assert ref.tolist() == exp
                assert ref[3] == 0
            assert SO.distinct_count(ids, X, None, 0, False)[2] == rng_   # every id of the set is met
    ids, X = SO.contention_inputs()
    assert SO.distinct_count(ids, X).tolist() == [32, pd.Series(ids[~np.isnan(X[1])]).nunique()]
    assert len({int(i - ids.min()) >> 5 for i in ids}) == 1             # one bitmap word


def _joint_codes(left, right):
    """Dense lexicographic ranks of the keys of both sides."""
    both = np.stack([np.concatenate([l, r]) for l, r in zip(left, right)], axis=1)
    _, inv = np.unique(both, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return inv[:len(left[0])], inv[len(left[0]):]


@pytest.mark.parametrize("two", [False, True])
def test_join_reference_equals_numpy_and_pandas(two):
    for nl in SO.JOIN_NL:
        for nr in SO.JOIN_NR:
            left, right = SO.join_inputs(nl, nr, two)
            assert len(left[0]) == nl and len(right[0]) == nr
            lo, hi = SO.join_bounds(left, right)
            lc, rc = _joint_codes(left, right)
            assert np.array_equal(lo, np.searchsorted(rc, lc, side="left"))
            assert np.array_equal(hi, np.searchsorted(rc, lc, side="right"))
    # the row pairs of pandas' inner merge, in its order, on an unsorted right frame
    left, right = SO.join_inputs(257, 1000, two)
    p = np.random.default_rng(3).permutation(1000)
    right = [k[p] for k in right]
    names = ["k1", "k2"][:len(left)]
    L = pd.DataFrame(dict(zip(names, left))).assign(li=np.arange(257))
    R = pd.DataFrame(dict(zip(names, right))).assign(rj=np.arange(1000))
    m = pd.merge(L, R, how="inner", on=names)
    li, rj = SO.join_pairs(left, right)
    assert len(li) > 1000 and np.array_equal(li, m["li"]) and np.array_equal(rj, m["rj"])


def test_join_inputs_hold_the_cases():
    for two in (False, True):
        for nl in (256, 257, 3000):
            left, right = SO.join_inputs(nl, 1000, two)
            lo, hi = SO.join_bounds(left, right)
            l1, r1 = left[0], right[0]
            assert (hi - lo).max() >= (100 if two else 500)              # the heavy key
            if nl % 2:    # INT64 minimum and maximum match (one-part keys: both copies)
                assert two or all(((l1 == k) & (hi - lo == 2)).any() for k in (SO.I64_MIN, SO.I64_MAX))
            else:         # below / above every right key
                assert ((lo == 0) & (hi == 0)).any() and ((lo == 1000) & (hi == 1000)).any()
            assert ((lo == hi) & (lo > 0) & (lo < 1000)).any()           # a miss in between
            assert (l1 < 0).any() and (r1 < 0).any()
            assert {7, 7 + (1 << 32), 7 + (1 << 33)} <= set(r1.tolist()) and 7 + (1 << 34) in l1
            assert SO.I64_MIN in l1 and SO.I64_MAX in l1
            assert (SO.I64_MIN in r1) == bool(nl % 2) and (SO.I64_MAX in r1) == bool(nl % 2)
            if two:   # left keys whose first part is on the right with other second parts only
                rt = set(zip(*[k.tolist() for k in right]))
                assert any(a in set(r1.tolist()) and (a, b) not in rt for a, b in zip(*[k.tolist() for k in left]))


def test_ffill_reference_equals_pandas_reindex():
    rec_off, rec_month, out_off, vals = SO.ffill_inputs("g700")
    month, src, out = SO.ffill_expand(rec_off, rec_month, out_off, vals)
    checked = 0
    for g in range(len(rec_off) - 1):
        r0, r1, o0, o1 = rec_off[g], rec_off[g + 1], out_off[g], out_off[g + 1]
        m = rec_month[r0:r1]
        if o1 == o0 or (np.diff(m) <= 0).any():     # reindex needs unique labels
            continue
        want = pd.Series(np.arange(r0, r1), index=m).reindex(np.arange(m[0], m[0] + (o1 - o0)), method="ffill")
        assert np.array_equal(src[o0:o1], want.to_numpy()) and np.array_equal(month[o0:o1], want.index)
        checked += 1
    assert checked > 500
    assert np.array_equal(out.view(np.int64), vals[:, src].view(np.int64))
    assert np.isnan(out[0]).any() and np.signbit(out[1][out[1] == 0]).any() and np.isinf(out[2]).any()
    counts, nrec = np.diff(out_off), np.diff(rec_off)
    assert counts[0] == 0 and counts[350] == 0 and counts[351] == 0 and counts[-1] == 0
    assert (nrec == 1).sum() > 100 and (np.diff(rec_month) > 24).any()
    assert any((np.diff(rec_month[rec_off[g]:rec_off[g + 1]]) == 0).any() for g in range(700))   # two records, one month
    for name, (G, nout) in SO.FFILL_CASES.items():
        ro, _, oo, _ = SO.ffill_inputs(name)
        assert len(ro) - 1 == G and (nout is None or oo[-1] == nout)


def test_beta_reference_equals_numpy_windows(beta):
    """Against oracle/chars_oracle.py's restatement of the polars windows (numpy sums) and
    pandas' drop_duplicates(keep="last") per (firm, month)."""
    from oracle import chars_oracle as CO
    inp, refs = beta
    lens = np.diff(inp["seg_off"])
    firm = np.repeat(np.arange(len(lens)), lens)
    with np.errstate(invalid="ignore", divide="ignore"):
        lri, lrm = np.log(inp["ri"] + 1.0), np.log(inp["rm"] + 1.0)
    qmonth = inp["q_day0"].astype("datetime64[D]").astype("datetime64[M]")
    assert np.array_equal(CO.week_start(inp["day"]), [SO.week_start(int(d)) for d in inp["day"]])
    for p, ref in refs.items():
        f, s, b = CO.rolling_beta_windows(firm, inp["day"], lri, lrm, period_weeks=p)
        w = pd.DataFrame({"f": f, "m": s.astype("datetime64[D]").astype("datetime64[M]"), "beta": b})
        w = w.drop_duplicates(subset=["f", "m"], keep="last")
        q = pd.DataFrame({"f": inp["q_seg"], "m": qmonth}).merge(w, on=["f", "m"], how="left")
        bad, _ = SO.beta_compare(q["beta"].to_numpy(), ref)
        assert bad.size == 0, (p, bad[:5])


def test_beta_inputs_meet_their_conditions(beta):
    inp, refs = beta
    lens = np.diff(inp["seg_off"])
    assert tuple(lens[:len(SO.BETA_LENS)]) == SO.BETA_LENS
    assert inp["day"].min() < -2900 and inp["day"].max() > 0
    gap = inp["day"][inp["seg_off"][inp["gap_firm"]]:inp["seg_off"][inp["gap_firm"] + 1]]
    assert np.diff(gap).max() > 156 * 7
    assert np.isnan(inp["ri"]).sum() >= 3 and (inp["ri"] == -1).sum() == 1 and (inp["rm"] == -1).sum() == 1
    assert (lens[inp["q_seg"]] == 0).sum() >= 3                         # queries on the empty firm
    shares = SO.beta_conditions(refs)
    assert all(s <= 0.02 for s in shares.values()), shares


# ---------------------------------------------------------------- (b) wrong variants are told apart
def _one_pass(v):
    n = len(v)
    if n == 0 or not np.isfinite(v).all():
        return SO.moments(v)
    mean = v.sum() / n
    return n, mean, (math.sqrt(((v * v).sum() - n * mean * mean) / (n - 1)) if n > 1 else np.nan)


def _level_ignored(v, level=None, min_level=0, finite_only=True):
    return SO.eligible(v, None, 0, finite_only)


def _level_strict(v, level=None, min_level=0, finite_only=True):
    return SO.eligible(v, level, min_level + 1, finite_only)


def _inf_counted(v, level=None, min_level=0, finite_only=True):
    return SO.eligible(v, level, min_level, False)


MOMENT_VARIANTS = {"one-pass variance": dict(moments=_one_pass), "level ignored": dict(eligible=_level_ignored),
                   "> for >=": dict(eligible=_level_strict), "inf counted": dict(eligible=_inf_counted)}


@pytest.mark.parametrize("variant", MOMENT_VARIANTS)
def test_moments_inputs_reject(mom, variant):
    seg_off, X, level = mom
    hit = [(ml, fo) for lv, ml, fo in _runs(level)
           if SO.moments_mismatches(SO.segment_moments(X, seg_off, lv, ml, fo, **MOMENT_VARIANTS[variant]),
                                    SO.segment_moments(X, seg_off, lv, ml, fo))]
    assert hit, variant
    if variant == "one-pass variance":      # every run with rows left, by column 1's long segments
        assert len(hit) == 8


@pytest.mark.parametrize("variant", ["level ignored", "> for >=", "inf counted"])
def test_distinct_inputs_reject(variant):
    kw = {k: v for k, v in MOMENT_VARIANTS[variant].items()}
    for name in SO.DISTINCT_ID_SETS:
        if name == "range1":
            continue
        for edges in (False, True):
            ids, X, level = SO.distinct_inputs(name, edges)
            assert any(SO.distinct_count(ids, X, lv, ml, fo, **kw).tolist() != SO.distinct_count(ids, X, lv, ml, fo).tolist()
                       for lv, ml, fo in _runs(level)), (variant, name, edges)
    # rows skipped by a grid without its stride loop, and a bitmap OR that loses updates
    ids, X = SO.distinct_big_inputs()
    full, cut = SO.distinct_count(ids, X), SO.distinct_count(ids[:4096 * 256], X[:, :4096 * 256])
    assert (full - cut).tolist() == [300, 150]


@pytest.mark.parametrize("two", [False, True])
def test_join_inputs_reject_upper_for_lower_bound(two):
    for nl in SO.JOIN_NL:
        for nr in SO.JOIN_NR:
            left, right = SO.join_inputs(nl, nr, two)
            lo, hi = SO.join_bounds(left, right)
            wrong, _ = SO.join_bounds(left, right, lower=bisect.bisect_right)
            if (hi > lo).any():
                assert not np.array_equal(wrong, lo)
            else:
                assert nl == 1
    # a compare of the first part only, or of the low 32 bits only, is told apart too
    left, right = SO.join_inputs(3000, 1000, True)
    lo, hi = SO.join_bounds(left, right)
    lo1, hi1 = SO.join_bounds(left[:1], right[:1])
    assert not np.array_equal(lo, lo1) and not np.array_equal(hi, hi1)
    left, right = SO.join_inputs(3000, 1000, False)
    lo, hi = SO.join_bounds(left, right)
    m = (1 << 32) - 1
    r32 = np.sort(right[0] & m)
    assert not np.array_equal(hi - lo, np.searchsorted(r32, left[0] & m, side="right") -
                              np.searchsorted(r32, left[0] & m, side="left"))


@pytest.mark.parametrize("name", SO.FFILL_CASES)
def test_ffill_inputs_reject_first_record(name):
    rec_off, rec_month, out_off, vals = SO.ffill_inputs(name)
    _, src, out = SO.ffill_expand(rec_off, rec_month, out_off, vals)
    _, wsrc, wout = SO.ffill_expand(rec_off, rec_month, out_off, vals, pick=lambda months, m: 0)
    if name != "g700_sparse257":            # (one month per group there: the first record, or its twin)
        assert not np.array_equal(src, wsrc) and not np.array_equal(out.view(np.int64), wout.view(np.int64))


def _week_start_truncating(d):
    return d - int(math.fmod(d + 3, 7))     # C's %: negative for d < -3


def _two_leaves(v):
    """A window past the 128-row leaf as two leaves of half its rows each: an odd window (129
    rows) loses its last row.  Two leaves that split the rows correctly -- numpy's pairwise
    sum of 129 values -- are within rounding of the reference, as
    test_beta_reference_equals_numpy_windows shows: that is no wrong variant."""
    h = len(v) // 2
    return math.fsum(v) if len(v) <= SO.PREFIX_ROWS else math.fsum(v[:h]) + math.fsum(v[h:2 * h])


@pytest.mark.parametrize("period", SO.BETA_PERIODS)
def test_beta_inputs_reject(beta, period):
    inp, refs = beta
    ref = refs[period]
    bad, _ = SO.beta_compare(SO.beta_reference(inp, period, last_first=False)["beta"], ref)
    assert bad.size > 50, "first instead of last window of the month"
    bad, _ = SO.beta_compare(SO.beta_reference(inp, period, week_start=_week_start_truncating)["beta"], ref)
    assert bad.size > 20 and (inp["q_day0"][bad] < 0).all(), "d % 7 without the negative fix-up"
    bad, _ = SO.beta_compare(SO.beta_reference(inp, period, window_sum=_two_leaves)["beta"], ref)
    if period == 26:
        assert (ref["rows"][bad] == 129).sum() >= 5, "the 129-row window summed as two leaves"
    assert (ref["rows"][bad] > SO.PREFIX_ROWS).all()


# ---------------------------------------------------------------- (c) refusals before any HIP call
def test_argument_checks_need_no_device():
    from fmcore import _lib as L
    lib = L.load()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    EINVAL = -1

    def distinct(id_range, nrows=4, ncols=1):
        return lib.fm_distinct_count(p, nrows, p, 8, ncols, None, 0, 1, 0, id_range, p, p, None)

    assert distinct(0) == EINVAL and b"id range" in lib.fm_last_error()
    assert distinct((1 << 34) + 1) == EINVAL and distinct(-5) == EINVAL
    assert distinct(8, nrows=-1) == EINVAL and distinct(8, ncols=0) == EINVAL and distinct(8, ncols=-1) == EINVAL

    def moments(ncols=1, nseg=1):
        return lib.fm_segment_moments(p, 8, ncols, p, nseg, None, 0, 1, p, p, p, None)

    assert moments(ncols=0) == EINVAL and moments(ncols=-1) == EINVAL and moments(nseg=-1) == EINVAL

    def join(lk2, rk2, nl=4, nr=4):
        return lib.fm_sorted_join(p, lk2, nl, p, rk2, nr, p, p, None)

    assert join(p, None) == EINVAL and b"second key parts" in lib.fm_last_error()
    assert join(None, p) == EINVAL
    assert join(None, None, nl=-1) == EINVAL and join(p, p, nr=-1) == EINVAL
    assert join(None, None, nl=0) == 0 and join(p, p, nl=0, nr=0) == 0      # nothing to do: FM_OK

    def expand(ngroups=1, nout=4, ncols=1, vals=p):
        return lib.fm_ffill_expand(p, p, p, ngroups, nout, vals, 8, ncols, vals, 8, p, p, None)

    assert expand(ngroups=-1) == EINVAL and expand(nout=-1) == EINVAL and expand(ncols=-1) == EINVAL
    assert expand(vals=None) == EINVAL and expand(vals=None, ncols=0, nout=0) == 0

    def beta(n=4, nseg=1, period_days=7, nq=1):
        return lib.fm_rolling_beta(p, p, p, n, p, nseg, period_days, p, p, p, nq, p, p, None)

    assert beta(period_days=0) == EINVAL and beta(period_days=-7) == EINVAL
    assert beta(n=-1) == EINVAL and beta(nseg=-1) == EINVAL and beta(nq=-1) == EINVAL
    assert beta(nq=0) == 0
