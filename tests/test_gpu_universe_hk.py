"""get_subsets' NYSE breakpoints on 32-bit high-word keys (universe_month / hk_select).

Every case runs through both launches that hold universe_month -- E.universe (fm_universe:
universe_kernel<8 | 20 | 32 | 64> by the panel's longest month) and
E.select_cuts(..., universe=(0.2, 0.5)) (the select fix-up's launch for months of <= 5,120
rows) -- and compares the breakpoints bit for bit with oracle.fm_oracle.pandas_quantile over
the month's NYSE non-NaN `me`, the level bytes with (me >= a) + (me >= b), NaN False.

The shapes are the smallest at which the path can go wrong: months whose located bin
overflows the candidate list (the block-uniform fallback to the 64-bit histogram select),
keys at the ends of the order (negatives, both zeros, subnormals, +-inf), the widest key
range, month lengths around the wave / workgroup / register-budget edges, months with 0, 1
and 2 NYSE values, and the bench panel.  CROWD is above every list capacity the path can
be built with (64, 128 or 256 keys)."""
import numpy as np
import pytest

from oracle import fm_oracle as O

pytestmark = pytest.mark.gpu

CROWD = 300


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _same(a, b):
    """Bit-exact up to NaN payloads: same NaN positions, same values, same sign of zeros."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return np.array_equal(a[m], b[m]) and np.array_equal(np.signbit(a[m]), np.signbit(b[m]))


def _hi_words(x):
    return (np.asarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def _expected(x, m):
    v = x[m & ~np.isnan(x)]
    ea = O.pandas_quantile(v, 0.2) if v.size else np.nan
    eb = O.pandas_quantile(v, 0.5) if v.size else np.nan
    with np.errstate(invalid="ignore"):
        lev = (x >= ea).astype(np.uint8) + (x >= eb).astype(np.uint8)
    return ea, eb, lev


def _check(E, segs, masks):
    """Months `segs` (me) / `masks` (NYSE) as one panel, through both launches; returns the
    oracle's breakpoints [(a, b)] per month."""
    rng = np.random.default_rng(len(segs))
    me = np.concatenate(segs)
    ny = np.concatenate(masks).astype(np.uint8)
    labels = np.repeat(np.arange(len(segs)), [len(x) for x in segs])
    panel = E.panel_from_arrays([rng.standard_normal(me.size)], ["x"], labels, me=me, nyse=ny)
    assert np.array_equal(panel.order, np.arange(me.size))
    exp = [_expected(x, m.astype(bool)) for x, m in zip(segs, masks)]
    off = panel.seg_off_h
    runs = (("fm_universe", E.universe(panel)),
            ("fm_select_universe", E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY, universe=(0.2, 0.5))[1]))
    for name, (a, b, level) in runs:
        a, b, level = a.cpu().numpy(), b.cpu().numpy(), level.cpu().numpy()
        for t, (ea, eb, lev) in enumerate(exp):
            assert _same([a[t]], [ea]) and _same([b[t]], [eb]), (name, t, a[t], ea, b[t], eb)
            assert np.array_equal(level[off[t]:off[t + 1]], lev), (name, t)
    return [(ea, eb) for ea, eb, _ in exp]


def _with_others(rng, nyse_vals, n_other):
    """A month of the NYSE values plus n_other non-NYSE lognormal rows (5 % NaN), shuffled."""
    other = np.exp(rng.normal(5, 2, n_other))
    other[rng.random(n_other) < 0.05] = np.nan
    x = np.concatenate([nyse_vals, other])
    m = np.concatenate([np.ones(len(nyse_vals), dtype=bool), np.zeros(n_other, dtype=bool)])
    p = rng.permutation(x.size)
    return x[p], m[p]


def test_low_word_only_differences(E):
    """3,000 NYSE values 1000 + i 2^-30 share one high word (the located bin is one high word
    wide and over capacity: the 64-bit fallback); then two high words only, half near 1.0 and
    half near 2.0 (the median's two ranks are the last key of one word and the first of the
    other)."""
    rng = np.random.default_rng(801)
    one = 1000.0 + np.arange(3000) * 2.0 ** -30
    assert np.unique(one).size == 3000 and np.unique(_hi_words(one)).size == 1
    two = np.concatenate([1.0 + np.arange(1500) * 2.0 ** -40, 2.0 + np.arange(1500) * 2.0 ** -40])
    assert np.unique(two).size == 3000 and np.unique(_hi_words(two)).size == 2
    segs, masks = zip(_with_others(rng, one, 500), _with_others(rng, two, 500),
                      _with_others(rng, one[:1800], 200))   # <= 2,048 rows on its own below
    _check(E, segs, masks)
    _check(E, segs[2:], masks[2:])


@pytest.mark.parametrize("n", [1900, 4000])
def test_exact_ties_straddle_each_quantile(E, n):
    """More than the list capacity of equal values around rank 0.2 (n - 1) and around rank
    0.5 (n - 1), distinct values elsewhere (n = 1,900: months of <= 2,048 rows)."""
    rng = np.random.default_rng(802 + n)
    ia, ib = int(0.2 * (n - 1)), int(0.5 * (n - 1))
    v = np.sort(np.exp(rng.normal(5, 2, n)))
    assert np.unique(v).size == n
    v[ia - CROWD // 2:ia + CROWD // 2 + 1] = v[ia]
    v[ib - CROWD // 2:ib + CROWD // 2 + 1] = v[ib]
    # one month of NYSE rows only, one with NaN and non-NYSE rows between them
    x2 = np.concatenate([v, np.full(n // 20, np.nan)])
    m2 = np.ones(x2.size, dtype=bool)
    extra = 40 if n < 2000 else 1000
    x2 = np.concatenate([x2, np.exp(rng.normal(5, 2, extra))])
    m2 = np.concatenate([m2, np.zeros(extra, dtype=bool)])
    p = rng.permutation(x2.size)
    exp = _check(E, [rng.permutation(v), x2[p]], [np.ones(n, dtype=bool), m2[p]])
    assert exp[0] == (v[ia], v[ib])


def test_key_order_edge_cases(E):
    """Negative me, both zeros, subnormals, +-inf and 5 % NaN on NYSE and non-NYSE rows.  The
    months are built so that no expected breakpoint is an exact zero (the restatement leaves
    the sign of a zero breakpoint among both signed zeros undefined): asserted below."""
    rng = np.random.default_rng(803)
    tiny = 5e-324
    segs, masks = [], []
    for n, neg_share in ((4000, 0.7), (4000, 0.3), (1500, 0.7)):
        mag = np.exp(rng.normal(0, 6, n))
        x = np.where(rng.random(n) < neg_share, -mag, mag)
        k = n // 100
        special = np.concatenate([np.full(k, 0.0), np.full(k, -0.0), tiny * rng.integers(1, 1 << 40, k),
                                  -tiny * rng.integers(1, 1 << 40, k), np.full(3, np.inf), np.full(3, -np.inf)])
        x[rng.choice(n, special.size, replace=False)] = special
        x[rng.random(n) < 0.05] = np.nan
        segs.append(x)
        masks.append(rng.random(n) < 0.5)
    # subnormals only around the breakpoints: 30 negative ones, both zeros, 10 positive ones
    sub = np.concatenate([-tiny * np.arange(1, 31), [-0.0, 0.0], tiny * np.arange(1, 11), [np.inf, -np.inf]])
    segs.append(rng.permutation(sub))
    masks.append(np.ones(sub.size, dtype=bool))
    # the smallest and the largest keys are NYSE values: -inf / +inf bound the histogram
    x = np.concatenate([[-np.inf, np.inf], rng.normal(-3, 1, 600), [np.nan] * 10])
    segs.append(rng.permutation(x))
    masks.append(np.ones(x.size, dtype=bool))
    exp = _check(E, segs, masks)
    for t, (x, m) in enumerate(zip(segs, masks)):
        v = x[m & ~np.isnan(x)]
        assert np.any(v == 0.0) or t == 4
        assert exp[t][0] != 0.0 and exp[t][1] != 0.0, t
        assert not np.isnan(exp[t][0]) and not np.isnan(exp[t][1]), t
    assert all(np.any(np.signbit(s[m & (s == 0.0)])) and np.any(~np.signbit(s[m & (s == 0.0)]))
               for s, m in zip(segs[:4], masks[:4]))


def test_widest_key_range_with_a_crowd(E):
    """1e-300 .. 1e300 in one month (the largest shift: a bin is about one binade) with more
    than the list capacity of distinct values just above 1.0, where the median falls."""
    rng = np.random.default_rng(804)
    wide = 10.0 ** rng.uniform(-300, 300, 2000)
    wide[:2] = (1e-300, 1e300)
    crowd = 1.0 + rng.random(2 * CROWD) * 1e-3
    v = np.concatenate([wide, crowd])
    med = np.sort(v)[(v.size - 1) // 2]
    assert 1.0 <= med <= 1.001 and np.unique(_hi_words(crowd)).size > CROWD
    x, m = _with_others(rng, v, 800)
    small = np.concatenate([wide[:1200], crowd])   # the same in a month of <= 2,048 rows
    _check(E, [x, rng.permutation(v)], [m, np.ones(v.size, dtype=bool)])
    _check(E, [rng.permutation(small)], [np.ones(small.size, dtype=bool)])


def _lognormal_month(rng, n):
    x = np.exp(rng.normal(5, 2, n))
    x[rng.random(n) < 0.05] = np.nan
    return x, rng.random(n) < 0.4


@pytest.mark.parametrize("lengths", [(1, 2, 63, 64, 65, 255, 256, 257), (5119, 5120, 300), (6000, 257),
                                     (16384, 7)])
def test_month_lengths(E, lengths):
    """Lengths around the wave and workgroup width, the <20> edge (5,119 / 5,120), a month on
    universe_kernel<32> and one of 16,384 rows (<64>); one panel per instantiation."""
    rng = np.random.default_rng(805 + lengths[0])
    segs, masks = zip(*[_lognormal_month(rng, n) for n in lengths])
    _check(E, segs, masks)


@pytest.mark.parametrize("n", [900, 4000])
def test_nyse_extremes(E, n):
    """Months with no NYSE row, with every NYSE me NaN, with exactly 1 and exactly 2 NYSE
    values (one of them also beside NYSE rows whose me is NaN)."""
    rng = np.random.default_rng(806 + n)
    segs, masks = [], []
    x = np.exp(rng.normal(5, 2, n))
    segs.append(x)
    masks.append(np.zeros(n, dtype=bool))
    x = np.exp(rng.normal(5, 2, n))
    m = rng.random(n) < 0.4
    x[m] = np.nan
    segs.append(x)
    masks.append(m)
    for k in (1, 2):
        x = np.exp(rng.normal(5, 2, n))
        m = np.zeros(n, dtype=bool)
        m[rng.choice(n, k, replace=False)] = True
        segs.append(x)
        masks.append(m)
        x = x.copy()
        m = m.copy()
        nanrows = rng.choice(np.nonzero(~m)[0], 50, replace=False)
        x[nanrows] = np.nan
        m[nanrows] = True
        segs.append(x)
        masks.append(m)
    exp = _check(E, segs, masks)
    assert np.isnan(exp[0][0]) and np.isnan(exp[1][1]) and not np.isnan(exp[2][0])


def test_bench_panel_months(E):
    """E.panel_synthetic(24, 5000, 1): all 24 months' breakpoints and levels against the
    oracle, through both launches."""
    panel = E.panel_synthetic(24, 5000, 1)
    me = panel.me.cpu().numpy()
    ny = panel.nyse.cpu().numpy().astype(bool)
    off = panel.seg_off_h
    runs = (("fm_universe", E.universe(panel)),
            ("fm_select_universe", E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY, center=True,
                                                 universe=(0.2, 0.5))[1]))
    exp = [_expected(me[off[t]:off[t + 1]], ny[off[t]:off[t + 1]]) for t in range(panel.nseg)]
    assert panel.nseg == 24 and not any(np.isnan(e[0]) or np.isnan(e[1]) for e in exp)
    for name, (a, b, level) in runs:
        a, b, level = a.cpu().numpy(), b.cpu().numpy(), level.cpu().numpy()
        for t, (ea, eb, lev) in enumerate(exp):
            assert _same([a[t]], [ea]) and _same([b[t]], [eb]), (name, t)
            assert np.array_equal(level[off[t]:off[t + 1]], lev), (name, t)
