"""The 16-wide solve (fm_solve, solve16_kernel) across its column bounds, wave slots and side
paths, on small panels through engine.fm_pass: 8 months x 300 firms, 14 regressors + y, three
universe levels.

The per-wave factorization is instantiated for a few compile-time column bounds (3, 5, 7, 14)
and a wave takes the smallest bound >= the largest K of its four problems.  So: every bound and
every K that rounds up into it against the oracle's per-month OLS (oracle/fm_oracle.ols_pinv); a problem's
records independent, bit for bit, of what shares its wave and of the round it runs in; the
paths around the fast one on both panel layouts; and a pivot below 2^-767.

Monthly records are compared as tests/test_gpu_parity.py does: |a-b| <= 1e-9 * max(|b|, RMS of
the series) (tests/fmtol.py).
"""
import numpy as np
import pytest
import torch

from fmtol import RTOL, assert_series_close
from oracle import fm_oracle as O

pytestmark = pytest.mark.gpu

T, N, NX = 8, 300, 14
YC = NX          # panel column of y
NLEV = 3


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _data(seed, nan_rate):
    """Month-major rows: 14 correlated, differently located and scaled regressors, y, a level."""
    rng = np.random.default_rng(seed)
    n = T * N
    z = rng.standard_normal((n, NX))
    x = z + 0.3 * np.roll(z, 1, axis=1)
    x = x * np.linspace(0.5, 3.0, NX) + np.linspace(-2.0, 5.0, NX)
    y = 0.01 + x @ np.linspace(0.1, -0.1, NX) + rng.standard_normal(n)
    cols = [x[:, j].copy() for j in range(NX)] + [y]
    for c in cols:
        c[rng.random(n) < nan_rate] = np.nan
    level = rng.integers(0, NLEV, n).astype(np.uint8)
    labels = np.repeat(np.arange(T), N)
    return cols, level, labels


@pytest.fixture(scope="module")
def base():
    return _data(101, 0.03)


@pytest.fixture(scope="module")
def clean():
    return _data(202, 0.0)


def _pass(E, cols, level, labels, models, layout="f64", **kw):
    names = [f"x{j}" for j in range(NX)] + ["y"]
    panel = E.panel_from_arrays(cols, names, labels, layout=layout)
    assert np.array_equal(panel.order, np.arange(len(labels)))   # rows are month-major already
    lev = torch.from_numpy(level).to(panel.device)
    res = E.fm_pass(panel, models, level=lev, nlevels=NLEV, moments=True, **kw)
    return res, res.rec.cpu().numpy(), res.status.cpu().numpy(), res.moments.cpu().numpy()


def _ref(cols, level, xs, u):
    """Per-month OLS of y on [1, x_xs] over the rows of level >= u without a NaN in xs or y:
    (params [T, K+1], R2 [T], N [T]); months with N < K + 1 are skipped (NaN params)."""
    K = len(xs)
    X = np.column_stack([cols[j] for j in xs])
    y = cols[YC]
    ok = (level >= u) & ~np.isnan(y) & ~np.isnan(X).any(axis=1)
    params = np.full((T, K + 1), np.nan)
    r2 = np.full(T, np.nan)
    cnt = np.zeros(T, dtype=np.int64)
    for t in range(T):
        m = ok.copy()
        m[:t * N] = False
        m[(t + 1) * N:] = False
        cnt[t] = m.sum()
        if cnt[t] < K + 1:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            params[t], r2[t] = O.ols_pinv(np.column_stack([np.ones(cnt[t]), X[m]]), y[m])
    return params, r2, cnt


def _check(E, res, rec, st, k, ref, what, rtol=RTOL, skipped=()):
    params, r2, cnt = ref
    K = params.shape[1] - 1
    fitted = (st[:, k] & E.L.FM_ST_FITTED) != 0
    assert np.array_equal(fitted, cnt >= K + 1), what
    assert np.array_equal(rec[:, k, res.pmax + 1].astype(np.int64), cnt), what
    for t in skipped:
        assert st[t, k] == E.L.FM_ST_SKIPPED and np.isnan(rec[t, k, :res.pmax + 1]).all(), (what, t)
    assert_series_close(rec[fitted, k, res.pmax], r2[fitted], f"{what} R2", rtol=rtol)
    for j in range(K + 1):
        assert_series_close(rec[fitted, k, j], params[fitted, j], f"{what} param {j}", rtol=rtol)


# ---------------------------------------------------------------- 1. every bound, every K
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 9, 13, 14])
def test_every_column_bound_vs_oracle(E, base, K):
    """A single-model list (its three levels: one wave, bound = the smallest instantiated one
    >= K): K = 1..3 -> 3, 4..5 -> 5, 6..7 -> 7, 9..14 -> 14."""
    cols, level, labels = base
    xs = list(range(K))
    res, rec, st, _ = _pass(E, cols, level, labels, [E.Model(f"k{K}", y=YC, xs=xs, levels=(0, 1, 2))])
    assert [(p.level, p.K) for p in res.problems] == [(0, K), (1, K), (2, K)]
    for k, p in enumerate(res.problems):
        _check(E, res, rec, st, k, _ref(cols, level, xs, p.level), f"K={K} level {p.level}")


# ---------------------------------------------------------------- 2. independence from the neighbours
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _problem_bits(res, rec, st, mom, model, level):
    """Everything the solve wrote for (model, level), in a layout that does not depend on the
    list's pmax: params, R2, N, status, and n / means / centered moments."""
    k = [j for j, p in enumerate(res.problems) if (p.model, p.level) == (model, level)]
    assert len(k) == 1
    k = k[0]
    K1 = res.problems[k].K + 1
    return (_bits(rec[:, k, :K1]), _bits(rec[:, k, res.pmax]), _bits(rec[:, k, res.pmax + 1]), st[:, k].copy(),
            _bits(mom[:, k, :1 + K1 + K1 * K1]))


def test_problem_bits_independent_of_neighbours(E, clean):
    """A K = 4 and a K = 7 problem (level 1) alone, beside three K = 14 problems (the K = 7 one
    shares their wave and its bound 14; the K = 4 one runs under bound 5 in the next wave), and
    in a list of 13 problems (two rounds of twelve; nested models: 5 patterns x 3 levels):
    records, status words and moments of the same (model, level) have identical bits.  The
    panel has no NaN, so every row falls into the one pattern holding all the list's models
    and each problem's Gram is the same sum in every arrangement."""
    cols, level, labels = clean
    M = lambda K, lv: E.Model(f"k{K}", y=YC, xs=list(range(K)), levels=lv)   # noqa: E731
    out = {}
    for K in (4, 7):
        res, rec, st, mom = _pass(E, cols, level, labels, [M(K, (1,))])
        out[("alone", K)] = _problem_bits(res, rec, st, mom, 0, 1)
        _check(E, res, rec, st, 0, _ref(cols, level, list(range(K)), 1), f"alone K={K}")
    res, rec, st, mom = _pass(E, cols, level, labels, [M(14, (0, 1, 2)), M(4, (1,)), M(7, (1,))])
    assert res.nprob == 5
    out[("beside14", 4)] = _problem_bits(res, rec, st, mom, 1, 1)
    out[("beside14", 7)] = _problem_bits(res, rec, st, mom, 2, 1)
    lst = [M(14, (0, 1, 2)), M(9, (0, 1, 2)), M(7, (0, 1, 2)), M(4, (0, 1, 2)), M(3, (1,))]
    res, rec, st, mom = _pass(E, cols, level, labels, lst)
    assert res.nprob == 13
    out[("rounds", 4)] = _problem_bits(res, rec, st, mom, 3, 1)
    out[("rounds", 7)] = _problem_bits(res, rec, st, mom, 2, 1)
    for k, p in enumerate(res.problems):     # the second round's problems are right, too
        _check(E, res, rec, st, k, _ref(cols, level, list(range(p.K)), p.level), f"13 problems #{k}")
    for K in (4, 7):
        a = out[("alone", K)]
        for arr in ("beside14", "rounds"):
            for x, y, what in zip(a, out[(arr, K)], ("params", "R2", "N", "status", "moments")):
                assert np.array_equal(x, y), (K, arr, what)


# ---------------------------------------------------------------- 3. the paths around the fast one
XS3 = [0, 1, 2]


def _m3(E, **kw):
    return [E.Model("m3", y=YC, xs=XS3, levels=(0, 1, 2), **kw)]


@pytest.mark.parametrize("layout", ["f64", "planes"])
def test_month_with_too_few_rows_skipped(E, base, layout):
    cols, level, labels = base
    cols = [c.copy() for c in cols]
    m2 = np.flatnonzero(labels == 2)
    cols[YC][m2[3:]] = np.nan          # month 2: at most K = 3 valid rows at any level
    res, rec, st, _ = _pass(E, cols, level, labels, _m3(E), layout)
    for k, p in enumerate(res.problems):
        ref = _ref(cols, level, XS3, p.level)
        assert ref[2][2] < 4
        _check(E, res, rec, st, k, ref, f"skip level {p.level}", skipped=(2,))


@pytest.mark.parametrize("layout", ["f64", "planes"])
def test_exactly_collinear_pair(E, base, layout):
    """x2 = 2 x1 in every month: the pivot collapses, the wave takes the Jacobi path (its Gram
    rebuilt from the buckets, the images being overwritten by then) and the month is refitted
    from its rows; statsmodels' minimum-norm solution."""
    cols, level, labels = base
    cols = [c.copy() for c in cols]
    cols[2] = 2.0 * cols[1]
    res, rec, st, _ = _pass(E, cols, level, labels, _m3(E), layout)
    assert ((st & E.L.FM_ST_RANK_DEF) != 0).all()
    for k, p in enumerate(res.problems):
        _check(E, res, rec, st, k, _ref(cols, level, XS3, p.level), f"collinear level {p.level}")


@pytest.mark.parametrize("layout", ["f64", "planes"])
def test_near_collinear_column_refit(E, base, layout):
    """x2 = x1 + 1e-4 sd(x1) noise: 1 - R^2 of x2 on x1 ~ 1e-8, between the Cholesky's 1e-9 and
    the refit's 1e-6 thresholds, so the months are factored, flagged FM_ST_REFIT and refitted
    inline.  Tolerance as test_conditioning_sweep_vs_pinv: max(1e-9, 2e-13 / noise)."""
    cols, level, labels = base
    cols = [c.copy() for c in cols]
    noise = 1e-4
    rng = np.random.default_rng(5)
    cols[2] = cols[1] + noise * np.nanstd(cols[1]) * rng.standard_normal(T * N)
    res, rec, st, _ = _pass(E, cols, level, labels, _m3(E), layout)
    assert ((st & E.L.FM_ST_REFIT) != 0).all() and ((st & E.L.FM_ST_RANK_DEF) == 0).all()
    for k, p in enumerate(res.problems):
        _check(E, res, rec, st, k, _ref(cols, level, XS3, p.level), f"near-collinear level {p.level}",
               rtol=max(RTOL, 2e-13 / noise))


@pytest.mark.parametrize("layout", ["f64", "planes"])
def test_regressor_constant_within_a_month(E, base, layout):
    """x1 = 1.5 throughout month 3.  With the constant check (add_constant's 'skip') the month
    is flagged FM_ST_CONST_COL and no other; without it ('add', Figure 1) the intercept is
    split over [1, x1] by the minimum norm, as the oracle's pinv does."""
    cols, level, labels = base
    cols = [c.copy() for c in cols]
    m3 = labels == 3
    cols[1][m3 & ~np.isnan(cols[1])] = 1.5
    res, rec, st, _ = _pass(E, cols, level, labels, _m3(E), layout)
    flagged = (st & E.L.FM_ST_CONST_COL) != 0
    assert flagged[3].all() and not np.delete(flagged, 3, axis=0).any()
    res, rec, st, _ = _pass(E, cols, level, labels, _m3(E, const_check=False), layout, const_check=False)
    assert ((st & E.L.FM_ST_CONST_COL) == 0).all()
    for k, p in enumerate(res.problems):
        _check(E, res, rec, st, k, _ref(cols, level, XS3, p.level), f"const level {p.level}")


@pytest.mark.parametrize("layout", ["f64", "planes"])
def test_inf_in_y(E, base, layout):
    """+inf in one month's y, +inf and -inf in another's (level 2 rows, so every problem has
    them): pinv(X) @ y gives +-inf or NaN coefficients and a NaN R2, as statsmodels does."""
    cols, level, labels = base
    cols = [c.copy() for c in cols]
    ok = (level == 2) & ~np.isnan(np.column_stack([cols[j] for j in XS3 + [YC]])).any(axis=1)
    r1 = np.flatnonzero(ok & (labels == 1))
    r5 = np.flatnonzero(ok & (labels == 5))
    cols[YC][r1[0]] = np.inf
    cols[YC][r5[0]] = np.inf
    cols[YC][r5[1]] = -np.inf
    res, rec, st, _ = _pass(E, cols, level, labels, _m3(E), layout)
    assert ((st[[1, 5]] & E.L.FM_ST_INF_IN_Y) != 0).all()
    for k, p in enumerate(res.problems):
        ref = _ref(cols, level, XS3, p.level)
        assert np.isinf(ref[0][1]).any() and np.isnan(ref[0][5]).any()
        _check(E, res, rec, st, k, ref, f"inf y level {p.level}")


# ---------------------------------------------------------------- 4. the small pivot
@pytest.mark.parametrize("scale", [1e-150, 1e-160])
def test_small_pivot_scaled_regressor(E, clean, scale):
    """One regressor of a well-conditioned K = 3 model times 1e-160 (and 1e-150): its centered
    sum of squares, the Cholesky pivot, is far below 2^-767, where the reciprocal square root
    estimate needs its input rescaled.  The slopes are finite; the scaled column's, times the
    scale, and all other coefficients equal the unscaled run's at the monthly-record tolerance.

    At 1e-150 the pivot (~3e-298) is a normal number and the Cholesky path holds (rsq_nr's
    rescaling).  At 1e-160 the squares ~1e-320 are subnormal where fm_gram sums them (the Gram
    diagonal, ~3e-318, carries about 20 bits), so the solve flags the problem FM_ST_REFIT on its
    tiny centered sum of squares and the row refit, with the column scaled by an exact power of
    two, gives the coefficients.  Measured on MI355X: worst scaled error 7.6e-16 and 3.8e-15."""
    cols, level, labels = clean
    res0, rec0, st0, _ = _pass(E, cols, level, labels, _m3(E))
    for k, p in enumerate(res0.problems):
        _check(E, res0, rec0, st0, k, _ref(cols, level, XS3, p.level), f"unscaled level {p.level}")
    cols = [c.copy() for c in cols]
    cols[1] = cols[1] * scale
    res, rec, st, _ = _pass(E, cols, level, labels, _m3(E))
    assert ((st & E.L.FM_ST_FITTED) != 0).all()
    assert (((st & E.L.FM_ST_REFIT) != 0) == (scale < 1e-155)).all()   # which path each scale takes
    print(f"small pivot {scale:g}: finite {bool(np.isfinite(rec[:, :, :4]).all())}")
    assert np.isfinite(rec[:, :, :4]).all()
    worst = 0.0
    for k in range(res.nprob):
        for j in range(4):
            got = rec[:, k, j] * (scale if j == 2 else 1.0)
            exp = rec0[:, k, j]
            worst = max(worst, float(np.max(np.abs(got - exp) / np.maximum(np.abs(exp), np.sqrt(np.mean(exp ** 2))))))
    print(f"small pivot {scale:g}: worst scaled error {worst:.3e} (tolerance {RTOL:.0e})")
    for k in range(res.nprob):
        for j in range(4):
            got = rec[:, k, j] * (scale if j == 2 else 1.0)
            assert_series_close(got, rec0[:, k, j], f"problem {k} param {j}")
        assert_series_close(rec[:, k, res.pmax], rec0[:, k, res0.pmax], f"problem {k} R2")
