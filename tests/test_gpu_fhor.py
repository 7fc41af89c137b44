"""GPU tests of fm_forecast_horizon (extension A17; the paper's Section 4, second approach), its
engine entry points, PipelineConfig(extrapolate=k), build_table_3_extrapolated and
forecast_extrapolation: bit for bit against the exact numpy restatement (tests/fhor_oracle.py,
(a)), at the project's 1e-9 rule against the plain numpy chain ((b)), against fm_forecast_dist on
the same inputs, across the kernel's three forms and two sources, and end to end against
oracle.fm_oracle's forecasts and horizon_oracle's compounded returns."""
import numpy as np
import pytest
import torch

import fhor_oracle as HO
import horizon_oracle as RO
import pipe_port_oracle as PPO
from fmtol import RTOL, assert_series_close, scalar_close
from test_gpu_fdist import EDGE_LENS, _edge_months, _months, _select_months
from test_gpu_pipeline_portfolios import SEL3, _dev, _panel, _random_coef, _random_panel

pytestmark = pytest.mark.gpu

LAYOUTS = ["f64", "planes"]
OUTS = ("rec", "cnt", "status")
A3, G3 = 3.0, 1.0 + 0.9 + 0.9 * 0.9   # the paper's scaling to k = 3 months


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _host(h, extra=()):
    torch.cuda.synchronize()
    d = {k: getattr(h, k).cpu().numpy() for k in OUTS}
    for k in extra:
        d[k] = getattr(h, k).cpu().numpy()
    return d


def _assert_same_bytes(got, exp, what):
    for k in exp:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


def _vector(E, seg_off, F, ret, level=None, a=A3, g=G3, **kw):
    h = E.forecast_horizon_vector(_dev(E, seg_off), _dev(E, F), _dev(E, ret), a, g, level=_dev(E, level),
                                  scaled_out=True, **kw)
    return _host(h, ("scaled",))


def _returns(seed, F, slope=0.5, nan_rate=0.03):
    """A realised return for every row: related to the forecast where there is one, 3 % NaN."""
    rng = np.random.default_rng(seed)
    r = rng.normal(0.0, 0.1, len(F))
    ok = np.isfinite(F)
    r[ok] += slope * np.clip(F[ok], -1.0, 1.0)
    r[rng.random(len(F)) < nan_rate] = np.nan
    return r


def _check_exact(got, exp, what):
    """Against (a): cnt, status, m, the scaled forecasts, the quantiles and every column (a) reaches
    without a square root bit for bit; the standard deviation at the project's 1e-9 rule."""
    assert np.array_equal(got["cnt"], exp["cnt"]) and np.array_equal(got["status"], exp["status"]), what
    for c in [0, 2, 3, 4, 5] + list(range(HO.NREC, exp["rec"].shape[-1])):
        assert HO.same_bits(got["rec"][..., c], exp["rec"][..., c]), (what, "rec", c)
    assert HO.same_bits(got["scaled"], exp["scaled"]), (what, "scaled")
    for j in range(exp["rec"].shape[0]):
        assert_series_close(got["rec"][j, :, 1], exp["rec"][j, :, 1], f"{what} sd[{j}]")


def _check_chain(got, exp, what):
    """Against (b): counts and status exact, everything else at the project's 1e-9 rule."""
    assert np.array_equal(got["cnt"], exp["cnt"]) and np.array_equal(got["status"], exp["status"]), what
    for j in range(exp["rec"].shape[0]):
        for c in range(exp["rec"].shape[-1]):
            assert_series_close(got["rec"][j, :, c], exp["rec"][j, :, c], f"{what} rec[{j}, :, {c}]")
        if "scaled" in got:
            assert_series_close(got["scaled"][j], exp["scaled"][j], f"{what} scaled[{j}]")


# ---------------------------------------------------------------- 1. edge months, vector source
def _edge_inputs(longest):
    """test_gpu_fdist's edge months with a return: 3 % NaN; the two-row month keeps one return
    (nR = 1); the month whose forecasts differ in the low 32 bits only -- it is there for the order
    statistics' low key words, and a regression on a spread of 200 ulps is rounding noise in any
    order of operations -- is the month without a return (nR = 0)."""
    seg_off, F = _edge_months(longest)
    ret = _returns(13, F)
    nlen = sum(n <= longest for n in EDGE_LENS)
    s = seg_off
    ret[s[1]:s[2]] = 0.02
    ret[s[2]:s[3]] = 0.03, np.nan
    ret[s[nlen + 3]:s[nlen + 4]] = np.nan
    ret[s[nlen + 1] + 5] = 0.125          # the all-equal month keeps returns: a constant G, a NaN slope
    return seg_off, F, ret, nlen


@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("min_level", [0, 1])
@pytest.mark.parametrize("longest", [1024, 1025], ids=["256x4", "512x10"])
def test_edge_months_vs_restatements(E, longest, min_level, min_count):
    seg_off, F, ret, nlen = _edge_inputs(longest)
    level = np.random.default_rng(12).integers(0, 3, len(F)).astype(np.uint8)
    level[int(seg_off[1]):int(seg_off[3])] = 2                   # the one- and two-row months stay eligible
    q = (0.1, 0.5, 0.9)
    got = _vector(E, seg_off, F, ret, level, min_level=min_level, q=q, min_count=min_count)
    kw = dict(level=level, min_levels=[min_level], q=q, min_count=min_count)
    exact = HO.batch(HO.forecast_horizon_exact, seg_off, [F], ret, A3, G3, **kw)
    chain = HO.batch(HO.forecast_horizon, seg_off, [F], ret, A3, G3, **kw)
    assert int(np.diff(seg_off).max()) == longest
    c, st = exact["cnt"][0], exact["status"][0]
    assert list(c[0]) == [0, 0] and list(c[1]) == [1, 1] and list(c[2]) == [2, 1]
    assert (st[:3] == (min_count == 1) * np.array([0, 1, 1])).all()
    assert c[nlen, 0] == 0 and st[nlen] == 0                                     # the all-NaN month
    assert c[nlen + 3, 1] == 0 and st[nlen + 3] == 1 and np.isnan(exact["rec"][0, nlen + 3, 2:5]).all()
    assert c[nlen + 1, 1] > 2 and np.isnan(exact["rec"][0, nlen + 1, 2:5]).all()  # the all-equal month
    assert np.all(exact["rec"][0, nlen + 1, [0, 6, 7, 8]] == A3 * 0.03125) and exact["rec"][0, nlen + 1, 1] == 0.0
    assert np.isfinite(exact["rec"][0, st == 1][:, [0, 5, 6, 7, 8]]).all()
    if min_level == 0:
        assert c[nlen + 4, 0] == 78
    assert np.isfinite(exact["rec"][0, c[:, 1] >= 3][:, 2:5]).sum() >= 3 * (nlen - 4)
    assert np.isnan(got["scaled"][0, int(seg_off[nlen]):int(seg_off[nlen + 1])]).all()
    what = f"edge {longest} level>={min_level} min_count={min_count}"
    _check_exact(got, exact, what)
    _check_chain(got, chain, what)


# ---------------------------------------------------------------- 2. the select paths
@pytest.mark.parametrize("q", [(0.001, 0.01, 0.1, 0.25, 0.5, 0.9, 0.99, 0.999), ()], ids=["nq8", "nq0"])
def test_select_paths_vs_restatements(E, q):
    seg_off, F = _select_months()
    ret = _returns(22, F)
    got = _vector(E, seg_off, F, ret, q=q)
    exact = HO.batch(HO.forecast_horizon_exact, seg_off, [F], ret, A3, G3, q=q)
    assert list(exact["cnt"][0, :, 0]) == [2048, 2049, 5000, 3000, 5000] and exact["rec"].shape == (1, 5, HO.NREC + len(q))
    assert np.isnan(exact["rec"][0, 3, 2:5]).all() and np.isfinite(exact["rec"][0, [0, 1, 2, 4], 2:5]).all()
    _check_exact(got, exact, f"select nq={len(q)}")
    _check_chain(got, HO.batch(HO.forecast_horizon, seg_off, [F], ret, A3, G3, q=q), f"select nq={len(q)}")
    # the 1,024 x 16 form runs its own sample select and its own sums: the same bytes
    _assert_same_bytes(_vector(E, seg_off, F, ret, q=q, max_seg_len=6000), got, "select, 1024 x 16")


# ---------------------------------------------------------------- 3. agreement with fm_forecast_dist
def test_agrees_with_forecast_dist(E):
    """On the same inputs m and the count are fm_forecast_dist's mean and count byte for byte.  With
    a = 0 and g = 1, G = F - m: where a quantile is an order statistic (the interpolation weight is
    zero), or where every operation is exact, mapping the sibling's quantile through 0 * m + 1 * (q
    - m) gives this kernel's quantile bit for bit.  (Between two order statistics the two round
    differently: this kernel interpolates the mapped neighbours, as the header says.)"""
    q = (0.1, 0.5, 0.9)
    seg_off, F, ret, _ = _edge_inputs(1025)
    level = np.random.default_rng(12).integers(0, 3, len(F)).astype(np.uint8)
    for min_level in (0, 1):
        got = _vector(E, seg_off, F, ret, level, min_level=min_level, q=q)
        d = E.forecast_dist_vector(_dev(E, seg_off), _dev(E, F), level=_dev(E, level), min_level=min_level, q=q)
        torch.cuda.synchronize()
        dr, dc = d.rec.cpu().numpy(), d.cnt.cpu().numpy()
        assert got["rec"][..., 5].tobytes() == dr[..., 0].tobytes() and got["cnt"][..., 0].tobytes() == dc.tobytes()
        assert np.array_equal(got["status"], d.status.cpu().numpy())
    # months of 101, 201 and 1,001 eligible rows: (n - 1) q is a whole number for q = .1, .5, .9; and a
    # month of 64 multiples of 2^-10, whose mean, deviations and midpoints are all exact
    rng = np.random.default_rng(33)
    parts = [rng.standard_t(3, n) * 0.02 + 0.01 for n in (101, 201, 1001)]
    parts.append(rng.integers(-500, 501, 64) / 1024.0)
    seg_off, F = _months(parts)
    for n in (101, 201, 1001):
        assert all(float(np.float64(n - 1) * np.float64(lv)).is_integer() for lv in q)
    qs = [q, q, q, (0.25, 0.5, 0.75)]
    got = _vector(E, seg_off, F, _returns(34, F), a=0.0, g=1.0, q=q)
    got4 = _vector(E, seg_off, F, _returns(34, F), a=0.0, g=1.0, q=qs[3])
    for lv, g in ((q, got), (qs[3], got4)):
        d = E.forecast_dist_vector(_dev(E, seg_off), _dev(E, F), q=lv)
        torch.cuda.synchronize()
        dr = d.rec.cpu().numpy()[0]
        m = dr[:, :1]
        mapped = 0.0 * m + 1.0 * (dr[:, 2:] - m)
        rows = [3] if lv is qs[3] else [0, 1, 2]
        assert HO.same_bits(g["rec"][0, rows, HO.NREC:], mapped[rows]), lv
        assert g["rec"][0, :, 5].tobytes() == dr[:, 0].tobytes()


# ---------------------------------------------------------------- 4. form independence, locality
def test_form_independence(E):
    """The same 900-row months under max_seg_len 900 / 2,000 / 6,000 (the 256 x 4, 512 x 10 and
    1,024 x 16 forms), month-sharded and repeated: the same bytes in every output."""
    rng = np.random.default_rng(31)
    parts = [rng.standard_t(3, 900) * 0.02 for _ in range(5)]
    for p in parts:
        p[rng.random(900) < 0.05] = np.nan
    seg_off, F = _months(parts)
    level = rng.integers(0, 3, len(F)).astype(np.uint8)
    Fs = np.stack([F, F[::-1].copy()])
    ret = _returns(32, F)
    kw = dict(min_level=[0, 1], q=(0.1, 0.9))
    base = _vector(E, seg_off, Fs, ret, level, max_seg_len=900, **kw)
    _check_exact(base, HO.batch(HO.forecast_horizon_exact, seg_off, Fs, ret, A3, G3, level, [0, 1], (0.1, 0.9)), "900-row months")
    for msl in (2000, 6000):
        _assert_same_bytes(_vector(E, seg_off, Fs, ret, level, max_seg_len=msl, **kw), base, f"max_seg_len {msl}")
    _assert_same_bytes(_vector(E, seg_off, Fs, ret, level, **kw), base, "repeated")
    lo = _vector(E, seg_off[:3], Fs[:, :1800].copy(), ret[:1800], level[:1800], **kw)
    hi = _vector(E, seg_off[2:] - seg_off[2], Fs[:, 1800:].copy(), ret[1800:], level[1800:], max_seg_len=6000, **kw)
    _assert_same_bytes({k: np.concatenate([lo[k], hi[k]], axis=1) for k in base}, base, "month-sharded")


# ---------------------------------------------------------------- 5. fused equals composition
def _composition(E, panel, d, coef, sel, cuts, **kw):
    """clip the whole panel, one forecast vector per sort, then the vector source."""
    src = E.clip(panel, cuts) if cuts is not None else panel.values()
    F = torch.stack([E.forecast(panel, coef[j, :, :len(xs) + 1].contiguous(), cols=src[xs].contiguous())
                     for j, (xs, _) in enumerate(sel)])
    h = E.forecast_horizon_vector(panel.seg_off, F, _dev(E, d["cols"][0]), A3, G3, level=_dev(E, d["level"]),
                                  min_level=[lv for _, lv in sel], max_seg_len=panel.max_seg_len, scaled_out=True, **kw)
    out = _host(h, ("scaled",))
    out["forecast"] = F.cpu().numpy()
    return out


def _fused(E, panel, d, coef, sel, cuts, **kw):
    h = E.forecast_horizon(panel, coef, sel, _dev(E, d["cols"][0]), A3, G3, cuts=cuts, level=_dev(E, d["level"]),
                           scaled_out=True, forecast_out=True, **kw)
    return _host(h, ("scaled", "forecast"))


@pytest.fixture(scope="module")
def edge():
    d = _random_panel(3, 12, 250, 300, 6, edge=True)
    d["coef"] = _random_coef(4, 3, 12, 6, nan_at=(1, 9, 2))   # sort 1, month 9: a NaN slope
    return d


@pytest.mark.parametrize("clipped", [True, False], ids=["cuts", "nocuts"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_equals_composition(E, edge, layout, clipped):
    panel = _panel(E, edge, layout)
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY) if clipped else None
    coef = _dev(E, edge["coef"])
    kw = dict(q=(0.1, 0.5, 0.9), min_count=10)
    exp = _composition(E, panel, edge, coef, SEL3, cuts, **kw)
    got = _fused(E, panel, edge, coef, SEL3, cuts, **kw)
    s = edge["seg_off"]
    assert exp["status"][1, 9] == 0 and exp["cnt"][1, 9, 0] == 0 and np.isnan(exp["scaled"][1, s[9]:s[10]]).all()
    assert (exp["status"][:, 7] == 0).all() and 0 < exp["cnt"][0, 7, 0] < 10   # below min_count, not empty
    assert exp["status"][0].sum() == 11 and (exp["cnt"][..., 1] < exp["cnt"][..., 0]).any()
    _assert_same_bytes(got, exp, f"{layout} clipped={clipped}")
    if layout == "f64" and clipped:
        lo, hi = PPO.winsor_cuts(edge["cols"], edge["seg_off"])
        Fs = [PPO.forecast(edge["cols"], edge["seg_off"], edge["coef"][j], xs, lo, hi) for j, (xs, _) in enumerate(SEL3)]
        assert np.array_equal(got["forecast"], np.stack(Fs), equal_nan=True)
        _check_exact(got, HO.batch(HO.forecast_horizon_exact, edge["seg_off"], Fs, edge["cols"][0], A3, G3, edge["level"],
                                   [lv for _, lv in SEL3], kw["q"], kw["min_count"]), "edge panel")


@pytest.mark.parametrize("T,N,K,layout", [(3, 1000, 30, "f64"), (3, 1000, 30, "planes"), (2, 5000, 14, "f64"),
                                          (2, 5000, 14, "planes"), (1, 16384, 2, "f64")])
def test_instantiations(E, T, N, K, layout):
    d = _random_panel(50 + K, T, N, N, K + 1)
    panel = _panel(E, d, layout)
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    sel = [(list(range(1, K + 1)), 0), (list(range(K, 0, -1)), 1)]
    coef = _dev(E, _random_coef(60 + K, 2, T, K + 1))
    exp = _composition(E, panel, d, coef, sel, cuts)
    assert exp["status"].all() and (exp["cnt"][..., 1] > N // 4).all() and np.isfinite(exp["rec"]).all()
    _assert_same_bytes(_fused(E, panel, d, coef, sel, cuts), exp, f"{T}x{N} K={K} {layout}")


def test_more_sorts_than_one_launch(E, edge):
    """18 sorts: FM_MAX_SORTS = 16 per launch, so two launches write one batched result, from the
    panel and from vectors."""
    from fmcore import _lib as L
    panel = _panel(E, edge, "planes")
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    coef = _dev(E, edge["coef"])
    one = _fused(E, panel, edge, coef, SEL3, cuts)
    reps = 6
    assert 3 * reps > L.FM_MAX_SORTS
    exp = {k: np.concatenate([v] * reps) for k, v in one.items()}
    _assert_same_bytes(_fused(E, panel, edge, coef.repeat(reps, 1, 1), SEL3 * reps, cuts), exp, "18 sorts, fused")
    got = _vector(E, edge["seg_off"], exp["forecast"], edge["cols"][0], edge["level"], min_level=[lv for _, lv in SEL3] * reps)
    _assert_same_bytes(got, {k: exp[k] for k in OUTS + ("scaled",)}, "18 sorts, vectors")


# ---------------------------------------------------------------- 6. refusal, empty calls
def test_too_long_month_refused(E):
    from fmcore._lib import FMError
    N = 16385
    d = _random_panel(71, 1, N, N, 3)
    panel = _panel(E, d, "f64")
    dev = panel.device
    out = E.ForecastHorizon(rec=torch.full((1, 1, 8), 7.0, dtype=torch.float64, device=dev),
                            cnt=torch.full((1, 1, 2), 7, dtype=torch.int32, device=dev),
                            status=torch.full((1, 1), 7, dtype=torch.int32, device=dev),
                            scaled=torch.full((1, N), 7.0, dtype=torch.float64, device=dev))
    ret = panel.values()[0].contiguous()
    with pytest.raises(FMError, match=r"\(-3\).*16384"):
        E.forecast_horizon(panel, _dev(E, _random_coef(1, 1, 1, 3)), [([1, 2], 0)], ret, A3, G3, scaled_out=True, out=out)
    with pytest.raises(FMError, match=r"\(-3\)"):
        E.forecast_horizon_vector(panel.seg_off, panel.values()[1].contiguous(), ret, A3, G3)
    h = _host(out, ("scaled",))
    assert (h["rec"] == 7.0).all() and (h["cnt"] == 7).all() and (h["status"] == 7).all() and (h["scaled"] == 7.0).all()


def test_empty_calls(E, edge):
    panel = _panel(E, edge, "f64")
    ret = panel.values()[0].contiguous()
    h = E.forecast_horizon(panel, _dev(E, edge["coef"])[:0], [], ret, A3, G3, scaled_out=True, forecast_out=True)
    assert h.rec.shape == (0, 12, 8) and h.cnt.shape == (0, 12, 2) and h.scaled.shape == (0, panel.nrows)
    assert h.forecast.shape == (0, panel.nrows)
    dev = panel.device
    none = torch.empty(0, dtype=torch.float64, device=dev)
    h = E.forecast_horizon_vector(torch.zeros(1, dtype=torch.int64, device=dev), none, none, A3, G3)
    torch.cuda.synchronize()
    assert h.rec.shape == (1, 0, 8) and h.cnt.shape == (1, 0, 2) and h.status.shape == (1, 0)


# ---------------------------------------------------------------- 7. the pipeline
K3 = 3


def _pipe_panel(E, layout, ids=True):
    fx = PPO.pipeline_fixture()
    a = fx["arrays"]
    return E.panel_from_arrays(fx["cols"], fx["names"], a["month"], me=a["me"], nyse=a["nyse"], layout=layout,
                               ids=a["permno"] if ids else None)


def _pipe_cfg(LW, **kw):
    c = PPO.PIPE
    return LW.PipelineConfig(**dict(dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"]), **kw))


@pytest.fixture(scope="module")
def pipe_runs(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    ex = dict(extrapolate=K3, extrapolate_decay=0.9)
    cfgs = dict(extr=ex, planes=ex, all=dict(ex, portfolios=PPO.PIPE["nport"], forecast_dist=True),
                ports=dict(portfolios=PPO.PIPE["nport"]), dist=dict(forecast_dist=True), off={})
    runs = {k: LW.run_pipeline(_pipe_panel(E, "planes" if k == "planes" else "f64"), _pipe_cfg(LW, **kw),
                               model_cols=fx["model_cols"]) for k, kw in cfgs.items()}
    torch.cuda.synchronize()
    return runs


@pytest.fixture(scope="module")
def pipe_expected():
    """(b) fed pipe_port_oracle's forecasts and levels and horizon_oracle's 3-month returns."""
    keys, pe = PPO.pipeline_expected()
    fx = PPO.pipeline_fixture()
    a, so = fx["arrays"], fx["seg_off"]
    link = RO.month_links(a["permno"], so, np.unique(a["month"]).astype(np.int32), 1)
    ret3 = RO.horizon_return(a["retx"], link, so, K3)
    exp = HO.batch(HO.forecast_horizon, so, pe["F"], ret3, float(K3), G3, pe["level"], [u for _, u in keys], (0.1, 0.9))
    return keys, exp, ret3


def test_pipeline_vs_oracle_alone(pipe_runs, pipe_expected):
    keys, exp, ret3 = pipe_expected
    fx = PPO.pipeline_fixture()
    T = len(fx["seg_off"]) - 1
    # the condition, on the restatement itself: at least 20 months with coefficients per sort, of which
    # only the last k - 1 = 2 lose every return (gaps remove rows, not months)
    assert (exp["status"].sum(axis=1) >= 20).all()
    finite = np.isfinite(exp["rec"][..., 2])
    assert (finite.sum(axis=1) >= 15).all() and (finite.sum(axis=1) == exp["status"].sum(axis=1) - 2).all()
    assert (exp["status"][:, T - 2:] == 1).all() and (exp["cnt"][:, T - 2:, 1] == 0).all()
    assert (exp["cnt"][:, T - 2:, 0] > 0).all() and np.isnan(exp["rec"][:, T - 2:, 2:5]).all()
    assert np.isnan(ret3[fx["seg_off"][T - 2]:]).all() and 0.5 < np.isfinite(ret3[:fx["seg_off"][T - 2]]).mean() < 0.95
    out = pipe_runs["extr"]
    assert out.portfolios is None and out.forecast_dist is None and pipe_runs["off"].extrapolated is None
    assert pipe_runs["off"].extrapolated_summary is None and pipe_runs["off"].extrapolated_problems is None
    assert [(out.model_names[out.res.problems[k].model], out.res.problems[k].level)
            for k in out.extrapolated_problems] == keys
    got = _host(out.extrapolated)
    assert got["rec"].shape == (len(keys), T, 8)
    _check_chain(got, exp, "pipeline")
    s = out.extrapolated_summary
    gm, gn = s.mean.cpu().numpy(), s.nobs.cpu().numpy()
    assert gm.shape == (len(keys), 8)
    for j in range(len(keys)):
        for c in range(8):
            x = exp["rec"][j, exp["status"][j] == 1, c]
            x = x[~np.isnan(x)]
            assert gn[j, c] == len(x) and len(x) >= 15, (j, c)
            assert scalar_close(gm[j, c], x.mean(), RTOL, float(np.sqrt(np.mean(x * x)))), (j, c)


def test_pipeline_layouts_and_companions_identical(pipe_runs):
    """The planes-only panel gives the same bytes; with portfolios and forecast_dist on as well,
    every result equals its stand-alone run bit for bit."""
    from test_gpu_pipeline_portfolios import _host as port_host
    from test_gpu_fdist import _host as dist_host
    base = _host(pipe_runs["extr"].extrapolated)
    _assert_same_bytes(_host(pipe_runs["planes"].extrapolated), base, "planes")
    _assert_same_bytes(_host(pipe_runs["all"].extrapolated), base, "with companions")
    _assert_same_bytes(port_host(pipe_runs["all"].portfolios), port_host(pipe_runs["ports"].portfolios), "portfolios")
    _assert_same_bytes(dist_host(pipe_runs["all"].forecast_dist), dist_host(pipe_runs["dist"].forecast_dist), "forecast_dist")
    for r in ("planes", "all"):
        for k in ("mean", "se", "tstat", "nobs"):
            a, b = (getattr(pipe_runs[x].extrapolated_summary, k).cpu().numpy() for x in (r, "extr"))
            assert a.tobytes() == b.tobytes(), (r, k)
    assert pipe_runs["all"].extrapolated_problems == pipe_runs["all"].portfolio_problems
    # m is the sibling's mean, byte for byte, inside the pipeline too
    assert _host(pipe_runs["all"].extrapolated)["rec"][..., 5].tobytes() == \
        dist_host(pipe_runs["all"].forecast_dist)["rec"][..., 0].tobytes()


def test_pipeline_off_is_unchanged(pipe_runs):
    """extrapolate=None: no extrapolation fields, and with it on every other field is byte-identical."""
    on, off = pipe_runs["extr"], pipe_runs["off"]
    assert on.model_names == off.model_names and on.model_cols == off.model_cols and on.y_col == off.y_col == "retx"
    for name in ("portfolios", "portfolio_summary", "portfolio_problems", "forecast_dist", "forecast_dist_summary",
                 "forecast_dist_problems", "forecast_compare", "forecast_compare_summary", "forecast_compare_pairs"):
        assert getattr(on, name) is None and getattr(off, name) is None, name

    def tensors(out):
        """The run's other tensors as host arrays; the tables indexed by fitted-month row up to each
        problem's count and the moments up to each problem's own size (beyond is never written)."""
        h = lambda t: t.cpu().numpy()   # noqa: E731
        count = h(out.ix.count)
        rows = np.arange(out.ix.idx.shape[1])[None, :] < count[:, None]
        fitted = (h(out.res.status) & 1) != 0
        mom = h(out.res.moments)
        d = {"res.rec": h(out.res.rec), "res.status": h(out.res.status), "ix.count": count, "ix.idx": h(out.ix.idx)[rows],
             "rolling": h(out.rolling)[rows], "pred": h(out.pred)[rows], "pred_status": h(out.pred_status)[rows],
             "level": h(out.level), "breakpoints[0]": h(out.breakpoints[0]), "breakpoints[1]": h(out.breakpoints[1])}
        for k, p in enumerate(out.res.problems):
            d[f"res.moments[{k}]"] = mom[fitted[:, k], k, :1 + (p.K + 1) + (p.K + 1) ** 2]
        for name in ("summary", "pred_summary"):
            for k in ("mean", "se", "tstat", "nobs"):
                d[f"{name}.{k}"] = h(getattr(getattr(out, name), k))
        for k in ("lo", "hi", "nvalid", "center"):
            d[f"cuts.{k}"] = h(getattr(out.cuts, k))
        return d

    ta, tb = tensors(on), tensors(off)
    assert set(ta) == set(tb)
    for k in tb:
        assert ta[k].shape == tb[k].shape and ta[k].dtype == tb[k].dtype and ta[k].tobytes() == tb[k].tobytes(), k


def test_pipeline_config_errors(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    with pytest.raises(ValueError, match="extrapolate needs a panel with firm ids"):
        LW.run_pipeline(_pipe_panel(E, "f64", ids=False), _pipe_cfg(LW, extrapolate=K3), model_cols=fx["model_cols"])
    with pytest.raises(ValueError, match="extrapolate excludes standardize"):
        LW.run_pipeline(_pipe_panel(E, "f64"), _pipe_cfg(LW, extrapolate=K3, standardize=True), model_cols=fx["model_cols"])


# ---------------------------------------------------------------- 8. drop-in
def _frame():
    from fmcore import synth
    return synth.synth_frame(40, 300, 5, present_rate=0.9, shuffle=True)


def test_build_table_3_extrapolated(E):
    """The table against (b) fed the device's own monthly forecasts of the same frame (fm_forecast_dist's
    forecast_out), its universe levels and horizon_oracle's 3-month returns."""
    from fmcore import lewellen as LW
    from fmdrop import calc_Lewellen_2014 as CL
    df = _frame()
    kw = dict(window=12, min_periods=6, lag=1)
    tab = CL.build_table_3_extrapolated(df, K3, nw_lags=4, extrapolate_nw_lags=6, **kw)
    out = CL.lewellen_pipeline(df, extrapolate=K3, extrapolate_nw_lags=6, **kw)
    probs = out.extrapolated_problems
    keys = [(out.model_names[out.res.problems[k].model], LW.SUBSET_NAMES[out.res.problems[k].level]) for k in probs]
    assert list(tab.index) == keys and len(keys) == 9 and tab.index.names == ["model", "universe"]
    assert list(tab.columns) == ["Avg", "Std", "p10", "p90", "Slope", "S.E.", "t-stat", "R2"]
    s = out.extrapolated_summary
    mean, se, t = s.mean.cpu().numpy(), s.se.cpu().numpy(), s.tstat.cpu().numpy()
    assert tab[["Avg", "Std"]].to_numpy().tobytes() == np.ascontiguousarray(mean[:, :2]).tobytes()
    assert tab[["p10", "p90"]].to_numpy().tobytes() == np.ascontiguousarray(mean[:, 6:]).tobytes()
    for col, x in (("Slope", mean[:, 2]), ("S.E.", se[:, 2]), ("t-stat", t[:, 2]), ("R2", mean[:, 4])):
        assert tab[col].to_numpy().tobytes() == np.ascontiguousarray(x).tobytes(), col
    assert np.isfinite(tab.to_numpy()).all()
    other = CL.build_table_3_extrapolated(df, K3, decay=1.0, q=(0.25, 0.5, 0.75), **kw)
    assert list(other.columns) == ["Avg", "Std", "p25", "p50", "p75", "Slope", "S.E.", "t-stat", "R2"]
    assert np.allclose(other["Avg"], tab["Avg"], rtol=1e-12) and (other["Std"] > tab["Std"]).all()
    assert np.allclose(other["R2"], tab["R2"], rtol=1e-6)        # an affine map of the regressor
    # the restatement on the device's forecasts
    panel, model_cols = CL._pipeline_panel(df)
    coef = E.lagged_coefficients(out.rolling, out.ix, probs, 1)
    sel = [([panel.col(c) for c in model_cols[out.model_names[out.res.problems[k].model]]], out.res.problems[k].level)
           for k in probs]
    d = E.forecast_dist(panel, coef, sel, cuts=out.cuts, level=out.level, forecast_out=True)
    torch.cuda.synchronize()
    so = panel.seg_off_h
    ids, months = panel.ids.cpu().numpy(), np.asarray(panel.month_index)
    ret3 = RO.horizon_return(panel.column_host(panel.col("retx")), RO.month_links(ids, so, months, 1), so, K3)
    exp = HO.batch(HO.forecast_horizon, so, d.forecast.cpu().numpy(), ret3, float(K3), G3, out.level.cpu().numpy(),
                   [lv for _, lv in sel], (0.1, 0.9))
    for j in range(len(probs)):
        ok = exp["status"][j] == 1
        for col, c in (("Avg", 0), ("Std", 1), ("p10", 6), ("p90", 7), ("Slope", 2), ("R2", 4)):
            x = exp["rec"][j, ok, c]
            x = x[~np.isnan(x)]
            assert len(x) >= 20 and scalar_close(tab[col].iloc[j], x.mean(), RTOL, float(np.sqrt(np.mean(x * x)))), (j, col)


def test_forecast_extrapolation_frames(E):
    """The frame-level entry point on the shuffled frame with a caller's forecast column: (b) fed
    horizon_oracle's pandas formulation of the 3-month returns; months with status 0 are absent."""
    from fmdrop import calc_Lewellen_2014 as CL
    df = _frame()
    rng = np.random.default_rng(41)
    F = 0.01 + 0.3 * df["return_12_2"].to_numpy() * 0.05 + rng.normal(0.0, 0.01, len(df))
    month = df["mthcaldt"].dt.year.to_numpy() * 12 + df["mthcaldt"].dt.month.to_numpy() - 1
    first = month == month.min()
    F[first] = np.nan                                            # a month without a forecast
    q = (0.1, 0.5, 0.9)
    monthly, summary = CL.forecast_extrapolation(df, F, K3, q=q, nw_lags=6)
    order = np.lexsort((df["permno"].to_numpy(), month))
    ret3 = RO.pandas_horizon(df["permno"].to_numpy(), month, df["retx"].to_numpy(), K3)
    so = np.concatenate([[0], np.cumsum(np.bincount(month - month.min()))]).astype(np.int64)
    exp = HO.forecast_horizon(so, F[order], ret3[order], float(K3), G3, q=q)
    cols = ["mean", "std", "slope", "intercept", "r2", "mean_1m", "p10", "p50", "p90"]
    assert list(monthly.columns) == cols + ["n", "n_ret"] and monthly.index.name == "mthcaldt"
    ok = exp["status"] == 1
    assert ok.sum() == 39 and len(monthly) == 39 and monthly.index.is_monotonic_increasing
    assert list(monthly["n"]) == list(exp["cnt"][ok, 0]) and list(monthly["n_ret"]) == list(exp["cnt"][ok, 1])
    assert (monthly["n_ret"].to_numpy()[-2:] == 0).all() and (monthly["n_ret"].to_numpy()[:-2] > 100).all()
    for c, name in enumerate(cols):
        assert_series_close(monthly[name].to_numpy(), exp["rec"][ok, c], name)
    assert list(summary.index) == cols and list(summary.columns) == ["mean", "se", "tstat", "nobs"]
    assert list(summary["nobs"]) == [39, 39, 37, 37, 37, 39, 39, 39, 39]
    x = exp["rec"][ok, 2]
    x = x[~np.isnan(x)]
    assert scalar_close(summary["mean"]["slope"], x.mean(), RTOL, float(np.sqrt(np.mean(x * x))))
    assert np.isfinite(summary[["mean", "nobs"]].to_numpy()).all()   # (the reference's NW variance may be negative)
    large, _ = CL.forecast_extrapolation(df, F, K3, universe="large")
    assert (large["n"].to_numpy() <= monthly["n"].reindex(large.index).to_numpy()).all() and len(large) >= 30
    plain, _ = CL.forecast_extrapolation(df, F, K3, decay=1.0, q=q)
    assert_series_close(plain["mean"].to_numpy(), monthly["mean"].to_numpy(), "decay 1: the same mean", rtol=1e-12)
    with pytest.raises(ValueError, match="decay must lie in"):
        CL.forecast_extrapolation(df, F, K3, decay=0.0)
