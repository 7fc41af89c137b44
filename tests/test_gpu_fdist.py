"""GPU tests of fm_forecast_dist (extension A14; paper Table 3's univariate properties), its engine
entry points, PipelineConfig(forecast_dist=True) and build_table_3: against the numpy restatement
(tests/fdist_oracle.py), bit for bit against the composition clip -> forecast -> forecast_dist_vector
and across the kernel's three forms, and end to end against oracle.fm_oracle's forecasts."""
import numpy as np
import pytest
import torch

import fdist_oracle as FO
import pipe_port_oracle as PPO
from fmtol import RTOL, assert_series_close, scalar_close
from test_gpu_pipeline_portfolios import SEL3, _dev, _panel, _pipe_panel, _random_coef, _random_panel

pytestmark = pytest.mark.gpu

LAYOUTS = ["f64", "planes"]
OUTS = ("rec", "cnt", "status")


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _host(d, forecast=False):
    torch.cuda.synchronize()
    h = {k: getattr(d, k).cpu().numpy() for k in OUTS}
    if forecast:
        h["forecast"] = d.forecast.cpu().numpy()
    return h


def _assert_same_bytes(got, exp, what):
    for k in exp:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


def _months(parts):
    seg_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return seg_off, np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])


def _check_restatement(got, exp, what):
    """cnt and status exact, quantiles exact, mean and sd at the project's 1e-9 rule; sd NaN exactly
    where the month has one eligible row."""
    assert np.array_equal(got["cnt"], exp["cnt"]) and np.array_equal(got["status"], exp["status"]), what
    assert np.array_equal(got["rec"][..., 2:], exp["rec"][..., 2:], equal_nan=True), what
    for j in range(exp["rec"].shape[0]):
        assert_series_close(got["rec"][j, :, 0], exp["rec"][j, :, 0], f"{what} mean[{j}]")
        assert_series_close(got["rec"][j, :, 1], exp["rec"][j, :, 1], f"{what} sd[{j}]")
        one = (exp["cnt"][j] == 1) & (exp["status"][j] == 1)
        assert np.array_equal(np.isnan(got["rec"][j, :, 1]), one | (exp["status"][j] == 0)), what


def _vector(E, seg_off, F, level=None, **kw):
    d = E.forecast_dist_vector(_dev(E, seg_off), _dev(E, F), level=_dev(E, level), **kw)
    return _host(d)


# ---------------------------------------------------------------- 1. edge months, plain source
EDGE_LENS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]


def _edge_months(longest):
    rng = np.random.default_rng(11)
    parts = [rng.standard_t(3, n) * 0.02 + 0.01 for n in EDGE_LENS if n <= longest]
    for p in parts:
        p[rng.random(len(p)) < 0.03] = np.nan
    parts[1][:] = 0.25                                           # one eligible row: sd NaN
    parts[2][:] = 0.5, -0.25
    parts.append(np.full(50, np.nan))                            # all NaN
    parts.append(np.full(100, 0.03125))                          # all equal
    z = np.concatenate([-rng.random(45), [-0.0] * 5, [0.0] * 5, rng.random(45)])   # signed zeros at the median
    parts.append(rng.permutation(z))
    parts.append(rng.permutation(1.0 + np.arange(200) * 2.0 ** -52))   # differ in the low 32 bits only
    w = rng.normal(size=80)
    w[[3, 40]] = np.inf, -np.inf                                 # +-inf: ineligible
    parts.append(w)
    return _months(parts)


@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("min_level", [0, 1])
@pytest.mark.parametrize("longest", [1024, 1025], ids=["256x4", "512x10"])
def test_edge_months_vs_restatement(E, longest, min_level, min_count):
    seg_off, F = _edge_months(longest)
    level = np.random.default_rng(12).integers(0, 3, len(F)).astype(np.uint8)
    level[int(seg_off[1]):int(seg_off[3])] = 2                   # the one- and two-row months stay eligible
    q = (0.1, 0.5, 0.9)
    got = _vector(E, seg_off, F, level, min_level=min_level, q=q, min_count=min_count)
    exp = FO.forecast_dist_batch(seg_off, [F], level, [min_level], q, min_count)
    assert int(np.diff(seg_off).max()) == longest
    assert exp["cnt"][0, 1] == 1 and exp["cnt"][0, 0] == 0 and (exp["status"][0, :3] == (min_count == 1) * np.array([0, 1, 1])).all()
    nlen = sum(n <= longest for n in EDGE_LENS)
    assert exp["cnt"][0, nlen] == 0 and exp["status"][0, nlen] == 0          # the all-NaN month
    assert np.all(exp["rec"][0, nlen + 1, [0, 2, 3, 4]] == 0.03125) and exp["rec"][0, nlen + 1, 1] == 0.0
    if min_level == 0:
        assert exp["rec"][0, nlen + 2, 3] == 0.0                             # a zero median between signed zeros
        assert exp["cnt"][0, nlen + 4] == 78
    _check_restatement(got, exp, f"edge {longest} level>={min_level} min_count={min_count}")


# ---------------------------------------------------------------- 2. the select paths
def _select_months():
    rng = np.random.default_rng(21)
    a = rng.normal(size=2100)
    a[rng.choice(2100, 52, replace=False)] = np.nan              # 2,048 eligible rows: the full sort
    b = rng.normal(size=2100)
    b[rng.choice(2100, 51, replace=False)] = np.nan              # 2,049: the sample select
    grid = rng.choice(np.linspace(-0.03, 0.03, 7), 5000)         # heavy ties: overfull buckets
    equal = np.full(3000, -0.0078125)
    out = rng.normal(size=5000)
    out[[17, 4000]] = 1e6, -1e6                                  # two far outliers
    return _months([a, b, grid, equal, out])


@pytest.mark.parametrize("q", [(0.001, 0.01, 0.1, 0.25, 0.5, 0.9, 0.99, 0.999), ()], ids=["nq8", "nq0"])
def test_select_paths_vs_restatement(E, q):
    seg_off, F = _select_months()
    got = _vector(E, seg_off, F, q=q)
    exp = FO.forecast_dist_batch(seg_off, [F], q=q)
    assert list(exp["cnt"][0]) == [2048, 2049, 5000, 3000, 5000] and exp["rec"].shape == (1, 5, 2 + len(q))
    _check_restatement(got, exp, f"select nq={len(q)}")
    # the 1,024 x 16 form runs its own sample select: the same bytes
    _assert_same_bytes(_vector(E, seg_off, F, q=q, max_seg_len=6000), got, "select, 1024 x 16")
    if q:   # the sort kernel's own copy of the selection gives the same breakpoints
        Fd = _dev(E, F)
        p = E.portfolio_sort(_dev(E, seg_off), Fd, torch.zeros_like(Fd), nport=len(q) + 1, q=q)
        assert np.array_equal(p.bp.cpu().numpy(), got["rec"][0, :, 2:])


# ---------------------------------------------------------------- 3. form independence
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
    kw = dict(min_level=[0, 1], q=(0.1, 0.9))
    base = _vector(E, seg_off, Fs, level, max_seg_len=900, **kw)
    _check_restatement(base, FO.forecast_dist_batch(seg_off, Fs, level, [0, 1], (0.1, 0.9)), "900-row months")
    for msl in (2000, 6000):
        _assert_same_bytes(_vector(E, seg_off, Fs, level, max_seg_len=msl, **kw), base, f"max_seg_len {msl}")
    _assert_same_bytes(_vector(E, seg_off, Fs, level, **kw), base, "repeated")
    lo = _vector(E, seg_off[:3], Fs[:, :1800].copy(), level[:1800], **kw)
    hi = _vector(E, seg_off[2:] - seg_off[2], Fs[:, 1800:].copy(), level[1800:], max_seg_len=6000, **kw)
    _assert_same_bytes({k: np.concatenate([lo[k], hi[k]], axis=1) for k in OUTS}, base, "month-sharded")


# ---------------------------------------------------------------- 4. fused equals composition
def _composition(E, panel, d, coef, sel, cuts, **kw):
    """clip the whole panel, one forecast vector per sort, then the plain source."""
    src = E.clip(panel, cuts) if cuts is not None else panel.values()
    F = torch.stack([E.forecast(panel, coef[j, :, :len(xs) + 1].contiguous(), cols=src[xs].contiguous())
                     for j, (xs, _) in enumerate(sel)])
    dist = E.forecast_dist_vector(panel.seg_off, F, level=_dev(E, d["level"]), min_level=[lv for _, lv in sel],
                                  max_seg_len=panel.max_seg_len, **kw)
    h = _host(dist)
    h["forecast"] = F.cpu().numpy()
    return h


def _fused(E, panel, d, coef, sel, cuts, **kw):
    return _host(E.forecast_dist(panel, coef, sel, cuts=cuts, level=_dev(E, d["level"]), forecast_out=True, **kw), True)


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
    if clipped:
        assert np.isnan(cuts.lo.cpu().numpy()[5, 3])             # the NaN-cut month
    coef = _dev(E, edge["coef"])
    kw = dict(q=(0.1, 0.5, 0.9), min_count=10)
    exp = _composition(E, panel, edge, coef, SEL3, cuts, **kw)
    got = _fused(E, panel, edge, coef, SEL3, cuts, **kw)
    s = edge["seg_off"]
    assert exp["status"][1, 9] == 0 and exp["cnt"][1, 9] == 0 and np.isnan(exp["forecast"][1, s[9]:s[10]]).all()
    assert (exp["status"][:, 7] == 0).all() and 0 < exp["cnt"][0, 7] < 10   # below min_count, not empty
    assert exp["status"][0].sum() == 11 and np.isinf(edge["cols"][1]).sum() == 1
    _assert_same_bytes(got, exp, f"{layout} clipped={clipped}")
    if layout == "f64" and clipped:
        lo, hi = PPO.winsor_cuts(edge["cols"], edge["seg_off"])
        Fs = [PPO.forecast(edge["cols"], edge["seg_off"], edge["coef"][j], xs, lo, hi) for j, (xs, _) in enumerate(SEL3)]
        assert np.array_equal(got["forecast"], np.stack(Fs), equal_nan=True)
        _check_restatement(got, FO.forecast_dist_batch(edge["seg_off"], Fs, edge["level"], [lv for _, lv in SEL3],
                                                       kw["q"], kw["min_count"]), "edge panel")


@pytest.mark.parametrize("T,N,K,layout", [(3, 1000, 30, "f64"), (2, 5000, 14, "f64"), (2, 5000, 14, "planes"),
                                          (1, 16384, 14, "f64")])
def test_instantiations(E, T, N, K, layout):
    d = _random_panel(50 + K, T, N, N, K + 1)
    panel = _panel(E, d, layout)
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    sel = [(list(range(1, K + 1)), 0), (list(range(K, 0, -1)), 1)]
    coef = _dev(E, _random_coef(60 + K, 2, T, K + 1))
    exp = _composition(E, panel, d, coef, sel, cuts)
    assert exp["status"].all() and (exp["cnt"] > N // 4).all()
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
    got = _vector(E, edge["seg_off"], exp["forecast"], edge["level"], min_level=[lv for _, lv in SEL3] * reps)
    _assert_same_bytes(got, {k: exp[k] for k in OUTS}, "18 sorts, vectors")


# ---------------------------------------------------------------- 5. refusal, empty calls
def test_too_long_month_refused(E):
    from fmcore._lib import FMError
    N = 16385
    d = _random_panel(71, 1, N, N, 3)
    panel = _panel(E, d, "f64")
    dev = panel.device
    out = E.ForecastDist(rec=torch.full((1, 1, 4), 7.0, dtype=torch.float64, device=dev),
                         cnt=torch.full((1, 1), 7, dtype=torch.int32, device=dev),
                         status=torch.full((1, 1), 7, dtype=torch.int32, device=dev))
    with pytest.raises(FMError, match=r"\(-3\)"):
        E.forecast_dist(panel, _dev(E, _random_coef(1, 1, 1, 3)), [([1, 2], 0)], out=out)
    with pytest.raises(FMError, match=r"\(-3\)"):
        E.forecast_dist_vector(panel.seg_off, panel.values()[1].contiguous())
    h = _host(out)
    assert (h["rec"] == 7.0).all() and (h["cnt"] == 7).all() and (h["status"] == 7).all()


def test_empty_calls(E, edge):
    panel = _panel(E, edge, "f64")
    d = E.forecast_dist(panel, _dev(E, edge["coef"])[:0], [], forecast_out=True)
    assert d.rec.shape == (0, 12, 4) and d.cnt.shape == (0, 12) and d.forecast.shape == (0, panel.nrows)
    dev = panel.device
    d = E.forecast_dist_vector(torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    assert d.rec.shape == (1, 0, 4) and d.status.shape == (1, 0)


# ---------------------------------------------------------------- 6. the pipeline
def _pipe_cfg(LW, **kw):
    c = PPO.PIPE
    return LW.PipelineConfig(**dict(dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"]), **kw))


@pytest.fixture(scope="module")
def pipe_runs(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    cfgs = dict(dist=dict(forecast_dist=True), both=dict(forecast_dist=True, portfolios=PPO.PIPE["nport"]),
                ports=dict(portfolios=PPO.PIPE["nport"]), planes=dict(forecast_dist=True))
    runs = {k: LW.run_pipeline(_pipe_panel(E, "planes" if k == "planes" else "f64"), _pipe_cfg(LW, **kw),
                               model_cols=fx["model_cols"]) for k, kw in cfgs.items()}
    torch.cuda.synchronize()
    return runs


def test_pipeline_vs_oracle_alone(pipe_runs):
    """Expected values: the restatement fed the forecasts and levels of pipe_port_oracle (from
    oracle.fm_oracle's rolling coefficients and numpy alone)."""
    keys, pe = PPO.pipeline_expected()
    fx = PPO.pipeline_fixture()
    out = pipe_runs["dist"]
    assert out.portfolios is None and pipe_runs["ports"].forecast_dist is None
    assert [(out.model_names[out.res.problems[k].model], out.res.problems[k].level)
            for k in out.forecast_dist_problems] == keys
    exp = FO.forecast_dist_batch(fx["seg_off"], pe["F"], pe["level"], [u for _, u in keys], (0.1, 0.9))
    got = _host(out.forecast_dist)
    assert np.array_equal(got["cnt"], exp["cnt"]) and np.array_equal(got["status"], exp["status"])
    assert (exp["status"].sum(axis=1) >= 20).all()
    s = out.forecast_dist_summary
    gm, gn = s.mean.cpu().numpy(), s.nobs.cpu().numpy()
    assert gm.shape == (len(keys), 4)
    for j in range(len(keys)):
        ok = exp["status"][j] == 1
        for c in range(4):
            assert_series_close(got["rec"][j, :, c], exp["rec"][j, :, c], f"rec[{j}, :, {c}]")
            x = exp["rec"][j, ok, c]
            assert np.isfinite(x).all() and gn[j, c] == ok.sum()
            assert scalar_close(gm[j, c], x.mean(), RTOL, float(np.sqrt(np.mean(x * x)))), (j, c)


def test_pipeline_layouts_and_companions_identical(pipe_runs):
    """The planes-only panel gives the same bytes; with portfolios on as well, both results equal
    their stand-alone runs bit for bit."""
    from test_gpu_pipeline_portfolios import _host as port_host
    base = _host(pipe_runs["dist"].forecast_dist)
    _assert_same_bytes(_host(pipe_runs["planes"].forecast_dist), base, "planes")
    _assert_same_bytes(_host(pipe_runs["both"].forecast_dist), base, "with portfolios")
    _assert_same_bytes(port_host(pipe_runs["both"].portfolios), port_host(pipe_runs["ports"].portfolios), "portfolios")
    for k in ("mean", "se", "tstat", "nobs"):
        a, b = (getattr(pipe_runs[r].forecast_dist_summary, k).cpu().numpy() for r in ("both", "dist"))
        assert a.tobytes() == b.tobytes(), k
    assert pipe_runs["both"].forecast_dist_problems == pipe_runs["both"].portfolio_problems


def test_pipeline_config_errors(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    panel = _pipe_panel(E, "f64")
    with pytest.raises(ValueError, match="standardize"):
        LW.run_pipeline(panel, _pipe_cfg(LW, forecast_dist=True, standardize=True), model_cols=fx["model_cols"])
    with pytest.raises(ValueError, match="forecasts"):
        LW.run_pipeline(panel, _pipe_cfg(LW, forecast_dist=True, forecasts=False), model_cols=fx["model_cols"])


# ---------------------------------------------------------------- 7. drop-in
def test_build_table_3(E, pipe_runs):
    from fmcore import lewellen as LW, synth
    from fmdrop import calc_Lewellen_2014 as CL
    c = PPO.PIPE
    df = synth.synth_frame(c["T"], c["N"], c["seed"], nan_rate=c["nan_rate"], present_rate=c["present_rate"], shuffle=True)
    tab = CL.build_table_3(df, window=c["window"], min_periods=c["min_periods"], lag=c["lag"])
    keys, _ = PPO.pipeline_expected()
    assert list(tab.index) == [(m, LW.SUBSET_NAMES[u]) for m, u in keys] and tab.index.names == ["model", "universe"]
    assert list(tab.columns) == ["Avg", "Std", "p10", "p90", "Slope", "S.E.", "t-stat", "R2"]
    out = pipe_runs["dist"]
    ps, ds = out.pred_summary, out.forecast_dist_summary
    probs = out.forecast_dist_problems
    assert tab[["Avg", "Std", "p10", "p90"]].to_numpy().tobytes() == ds.mean.cpu().numpy().tobytes()
    assert tab["Slope"].to_numpy().tobytes() == ps.mean.cpu().numpy()[probs, 0].tobytes()
    assert tab["S.E."].to_numpy().tobytes() == ps.se.cpu().numpy()[probs, 0].tobytes()
    assert tab["t-stat"].to_numpy().tobytes() == ps.tstat.cpu().numpy()[probs, 0].tobytes()
    assert tab["R2"].to_numpy().tobytes() == ps.mean.cpu().numpy()[probs, 1].tobytes()


def test_forecast_distribution_frames(E):
    """The frame-level entry point on a shuffled frame: months with status 0 are absent."""
    import pandas as pd
    from fmdrop import calc_Lewellen_2014 as CL
    rng = np.random.default_rng(41)
    month = np.repeat(np.arange(6), [40, 1, 30, 25, 60, 3])
    n = len(month)
    df = pd.DataFrame({"mthcaldt": month, "permno": rng.permutation(n), "me": np.exp(rng.normal(5, 2, n)),
                       "primaryexch": np.where(rng.random(n) < 0.4, "N", "Q")})
    F = rng.normal(0.01, 0.02, n)
    F[month == 3] = np.nan
    p = rng.permutation(n)
    df, F = df.iloc[p].reset_index(drop=True), F[p]
    monthly, summary = CL.forecast_distribution(df, F)
    order = np.lexsort((df["permno"].to_numpy(), df["mthcaldt"].to_numpy()))
    exp = FO.forecast_dist(np.concatenate([[0], np.cumsum(np.bincount(month))]), F[order])
    assert list(monthly.columns) == ["mean", "std", "p10", "p90", "n"] and list(monthly.index) == [0, 1, 2, 4, 5]
    assert monthly.index.name == "mthcaldt" and list(monthly["n"]) == [40, 1, 30, 60, 3]
    ok = exp["status"] == 1
    assert np.array_equal(monthly[["p10", "p90"]].to_numpy(), exp["rec"][ok, 2:])
    assert_series_close(monthly["mean"].to_numpy(), exp["rec"][ok, 0], "mean")
    assert_series_close(monthly["std"].to_numpy(), exp["rec"][ok, 1], "std")
    assert list(summary.index) == ["mean", "std", "p10", "p90"] and list(summary.columns) == ["mean", "tstat", "nobs"]
    assert list(summary["nobs"]) == [5, 4, 5, 5]
    assert scalar_close(summary["mean"]["p90"], exp["rec"][ok, 3].mean(), RTOL)
    large, _ = CL.forecast_distribution(df, F, universe="large")
    assert (large["n"].to_numpy() <= monthly["n"].reindex(large.index).to_numpy()).all() and len(large) >= 3
