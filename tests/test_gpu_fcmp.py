"""GPU tests of fm_forecast_compare (extension A15; paper Table 4, model comparison), its engine
entry points, PipelineConfig(forecast_compare=True) and build_table_4: against the numpy restatement
(tests/fcmp_oracle.py), bit for bit against the composition forecast vectors -> forecast_compare_vector
and across the kernel's three forms, and end to end on the pipeline fixture."""
import dataclasses

import numpy as np
import pytest
import torch

import fcmp_oracle as CO
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


def _host(c, forecast=False):
    torch.cuda.synchronize()
    h = {k: getattr(c, k).cpu().numpy() for k in OUTS}
    if forecast:
        h["forecast"] = c.forecast.cpu().numpy()
    return h


def _assert_same_bytes(got, exp, what):
    for k in exp:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


def _check_restatement(got, exp, what):
    """cnt and status exact, every series at the project's 1e-9 rule with the NaN pattern exact."""
    assert np.array_equal(got["cnt"], exp["cnt"]) and np.array_equal(got["status"], exp["status"]), what
    assert got["rec"].shape == exp["rec"].shape, what
    for p in range(exp["rec"].shape[0]):
        for c in range(CO.NREC):
            print(f"{what} pair {p} rec[:, {c}]: max |diff| "
                  f"{np.fmax.reduce(np.abs(got['rec'][p, :, c] - exp['rec'][p, :, c]), initial=0.0):.3e}")
            assert_series_close(got["rec"][p, :, c], exp["rec"][p, :, c], f"{what} pair {p} rec[:, {c}]")


def _vector(E, seg_off, Fs, ret, pairs, level=None, **kw):
    c = E.forecast_compare_vector(_dev(E, seg_off), _dev(E, Fs), _dev(E, ret), pairs, level=_dev(E, level), **kw)
    return _host(c)


# ---------------------------------------------------------------- 1. edge months, plain source
EDGE_LENS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]


def _related(rng, n):
    """F_a, F_b with a correlation near 0.45 and a return the residual predicts."""
    fa = rng.normal(0.01, 0.02, n)
    fb = 0.5 * fa + rng.normal(0.0, 0.02, n)
    return fa, fb, 1.5 * (fb - 0.5 * fa) + rng.normal(0.0, 0.1, n)


def _edge_months(longest):
    """-> seg_off, [F_a, F_b], ret and the named months' indices."""
    rng = np.random.default_rng(11)
    parts = [list(_related(rng, n)) for n in EDGE_LENS if n <= longest]
    for p in parts:
        for x in p:
            x[rng.random(len(x)) < 0.03] = np.nan
    parts[1] = [np.array([0.25]), np.array([0.5]), np.array([0.01])]                  # one row: no regression
    parts[2] = [np.array([0.5, -0.25]), np.array([0.125, 0.75]), np.array([0.01, np.nan])]   # two rows: a perfect fit, one return
    parts[3] = [np.array([0.01, 0.03, 0.02]), np.array([0.02, 0.01, 0.03]), np.array([0.05, -0.02, 0.01])]
    named = {}

    def add(name, n):
        named[name] = len(parts)
        parts.append(list(_related(rng, n)))
        return parts[-1]

    add("nan", 50)[1][:] = np.nan                                # one forecast all NaN
    m = add("same", 100)
    m[1] = m[0].copy()                                           # both forecasts identical
    add("const", 80)[0][:] = 0.25                                # constant F_a
    add("noret", 90)[2][:] = np.nan                              # returns all NaN
    m = add("finf", 80)
    m[0][[3, 40]] = np.inf, -np.inf                              # +-inf in a forecast: the row is ineligible
    m[1][7] = np.inf
    add("rinf", 80)[2][[5, 50]] = np.inf, -np.inf                # +-inf in the return: outside R only
    seg_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    Fs = np.stack([np.concatenate([p[i] for p in parts]) for i in (0, 1)])
    return seg_off, Fs, np.concatenate([p[2] for p in parts]), named


@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("min_level", [0, 1])
@pytest.mark.parametrize("longest", [1024, 1025], ids=["256x4", "512x10"])
def test_edge_months_vs_restatement(E, longest, min_level, min_count):
    seg_off, Fs, ret, named = _edge_months(longest)
    assert int(np.diff(seg_off).max()) == longest
    level = np.random.default_rng(12).integers(0, 3, Fs.shape[1]).astype(np.uint8)
    level[int(seg_off[1]):int(seg_off[4])] = 2                   # the one-, two- and three-row months stay whole
    pairs = [(0, 1, min_level)]
    got = _vector(E, seg_off, Fs, ret, pairs, level, min_count=min_count)
    exp = CO.forecast_compare_batch(seg_off, Fs, ret, pairs, level, min_count)
    rec, cnt, st = exp["rec"][0], exp["cnt"][0], exp["status"][0]
    # the cases the months are built for are all there, in the restatement's own output
    assert list(cnt[:4, 0]) == [0, 1, 2, 3] and list(st[:4]) == [0, 0, int(min_count <= 2), 1]
    assert cnt[2, 1] == 1 and (min_count > 2 or (np.isfinite(rec[2, :4]).all() and np.isnan(rec[2, 4:]).all()))
    t = named["nan"]
    assert cnt[t, 0] == 0 and st[t] == 0 and np.isnan(rec[t]).all()
    t = named["same"]
    assert st[t] == 1 and rec[t, 1] == 1.0 and rec[t, 3] == 0.0 and np.isnan(rec[t, 4])
    t = named["const"]
    assert st[t] == 1 and np.isnan(rec[t, 0]) and np.isnan(rec[t, 1])
    t = named["noret"]
    assert st[t] == 1 and cnt[t, 1] == 0 and np.isnan(rec[t, 4:]).all() and np.isfinite(rec[t, :4]).all()
    if min_level == 0:
        assert list(cnt[named["finf"]]) == [77, 77] and list(cnt[named["rinf"]]) == [80, 78]
    # the restatement alone is stable: away from the built degenerate months the residual does not cancel
    plain = (st == 1) & np.isfinite(rec[:, 0])
    plain[[2, named["same"]]] = False
    assert plain.sum() >= 12 and (np.abs(rec[plain, 0]) < 0.99).all(), np.abs(rec[plain, 0]).max()
    _check_restatement(got, exp, f"edge {longest} level>={min_level} min_count={min_count}")
    # the two exact results, on the device itself
    t = named["same"]
    assert got["rec"][0, t, 1] == 1.0 and got["rec"][0, t, 3] == 0.0 and np.isnan(got["rec"][0, t, 4:]).all()


# ---------------------------------------------------------------- 2. form independence
def test_form_independence(E):
    """The same 900-row months under max_seg_len 900 / 2,000 / 6,000 (the 256 x 4, 512 x 10 and
    1,024 x 16 forms), repeated and month-sharded into two calls: the same bytes in every output."""
    rng = np.random.default_rng(31)
    parts = [_related(rng, 900) for _ in range(5)]
    seg_off = (900 * np.arange(6)).astype(np.int64)
    Fa, Fb, ret = (np.concatenate([p[i] for p in parts]) for i in range(3))
    Fs = np.stack([Fa, Fb, 0.3 * Fa - 0.2 * Fb + rng.normal(0.0, 0.01, Fa.size)])
    for x in (Fs[0], Fs[1], Fs[2], ret):
        x[rng.random(x.size) < 0.05] = np.nan
    level = rng.integers(0, 3, Fa.size).astype(np.uint8)
    pairs = [(0, 1, 0), (1, 2, 1), (0, 2, 2), (2, 0, 0)]
    base = _vector(E, seg_off, Fs, ret, pairs, level, max_seg_len=900)
    _check_restatement(base, CO.forecast_compare_batch(seg_off, Fs, ret, pairs, level), "900-row months")
    for msl in (2000, 6000):
        _assert_same_bytes(_vector(E, seg_off, Fs, ret, pairs, level, max_seg_len=msl), base, f"max_seg_len {msl}")
    _assert_same_bytes(_vector(E, seg_off, Fs, ret, pairs, level), base, "repeated")
    lo = _vector(E, seg_off[:3], Fs[:, :1800].copy(), ret[:1800], pairs, level[:1800])
    hi = _vector(E, seg_off[2:] - seg_off[2], Fs[:, 1800:].copy(), ret[1800:], pairs, level[1800:], max_seg_len=6000)
    _assert_same_bytes({k: np.concatenate([lo[k], hi[k]], axis=1) for k in OUTS}, base, "month-sharded")


# ---------------------------------------------------------------- 3. fused equals composition
def _fused(E, panel, d, coef, sel, pairs, cuts, **kw):
    c = E.forecast_compare(panel, coef, sel, pairs, cuts=cuts, ret=d["ret"], level=_dev(E, d["level"]),
                           forecast_out=True, **kw)
    return c, _host(c, True)


def _composition(E, panel, d, fused, pairs, **kw):
    """The fused call's own forecast vectors and the return column through the plain source."""
    r = panel.values()[d["ret"]].contiguous()
    c = E.forecast_compare_vector(panel.seg_off, fused.forecast, r, pairs, level=_dev(E, d["level"]),
                                  max_seg_len=panel.max_seg_len, **kw)
    h = _host(c)
    h["forecast"] = fused.forecast.cpu().numpy()
    return h


@pytest.fixture(scope="module")
def edge():
    d = _random_panel(3, 12, 250, 300, 6, edge=True)
    d["coef"] = _random_coef(4, 3, 12, 6, nan_at=(1, 9, 2))   # sort 1, month 9: a NaN slope
    return d


# forecast 0 is forecast a of two pairs; (1, 1): a forecast against itself
PAIRS3 = [(0, 1, 0), (0, 2, 1), (1, 2, 2), (1, 1, 0)]


@pytest.mark.parametrize("clipped", [True, False], ids=["cuts", "nocuts"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_equals_composition(E, edge, layout, clipped):
    panel = _panel(E, edge, layout)
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY) if clipped else None
    coef = _dev(E, edge["coef"])
    kw = dict(min_count=10)
    fused, got = _fused(E, panel, edge, coef, SEL3, PAIRS3, cuts, **kw)
    exp = _composition(E, panel, edge, fused, PAIRS3, **kw)
    s = edge["seg_off"]
    assert np.isnan(got["forecast"][1, s[9]:s[10]]).all()                     # the NaN coefficient's month
    assert (got["status"][[0, 2, 3], 9] == 0).all() and (got["cnt"][[0, 2, 3], 9] == 0).all() and got["status"][1, 9] == 1
    assert (got["status"][:, 7] == 0).all() and 0 < got["cnt"][0, 7, 0] < 10   # below min_count, not empty
    ok = got["status"][3] == 1
    assert ok.sum() == 10 and (got["rec"][3, ok, 1] == 1.0).all() and (got["rec"][3, ok, 3] == 0.0).all()
    assert np.isnan(got["rec"][3, :, 4:]).all()
    _assert_same_bytes(got, exp, f"{layout} clipped={clipped}")
    dist = E.forecast_dist(panel, coef, SEL3, cuts=cuts, level=_dev(E, edge["level"]), forecast_out=True)
    assert dist.forecast.cpu().numpy().tobytes() == got["forecast"].tobytes()
    if layout == "f64" and clipped:
        lo, hi = PPO.winsor_cuts(edge["cols"], edge["seg_off"])
        Fs = np.stack([PPO.forecast(edge["cols"], edge["seg_off"], edge["coef"][j], xs, lo, hi) for j, (xs, _) in enumerate(SEL3)])
        assert np.array_equal(got["forecast"], Fs, equal_nan=True)
        _check_restatement(got, CO.forecast_compare_batch(edge["seg_off"], Fs, edge["cols"][0], PAIRS3, edge["level"],
                                                          kw["min_count"]), "edge panel")


@pytest.mark.parametrize("T,N,K,layout", [(3, 1000, 30, "f64"), (2, 5000, 14, "f64"), (2, 5000, 14, "planes"),
                                          (1, 16384, 14, "f64")])
def test_instantiations(E, T, N, K, layout):
    d = _random_panel(50 + K, T, N, N, K + 1)
    panel = _panel(E, d, layout)
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    sel = [(list(range(1, K + 1)), 0), (list(range(K, 0, -1)), 1)]
    pairs = [(0, 1, 0), (1, 0, 1)]
    coef = _dev(E, _random_coef(60 + K, 2, T, K + 1))
    fused, got = _fused(E, panel, d, coef, sel, pairs, cuts)
    assert got["status"].all() and (got["cnt"] > N // 4).all() and np.isfinite(got["rec"]).all()
    _assert_same_bytes(got, _composition(E, panel, d, fused, pairs), f"{T}x{N} K={K} {layout}")


# ---------------------------------------------------------------- 4. batching
def test_more_pairs_than_one_launch(E, edge):
    """19 pairs over 18 forecasts: FM_MAX_PAIRS = FM_MAX_SORTS = 16 per launch, so several launches
    write one batched result, equal to the per-pair results; the last launch's forecasts (0, 15, 16,
    17) are not consecutive."""
    from fmcore import _lib as L
    panel = _panel(E, edge, "planes")
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    coef = _dev(E, edge["coef"])
    _, one = _fused(E, panel, edge, coef, SEL3, [(0, 1, 0), (1, 2, 1), (0, 2, 2), (0, 2, 0)], cuts)
    reps = 6
    pairs = [(3 * r + a, 3 * r + b, lv) for r in range(reps) for a, b, lv in ((0, 1, 0), (1, 2, 1), (0, 2, 2))] + [(0, 17, 0)]
    assert len(pairs) > L.FM_MAX_PAIRS and 3 * reps > L.FM_MAX_SORTS
    assert [p0 for p0, _, _ in E._pair_batches("t", pairs, 3 * reps)[1]] == [0, 15]
    exp = {k: np.concatenate([one[k][:3]] * reps + [one[k][3:]]) for k in OUTS}
    exp["forecast"] = np.concatenate([one["forecast"]] * reps)
    _, got = _fused(E, panel, edge, coef.repeat(reps, 1, 1), SEL3 * reps, pairs, cuts)
    _assert_same_bytes(got, exp, "19 pairs, fused")
    r = panel.values()[edge["ret"]].contiguous()
    vec = _host(E.forecast_compare_vector(panel.seg_off, _dev(E, exp["forecast"]), r, pairs, level=_dev(E, edge["level"])))
    _assert_same_bytes(vec, {k: exp[k] for k in OUTS}, "19 pairs, vectors")


# ---------------------------------------------------------------- 5. refusal, empty calls
def test_too_long_month_refused(E):
    from fmcore._lib import FMError
    N = 16385
    d = _random_panel(71, 1, N, N, 3)
    panel = _panel(E, d, "f64")
    dev = panel.device
    out = E.ForecastCompare(rec=torch.full((1, 1, 7), 7.0, dtype=torch.float64, device=dev),
                            cnt=torch.full((1, 1, 2), 7, dtype=torch.int32, device=dev),
                            status=torch.full((1, 1), 7, dtype=torch.int32, device=dev))
    with pytest.raises(FMError, match=r"\(-3\)"):
        E.forecast_compare(panel, _dev(E, _random_coef(1, 2, 1, 3)), [([1, 2], 0), ([2, 1], 0)], [(0, 1, 0)], ret=0, out=out)
    with pytest.raises(FMError, match=r"\(-3\)"):
        E.forecast_compare_vector(panel.seg_off, panel.values()[1:3].contiguous(), panel.values()[0].contiguous(), [(0, 1, 0)])
    h = _host(out)
    assert (h["rec"] == 7.0).all() and (h["cnt"] == 7).all() and (h["status"] == 7).all()


def test_empty_calls(E, edge):
    panel = _panel(E, edge, "f64")
    coef = _dev(E, edge["coef"])
    c = E.forecast_compare(panel, coef[:0], [], [], ret=0, forecast_out=True)
    assert c.rec.shape == (0, 12, 7) and c.cnt.shape == (0, 12, 2) and c.status.shape == (0, 12)
    assert c.forecast.shape == (0, panel.nrows)
    c = E.forecast_compare(panel, coef, SEL3, [], ret=0)          # forecasts, but no pair
    assert c.rec.shape == (0, 12, 7) and c.forecast is None
    dev = panel.device
    c = E.forecast_compare_vector(torch.zeros(1, dtype=torch.int64, device=dev), torch.empty((2, 0), dtype=torch.float64, device=dev),
                                  torch.empty(0, dtype=torch.float64, device=dev), [(0, 1, 0)])
    torch.cuda.synchronize()
    assert c.rec.shape == (1, 0, 7) and c.cnt.shape == (1, 0, 2) and c.status.shape == (1, 0)


# ---------------------------------------------------------------- 6. the pipeline
def _pipe_cfg(LW, **kw):
    c = PPO.PIPE
    return LW.PipelineConfig(**dict(dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"]), **kw))


@pytest.fixture(scope="module")
def pipe_runs(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    cfgs = dict(cmp=("f64", dict(forecast_compare=True)), planes=("planes", dict(forecast_compare=True)), off=("f64", {}))
    runs = {k: LW.run_pipeline(_pipe_panel(E, layout), _pipe_cfg(LW, **kw), model_cols=fx["model_cols"])
            for k, (layout, kw) in cfgs.items()}
    torch.cuda.synchronize()
    return runs


def _pair_keys(out):
    pr = out.res.problems
    return [(pr[a].level, out.model_names[pr[a].model], out.model_names[pr[b].model]) for a, b in out.forecast_compare_pairs]


def test_pipeline_vs_restatement(E, pipe_runs):
    """Expected values: the restatement fed the forecasts forecast_dist(forecast_out=True) returns for
    the pipeline's own coefficient rows, cuts and levels."""
    fx = PPO.pipeline_fixture()
    out = pipe_runs["cmp"]
    names = list(fx["model_cols"])
    assert _pair_keys(out) == [(u, names[i], names[j]) for u in (0, 1, 2) for i, j in ((0, 1), (0, 2), (1, 2))]
    pr = out.res.problems
    probs = [k for k, p in enumerate(pr) if out.model_names[p.model] != "Figure 1"]
    pairs = [(probs.index(a), probs.index(b), pr[a].level) for a, b in out.forecast_compare_pairs]
    assert all(pr[a].level == pr[b].level for a, b in out.forecast_compare_pairs)
    panel = _pipe_panel(E, "f64")
    coef = E.lagged_coefficients(out.rolling, out.ix, probs, PPO.PIPE["lag"])
    sel = [([panel.col(c) for c in fx["model_cols"][out.model_names[pr[k].model]]], pr[k].level) for k in probs]
    dist = E.forecast_dist(panel, coef, sel, cuts=out.cuts, level=out.level, forecast_out=True)
    exp = CO.forecast_compare_batch(fx["seg_off"], dist.forecast.cpu().numpy(), fx["cols"][fx["names"].index("retx")],
                                    pairs, out.level.cpu().numpy())
    got = _host(out.forecast_compare)
    assert (exp["status"].sum(axis=1) >= 20).all() and got["rec"].shape == (9, PPO.PIPE["T"], 7)
    _check_restatement(got, exp, "pipeline")
    s = out.forecast_compare_summary
    gm, gn = s.mean.cpu().numpy(), s.nobs.cpu().numpy()
    assert gm.shape == (9, 7)
    for p in range(9):
        ok = exp["status"][p] == 1
        for c in range(7):
            x = exp["rec"][p, ok, c]
            assert np.isfinite(x).all() and gn[p, c] == ok.sum()
            assert scalar_close(gm[p, c], x.mean(), RTOL, float(np.sqrt(np.mean(x * x)))), (p, c)


def _other_fields(out):
    """Every output of a pipeline run but the comparison's, as host arrays by name; the tables that are
    indexed by fitted-month row (ix.idx, rolling, pred, pred_status) up to each problem's count and
    the moments of the fitted months: what lies beyond is never written."""
    h = lambda t: t.cpu().numpy()
    count = h(out.ix.count)
    rows = np.arange(out.ix.idx.shape[1])[None, :] < count[:, None]           # [P, T]
    fitted = (h(out.res.status) & 1) != 0                                     # [T, P]
    d = {"res.rec": h(out.res.rec), "res.status": h(out.res.status), "res.moments": h(out.res.moments)[fitted],
         "ix.count": count, "ix.idx": h(out.ix.idx)[rows], "rolling": h(out.rolling)[rows], "pred": h(out.pred)[rows],
         "pred_status": h(out.pred_status)[rows], "level": h(out.level),
         "breakpoints[0]": h(out.breakpoints[0]), "breakpoints[1]": h(out.breakpoints[1])}
    for name in ("summary", "pred_summary"):
        for k in ("mean", "se", "tstat", "nobs"):
            d[f"{name}.{k}"] = h(getattr(getattr(out, name), k))
    for k in ("lo", "hi", "nvalid", "center"):
        d[f"cuts.{k}"] = h(getattr(out.cuts, k))
    return d


def test_pipeline_layouts_identical_and_nothing_else_moves(pipe_runs):
    """The planes-only panel gives the same bytes; switching the option on leaves every other output
    of the run as it was, bit for bit."""
    base = _host(pipe_runs["cmp"].forecast_compare)
    _assert_same_bytes(_host(pipe_runs["planes"].forecast_compare), base, "planes")
    for k in ("mean", "se", "tstat", "nobs"):
        a, b = (getattr(pipe_runs[r].forecast_compare_summary, k).cpu().numpy() for r in ("planes", "cmp"))
        assert a.tobytes() == b.tobytes(), k
    off, on = pipe_runs["off"], pipe_runs["cmp"]
    assert off.forecast_compare is None and off.forecast_compare_summary is None and off.forecast_compare_pairs is None
    assert on.portfolios is None and on.forecast_dist is None
    assert [dataclasses.asdict(p) for p in on.res.problems] == [dataclasses.asdict(p) for p in off.res.problems]
    assert on.model_names == off.model_names and on.model_cols == off.model_cols
    _assert_same_bytes(_other_fields(on), _other_fields(off), "forecast_compare on / off")


def test_pipeline_config_errors(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    panel = _pipe_panel(E, "f64")
    with pytest.raises(ValueError, match="forecast_compare excludes standardize"):
        LW.run_pipeline(panel, _pipe_cfg(LW, forecast_compare=True, standardize=True), model_cols=fx["model_cols"])
    with pytest.raises(ValueError, match="forecast_compare needs forecasts"):
        LW.run_pipeline(panel, _pipe_cfg(LW, forecast_compare=True, forecasts=False), model_cols=fx["model_cols"])


# ---------------------------------------------------------------- 7. drop-in
def test_build_table_4(E, pipe_runs):
    from fmcore import lewellen as LW, synth
    from fmdrop import calc_Lewellen_2014 as CL
    c = PPO.PIPE
    df = synth.synth_frame(c["T"], c["N"], c["seed"], nan_rate=c["nan_rate"], present_rate=c["present_rate"], shuffle=True)
    tab = CL.build_table_4(df, window=c["window"], min_periods=c["min_periods"], lag=c["lag"])
    assert list(tab.index) == [(LW.SUBSET_NAMES[u], f"Model {j} on Model {i}") for u in (0, 1, 2)
                               for i, j in ((1, 2), (1, 3), (2, 3))]
    assert tab.index.names == ["universe", "comparison"]
    assert list(tab.columns) == ["Correlation", "Slope", "Res. std.", "Pred. slope", "S.E.", "t-stat"]
    s = pipe_runs["cmp"].forecast_compare_summary
    mean, se, t = s.mean.cpu().numpy(), s.se.cpu().numpy(), s.tstat.cpu().numpy()
    assert tab[["Correlation", "Slope", "Res. std.", "Pred. slope"]].to_numpy().tobytes() == \
        np.ascontiguousarray(mean[:, [0, 1, 3, 4]]).tobytes()
    assert tab["S.E."].to_numpy().tobytes() == se[:, 4].tobytes() and tab["t-stat"].to_numpy().tobytes() == t[:, 4].tobytes()
    assert np.isfinite(tab.to_numpy()).all() and (np.abs(tab["Correlation"]) <= 1.0).all()


def test_forecast_comparison_frames(E):
    """The frame-level entry point on a shuffled frame: months with status 0 are absent."""
    import pandas as pd
    from fmdrop import calc_Lewellen_2014 as CL
    rng = np.random.default_rng(41)
    month = np.repeat(np.arange(6), [40, 1, 30, 25, 60, 3])
    n = len(month)
    df = pd.DataFrame({"mthcaldt": month, "permno": rng.permutation(n), "me": np.exp(rng.normal(5, 2, n)),
                       "primaryexch": np.where(rng.random(n) < 0.4, "N", "Q")})
    Fa, Fb, r = _related(rng, n)
    Fb[month == 3] = np.nan
    r[rng.random(n) < 0.1] = np.nan
    df["retx"] = r
    p = rng.permutation(n)
    df, Fa, Fb = df.iloc[p].reset_index(drop=True), Fa[p], Fb[p]
    monthly, summary = CL.forecast_comparison(df, Fa, Fb)
    order = np.lexsort((df["permno"].to_numpy(), df["mthcaldt"].to_numpy()))
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(month))])
    exp = CO.forecast_compare(seg_off, Fa[order], Fb[order], df["retx"].to_numpy()[order])
    assert list(monthly.columns) == CL.COMPARISON_COLUMNS + ["n", "n_ret"] and list(monthly.index) == [0, 2, 4, 5]
    assert monthly.index.name == "mthcaldt" and list(monthly["n"]) == [40, 30, 60, 3]
    ok = exp["status"] == 1
    assert list(monthly["n_ret"]) == list(exp["cnt"][ok, 1])
    for j, c in enumerate(CL.COMPARISON_COLUMNS):
        assert_series_close(monthly[c].to_numpy(), exp["rec"][ok, j], c)
    assert list(summary.index) == CL.COMPARISON_COLUMNS and list(summary.columns) == ["mean", "se", "tstat", "nobs"]
    assert list(summary["nobs"]) == [4] * 7
    assert scalar_close(summary["mean"]["slope"], exp["rec"][ok, 1].mean(), RTOL)
    large, _ = CL.forecast_comparison(df, Fa, Fb, universe="large")
    assert (large["n"].to_numpy() <= monthly["n"].reindex(large.index).to_numpy()).all() and len(large) >= 2
