"""GPU tests of the fused forecast-and-sort (fm_forecast_portfolio_sort), the lagged coefficient
tables (fm_lagged_coef) and PipelineConfig(portfolios=...): bit for bit against the composition
clip -> forecast -> portfolio_sort of the existing entry points, against the numpy restatement
(tests/pipe_port_oracle.py), and end to end against oracle.fm_oracle alone."""
import numpy as np
import pytest
import torch

import pipe_port_oracle as PPO
import port_oracle as PO
from fmtol import RTOL, assert_series_close, scalar_close

pytestmark = pytest.mark.gpu

LAYOUTS = ["f64", "planes"]
OUTS = ("bp", "port", "rec", "cnt", "status")


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _dev(E, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(E.require_device())


def _host(p, forecast=False):
    torch.cuda.synchronize()
    h = {k: getattr(p, k).cpu().numpy() for k in OUTS}
    if forecast:
        h["forecast"] = p.forecast.cpu().numpy()
    return h


def _panel(E, d, layout):
    """A DevicePanel of the host panel ``d`` (rows already month-sorted) in ``layout``."""
    month = np.repeat(np.arange(len(d["seg_off"]) - 1), np.diff(d["seg_off"]))
    names = [f"c{i}" for i in range(len(d["cols"]))]
    return E.panel_from_arrays(d["cols"], names, month, me=d["W"], nyse=d["nyse"], layout=layout)


def _composition(E, panel, d, coef, sel, cuts, **kw):
    """The parent's way: clip the whole panel, then per sort one forecast vector and one sort."""
    vals = panel.values()
    src = E.clip(panel, cuts) if cuts is not None else vals
    outs = []
    for j, (xs, lv) in enumerate(sel):
        K = len(xs)
        F = E.forecast(panel, coef[j, :, :K + 1].contiguous(), cols=src[xs].contiguous())
        p = E.portfolio_sort(panel.seg_off, F, vals[d["ret"]].contiguous(), weight=_dev(E, d["W"]),
                             level=_dev(E, d["level"]), nyse=_dev(E, d["nyse"]), min_level=lv,
                             max_seg_len=panel.max_seg_len, **kw)
        h = _host(p)
        h["forecast"] = F.cpu().numpy()
        outs.append(h)
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def _fused(E, panel, d, coef, sel, cuts, **kw):
    p = E.forecast_portfolio_sort(panel, coef, sel, cuts=cuts, ret=d["ret"], weight=_dev(E, d["W"]),
                                  level=_dev(E, d["level"]), nyse=_dev(E, d["nyse"]), forecast_out=True, **kw)
    return _host(p, forecast=True)


def _assert_same_bytes(got, exp, what):
    for k in exp:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


def _random_panel(seed, T, lo, hi, C, edge=False):
    """Ragged months, column 0 the return, columns 1.. the predictors."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=T)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    cols = [rng.normal(0.01, 0.15, n)] + [rng.standard_t(3, n) * (0.5 + c) for c in range(1, C)]
    cols[0][rng.random(n) < 0.05] = np.nan
    for c in range(1, C):
        cols[c][rng.random(n) < 0.02] = np.nan
    if edge:
        cols[1][int(seg_off[2]) + 7] = np.inf
        cols[2][int(seg_off[5]) + 11] = -np.inf
        cols[5][int(seg_off[3]) + 3:int(seg_off[4])] = np.nan    # 3 valid values: NaN cuts for (5, month 3)
        cols[1][int(seg_off[7]) + 8:int(seg_off[8])] = np.nan    # 8 valid values: fewer than min_count eligible
    W = np.exp(rng.normal(5.0, 2.0, n))
    W[rng.random(n) < 0.01] = np.nan
    return dict(seg_off=seg_off, cols=cols, ret=0, W=W, level=rng.integers(0, 3, n).astype(np.uint8),
                nyse=(rng.random(n) < 0.4).astype(np.uint8))


def _random_coef(seed, nsel, T, K1, nan_at=None):
    rng = np.random.default_rng(seed)
    coef = rng.normal(0.0, 0.01, (nsel, T, K1))
    if nan_at is not None:
        coef[nan_at] = np.nan
    return coef


# ---------------------------------------------------------------- 1 / 2. the ragged edge panel
SEL3 = [([1], 0), ([1, 2, 3], 1), ([1, 2, 3, 4, 5], 2)]


@pytest.fixture(scope="module")
def edge():
    d = _random_panel(3, 12, 250, 300, 6, edge=True)
    d["coef"] = _random_coef(4, 3, 12, 6, nan_at=(1, 9, 2))   # sort 1, month 9: a NaN slope
    return d


@pytest.fixture(scope="module")
def edge_cuts_host(edge):
    return PPO.winsor_cuts(edge["cols"], edge["seg_off"])


@pytest.mark.parametrize("clipped", [True, False], ids=["cuts", "nocuts"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_equals_composition(E, edge, layout, clipped):
    panel = _panel(E, edge, layout)
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY) if clipped else None
    if clipped:
        lo = cuts.lo.cpu().numpy()
        assert np.isnan(lo[5, 3]) and np.isfinite(np.delete(lo, 3, axis=1)).all()
    coef = _dev(E, edge["coef"])
    exp = _composition(E, panel, edge, coef, SEL3, cuts)
    got = _fused(E, panel, edge, coef, SEL3, cuts)
    # the cases the panel is built for are all there
    assert exp["status"][1, 9] == 0 and np.isnan(exp["forecast"][1, edge["seg_off"][9]:edge["seg_off"][10]]).all()
    assert (exp["status"][:, 7] == 0).all() and exp["status"][2, 3] == 0
    assert exp["status"][0].sum() == 11 and exp["status"][1].sum() == 10 and exp["status"][2].sum() == 10
    assert np.isinf(edge["cols"][1]).sum() == 1 and np.isinf(edge["cols"][2]).sum() == 1
    _assert_same_bytes(got, exp, f"{layout} clipped={clipped}")


def test_fused_vs_restatement(E, edge, edge_cuts_host):
    panel = _panel(E, edge, "f64")
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    lo, hi = edge_cuts_host
    assert np.array_equal(cuts.lo.cpu().numpy(), lo, equal_nan=True)
    assert np.array_equal(cuts.hi.cpu().numpy(), hi, equal_nan=True)
    got = _fused(E, panel, edge, _dev(E, edge["coef"]), SEL3, cuts)
    exp = PPO.forecast_portfolio_sort(edge["cols"], edge["seg_off"], edge["coef"], SEL3, lo, hi, ret=0, W=edge["W"],
                                      level=edge["level"], nyse=edge["nyse"], nport=10)
    _check_restatement(got, exp, "edge")


def test_more_sorts_than_one_launch(E, edge):
    """18 sorts: FM_MAX_SORTS = 16 per launch, so two launches write one batched result."""
    from fmcore import _lib as L
    panel = _panel(E, edge, "planes")
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    coef = _dev(E, edge["coef"])
    one = _fused(E, panel, edge, coef, SEL3, cuts)
    reps = 6
    assert 3 * reps > L.FM_MAX_SORTS
    got = _fused(E, panel, edge, coef.repeat(reps, 1, 1), SEL3 * reps, cuts)
    _assert_same_bytes(got, {k: np.concatenate([v] * reps) for k, v in one.items()}, "18 sorts")


def _check_restatement(got, exp, what):
    for k in ("status", "port", "cnt"):
        assert np.array_equal(got[k], exp[k]), (what, k)
    assert np.array_equal(got["bp"], exp["bp"], equal_nan=True), what
    nsel, _, n1, _ = exp["rec"].shape
    for j in range(nsel):
        for k in range(n1):
            for c in range(4):
                assert_series_close(got["rec"][j, :, k, c], exp["rec"][j, :, k, c], f"{what} rec[{j}, :, {k}, {c}]")


# ---------------------------------------------------------------- 3. the three instantiations
@pytest.mark.parametrize("T,N,K,layout", [(3, 1000, 30, "f64"), (2, 5000, 14, "f64"), (2, 5000, 14, "planes"),
                                          (1, 16384, 14, "f64")])
def test_instantiations(E, T, N, K, layout):
    d = _random_panel(50 + K, T, N, N, K + 1)
    panel = _panel(E, d, layout)
    cuts = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY)
    sel = [(list(range(1, K + 1)), 0), (list(range(K, 0, -1)), 1)]
    coef = _dev(E, _random_coef(60 + K, 2, T, K + 1))
    kw = dict(nyse_breakpoints=True)
    exp = _composition(E, panel, d, coef, sel, cuts, **kw)
    assert exp["status"].all() and (exp["cnt"] > 0).all()
    got = _fused(E, panel, d, coef, sel, cuts, **kw)
    _assert_same_bytes(got, exp, f"{T}x{N} K={K} {layout}")


def test_too_long_month_refused(E):
    from fmcore._lib import FMError
    N = 16385
    d = _random_panel(71, 1, N, N, 3)
    panel = _panel(E, d, "f64")
    out = E.Portfolios(bp=torch.full((1, 1, 9), 7.0, dtype=torch.float64, device=panel.device),
                       port=torch.full((1, N), 77, dtype=torch.uint8, device=panel.device),
                       rec=torch.full((1, 1, 11, 4), 7.0, dtype=torch.float64, device=panel.device),
                       cnt=torch.full((1, 1, 10), 7, dtype=torch.int32, device=panel.device),
                       status=torch.full((1, 1), 7, dtype=torch.int32, device=panel.device))
    with pytest.raises(FMError, match=r"\(-3\)"):
        E.forecast_portfolio_sort(panel, _dev(E, _random_coef(1, 1, 1, 3)), [([1, 2], 0)], ret=0, out=out)
    h = _host(out)
    assert (h["bp"] == 7.0).all() and (h["port"] == 77).all() and (h["rec"] == 7.0).all()
    assert (h["cnt"] == 7).all() and (h["status"] == 7).all()


# ---------------------------------------------------------------- 4. bad arguments, the empty call
def test_bad_arguments_raise(E, edge):
    from fmcore import _lib as L
    panel = _panel(E, edge, "both")
    coef = _dev(E, edge["coef"])

    def run(sel, coef=coef, **kw):
        return E.forecast_portfolio_sort(panel, coef[:len(sel)], sel, ret=0, **kw)

    run([([1, 2], 0)])   # the good call
    for sel in ([([], 0)], [(list(range(31)), 0)], [([1, 6], 0)], [([1, -1], 0)]):   # K = 0, K = 31, column >= C, < 0
        c = coef if len(sel[0][0]) < 31 else _dev(E, _random_coef(1, 1, 12, 32))
        with pytest.raises(L.FMError):
            run(sel, coef=c)
    with pytest.raises(L.FMError, match="coef_stride"):
        run([([1, 2, 3], 0)], coef=coef[:, :, :3].contiguous())
    with pytest.raises(L.FMError, match="nport"):
        run([([1], 0)], nport=1)
    # both layouts, neither: through the struct of the last good launch
    run([([1, 2], 0)])
    a = E.LAST_LAUNCH["fm_forecast_portfolio_sort"][1]
    f = a.src
    assert f.cols and not f.hi_plane
    f.hi_plane, f.lo_plane, f.plane_stride = panel.planes[0].data_ptr(), panel.planes[1].data_ptr(), panel.planes.stride(1)
    with pytest.raises(L.FMError, match="exactly one"):
        L.call("fm_forecast_portfolio_sort", L.C.byref(a), E._stream())
    f.cols = f.hi_plane = f.lo_plane = None
    with pytest.raises(L.FMError, match="exactly one"):
        L.call("fm_forecast_portfolio_sort", L.C.byref(a), E._stream())
    # empty calls: no sort, no month
    p = E.forecast_portfolio_sort(panel, coef[:0], [], ret=0, forecast_out=True)
    assert p.rec.shape == (0, 12, 11, 4) and p.port.shape == (0, panel.nrows) and p.forecast.shape == (0, panel.nrows)
    dev = panel.device
    seg0 = np.zeros(1, dtype=np.int64)
    empty = E.DevicePanel(cols=torch.empty((3, 0), dtype=torch.float64, device=dev), names=["a", "b", "c"],
                          seg_off=torch.from_numpy(seg0).to(dev), seg_off_h=seg0)
    p = E.forecast_portfolio_sort(empty, torch.empty((1, 0, 3), dtype=torch.float64, device=dev), [([1, 2], 0)], ret=0)
    torch.cuda.synchronize()
    assert p.rec.shape == (1, 0, 11, 4) and p.port.shape == (1, 0) and p.status.shape == (1, 0)


# ---------------------------------------------------------------- 5. lagged coefficients
def test_lagged_coefficients(E):
    rng = np.random.default_rng(9)
    T, P, pmax, lag = 40, 4, 6, 2
    st = (rng.random((T, P)) < 0.8).astype(np.int32)
    st[:, 2] = 0
    st[5, 2] = 1                      # count = 1 <= lag: all NaN
    st[:, 3] = 1                      # every month fitted
    status = _dev(E, st)
    ix = E.ts_compact(status, P, 1, T, P)
    roll_h = rng.normal(size=(P, T, pmax))
    roll_h[0, 3] = np.nan             # an incomplete rolling row travels as it is
    roll = _dev(E, roll_h)
    problems = [3, 0, 2, 1, 0]
    got = E.lagged_coefficients(roll, ix, problems, lag)
    torch.cuda.synchronize()
    idx, cnt = ix.idx.cpu().numpy(), ix.count.cpu().numpy()
    assert cnt[2] == 1 and (cnt[:2] < T).all() and cnt[3] == T
    exp = PPO.lagged_coef(roll.cpu().numpy(), idx, cnt, problems, lag)
    assert got.shape == (5, T, pmax)
    assert got.cpu().numpy().tobytes() == exp.tobytes()
    assert np.isnan(exp[2]).all() and np.isnan(exp[1][st[:, 0] == 0]).all() and np.isfinite(exp[0][lag:]).all()
    with pytest.raises(ValueError):
        E.lagged_coefficients(roll, ix, [4], lag)


# ---------------------------------------------------------------- 6. the pipeline
def _pipe_panel(E, layout):
    fx = PPO.pipeline_fixture()
    a = fx["arrays"]
    return E.panel_from_arrays(fx["cols"], fx["names"], a["month"], me=a["me"], nyse=a["nyse"], layout=layout)


def _pipe_cfg(LW, **kw):
    c = PPO.PIPE
    return LW.PipelineConfig(**dict(dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"],
                                         portfolios=c["nport"]), **kw))


@pytest.fixture(scope="module")
def pipe_runs(E):
    """The pipeline with portfolios on both layouts and, on f64, without: run once."""
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    runs = {lay: LW.run_pipeline(_pipe_panel(E, lay), _pipe_cfg(LW), model_cols=fx["model_cols"]) for lay in LAYOUTS}
    runs["off"] = LW.run_pipeline(_pipe_panel(E, "f64"), _pipe_cfg(LW, portfolios=None), model_cols=fx["model_cols"])
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pipeline_sorts_equal_restatement(E, pipe_runs, layout):
    """(i) every sort equals the host restatement fed with the run's own device outputs, (iii) the
    sorted months are the fitted rows i >= lag with a complete lagged coefficient row, (iv) the
    summary."""
    fx = PPO.pipeline_fixture()
    out = pipe_runs[layout]
    lag, nport = PPO.PIPE["lag"], PPO.PIPE["nport"]
    probs = out.portfolio_problems
    assert [(out.model_names[out.res.problems[k].model], out.res.problems[k].level) for k in probs] == \
        [(m, u) for m in fx["model_cols"] for u in (0, 1, 2)]
    roll, idx, cnt = out.rolling.cpu().numpy(), out.ix.idx.cpu().numpy(), out.ix.count.cpu().numpy()
    coef = PPO.lagged_coef(roll, idx, cnt, probs, lag)
    sel = [([fx["names"].index(c) for c in fx["model_cols"][out.model_names[out.res.problems[k].model]]],
            out.res.problems[k].level) for k in probs]
    a = fx["arrays"]
    exp = PPO.forecast_portfolio_sort(fx["cols"], fx["seg_off"], coef, sel, out.cuts.lo.cpu().numpy(),
                                      out.cuts.hi.cpu().numpy(), ret=fx["names"].index("retx"), W=a["me"],
                                      level=out.level.cpu().numpy(), nyse=a["nyse"].astype(np.uint8), nport=nport)
    got = _host(out.portfolios)
    _check_restatement(got, exp, layout)
    for j, k in enumerate(probs):
        K = out.res.problems[k].K
        want = np.zeros(len(fx["seg_off"]) - 1, dtype=np.int32)
        for i in range(lag, cnt[k]):
            want[idx[k, i]] = int(not np.isnan(roll[k, i - lag, :K + 1]).any())
        assert np.array_equal(got["status"][j], want), (layout, j)
        assert want.sum() >= 20
    s = out.portfolio_summary
    gm, gs, gt, gn = (x.cpu().numpy() for x in (s.mean, s.se, s.tstat, s.nobs))
    assert gm.shape == (len(probs), nport + 1, 4)
    for j in range(len(probs)):
        mean, se, t, nobs = PO.portfolio_summary(exp["rec"][j], exp["status"][j], 4)
        assert np.array_equal(gn[j], nobs)
        for k in range(nport + 1):
            for c in range(4):
                x = exp["rec"][j][exp["status"][j] == 1][:, k, c]
                assert np.isfinite(x).all()
                rms = float(np.sqrt(np.mean(x * x)))
                assert scalar_close(gm[j, k, c], mean[k, c], RTOL, rms), (j, k, c)
                assert scalar_close(gs[j, k, c], se[k, c], RTOL), (j, k, c)
                assert scalar_close(gt[j, k, c], t[k, c], RTOL, rms / se[k, c]), (j, k, c)


def test_pipeline_layouts_identical(pipe_runs):
    """(ii) the f64 and the planes-only panel give the same bytes."""
    _assert_same_bytes(_host(pipe_runs["planes"].portfolios), _host(pipe_runs["f64"].portfolios), "layouts")
    a, b = pipe_runs["planes"].portfolio_summary, pipe_runs["f64"].portfolio_summary
    for k in ("mean", "se", "tstat", "nobs"):
        assert getattr(a, k).cpu().numpy().tobytes() == getattr(b, k).cpu().numpy().tobytes(), k


def test_pipeline_off_is_unchanged(pipe_runs):
    """(v) portfolios=None: no portfolio fields, every other field byte-identical."""
    on, off = pipe_runs["f64"], pipe_runs["off"]
    assert off.portfolios is None and off.portfolio_summary is None and off.portfolio_problems is None
    assert on.model_names == off.model_names and on.model_cols == off.model_cols

    def same(x, y, what):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), what

    for k in ("rec", "status"):
        same(getattr(on.res, k), getattr(off.res, k), k)
    same(on.ix.count, off.ix.count, "count")
    cnt = on.ix.count.cpu().numpy()
    for k, p in enumerate(on.res.problems):
        # the written part: n, K+1 means, (K+1)^2 centered moments; the fitted months
        m = 1 + (p.K + 1) + (p.K + 1) ** 2
        same(on.res.moments[:, k, :m], off.res.moments[:, k, :m], f"moments[{k}]")
        same(on.ix.idx[k, :cnt[k]], off.ix.idx[k, :cnt[k]], f"idx[{k}]")
    for name in ("summary", "pred_summary"):
        for k in ("mean", "se", "tstat", "nobs"):
            same(getattr(getattr(on, name), k), getattr(getattr(off, name), k), f"{name}.{k}")
    for k in ("rolling", "pred", "pred_status", "level"):
        same(getattr(on, k), getattr(off, k), k)
    for k in ("lo", "hi", "nvalid", "center"):
        same(getattr(on.cuts, k), getattr(off.cuts, k), f"cuts.{k}")
    for x, y in zip(on.breakpoints, off.breakpoints):
        same(x, y, "breakpoints")


def test_pipeline_config_errors(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    panel = _pipe_panel(E, "f64")
    with pytest.raises(ValueError, match="standardize"):
        LW.run_pipeline(panel, _pipe_cfg(LW, standardize=True), model_cols=fx["model_cols"])
    with pytest.raises(ValueError, match="forecasts"):
        LW.run_pipeline(panel, _pipe_cfg(LW, forecasts=False), model_cols=fx["model_cols"])


# ---------------------------------------------------------------- 7. end to end against the oracle alone
def test_pipeline_vs_oracle_alone(pipe_runs):
    """Expected values from oracle.fm_oracle.pipeline_arrays' rolling coefficients, numpy
    forecasts on its winsorized columns and port_oracle; the fixture's margin between forecasts
    and breakpoints is asserted by tests/test_pipeline_portfolios_host.py.  No month excluded."""
    keys, exp = PPO.pipeline_expected()
    out = pipe_runs["f64"]
    assert [(out.model_names[out.res.problems[k].model], out.res.problems[k].level)
            for k in out.portfolio_problems] == keys
    got = _host(out.portfolios)
    assert np.array_equal(out.level.cpu().numpy(), exp["level"])
    for k in ("status", "port", "cnt"):
        assert np.array_equal(got[k], exp[k]), k
    nsel, T, n1, _ = exp["rec"].shape
    for j in range(nsel):
        for b in range(n1 - 2):
            assert_series_close(got["bp"][j, :, b], exp["bp"][j, :, b], f"bp[{j}, :, {b}]")
        for k in range(n1):
            for c in range(4):
                assert_series_close(got["rec"][j, :, k, c], exp["rec"][j, :, k, c], f"rec[{j}, :, {k}, {c}]")


# ---------------------------------------------------------------- 8. drop-in
def test_build_table_5(E, pipe_runs):
    from fmcore import lewellen as LW, synth
    from fmdrop import calc_Lewellen_2014 as CL
    c = PPO.PIPE
    nport = c["nport"]
    df = synth.synth_frame(c["T"], c["N"], c["seed"], nan_rate=c["nan_rate"], present_rate=c["present_rate"],
                           shuffle=True)
    frames = CL.build_table_5(df, nport=nport, window=c["window"], min_periods=c["min_periods"], lag=c["lag"])
    keys, _ = PPO.pipeline_expected()
    assert list(frames) == [(m, LW.SUBSET_NAMES[u]) for m, u in keys]
    got = _host(pipe_runs["f64"].portfolios)
    s = pipe_runs["f64"].portfolio_summary
    mean, tstat, nobs = s.mean.cpu().numpy(), s.tstat.cpu().numpy(), s.nobs.cpu().numpy()
    months = np.unique(df["mthcaldt"].values)
    labels = list(range(nport)) + ["H-L"]
    for j, key in enumerate(frames):
        monthly, summary = frames[key]
        srt = got["status"][j] == 1
        ns = int(srt.sum())
        assert list(monthly.columns) == ["ew_ret", "ew_pred", "vw_ret", "vw_pred", "n"]
        assert monthly.shape == (ns * (nport + 1), 5) and monthly.index.names == ["mthcaldt", "portfolio"]
        assert list(monthly.index.get_level_values(1)[:nport + 1]) == labels
        assert np.array_equal(monthly.index.get_level_values(0).unique().values, months[srt])
        vals = monthly[["ew_ret", "ew_pred", "vw_ret", "vw_pred"]].to_numpy().reshape(ns, nport + 1, 4)
        assert vals.tobytes() == got["rec"][j][srt].tobytes(), key
        n = monthly["n"].to_numpy().reshape(ns, nport + 1)
        cnt = got["cnt"][j][srt]
        assert np.array_equal(n[:, :nport], cnt) and np.array_equal(n[:, nport], cnt[:, 0] + cnt[:, -1])
        assert list(summary.index) == labels and summary.shape == (nport + 1, 12)
        for ci, name in enumerate(["ew_ret", "ew_pred", "vw_ret", "vw_pred"]):
            assert list(summary[name].columns) == ["mean", "tstat", "nobs"]
            assert summary[name]["mean"].to_numpy().tobytes() == mean[j, :, ci].tobytes()
            assert summary[name]["tstat"].to_numpy().tobytes() == tstat[j, :, ci].tobytes()
            assert np.array_equal(summary[name]["nobs"].to_numpy(), nobs[j, :, ci])
