"""GPU tests of the weighted cross-sections (A22): engine.fm_pass_wls (fm_wls) against the numpy
restatement (tests/wls_oracle.py) and the longdouble check, against fm_pass at unit weights, the
dropped-row, bit-identity, cancellation and degenerate-month rules of the header, and
PipelineConfig(wls_weights=...) with the drop-in's weight_col end to end."""
import numpy as np
import pytest
import torch

import pipe_port_oracle as PPO
import wls_oracle as WO
from fmtol import RTOL, assert_series_close, scalar_close

pytestmark = pytest.mark.gpu

NLEV = 3


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _dev(E, a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(E.require_device())


def _panel(E, cols, seg_off, w):
    """A DevicePanel straight from month-sorted arrays (empty months included), me = the weights."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    return E.DevicePanel(cols=_dev(E, np.stack(cols)), names=[f"c{i}" for i in range(len(cols))],
                         seg_off=_dev(E, seg_off), seg_off_h=seg_off, me=_dev(E, w))


def _models(E, models):
    return [E.Model(f"m{i}", y=y, xs=list(xs), levels=tuple(levels)) for i, (y, xs, levels) in enumerate(models)]


def _host(res):
    torch.cuda.synchronize()
    return res.rec.cpu().numpy(), res.status.cpu().numpy(), None if res.moments is None else res.moments.cpu().numpy()


def _run(E, d, models=WO.MODELS, w=None, cuts=None, nlevels=NLEV, moments=True):
    panel = _panel(E, d["cols"], d["seg_off"], d["w"] if w is None else w)
    level = _dev(E, d.get("level"))
    res = E.fm_pass_wls(panel, _models(E, models), weight="me", level=level, nlevels=nlevels if level is not None else 1,
                        cuts=cuts, moments=moments)
    return res, _host(res)


E_ST_SKIPPED, E_ST_INF = 0x2, 0x4 | 0x8   # FM_ST_SKIPPED, FM_ST_INF_IN_X | FM_ST_INF_IN_Y


def _written(res, rec, status, mom):
    """The bytes a call defines: rec, status and, per problem, the written part of the moment rows of the
    months that have one (N >= K + 1 and no inf)."""
    out = [rec.tobytes(), status.tobytes()]
    if mom is not None:
        for k, p in enumerate(res.problems):
            has = (status[:, k] & (E_ST_SKIPPED | E_ST_INF)) == 0
            out.append(mom[has, k, :1 + (p.K + 1) + (p.K + 1) ** 2].tobytes())
    return out


@pytest.fixture(scope="module")
def parity(E):
    d = WO.parity_panel()
    res, host = _run(E, d)
    return d, res, host


# ---------------------------------------------------------------- 1. against the restatement
def test_against_restatement(parity):
    d, res, (rec, status, mom) = parity
    ref = WO.fm_wls(d["cols"], d["seg_off"], WO.MODELS, d["w"], d["level"], moments=True)
    WO.assert_well_conditioned(ref)
    assert [(p.model, p.level, p.K) for p in res.problems] == ref["problems"] and res.pmax == ref["pmax"]
    WO.assert_result_close(rec, status, mom, ref, "parity")


def test_against_restatement_with_cuts(E):
    d = WO.parity_panel()
    lo, hi = PPO.winsor_cuts(d["cols"], d["seg_off"])
    assert np.isnan(lo[:, :2]).all() and np.isfinite(lo[:, 2:]).all()     # months of 0 and 3 rows have no cuts
    cuts = E.Cuts(_dev(E, lo), _dev(E, hi), None)
    res, (rec, status, mom) = _run(E, d, cuts=cuts)
    ref = WO.fm_wls(d["cols"], d["seg_off"], WO.MODELS, d["w"], d["level"], lo, hi, moments=True)
    WO.assert_well_conditioned(ref)
    WO.assert_result_close(rec, status, mom, ref, "parity, cuts")
    # a pivot changes no result beyond rounding: the cuts' midpoint as the first pass's shift
    shift = np.where(np.isfinite(lo), 0.5 * (lo + hi), 0.0)
    panel = _panel(E, d["cols"], d["seg_off"], d["w"])
    res2 = E.fm_pass_wls(panel, _models(E, WO.MODELS), level=_dev(E, d["level"]), nlevels=NLEV, cuts=cuts,
                         shift=_dev(E, shift), moments=True)
    WO.assert_result_close(*_host(res2), ref, "parity, cuts, shift")


# ---------------------------------------------------------------- 2. unit weights: the OLS kernels
def test_unit_weights_equal_fm_pass(E, parity):
    d = parity[0]
    ones = np.ones_like(d["w"])
    res, (rec, status, _) = _run(E, d, w=ones)
    panel = _panel(E, d["cols"], d["seg_off"], ones)
    ols = E.fm_pass(panel, _models(E, WO.MODELS), level=_dev(E, d["level"]), nlevels=NLEV)
    orec, ostatus, _ = _host(ols)
    pmax = res.pmax
    assert ols.pmax == pmax and np.array_equal(rec[:, :, pmax + 1], orec[:, :, pmax + 1])       # N
    for bit in (E.L.FM_ST_FITTED, E.L.FM_ST_SKIPPED):
        assert np.array_equal(status & bit, ostatus & bit), bit
    assert (status & E.L.FM_ST_FITTED).sum() > 200
    for k, p in enumerate(res.problems):
        for c in list(range(p.K + 1)) + [pmax]:
            assert_series_close(rec[:, k, c], orec[:, k, c], f"rec[:, {k}, {c}]", RTOL)


# ---------------------------------------------------------------- 3. bad weights
def test_bad_weights_equal_removed_rows(E, parity):
    d, _, _ = parity
    rng = np.random.default_rng(4)
    n = len(d["w"])
    w = d["w"].copy()
    bad = rng.random(n) < 0.1
    t_all = 10                                            # a month whose weights are all bad
    bad[int(d["seg_off"][t_all]):int(d["seg_off"][t_all + 1])] = True
    w[bad] = rng.choice([np.nan, np.inf, 0.0, -1.0, -np.inf], size=int(bad.sum()))
    for v in (np.nan, np.inf, 0.0, -1.0):
        assert (w[bad] == v).any() or (np.isnan(v) and np.isnan(w[bad]).any())
    res, (rec, status, mom) = _run(E, d, w=w)
    assert (status[t_all] == E.L.FM_ST_SKIPPED).all() and (rec[t_all, :, res.pmax + 1] == 0).all()
    month = np.repeat(np.arange(len(d["seg_off"]) - 1), np.diff(d["seg_off"]))
    keep = ~bad
    seg2 = np.concatenate([[0], np.cumsum(np.bincount(month[keep], minlength=len(d["seg_off"]) - 1))]).astype(np.int64)
    d2 = dict(cols=[c[keep] for c in d["cols"]], seg_off=seg2, w=d["w"][keep], level=d["level"][keep])
    res2, (rec2, status2, mom2) = _run(E, d2)
    assert _written(res, rec, status, mom) == _written(res2, rec2, status2, mom2)
    assert (status & E.L.FM_ST_FITTED).sum() > 150


# ---------------------------------------------------------------- 4. bits
def test_bits(E, parity):
    d, res, (rec, status, mom) = parity
    full = _written(res, rec, status, mom)
    # a repeat
    res_b, host_b = _run(E, d)
    assert _written(res_b, *host_b) == full
    # weights times 2^-7
    res_c, host_c = _run(E, d, w=d["w"] * 2.0 ** -7)
    assert _written(res_c, *host_c) == full
    # a sub-range of the months
    t0, t1 = 5, 17
    r0, r1 = int(d["seg_off"][t0]), int(d["seg_off"][t1])
    sub = dict(cols=[c[r0:r1] for c in d["cols"]], seg_off=d["seg_off"][t0:t1 + 1] - r0, w=d["w"][r0:r1],
               level=d["level"][r0:r1])
    res_d, (rec_d, status_d, mom_d) = _run(E, sub)
    assert _written(res_d, rec_d, status_d, mom_d) == _written(res, rec[t0:t1], status[t0:t1], mom[t0:t1])
    # a subset of the problems (the widest model stays, so the record layout does)
    pick = [(0, WO.XS14, (0, 2)), (0, [1, 2, 3], (1,))]
    res_e, (rec_e, status_e, mom_e) = _run(E, d, models=pick)
    at = {(tuple(WO.MODELS[p.model][1]), p.level): k for k, p in enumerate(res.problems)}
    ks = [at[tuple(pick[p.model][1]), p.level] for p in res_e.problems]
    assert ks == [at[tuple(WO.XS14), 0], at[tuple(WO.XS14), 2], at[(1, 2, 3), 1]] and res_e.pmax == res.pmax
    sel = type("R", (), {"problems": [res.problems[k] for k in ks]})
    assert _written(res_e, rec_e, status_e, mom_e) == _written(sel, rec[:, ks], status[:, ks], mom[:, ks])


# ---------------------------------------------------------------- 4b. months longer than the LDS ring
@pytest.fixture(scope="module")
def long_runs(E):
    d = WO.long_panel()
    res, host = _run(E, d, models=WO.LONG_MODELS)
    return d, res, host


def test_long_months_against_restatement(E, long_runs):
    """Months of up to 1,536 rows (up to 1,276 used: the ring wraps, a wave owns several tiles, the
    next block's loads fly under the MFMAs), with NaN, levels and bad weights, with and without cuts."""
    d, res, (rec, status, mom) = long_runs
    ref = WO.fm_wls(d["cols"], d["seg_off"], WO.LONG_MODELS, d["w"], d["level"], moments=True)
    WO.assert_well_conditioned(ref)
    assert ref["rec"][:, 0, ref["pmax"] + 1].max() > 3 * WO.RING_ROWS
    WO.assert_result_close(rec, status, mom, ref, "long")
    lo, hi = PPO.winsor_cuts(d["cols"], d["seg_off"])
    res2, host2 = _run(E, d, models=WO.LONG_MODELS, cuts=E.Cuts(_dev(E, lo), _dev(E, hi), None))
    ref2 = WO.fm_wls(d["cols"], d["seg_off"], WO.LONG_MODELS, d["w"], d["level"], lo, hi, moments=True)
    WO.assert_well_conditioned(ref2)
    WO.assert_result_close(*host2, ref2, "long, cuts")


def test_long_months_bits(E, long_runs):
    """Across the ring's wrap: the dropped rows (bad weights, and rows with a NaN in any column, which
    no model uses) taken out, a repeat, weights x 2^-7, a sub-range of the months and a subset of
    the problems, all byte for byte."""
    d, res, (rec, status, mom) = long_runs
    full = _written(res, rec, status, mom)
    res_b, host_b = _run(E, d, models=WO.LONG_MODELS)
    assert _written(res_b, *host_b) == full
    res_c, host_c = _run(E, d, models=WO.LONG_MODELS, w=d["w"] * 2.0 ** -7)
    assert _written(res_c, *host_c) == full
    # rows removed: every row with a bad weight, and every row whose 15 columns hold a NaN in the return
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(d["w"]) & (d["w"] > 0) & ~np.isnan(d["cols"][0])
    T = len(d["seg_off"]) - 1
    month = np.repeat(np.arange(T), np.diff(d["seg_off"]))
    seg2 = np.concatenate([[0], np.cumsum(np.bincount(month[keep], minlength=T))]).astype(np.int64)
    assert 0.8 < keep.mean() < 0.92 and (np.diff(seg2)[[1, 2, 3, 5]] > WO.RING_ROWS).all()
    d2 = dict(cols=[c[keep] for c in d["cols"]], seg_off=seg2, w=d["w"][keep], level=d["level"][keep])
    res_r, host_r = _run(E, d2, models=WO.LONG_MODELS)
    assert _written(res_r, *host_r) == full
    # months 1 .. 3 alone
    r0, r1 = int(d["seg_off"][1]), int(d["seg_off"][4])
    sub = dict(cols=[c[r0:r1] for c in d["cols"]], seg_off=d["seg_off"][1:5] - r0, w=d["w"][r0:r1],
               level=d["level"][r0:r1])
    res_d, host_d = _run(E, sub, models=WO.LONG_MODELS)
    assert _written(res_d, *host_d) == _written(res, rec[1:4], status[1:4], mom[1:4])
    # the widest model's two problems alone
    res_e, host_e = _run(E, d, models=[WO.LONG_MODELS[1]])
    ks = [k for k, p in enumerate(res.problems) if p.model == 1]
    sel = type("R", (), {"problems": [res.problems[k] for k in ks]})
    assert len(ks) == 2 and res_e.pmax == res.pmax
    assert _written(res_e, *host_e) == _written(sel, rec[:, ks], status[:, ks], mom[:, ks])


# ---------------------------------------------------------------- 5. cancellation
def test_cancellation(E):
    """Predictors with mean 1e4 x their standard deviation (wls_oracle.CANCEL_OFFSET; that a float64
    raw-moment fit misses RTOL there is asserted in tests/test_wls_host.py) against longdouble."""
    d = WO.cancel_panel()
    res, (rec, status, _) = _run(E, d, models=WO.CANCEL_MODELS, moments=False)
    assert (status == E.L.FM_ST_FITTED).all()
    T = len(d["seg_off"]) - 1
    for k, (y, xs, _) in enumerate(WO.CANCEL_MODELS):
        ld = np.zeros((T, len(xs) + 2))
        for t in range(T):
            X, yv, w = WO.month_design(d, xs, y, t)
            ld[t, :-1], ld[t, -1] = WO.wls_longdouble(X, yv, w)
        for c in range(len(xs) + 1):
            assert_series_close(rec[:, k, c], ld[:, c], f"coef[{k}, {c}]", RTOL)
        assert_series_close(rec[:, k, res.pmax], ld[:, -1], f"R2[{k}]", RTOL)


# ---------------------------------------------------------------- 6. degenerate months
def test_degenerate_months(E):
    rng = np.random.default_rng(8)
    lens = [100, 130, 70, 90, 80, 110]
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    X = rng.normal(size=(4, n))
    X[0] = 0.02 + 0.3 * X[1] - 0.1 * X[3] + 0.1 * rng.normal(size=n)
    s = [slice(int(seg_off[t]), int(seg_off[t + 1])) for t in range(6)]
    X[2, s[0]] = 2.0 * X[1, s[0]]          # collinear
    X[2, s[1]] = 0.0                       # all zero
    X[2, s[2]] = 3.7                       # a nonzero constant
    X[1, s[4].start + 5] = np.inf          # inf in x
    X[0, s[5].start + 9] = -np.inf         # inf in y
    d = dict(cols=[X[c] for c in range(4)], seg_off=seg_off, w=np.exp(rng.normal(size=n)))
    models = [(0, [1, 2, 3], (0,)), (0, [1, 3], (0,))]
    res, (rec, status, _) = _run(E, d, models=models, moments=False)
    st = E.L
    assert list(status[:, 0]) == [st.FM_ST_RANK_DEF] * 3 + [st.FM_ST_FITTED, st.FM_ST_INF_IN_X, st.FM_ST_INF_IN_Y]
    assert list(status[:, 1]) == [st.FM_ST_FITTED] * 4 + [st.FM_ST_INF_IN_X, st.FM_ST_INF_IN_Y]
    assert np.isnan(rec[[0, 1, 2, 4, 5], 0, :res.pmax + 1]).all() and list(rec[:, 0, res.pmax + 1]) == lens
    ref = WO.fm_wls(d["cols"], seg_off, models, d["w"])
    WO.assert_result_close(rec, status, None, ref, "degenerate")


# ---------------------------------------------------------------- 7. the pipeline and the drop-in
def _pipe_panel(E):
    fx = PPO.pipeline_fixture()
    a = fx["arrays"]
    return E.panel_from_arrays(fx["cols"], fx["names"], a["month"], me=a["me"], nyse=a["nyse"].astype(np.uint8))


def _pipe_cfg(LW, **kw):
    c = PPO.PIPE
    return LW.PipelineConfig(**dict(dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"]), **kw))


@pytest.fixture(scope="module")
def pipe(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    cfg = _pipe_cfg(LW, wls_weights="me", portfolios=PPO.PIPE["nport"], forecast_dist=True, forecast_compare=True)
    with E.KernelTimer() as kt:
        out = LW.run_pipeline(_pipe_panel(E), cfg, model_cols=fx["model_cols"])
    torch.cuda.synchronize()
    return out, kt.names()


def test_pipeline_matches_chained_restatement(E, pipe):
    from fmcore import lewellen as LW
    out, tags = pipe
    assert "fm_wls" in tags and "fm_gram" not in tags and "fm_solve" not in tags
    fx = PPO.pipeline_fixture()
    a, names, seg_off, cols = fx["arrays"], fx["names"], fx["seg_off"], fx["cols"]
    T, c = len(seg_off) - 1, PPO.PIPE
    models = [(names.index("retx"), [names.index(x) for x in xs], (0, 1, 2)) for xs in fx["model_cols"].values()]
    models.append((names.index("retx"), [names.index(x) for x in LW.FIG1_VARS], (0, 2)))
    lo, hi, level = out.cuts.lo.cpu().numpy(), out.cuts.hi.cpu().numpy(), out.level.cpu().numpy()
    assert np.array_equal(level, PPO.universe_levels(a["me"], a["nyse"], seg_off))
    ref = WO.fm_wls(cols, seg_off, models, a["me"], level, lo, hi, moments=True)
    WO.assert_well_conditioned(ref)
    rec, status, mom = _host(out.res)
    WO.assert_result_close(rec, status, mom, ref, "pipeline")
    assert (status & E.L.FM_ST_FITTED).all() and np.isnan(a["me"]).any()      # some rows drop for their weight
    chain = WO.ts_chain(ref, cols, seg_off, models, a["me"], level, lo, hi, c["window"], c["min_periods"], c["lag"])
    s = out.summary
    gm, gt, gn = s.mean.cpu().numpy(), s.tstat.cpu().numpy(), s.nobs.cpu().numpy()
    roll, pred, pst = out.rolling.cpu().numpy(), out.pred.cpu().numpy(), out.pred_status.cpu().numpy()
    cnt, idx = out.ix.count.cpu().numpy(), out.ix.idx.cpu().numpy()
    pmax = ref["pmax"]
    for k, (_, _, K) in enumerate(ref["problems"]):
        ch = chain[k]
        nf = len(ch["months"])
        assert cnt[k] == nf == T and np.array_equal(idx[k, :nf], ch["months"])
        for col, (mean, t, nobs, rms, se) in ch["summary"].items():
            assert gn[k, col] == nobs
            assert scalar_close(gm[k, col], mean, RTOL, rms), (k, col)
            assert scalar_close(gt[k, col], t, RTOL, rms / se), (k, col)
        for col in range(K + 1):
            assert_series_close(roll[k, :nf, col], ch["rolling"][:, col], f"rolling[{k}, :, {col}]", RTOL)
        fitted = ~np.isnan(ch["pred"][:, 0])
        assert fitted.sum() == T - c["min_periods"] - c["lag"] + 1
        assert np.array_equal((pst[k, :nf] & E.L.FM_ST_FITTED) != 0, fitted)
        for col in range(3):      # the weighted predictive slope, its R2 and N
            assert_series_close(pred[k, :nf, col], ch["pred"][:, col], f"pred[{k}, :, {col}]", RTOL)
    # the portfolios: the existing sort oracle fed with the weighted rolling coefficients
    probs = out.portfolio_problems
    coef = PPO.lagged_coef(roll, idx, cnt, probs, c["lag"])
    sel = [(models[ref["problems"][k][0]][1], ref["problems"][k][1]) for k in probs]
    exp = PPO.forecast_portfolio_sort(cols, seg_off, coef, sel, lo, hi, ret=names.index("retx"), W=a["me"],
                                      level=level, nyse=a["nyse"].astype(np.uint8), nport=c["nport"])
    p = out.portfolios
    for key in ("status", "port", "cnt"):
        assert np.array_equal(getattr(p, key).cpu().numpy(), exp[key]), key
    grec = p.rec.cpu().numpy()
    for j in range(len(probs)):
        for b in range(c["nport"] + 1):
            for col in range(4):
                assert_series_close(grec[j, :, b, col], exp["rec"][j, :, b, col], f"port rec[{j}, :, {b}, {col}]")
    assert exp["status"].sum() >= 20 * len(probs)
    # the two other forecast stages ran behind the weighted slopes, over the same months
    assert (out.forecast_dist.status.cpu().numpy().sum(axis=1) >= exp["status"].sum(axis=1)).all()
    assert out.forecast_compare.status.cpu().numpy().any()


def test_drop_in_weight_col(E):
    from fmcore import synth
    from fmdrop import calc_Lewellen_2014 as CL
    from fmdrop import regressions as RG
    c = PPO.PIPE
    fx = PPO.pipeline_fixture()
    a, names, seg_off = fx["arrays"], fx["names"], fx["seg_off"]
    df = synth.synth_frame(c["T"], c["N"], c["seed"], nan_rate=c["nan_rate"], present_rate=c["present_rate"], shuffle=True)
    xs = list(fx["model_cols"].values())[0]
    frame = RG.run_monthly_cs_regressions(df, "retx", xs, weight_col="me")
    ref = WO.fm_wls(fx["cols"], seg_off, [(names.index("retx"), [names.index(x) for x in xs], (0,))], a["me"])
    WO.assert_well_conditioned(ref)
    assert list(frame.columns) == ["mthcaldt", "N", "R2"] + [f"slope_{x}" for x in xs] and len(frame) == c["T"]
    assert np.array_equal(frame["mthcaldt"].values, np.unique(df["mthcaldt"].values))
    assert np.array_equal(frame["N"].to_numpy(), ref["rec"][:, 0, ref["pmax"] + 1].astype(np.int64))
    assert_series_close(frame["R2"].to_numpy(), ref["rec"][:, 0, ref["pmax"]], "R2", RTOL)
    for i, x in enumerate(xs):
        assert_series_close(frame[f"slope_{x}"].to_numpy(), ref["rec"][:, 0, 1 + i], f"slope_{x}", RTOL)
    # the unweighted call is what it was; an inf regressor raises as on the OLS path
    ols = RG.run_monthly_cs_regressions(df, "retx", xs)
    assert list(ols.columns) == list(frame.columns) and (ols["N"] >= frame["N"]).all() and (ols["N"] > frame["N"]).any()
    bad = df.copy()
    whole = bad[["retx", "me"] + xs].notna().all(axis=1) & (bad["me"] > 0)
    bad.loc[whole.index[whole][7], xs[0]] = np.inf        # a row that takes part
    with pytest.raises(RG.MissingDataError, match="exog contains inf or nans"):
        RG.run_monthly_cs_regressions(bad, "retx", xs, weight_col="me")
    # Table 2 from weighted cross-sections: the same layout as the unweighted table
    subsets = {"All stocks": df}
    t2w, t2 = CL.build_table_2(subsets, None, weight_col="me"), CL.build_table_2(subsets, None)
    assert t2w.shape == t2.shape and list(t2w.index) == list(t2.index) and list(t2w.columns) == list(t2.columns)
    assert (t2w.to_numpy() != t2.to_numpy()).any()


def test_cfg_passes_through_the_drop_in(E, pipe):
    """wls_weights= in lewellen_pipeline's and build_table_5's **cfg reaches the pipeline: the frame's
    run gives the bytes of the panel's run."""
    from fmcore import synth
    from fmdrop import calc_Lewellen_2014 as CL
    c = PPO.PIPE
    out = pipe[0]
    df = synth.synth_frame(c["T"], c["N"], c["seed"], nan_rate=c["nan_rate"], present_rate=c["present_rate"], shuffle=True)
    kw = dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"], wls_weights="me")
    lp = CL.lewellen_pipeline(df, portfolios=c["nport"], **kw)
    torch.cuda.synchronize()
    assert lp.res.rec.cpu().numpy().tobytes() == out.res.rec.cpu().numpy().tobytes()
    assert lp.res.status.cpu().numpy().tobytes() == out.res.status.cpu().numpy().tobytes()
    assert lp.portfolios.rec.cpu().numpy().tobytes() == out.portfolios.rec.cpu().numpy().tobytes()
    frames = CL.build_table_5(df, nport=c["nport"], **kw)
    got = out.portfolios.rec.cpu().numpy()
    st = out.portfolios.status.cpu().numpy()
    assert len(frames) == got.shape[0]
    for j, key in enumerate(frames):
        monthly, _ = frames[key]
        vals = monthly[["ew_ret", "ew_pred", "vw_ret", "vw_pred"]].to_numpy().reshape(-1, c["nport"] + 1, 4)
        assert vals.tobytes() == got[j][st[j] == 1].tobytes(), key
    ols = CL.build_table_5(df, nport=c["nport"], window=c["window"], min_periods=c["min_periods"], lag=c["lag"])
    k0 = next(iter(frames))
    assert not np.array_equal(ols[k0][0]["ew_pred"].to_numpy(), frames[k0][0]["ew_pred"].to_numpy())


# ---------------------------------------------------------------- 8. off is what it was
def test_off_issues_the_same_launches_and_bytes(E, pipe):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    runs = []
    for kw in ({}, {"wls_weights": None}):
        with E.KernelTimer() as kt:
            out = LW.run_pipeline(_pipe_panel(E), _pipe_cfg(LW, **kw), model_cols=fx["model_cols"])
        torch.cuda.synchronize()
        runs.append((out, kt.events))
    (a, ea), (b, eb) = runs
    assert list(ea) == list(eb) and [len(v) for v in ea.values()] == [len(v) for v in eb.values()]
    assert "fm_wls" not in ea and "fm_gram" in ea and "fm_solve" in ea
    # the weighted run differs from it by that one launch in place of the two
    swap = {"fm_gram": "fm_wls", "fm_solve": None, "fm_pilot_shift": None}
    assert [swap.get(t, t) for t in ea if swap.get(t, t) is not None] == [t for t in pipe[1] if t in ea or t == "fm_wls"]
    fitted = (a.res.status.cpu().numpy() & 1) != 0
    for name in ("rec", "status"):
        assert getattr(a.res, name).cpu().numpy().tobytes() == getattr(b.res, name).cpu().numpy().tobytes(), name
    for k, p in enumerate(a.res.problems):
        m = 1 + (p.K + 1) + (p.K + 1) ** 2
        x, y = (r.res.moments[:, k, :m].cpu().numpy()[fitted[:, k]] for r in (a, b))
        assert x.tobytes() == y.tobytes(), f"moments[{k}]"
    for name in ("mean", "se", "tstat", "nobs"):
        assert getattr(a.summary, name).cpu().numpy().tobytes() == getattr(b.summary, name).cpu().numpy().tobytes()
    # and the OLS pass is the parent's: fm_pass on the same panel, cuts and levels gives the run's records
    ols = E.fm_pass(_pipe_panel(E), LW.build_models(_pipe_panel(E), fx["model_cols"])[0], level=a.level, nlevels=3,
                    cuts=a.cuts, shift=a.cuts.center, moments=True)
    assert ols.rec.cpu().numpy().tobytes() == a.res.rec.cpu().numpy().tobytes()
