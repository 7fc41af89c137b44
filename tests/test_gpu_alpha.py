"""GPU tests of the portfolio alphas (fm_portfolio_alpha, engine.portfolio_alphas,
PipelineConfig(alpha_factors=...), build_table_alphas; build-defined A18) against the numpy
restatement tests/alpha_oracle.py, on hand-made ``Portfolios`` tensors and on the small pipeline
panel of tests/test_gpu_pipeline_portfolios.py."""
import gc

import numpy as np
import pytest
import torch

import alpha_oracle as AO
import pipe_port_oracle as PPO
from fmtol import RTOL, assert_series_close
from test_gpu_fcmp import _other_fields
from test_gpu_pipeline_portfolios import LAYOUTS, _assert_same_bytes, _dev, _pipe_cfg, _pipe_panel
from test_gpu_pipeline_portfolios import _host as port_host

pytestmark = pytest.mark.gpu

NROW = 4   # three portfolios and the spread


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks(E):
    """After this module's fixtures are gone, hand its device memory back: a later module's
    torch.empty tensors then do not start from this module's bytes (res.moments has rows whose tails
    no kernel writes, and some pipeline tests compare them whole)."""
    yield
    E.LAST_LAUNCH.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ports(E, rec, status):
    return E.Portfolios(bp=None, port=None, rec=_dev(E, rec), cnt=None, status=_dev(E, status.astype(np.int32)))


def _host(a):
    torch.cuda.synchronize()
    return {k: getattr(a, k).cpu().numpy() for k in AO.OUTS}


def _run(E, rec, status, F, models, rf=None, nw_lags=0):
    return _host(E.portfolio_alphas(_ports(E, rec, status), _dev(E, F), models=models, rf=_dev(E, rf), nw_lags=nw_lags))


def _series(rng, F, S, nrow=NROW):
    """rec [S, T, nrow, 4]: returns with factor loadings and t4 noise in columns 0 and 2, NaN in the
    forecast columns 1 and 3 (which nothing here may read); the last row is row nrow-2 minus row 0."""
    T, K = F.shape
    rec = np.full((S, T, nrow, 4), np.nan)
    for c in (0, 2):
        b = rng.normal(0.6, 0.4, (S, nrow, K))
        rec[..., c] = 0.004 + np.einsum("tk,spk->stp", F, b) + 0.02 * rng.standard_t(4, (S, T, nrow))
        rec[:, :, nrow - 1, c] = rec[:, :, nrow - 2, c] - rec[:, :, 0, c]
    return rec


MODELS = {1: [[0]], 3: [[0], [0, 1, 2], [0, 2]], 6: [[0], [0, 1, 2], [0, 1, 2, 3, 4, 5], [3, 5]]}


def _edge_case(T, K):
    """Three sorts of one factor table with every edge of the definition planted (T >= 63)."""
    rng = np.random.default_rng(1000 * K + T)
    F = rng.normal(0.005, 0.04, (T, K))
    rec = _series(rng, F, 3)
    status = np.ones((3, T), dtype=np.int32)
    rf = 0.003 + rng.normal(0, 0.0005, T)
    if T >= 63:
        status[0, [5, 6, 40]] = 0                       # unsorted months
        rec[0, 10, 1, 0], rec[0, 11, 1, 0], rec[0, 12, 1, 2] = np.nan, np.inf, -np.inf
        if K >= 3:
            F[20:23, 1] = np.nan                        # one factor only: the models' months differ
            F[30, K - 1] = np.inf
            F[31, 2] = -np.inf
        rf[15], rf[16], rf[17] = np.nan, np.inf, -np.inf   # drops the portfolios' months, not the spread's
        rec[1, :, 1, 2] = np.nan                        # an all-NaN vw column
        rec[0, :, NROW - 1, 0] = 0.25                   # a constant dependent series (no rf on the spread): exact mean
        status[2] = 0
        status[2, 41:41 + K + 2] = 1                    # n = K + 2 for the model of all K factors
        rec[2, 42, 0, 0] = np.nan                       # ... and K + 1 for sort 2's first ew series
    return rec, status, F, rf


@pytest.mark.parametrize("K", [1, 3, 6])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 257, 600])
def test_edge_series_against_the_oracle(E, T, K):
    rec, status, F, rf = _edge_case(T, K)
    models = MODELS[K]
    full = models.index(list(range(K)))
    for lags, with_rf in ((0, True), (4, False), (16, True), (64, False), (4, True)):
        r = rf if with_rf else None
        exp = AO.portfolio_alphas(rec, status, F, models, r, lags)
        got = _run(E, rec, status, F, models, r, lags)
        if T < 3:
            assert np.array_equal(exp["nobs"], np.full_like(exp["nobs"], T)) and np.isnan(exp["coef"]).all() \
                and np.isnan(exp["stat"]).all()
        else:
            # the input conditions: every case is there, and no design sits near the pivot threshold
            piv = exp["pivot"][np.isfinite(exp["pivot"])]
            assert piv.size and piv.min() > 1e-6, piv.min()
            assert (exp["nobs"][1, 1, 1] == 0).all() and np.isnan(exp["stat"][1, 1, 1]).all()
            assert exp["nobs"][2, 1, 0, full] == K + 2 and np.isfinite(exp["coef"][2, 1, 0, full]).all()
            assert exp["nobs"][2, 0, 0, full] == K + 1 and np.isnan(exp["coef"][2, 0, 0, full]).all()
            assert np.isnan(exp["stat"][2, 0, 0, full]).all()
            assert np.isnan(exp["stat"][0, NROW - 1, 0, :, 0]).all() and (exp["stat"][0, NROW - 1, 0, :, 2] == 0.25).all()
            assert (exp["stat"][0, NROW - 1, 0, :, 3] == 0.0).all() and np.isfinite(exp["coef"][0, NROW - 1, 0, 0, :2]).all()
            assert exp["nobs"][0, 0, 0, 0] == T - 3 - (3 if with_rf else 0)
            assert exp["nobs"][0, NROW - 1, 1, 0] == T - 3 and exp["nobs"][0, 1, 0, 0] == T - 5 - (3 if with_rf else 0)
            if K >= 3:
                assert exp["nobs"][1, 0, 0, full] == exp["nobs"][1, 0, 0, 0] - 5
            assert exp["nobs"][exp["nobs"] >= 3].min() <= 8 < 16       # so L = 16 and L = 64 exceed some n
        AO.assert_alphas_close(got, exp, models, f"T={T} K={K} L={lags} rf={with_rf}")


def test_rank_rule(E):
    """A duplicated and a constant factor column: the models that hold them are refused (coefficients,
    both standard errors, R2 and s NaN; mean, sd and nobs written), the others are not."""
    rng = np.random.default_rng(7)
    for K, models, refused in ((3, [[0], [0, 1], [0, 2], [0, 1, 2]], [2, 3]),
                               (6, [[0, 1, 2, 3], [4], [1, 5], [0, 1, 2, 3, 4, 5]], [1, 2, 3])):
        F = rng.normal(0.005, 0.04, (65, K))
        if K == 3:
            F[:, 2] = F[:, 0]
        else:
            F[:, 4] = 0.25           # 65 * 0.25 is exact: the centred column is exactly zero
            F[:, 5] = F[:, 1]
        rec = _series(rng, F, 2)
        status = np.ones((2, 65), dtype=np.int32)
        exp = AO.portfolio_alphas(rec, status, F, models, None, 4)
        got = _run(E, rec, status, F, models, None, 4)
        for m in range(len(models)):
            if m in refused:
                assert exp["pivot"][..., m].max() < 1e-12
                assert np.isnan(exp["coef"][..., m, :]).all() and np.isnan(exp["stat"][..., m, :2]).all()
                assert np.isfinite(exp["stat"][..., m, 2:]).all() and (exp["nobs"][..., m] == 65).all()
            else:
                assert exp["pivot"][..., m].min() > 1e-3 and np.isfinite(exp["coef"][..., m, 0]).all()
        AO.assert_alphas_close(got, exp, models, f"rank K={K}")


# ---------------------------------------------------------------- 2. determinism and the boundary
def test_same_bytes_twice_and_on_a_subset(E):
    rec, status, F, rf = _edge_case(257, 6)
    models = MODELS[6]
    a = _run(E, rec, status, F, models, rf, 12)
    b = _run(E, rec, status, F, models, rf, 12)
    _assert_same_bytes(a, b, "two calls")
    sub = _run(E, rec[[0, 2]], status[[0, 2]], F, [models[0], models[2]], rf, 12)
    for k in AO.OUTS:
        want = np.ascontiguousarray(a[k][[0, 2]][:, :, :, [0, 2]])
        assert sub[k].shape == want.shape and sub[k].tobytes() == want.tobytes(), k


def test_longest_series_and_beyond(E):
    from fmcore._lib import FMError
    rng = np.random.default_rng(4096)
    F = rng.normal(0.005, 0.04, (4097, 6))
    rec = _series(rng, F, 1, nrow=2)
    status = np.ones((1, 4097), dtype=np.int32)
    status[0, [0, 77, 4095]] = 0
    models = [[0], [0, 1, 2, 3, 4, 5]]
    exp = AO.portfolio_alphas(rec[:, :4096], status[:, :4096], F[:4096], models, None, 12)
    assert (exp["nobs"] == 4093).all()
    got = _run(E, rec[:, :4096], status[:, :4096], F[:4096], models, None, 12)
    AO.assert_alphas_close(got, exp, models, "T=4096")
    with pytest.raises(FMError, match=r"fm_portfolio_alpha failed \(-3\)"):
        _run(E, rec, status, F, models, None, 12)


# ---------------------------------------------------------------- 3. single, batched, strided
def test_single_batched_and_strided_agree(E):
    rec, status, F, rf = _edge_case(65, 3)
    models = MODELS[3]
    full = _run(E, rec, status, F, models, rf, 4)
    for j in range(3):
        one = _run(E, rec[j], status[j], F, models, rf, 4)
        for k in AO.OUTS:
            assert one[k].shape == full[k].shape[1:] and one[k].tobytes() == full[k][j].tobytes(), (j, k)
    # the same records inside wider tensors: read in place through their strides
    big = torch.full((3, 65, NROW + 2, 6), float("nan"), dtype=torch.float64, device=E.require_device())
    big[:, :, 1:NROW + 1, 1:5] = _dev(E, rec)
    sbig = torch.zeros((3, 130), dtype=torch.int32, device=big.device)
    sbig[:, ::2] = _dev(E, status)
    view = E.Portfolios(bp=None, port=None, rec=big[:, :, 1:NROW + 1, 1:5], cnt=None, status=sbig[:, ::2])
    assert not view.rec.is_contiguous() and not view.status.is_contiguous()
    got = _host(E.portfolio_alphas(view, _dev(E, F), models=models, rf=_dev(E, rf), nw_lags=4))
    _assert_same_bytes(got, full, "strided")


def test_engine_refuses_wrong_tensors(E):
    rec, status, F, rf = _edge_case(63, 3)
    p = _ports(E, rec, status)
    Fd, rfd = _dev(E, F), _dev(E, rf)
    for kw, text in ((dict(factors=Fd.float()), "factors must be a float64"), (dict(factors=Fd[:62]), "factors must be"),
                     (dict(factors=Fd.cpu()), "factors must be"), (dict(factors=Fd[:, 0]), "factors must be"),
                     (dict(rf=rfd[:10]), "rf must be"), (dict(rf=rfd.float()), "rf must be"),
                     (dict(models=[[3]]), "distinct factor columns"), (dict(models=[[0]] * 5), "models per call")):
        args = dict(dict(factors=Fd, rf=rfd, models=None), **kw)
        with pytest.raises(ValueError, match=text):
            E.portfolio_alphas(p, args["factors"], models=args["models"], rf=args["rf"])
    with pytest.raises(ValueError, match="ports.status must be an int32"):
        E.portfolio_alphas(E.Portfolios(bp=None, port=None, rec=p.rec, cnt=None, status=p.status[:2]), Fd)
    with pytest.raises(ValueError, match="ports.rec must be a float64"):
        E.portfolio_alphas(E.Portfolios(bp=None, port=None, rec=p.rec.float(), cnt=None, status=p.status), Fd)
    a = E.portfolio_alphas(p, Fd, rf=rfd, nw_lags=4)
    assert a.tstat.shape == a.coef.shape == (3, NROW, 2, 2, 4) and a.nobs.dtype == torch.int32
    t, th = a.tstat.cpu().numpy(), a.tstat_hac.cpu().numpy()
    h = _host(a)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(t, h["coef"] / h["se"], equal_nan=True)
        assert np.array_equal(th, h["coef"] / h["se_hac"], equal_nan=True)


# ---------------------------------------------------------------- 4. pipeline
def _pipe_factors():
    rng = np.random.default_rng(2014)
    T = PPO.PIPE["T"]
    F = rng.normal(0.005, 0.04, (T, 3))
    F[11, 2] = np.nan
    return F, 0.003 + rng.normal(0, 0.0005, T)


PIPE_MODELS = [[0], [0, 1, 2]]


@pytest.fixture(scope="module")
def pipe_runs(E):
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    F, rf = _pipe_factors()
    runs = {lay: LW.run_pipeline(_pipe_panel(E, lay), _pipe_cfg(LW, alpha_factors=F, alpha_rf=rf, alpha_nw_lags=3),
                                 model_cols=fx["model_cols"]) for lay in LAYOUTS}
    runs["off"] = LW.run_pipeline(_pipe_panel(E, "f64"), _pipe_cfg(LW), model_cols=fx["model_cols"])
    torch.cuda.synchronize()
    return runs


@pytest.mark.parametrize("layout", LAYOUTS)
def test_pipeline_alphas(E, pipe_runs, layout):
    out = pipe_runs[layout]
    F, rf = _pipe_factors()
    got = _host(out.portfolio_alphas)
    nport = PPO.PIPE["nport"]
    assert got["coef"].shape == (9, nport + 1, 2, 2, 4) and got["nobs"].shape == (9, nport + 1, 2, 2)
    again = _host(E.portfolio_alphas(out.portfolios, _dev(E, F), models=None, rf=_dev(E, rf), nw_lags=3))
    _assert_same_bytes(got, again, "pipeline vs engine call")
    hp = port_host(out.portfolios)
    exp = AO.portfolio_alphas(hp["rec"], hp["status"], F, PIPE_MODELS, rf, 3)
    assert exp["nobs"].min() >= 15 and (exp["nobs"][..., 1] == exp["nobs"][..., 0] - 1).all()
    assert np.nanmin(exp["pivot"]) > 1e-6
    AO.assert_alphas_close(got, exp, PIPE_MODELS, f"pipeline {layout}")


def test_pipeline_nothing_else_moves(pipe_runs):
    on, off = pipe_runs["f64"], pipe_runs["off"]
    assert off.portfolio_alphas is None and on.portfolio_alphas is not None
    _assert_same_bytes(_host(pipe_runs["planes"].portfolio_alphas), _host(on.portfolio_alphas), "layouts")
    assert on.model_names == off.model_names and on.model_cols == off.model_cols
    assert on.portfolio_problems == off.portfolio_problems
    a, b = _other_fields(on), _other_fields(off)
    del a["res.moments"], b["res.moments"]
    _assert_same_bytes(a, b, "alpha_factors on / off")
    # the moments' written part (n, K + 1 means, (K + 1)^2 centred moments; the rest of a row is never written)
    fitted = (on.res.status.cpu().numpy() & 1) != 0
    for k, p in enumerate(on.res.problems):
        m = 1 + (p.K + 1) + (p.K + 1) ** 2
        x, y = (r.res.moments[:, k, :m].cpu().numpy()[fitted[:, k]] for r in (on, off))
        assert x.tobytes() == y.tobytes(), f"moments[{k}]"
    _assert_same_bytes(port_host(on.portfolios), port_host(off.portfolios), "portfolios on / off")
    for k in ("mean", "se", "tstat", "nobs"):
        a, b = (getattr(r.portfolio_summary, k).cpu().numpy() for r in (on, off))
        assert a.tobytes() == b.tobytes(), k


# ---------------------------------------------------------------- 5. drop-in
def test_build_table_alphas(E, pipe_runs):
    import pandas as pd
    from fmcore import lewellen as LW, synth
    from fmdrop import calc_Lewellen_2014 as CL
    c = PPO.PIPE
    nport = c["nport"]
    df = synth.synth_frame(c["T"], c["N"], c["seed"], nan_rate=c["nan_rate"], present_rate=c["present_rate"], shuffle=True)
    months = np.unique(df["mthcaldt"].values)
    F, rf = _pipe_factors()
    # dated on the first day of each month and in another row order: matched by calendar year and month
    first = pd.DatetimeIndex(months).to_period("M").to_timestamp()
    fac = pd.DataFrame(F, index=first, columns=["MKT", "SMB", "HML"])
    fac["RF"] = rf
    perm = np.random.default_rng(3).permutation(len(fac))
    kw = dict(nport=nport, window=c["window"], min_periods=c["min_periods"], lag=c["lag"], alpha_nw_lags=3)
    frames = CL.build_table_alphas(df, fac.iloc[perm], rf="RF", **kw)
    keys, _ = PPO.pipeline_expected()
    assert list(frames) == [(m, LW.SUBSET_NAMES[u]) for m, u in keys]
    got = _host(pipe_runs["f64"].portfolio_alphas)
    hp = port_host(pipe_runs["f64"].portfolios)
    exp = AO.portfolio_alphas(hp["rec"], hp["status"], F, PIPE_MODELS, rf, 3)
    cols = [x for w in ("ew", "vw") for x in [(w, "", s) for s in ("Avg", "Std", "Shp")] +
            [(w, fm, s) for fm in ("CAPM", "FF") for s in CL.ALPHA_COLUMNS]]
    for j, key in enumerate(frames):
        tab = frames[key]
        assert tab.shape == (nport + 1, len(cols)) and list(tab.columns) == cols
        assert list(tab.index) == list(range(nport)) + ["H-L"] and tab.index.name == "portfolio"
        for w, wn in enumerate(("ew", "vw")):
            assert tab[(wn, "", "Avg")].to_numpy().tobytes() == got["stat"][j, :, w, 0, 2].tobytes()
            assert tab[(wn, "", "Std")].to_numpy().tobytes() == got["stat"][j, :, w, 0, 3].tobytes()
            assert_series_close(tab[(wn, "", "Shp")].to_numpy(),
                                exp["stat"][j, :, w, 0, 2] / exp["stat"][j, :, w, 0, 3] * np.sqrt(12.0), f"Shp {key} {wn}")
            for m, fm in enumerate(("CAPM", "FF")):
                assert tab[(wn, fm, "alpha")].to_numpy().tobytes() == got["coef"][j, :, w, m, 0].tobytes()
                assert tab[(wn, fm, "R2")].to_numpy().tobytes() == got["stat"][j, :, w, m, 0].tobytes()
                assert np.array_equal(tab[(wn, fm, "nobs")].to_numpy(), exp["nobs"][j, :, w, m])
                with np.errstate(invalid="ignore", divide="ignore"):
                    assert np.array_equal(tab[(wn, fm, "t")].to_numpy(), got["coef"][j, :, w, m, 0] / got["se"][j, :, w, m, 0])
                    assert np.array_equal(tab[(wn, fm, "t_hac")].to_numpy(),
                                          got["coef"][j, :, w, m, 0] / got["se_hac"][j, :, w, m, 0])
    # a factor frame that lacks four months (two of them sorted ones at the end): nobs falls by the sorted ones
    gone = [0, 1, c["T"] - 2, c["T"] - 1]
    less = CL.build_table_alphas(df, fac.drop(fac.index[gone]), rf=fac["RF"], models={"M": ["MKT"]}, **kw)
    Fm = F.copy()
    Fm[gone] = np.nan
    exp2 = AO.portfolio_alphas(hp["rec"], hp["status"], Fm, [[0]], rf, 3)
    for j, key in enumerate(less):
        srt = hp["status"][j] == 1
        assert srt[gone[2:]].all()
        assert list(less[key].columns)[3:8] == [("ew", "M", s) for s in CL.ALPHA_COLUMNS]
        for w, wn in enumerate(("ew", "vw")):
            n2 = less[key][(wn, "M", "nobs")].to_numpy()
            assert np.array_equal(n2, exp2["nobs"][j, :, w, 0])
            assert np.array_equal(n2, frames[key][(wn, "CAPM", "nobs")].to_numpy() - int(srt[gone].sum()))
            assert_series_close(less[key][(wn, "M", "alpha")].to_numpy(), exp2["coef"][j, :, w, 0, 0], f"alpha {key} {wn}")
