"""GPU tests of the forecast-sorted portfolios (A12; fm_portfolio_sort) against the numpy
restatement of its definition (tests/port_oracle.py): breakpoints equal by value, portfolio
bytes / counts / status bit-exact, the monthly records per (portfolio, column) series within
RTOL = 1e-9 of max(|b|, RMS of the series) (a sum of <= 16,384 FP64 terms sits orders of
magnitude below that)."""
import numpy as np
import pytest
import torch

import port_oracle as PO
from fmtol import RTOL, assert_series_close, scalar_close

pytestmark = pytest.mark.gpu

COMBOS = [(0, False), (1, False), (0, True), (2, True)]   # (min_level, nyse_breakpoints)


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module")
def CL():
    from fmdrop import calc_Lewellen_2014
    return calc_Lewellen_2014


@pytest.fixture(scope="module")
def panel():
    return PO.random_panel()


@pytest.fixture(scope="module")
def panel_ref(panel):
    """The restatement on the random panel for the four combinations, computed once."""
    return {c: PO.portfolio_sort(panel["seg_off"], panel["F"], panel["R"], panel["W"], panel["level"], panel["nyse"],
                                 nport=10, min_level=c[0], nyse_breakpoints=c[1]) for c in COMBOS}


def _dev(E, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(E.require_device())


def _sort(E, pan, **kw):
    """engine.portfolio_sort on host arrays -> (Portfolios, dict of host arrays)."""
    p = E.portfolio_sort(_dev(E, pan["seg_off"]), _dev(E, pan["F"]), _dev(E, pan["R"]), weight=_dev(E, pan.get("W")),
                         level=_dev(E, pan.get("level")), nyse=_dev(E, pan.get("nyse")), **kw)
    torch.cuda.synchronize()
    return p, {k: getattr(p, k).cpu().numpy() for k in ("bp", "port", "rec", "cnt", "status")}


def _check(got, exp, what=""):
    assert np.array_equal(got["status"], exp["status"]), what
    assert np.array_equal(got["bp"], exp["bp"], equal_nan=True), what
    assert np.array_equal(got["port"], exp["port"]), what
    assert np.array_equal(got["cnt"], exp["cnt"]), what
    n1 = exp["rec"].shape[1]
    for k in range(n1):
        for c in range(4):
            assert_series_close(got["rec"][:, k, c], exp["rec"][:, k, c], f"{what} rec[:, {k}, {c}]")


def _bits(h):
    return {k: v.tobytes() for k, v in h.items()}


# ---------------------------------------------------------------- 1. random ragged panel
@pytest.mark.parametrize("combo", COMBOS)
def test_random_panel(E, panel, panel_ref, combo):
    exp = panel_ref[combo]
    assert exp["status"].all() and (exp["cnt"] > 0).all()   # every month sorted, no empty portfolio
    _, got = _sort(E, panel, nport=10, min_level=combo[0], nyse_breakpoints=combo[1])
    _check(got, exp, str(combo))


# ---------------------------------------------------------------- 2. edge months
def _edge_panel():
    rng = np.random.default_rng(11)
    F, R, W, NY = [], [], [], []

    def month(f, nyse=None, w=None):
        n = len(f)
        F.append(np.asarray(f, dtype=np.float64))
        r = rng.normal(0.01, 0.1, n)
        r[rng.random(n) < 0.05] = np.nan
        R.append(r)
        W.append(np.exp(rng.normal(4.0, 1.5, n)) if w is None else np.asarray(w, dtype=np.float64))
        NY.append((rng.random(n) < 0.5).astype(np.uint8) if nyse is None else np.asarray(nyse, dtype=np.uint8))

    for n in (0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        month(rng.normal(0.01, 0.02, n))
    month(np.full(100, np.nan))                                   # no finite forecast
    month(np.full(100, 0.0125))                                   # all equal: everything in portfolio 0
    z = np.concatenate([-rng.random(30), np.full(20, -0.0), np.full(20, 0.0), rng.random(30)])
    month(rng.permutation(z))                                     # breakpoints at +-0.0 between signed zeros
    month(1.0 + rng.integers(0, 1 << 20, 300) * 2.0 ** -52)       # differ only in the low 32 bits
    w = np.exp(rng.normal(4.0, 1.5, 120))
    w[::5], w[1::5], w[2::5] = 0.0, -w[1::5], np.nan
    month(rng.normal(0.01, 0.02, 120), w=w)                       # zero, negative and NaN weights
    month(rng.normal(0.01, 0.02, 80), nyse=np.zeros(80))          # no NYSE row
    ny = np.zeros(50)
    ny[rng.permutation(50)[:10]] = 1
    month(rng.normal(0.01, 0.02, 50), nyse=ny)                    # exactly min_count NYSE rows
    seg_off = np.concatenate([[0], np.cumsum([len(f) for f in F])]).astype(np.int64)
    return dict(seg_off=seg_off, F=np.concatenate(F), R=np.concatenate(R), W=np.concatenate(W),
                nyse=np.concatenate(NY))


@pytest.mark.parametrize("nyse_bp", [False, True])
def test_edge_months(E, nyse_bp):
    pan = _edge_panel()
    exp = PO.portfolio_sort(pan["seg_off"], pan["F"], pan["R"], pan["W"], None, pan["nyse"], nport=10,
                            nyse_breakpoints=nyse_bp)
    lens = np.diff(pan["seg_off"])
    t9, t10, tnan, teq, tzero, tnony, tmin = (list(lens).index(9), list(lens).index(10), 14, 15, 16, 19, 20)
    if not nyse_bp:
        assert exp["status"][[0, 1, t9, tnan]].tolist() == [0, 0, 0, 0] and exp["status"][t10] == 1
        assert (exp["bp"][tzero] == 0.0).any()
        a, b = pan["seg_off"][teq], pan["seg_off"][teq + 1]
        assert (exp["port"][a:b] == 0).all() and (exp["cnt"][teq, 1:] == 0).all()
        assert np.isnan(exp["rec"][teq, 10]).all()
    else:
        assert exp["status"][tnony] == 0 and exp["status"][tmin] == 1
    _, got = _sort(E, pan, nport=10, nyse_breakpoints=nyse_bp)
    _check(got, exp, f"nyse_bp={nyse_bp}")


# ---------------------------------------------------------------- 3. ties
def test_ties_and_summary_nobs(E, panel):
    grid = np.linspace(-0.02, 0.04, 7)
    f = panel["F"]
    F = np.where(np.isfinite(f), grid[np.abs(np.nan_to_num(f, nan=0.0, posinf=0.0)[:, None] - grid).argmin(axis=1)], f)
    pan = dict(panel, F=F)
    exp = PO.portfolio_sort(pan["seg_off"], F, pan["R"], pan["W"], nport=10)
    empty = exp["cnt"] == 0
    assert empty.any() and np.isnan(exp["rec"][:, :10, 0][empty]).all()
    assert np.isnan(exp["rec"][:, 10, 0]).any()
    p, got = _sort(E, dict(seg_off=pan["seg_off"], F=F, R=pan["R"], W=pan["W"]), nport=10)
    _check(got, exp, "ties")
    s = E.portfolio_summary(p, 4)
    mean, se, t, nobs = PO.portfolio_summary(exp["rec"], exp["status"], 4)
    assert np.array_equal(s.nobs.cpu().numpy(), nobs)
    assert (nobs < exp["status"].sum()).any()
    assert np.array_equal(np.isnan(s.mean.cpu().numpy()), np.isnan(mean))


# ---------------------------------------------------------------- 4. portfolio counts, custom levels
@pytest.fixture(scope="module")
def panel400():
    return PO.random_panel(seed=21, T=20, lo=400, hi=400)


@pytest.mark.parametrize("nport,q", [(2, None), (3, None), (5, None), (20, None), (3, (0.3, 0.7))])
def test_nport_and_levels(E, panel400, nport, q):
    pan = panel400
    exp = PO.portfolio_sort(pan["seg_off"], pan["F"], pan["R"], pan["W"], pan["level"], pan["nyse"], nport=nport, q=q)
    assert exp["status"].all()
    _, got = _sort(E, pan, nport=nport, q=q)
    assert got["rec"].shape == (20, nport + 1, 4) and got["bp"].shape == (20, nport - 1)
    _check(got, exp, f"nport={nport} q={q}")


# ---------------------------------------------------------------- 5. sizes at the limits, bad arguments
@pytest.mark.parametrize("combo", [(0, False), (1, True)])
@pytest.mark.parametrize("T,N", [(2, 5000), (1, 16384)])
def test_long_months(E, T, N, combo):
    """The bench's month and the longest month, with every row a breakpoint row (the sample
    select of months with more than 2,048 breakpoint rows) and with the NYSE rows of the upper
    universes only (5,000 rows: about 1,300 breakpoint rows, the full sort)."""
    pan = PO.random_panel(seed=31, T=T, lo=N, hi=N)
    exp = PO.portfolio_sort(pan["seg_off"], pan["F"], pan["R"], pan["W"], pan["level"], pan["nyse"], nport=10,
                            min_level=combo[0], nyse_breakpoints=combo[1])
    _, got = _sort(E, pan, nport=10, min_level=combo[0], nyse_breakpoints=combo[1])
    _check(got, exp, f"{T}x{N} {combo}")


def test_select_paths(E):
    """Months on either side of the 2,048-breakpoint-row threshold between the full sort and the
    sample select, and long months that defeat the sample select's buckets (a 7-value grid,
    all-equal forecasts, forecasts that differ in the low bits only, two far outliers): the
    order statistics are exact on every path."""
    rng = np.random.default_rng(41)
    grid = np.linspace(-0.02, 0.04, 7)
    fs = [rng.normal(0.01, 0.02, 2048), rng.normal(0.01, 0.02, 2049), grid[rng.integers(0, 7, 5000)],
          np.full(3000, 0.0125), 1.0 + rng.integers(0, 1 << 20, 4000) * 2.0 ** -52,
          np.concatenate([rng.normal(0.01, 0.02, 4998), [50.0, -50.0]]), rng.standard_t(2, 5120) * 0.02]
    seg_off = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int64)
    n = int(seg_off[-1])
    pan = dict(seg_off=seg_off, F=np.concatenate(fs), R=rng.normal(0.01, 0.1, n), W=np.exp(rng.normal(4.0, 1.5, n)))
    for nport in (10, 20):
        exp = PO.portfolio_sort(seg_off, pan["F"], pan["R"], pan["W"], nport=nport)
        assert exp["status"].all()
        _, got = _sort(E, pan, nport=nport)
        _check(got, exp, f"nport={nport}")


def test_bad_arguments_raise(E, panel400):
    from fmcore._lib import FMError
    pan = panel400
    with pytest.raises(FMError, match="exceed"):
        _sort(E, pan, max_seg_len=16385)
    for kw in (dict(nport=1), dict(nport=21), dict(nport=3, q=(0.7, 0.3)), dict(nport=3, q=(0.5, 0.5)),
               dict(nport=3, q=(0.0, 0.5)), dict(nport=3, q=(0.5, 1.0)), dict(nport=3, q=(0.5, float("nan"))),
               dict(min_count=0)):
        with pytest.raises(FMError):
            _sort(E, pan, **kw)
    with pytest.raises(FMError, match="nyse"):
        _sort(E, dict(pan, nyse=None), nyse_breakpoints=True)
    # an empty call is valid
    e = dict(seg_off=np.zeros(1, dtype=np.int64), F=np.zeros(0), R=np.zeros(0))
    _, got = _sort(E, e)
    assert got["rec"].shape == (0, 11, 4) and got["port"].shape == (0,)


# ---------------------------------------------------------------- 6. determinism, month shards
def test_deterministic_and_shardable(E, panel):
    kw = dict(nport=10, min_level=1, nyse_breakpoints=True)
    _, a = _sort(E, panel, **kw)
    _, b = _sort(E, panel, **kw)
    assert _bits(a) == _bits(b)
    off = panel["seg_off"]
    parts = []
    # the second shard also with a larger max_seg_len (another workgroup shape): the same bits
    for (t0, t1), msl in (((0, 23), None), ((23, 60), 2000)):
        r0, r1 = int(off[t0]), int(off[t1])
        sh = {k: panel[k][r0:r1] for k in ("F", "R", "W", "level", "nyse")}
        sh["seg_off"] = off[t0:t1 + 1] - r0
        parts.append(_sort(E, sh, max_seg_len=msl, **kw)[1])
    cat = {k: np.concatenate([parts[0][k], parts[1][k]]) for k in a}
    assert _bits(cat) == _bits(a)


# ---------------------------------------------------------------- 7. summary
@pytest.mark.parametrize("nw_lags", [4, 0])
def test_summary_vs_oracle(E, panel, panel_ref, nw_lags):
    exp = panel_ref[(0, False)]
    p, _ = _sort(E, panel, nport=10)
    s = E.portfolio_summary(p, nw_lags)
    gm, gs, gt, gn = (x.cpu().numpy() for x in (s.mean, s.se, s.tstat, s.nobs))
    mean, se, t, nobs = PO.portfolio_summary(exp["rec"], exp["status"], nw_lags)
    assert gm.shape == (11, 4) and np.array_equal(gn, nobs) and (nobs == 60).all()
    for k in range(11):
        for c in range(4):
            x = exp["rec"][:, k, c]
            rms = float(np.sqrt(np.mean(x * x)))
            assert scalar_close(gm[k, c], mean[k, c], RTOL, rms), (k, c, gm[k, c], mean[k, c])
            assert scalar_close(gs[k, c], se[k, c], RTOL), (k, c, gs[k, c], se[k, c])
            # t = mean / se: the mean's tolerance (RTOL * rms) over the standard error
            assert scalar_close(gt[k, c], t[k, c], RTOL, rms / se[k, c]), (k, c, gt[k, c], t[k, c])


# ---------------------------------------------------------------- 8. drop-in
def test_drop_in_frame(E, CL):
    from fmcore.synth import synth_frame
    nport = 10
    df = synth_frame(40, 300, 5, shuffle=True)
    df["forecast"] = 0.01 + 0.004 * df["log_bm"] + 0.003 * df["return_12_2"]
    monthly, summary = CL.forecast_sorted_portfolios(df, df["forecast"].values, weight_col="me", nport=nport,
                                                     universe="all_but_tiny")
    sub = CL.get_subsets(df)["All stocks"]   # sorted by (month, permno), with the universe mask
    months, counts = np.unique(sub["mthcaldt"].values, return_counts=True)
    seg_off = np.concatenate([[0], np.cumsum(counts)])
    exp = PO.portfolio_sort(seg_off, sub["forecast"].values, sub["retx"].values, sub["me"].values,
                            level=sub["is_all_but_tiny"].to_numpy().astype(np.uint8), nport=nport, min_level=1)
    srt = exp["status"] == 1
    assert srt.all()
    labels = list(range(nport)) + ["H-L"]
    assert list(monthly.columns) == ["ew_ret", "ew_pred", "vw_ret", "vw_pred", "n"]
    assert monthly.shape == (40 * (nport + 1), 5) and monthly.index.names == ["mthcaldt", "portfolio"]
    assert list(monthly.index.get_level_values(1)[:nport + 1]) == labels
    assert np.array_equal(monthly.index.get_level_values(0).unique().values, months)
    for c, name in enumerate(["ew_ret", "ew_pred", "vw_ret", "vw_pred"]):
        got = monthly[name].to_numpy().reshape(40, nport + 1)
        for k in range(nport + 1):
            assert_series_close(got[:, k], exp["rec"][:, k, c], f"{name}[{labels[k]}]")
    n = monthly["n"].to_numpy().reshape(40, nport + 1)
    assert np.array_equal(n[:, :nport], exp["cnt"])
    assert np.array_equal(n[:, nport], exp["cnt"][:, 0] + exp["cnt"][:, -1])
    assert list(summary.index) == labels and summary.shape == (nport + 1, 12)
    mean, se, t, nobs = PO.portfolio_summary(exp["rec"], exp["status"], 4)
    for c, name in enumerate(["ew_ret", "ew_pred", "vw_ret", "vw_pred"]):
        assert list(summary[name].columns) == ["mean", "tstat", "nobs"]
        assert np.array_equal(summary[name]["nobs"].to_numpy(), nobs[:, c])
        for k in range(nport + 1):
            rms = float(np.sqrt(np.mean(exp["rec"][:, k, c] ** 2)))
            assert scalar_close(summary[name]["mean"].iloc[k], mean[k, c], RTOL, rms), (name, k)
            assert scalar_close(summary[name]["tstat"].iloc[k], t[k, c], RTOL, rms / se[k, c]), (name, k)


# ---------------------------------------------------------------- 9. graph capture
def test_graph_capture(E, panel):
    kw = dict(nport=10, min_level=1, nyse_breakpoints=True, max_seg_len=int(np.diff(panel["seg_off"]).max()))
    t = {k: _dev(E, panel[k]) for k in ("seg_off", "F", "R", "W", "level", "nyse")}

    def run():
        return E.portfolio_sort(t["seg_off"], t["F"], t["R"], weight=t["W"], level=t["level"], nyse=t["nyse"], **kw)

    eager = run()
    torch.cuda.synchronize()
    want = {k: getattr(eager, k).cpu().numpy().tobytes() for k in ("bp", "port", "rec", "cnt", "status")}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    for _ in range(2):
        for k in want:
            getattr(out, k).zero_()
        g.replay()
        torch.cuda.synchronize()
        assert {k: getattr(out, k).cpu().numpy().tobytes() for k in want} == want
