"""GPU tests of the double-sorted portfolios (A21; fm_portfolio_double_sort) against the numpy
restatement of its definition (tests/dsort_oracle.py): status, cell bytes, counts and breakpoints
exact, the records bit for bit on the integer-valued fixture (every sum exact in any order, every
mean one division) and within RTOL = 1e-9 of max(|b|, RMS of the series) on real-valued data (a
sum of <= 16,384 FP64 terms sits orders of magnitude below that).

The module's name sorts behind every other GPU module on purpose.  Some of those compare buffers
between two pipeline runs down to tails that no kernel writes (res.moments beyond a problem's
(K + 1)^2 moments, tests/test_gpu_fcmp.py), so they pass or fail with the garbage the caching
allocator hands out, which every module collected in front of them changes."""
import ctypes

import numpy as np
import pytest
import torch

import alpha_oracle as AO
import dsort_oracle as DO
import port_oracle as PO
from fmtol import assert_series_close

pytestmark = pytest.mark.gpu

OUTS = ("rec_b", "rec_a", "cnt", "cell", "bpa", "bpb", "status")


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _dev(E, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(E.require_device())


def _host(ds):
    torch.cuda.synchronize()
    return {k: getattr(ds, k).cpu().numpy() for k in OUTS}


def _sort(E, pan, A=None, B=None, weight=True, **kw):
    """engine.double_sort on host arrays -> (DoubleSort, dict of host arrays with a leading [nsel])."""
    A = pan["A"] if A is None else A
    B = pan["B"] if B is None else B
    ds = E.double_sort(_dev(E, pan["seg_off"]), _dev(E, A), _dev(E, B), _dev(E, pan["R"]),
                       weight=_dev(E, pan.get("W")) if weight else None, level=_dev(E, pan.get("level")),
                       nyse=_dev(E, pan.get("nyse")), **kw)
    return ds, _host(ds)


def _oracle(pan, A=None, B=None, weight=True, **kw):
    A = pan["A"] if A is None else A
    B = pan["B"] if B is None else B
    return DO.double_sort_batch(pan["seg_off"], A, B, pan["R"], W=pan.get("W") if weight else None,
                                level=pan.get("level"), nyse=pan.get("nyse"), **kw)


def _check(got, exp, what="", exact=False):
    for k in ("status", "cell", "cnt"):
        assert got[k].shape == exp[k].shape and np.array_equal(got[k], exp[k]), (what, k)
    for k in ("bpa", "bpb"):
        assert np.array_equal(got[k], exp[k], equal_nan=True), (what, k)
    for k in ("rec_b", "rec_a"):
        g, e = got[k], exp[k]
        assert g.shape == e.shape, (what, k)
        if exact:
            assert np.array_equal(g, e, equal_nan=True), (what, k, np.flatnonzero(~((g == e) | (np.isnan(g) & np.isnan(e))))[:5])
            continue
        S, n1, T, n2, _ = e.shape
        for s in range(S):
            for i in range(n1):
                for j in range(n2):
                    for c in range(4):
                        assert_series_close(g[s, i, :, j, c], e[s, i, :, j, c], f"{what} {k}[{s}, {i}, :, {j}, {c}]")


def _bits(h):
    return {k: v.tobytes() for k, v in h.items()}


# ---------------------------------------------------------------- 1. integer-valued fixture: bit for bit
INT_CASES = {
    "independent 5x5": dict(na=5, nb=5),
    "conditional 5x5": dict(na=5, nb=5, conditional=True),
    "2x3 NYSE": dict(na=2, nb=3, qa=(0.5,), qb=(0.3, 0.7), nyse_breakpoints=True, min_level=1),
    "10x10": dict(na=10, nb=10),
    "10x10 conditional": dict(na=10, nb=10, conditional=True, min_count_bin=3),
}


@pytest.fixture(scope="module")
def ipanel():
    return DO.integer_panel()


@pytest.mark.parametrize("case", list(INT_CASES))
def test_integer_fixture_bits(E, ipanel, case):
    kw = INT_CASES[case]
    B = ipanel["B"][0]
    exp = _oracle(ipanel, B=B, **kw)
    assert exp["status"].all() and (exp["cnt"] > 0).any()
    _, got = _sort(E, ipanel, B=B, **kw)
    _check(got, exp, case, exact=True)


def test_integer_fixture_batch_shared_a(E, ipanel):
    """Three sorts in one launch: a shared (stride 0), b per sort."""
    exp = _oracle(ipanel)
    assert exp["rec_b"].shape[0] == 3 and exp["status"].all()
    ds, got = _sort(E, ipanel)
    _check(got, exp, "batch", exact=True)
    assert ds.by_b.rec.shape == (3 * 6, len(ipanel["seg_off"]) - 1, 6, 4) and ds.by_b.status.shape == (18, 6)


# ---------------------------------------------------------------- 2. real-valued ragged panel
REAL_CASES = {
    "independent": dict(),
    "conditional": dict(conditional=True),
    "level 1, NYSE": dict(min_level=1, nyse_breakpoints=True),
    "conditional 3x4 level 2": dict(na=3, nb=4, conditional=True, min_level=2, nyse_breakpoints=True),
}


@pytest.fixture(scope="module")
def rpanel():
    return DO.ragged_panel()


@pytest.fixture(scope="module")
def rpanel_ref(rpanel):
    return {c: _oracle(rpanel, **kw) for c, kw in REAL_CASES.items()}


@pytest.mark.parametrize("case", list(REAL_CASES))
def test_ragged_panel(E, rpanel, rpanel_ref, case):
    exp = rpanel_ref[case]
    assert exp["status"].all()                     # every month sorted
    if REAL_CASES[case].get("min_level", 0) == 0:
        assert (exp["cnt"] > 0).all()              # no empty cell: no NaN stands in for a number
        assert np.isfinite(exp["rec_b"]).all() and np.isfinite(exp["rec_a"]).all()
    _, got = _sort(E, rpanel, **REAL_CASES[case])
    _check(got, exp, case)


def test_independent_cells_equal_two_single_sorts(E, rpanel):
    """pa and pb out of the cell bytes = fm_portfolio_sort's port bytes on each signal masked where
    the other is not finite."""
    A, B = rpanel["A"], rpanel["B"]
    _, got = _sort(E, rpanel, na=5, nb=4, min_level=1)
    cell = got["cell"][0]
    seg, lv = _dev(E, rpanel["seg_off"]), _dev(E, rpanel["level"])
    Am, Bm = np.where(np.isfinite(B), A, np.nan), np.where(np.isfinite(A), B, np.nan)
    pa = E.portfolio_sort(seg, _dev(E, Am), _dev(E, rpanel["R"]), level=lv, nport=5, min_level=1, min_count=20)
    pb = E.portfolio_sort(seg, _dev(E, Bm), _dev(E, rpanel["R"]), level=lv, nport=4, min_level=1, min_count=20)
    pa, pb = pa.port.cpu().numpy(), pb.port.cpu().numpy()
    assert np.array_equal(cell == 255, pa == 255) and np.array_equal(cell == 255, pb == 255)
    ok = cell != 255
    assert ok.sum() > 1000
    assert np.array_equal(cell[ok] // 4, pa[ok]) and np.array_equal(cell[ok] % 4, pb[ok])


# ---------------------------------------------------------------- 3. edge months
def _edge_panel(lens, seed=3):
    rng = np.random.default_rng(seed)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    return dict(seg_off=seg_off, A=rng.normal(size=n), B=rng.normal(size=n), R=rng.normal(0.01, 0.1, n),
                W=np.exp(rng.normal(size=n)))


EDGE_LENS = {
    "256 x 4 form": [0, 1, 24, 25, 63, 64, 65, 255, 256, 257, 1023, 1024],
    "512 x 10 form": [1025, 40, 3000, 5120],     # 3000: more than 2,048 breakpoint rows, the sample select
    "1024 x 16 form": [5121, 300, 0],
    "16384 rows": [16384],                       # conditional bins of 3,277 rows: the sample select per bin
}


@pytest.mark.parametrize("conditional", [False, True])
@pytest.mark.parametrize("name", list(EDGE_LENS))
def test_edge_month_lengths(E, name, conditional):
    pan = _edge_panel(EDGE_LENS[name])
    exp = _oracle(pan, conditional=conditional)
    want = [int(L >= 25) for L in EDGE_LENS[name]]   # all rows are finite: min_count = na * nb = 25 breakpoint rows
    assert exp["status"][0].tolist() == want
    _, got = _sort(E, pan, conditional=conditional)
    _check(got, exp, name)


def test_too_long_month_refused_outputs_untouched(E):
    from fmcore import _lib as L
    dev = E.require_device()
    n = 64
    seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
    x = torch.arange(n, dtype=torch.float64, device=dev)
    bufs = dict(rec_b=torch.full((6 * 6 * 4,), 7.0, dtype=torch.float64, device=dev),
                rec_a=torch.full((6 * 6 * 4,), 7.0, dtype=torch.float64, device=dev),
                cnt=torch.full((25,), 7, dtype=torch.int32, device=dev), cell=torch.full((n,), 7, dtype=torch.uint8, device=dev),
                bpa=torch.full((4,), 7.0, dtype=torch.float64, device=dev), bpb=torch.full((20,), 7.0, dtype=torch.float64, device=dev),
                status=torch.full((1,), 7, dtype=torch.int32, device=dev))
    a = L.DsortArgs(a=x.data_ptr(), b=x.data_ptr(), ret=x.data_ptr(), seg_off=seg.data_ptr(), nrows=n, nseg=1, nsel=1,
                    max_seg_len=16385, na=5, nb=5, min_count=25, min_count_bin=5,
                    **{k: v.data_ptr() for k, v in bufs.items()})
    for j in range(4):
        a.qa[j] = a.qb[j] = (j + 1) / 5
    lib = L.load()
    rc = lib.fm_portfolio_double_sort(ctypes.byref(a), None)
    torch.cuda.synchronize()
    assert rc == -3 and b"16385" in lib.fm_last_error()     # FM_ETOOBIG
    for k, v in bufs.items():
        assert (v.cpu().numpy() == 7).all(), k
    a.max_seg_len = 16384
    assert lib.fm_portfolio_double_sort(ctypes.byref(a), None) == 0
    torch.cuda.synchronize()
    assert bufs["status"].item() == 1 and (bufs["cell"].cpu().numpy() != 7).all()
    with pytest.raises(L.FMError, match="exceed 16384"):
        E.double_sort(seg, x, x, x, max_seg_len=16385)


def _special_panel():
    """Six months of 400 rows, each one mechanism: (0) all-equal a, (1) heavy ties in b, (2) +-0.0
    around zero breakpoints, (3) NYSE rows all at a = 0 so that the upper a-bins hold no NYSE row,
    (4) exactly min_count breakpoint rows, (5) one row short of it."""
    rng = np.random.default_rng(17)
    T, N = 6, 400
    seg_off = (np.arange(T + 1) * N).astype(np.int64)
    A, B = rng.normal(size=T * N), rng.normal(size=T * N)
    nyse = (rng.random(T * N) < 0.5).astype(np.uint8)
    m = [slice(t * N, (t + 1) * N) for t in range(T)]
    A[m[0]] = 1.5
    B[m[1]] = rng.integers(0, 3, N).astype(np.float64)
    A[m[2]] = rng.choice([-1.0, -0.0, 0.0, 1.0], N, p=[0.05, 0.45, 0.45, 0.05])
    B[m[2]] = rng.choice([-2.0, -0.0, 0.0, 3.0], N, p=[0.05, 0.45, 0.45, 0.05])
    A[m[3]] = np.where(nyse[m[3]] != 0, 0.0, np.abs(A[m[3]]) + 1.0)
    for t, k in ((4, 25), (5, 24)):
        ny = np.zeros(N, dtype=np.uint8)
        ny[rng.choice(N, k, replace=False)] = 1
        nyse[m[t]] = ny
    return dict(seg_off=seg_off, A=A, B=B, R=rng.normal(0.01, 0.1, T * N), W=np.exp(rng.normal(size=T * N)), nyse=nyse)


@pytest.mark.parametrize("conditional", [False, True])
def test_special_months(E, conditional):
    pan = _special_panel()
    kw = dict(conditional=conditional, nyse_breakpoints=True)
    exp = _oracle(pan, **kw)
    assert exp["status"][0].tolist() == [1, 1, 1, 1, 1, 0]
    N = 400
    assert (exp["cell"][0][:N] // 5 == 0).all()                                  # all-equal a: everything in a-bin 0
    assert (exp["bpa"][0][2] == 0).all() and (exp["bpb"][0][2] == 0).any()        # zero breakpoints
    if conditional:
        assert np.isnan(exp["bpb"][0][0, 1:]).all() and np.isfinite(exp["bpb"][0][0, 0]).all()
        assert np.isnan(exp["bpb"][0][3, 1:]).all()                              # a-bins without NYSE rows
        c3 = exp["cell"][0][3 * N:4 * N]
        assert (c3[pan["nyse"][3 * N:4 * N] == 0] == 255).all() and (c3[pan["nyse"][3 * N:4 * N] != 0] < 5).all()
    _, got = _sort(E, pan, **kw)
    _check(got, exp, f"special conditional={conditional}")


def test_no_weight(E, rpanel):
    exp = _oracle(rpanel, weight=False, conditional=True)
    assert np.isnan(exp["rec_b"][..., 2:]).all() and np.isfinite(exp["rec_b"][..., :2]).all()
    _, got = _sort(E, rpanel, weight=False, conditional=True)
    _check(got, exp, "no weight")


# ---------------------------------------------------------------- 4. bits
@pytest.mark.parametrize("conditional", [False, True])
def test_bits_repeat_subrange_batch(E, rpanel, conditional):
    kw = dict(conditional=conditional, min_level=1)
    B3 = np.stack([rpanel["B"], rpanel["B"][::-1].copy(), np.where(rpanel["level"] > 0, rpanel["B"], -rpanel["B"])])
    _, full = _sort(E, rpanel, B=B3, **kw)
    _, again = _sort(E, rpanel, B=B3, **kw)
    assert _bits(full) == _bits(again)
    # one sort alone = the same sort inside the batch
    _, alone = _sort(E, rpanel, B=B3[1], **kw)
    for k in OUTS:
        assert alone[k][0].tobytes() == full[k][1].tobytes(), k
    # a sub-range of the months (the same row vectors, a slice of seg_off)
    lo, hi = 7, 19
    sub = dict(rpanel, seg_off=rpanel["seg_off"][lo:hi + 1])
    _, part = _sort(E, sub, B=B3, **kw)
    r0, r1 = int(rpanel["seg_off"][lo]), int(rpanel["seg_off"][hi])
    for k in ("cnt", "bpa", "bpb", "status"):
        assert part[k].tobytes() == np.ascontiguousarray(full[k][:, lo:hi]).tobytes(), k
    for k in ("rec_b", "rec_a"):
        assert part[k].tobytes() == np.ascontiguousarray(full[k][:, :, lo:hi]).tobytes(), k
    assert part["cell"][:, r0:r1].tobytes() == np.ascontiguousarray(full["cell"][:, r0:r1]).tobytes()


@pytest.mark.parametrize("conditional", [False, True])
def test_bits_across_forms(E, conditional):
    """A 700-row month alone (256 x 4 form), beside a 3,000-row month (512 x 10) and beside a
    6,000-row month (1024 x 16): the same bits."""
    pan = _edge_panel([700, 3000, 6000], seed=23)
    outs = []
    for T in (1, 2, 3):
        sub = dict(pan, seg_off=pan["seg_off"][:T + 1])
        _, h = _sort(E, sub, conditional=conditional)
        outs.append(h)
    for h in outs[1:]:
        for k in ("cnt", "bpa", "bpb", "status"):
            assert h[k][:, :1].tobytes() == outs[0][k].tobytes(), k
        for k in ("rec_b", "rec_a"):
            assert np.ascontiguousarray(h[k][:, :, :1]).tobytes() == outs[0][k].tobytes(), k
        assert h["cell"][:, :700].tobytes() == outs[0]["cell"][:, :700].tobytes()
    assert np.ascontiguousarray(outs[2]["rec_b"][:, :, :2]).tobytes() == outs[1]["rec_b"].tobytes()


# ---------------------------------------------------------------- 5. consumers
def test_consumers(E, rpanel, rpanel_ref):
    exp = rpanel_ref["conditional"]
    ds, got = _sort(E, rpanel, conditional=True)
    T = exp["status"].shape[1]
    s = E.portfolio_summary(ds.by_b, nw_lags=4)
    torch.cuda.synchronize()
    assert tuple(s.mean.shape) == (6, 6, 4)
    for i in range(6):
        mean, se, t, nobs = PO.portfolio_summary(exp["rec_b"][0, i], exp["status"][0], 4)
        assert np.array_equal(s.nobs[i].cpu().numpy(), nobs)
        assert_series_close(s.mean[i].cpu().numpy().ravel(), mean.ravel(), f"summary mean slab {i}")
        assert_series_close(s.tstat[i].cpu().numpy().ravel(), t.ravel(), f"summary t slab {i}")
    rng = np.random.default_rng(2)
    F = rng.normal(0.005, 0.04, (T, 2))
    al = E.portfolio_alphas(ds.by_a, _dev(E, F), models=[[0], [0, 1]], nw_lags=3)
    torch.cuda.synchronize()
    assert tuple(al.coef.shape) == (6, 6, 2, 2, 3)
    ref = AO.portfolio_alphas(exp["rec_a"][0, 5], exp["status"][0], F, [[0], [0, 1]], nw_lags=3)   # the b-neutral slab
    gota = {k: getattr(al, k)[5].cpu().numpy() for k in AO.OUTS}
    AO.assert_alphas_close(gota, ref, [[0], [0, 1]], "alphas of the b-neutral a portfolios")
    for axis, rec, w, c in (("b", "rec_b", True, 2), ("b", "rec_b", False, 0), ("a", "rec_a", True, 2)):
        f = E.sort_factors(ds, axis=axis, weighted=w)
        assert tuple(f.shape) == (T, 1) and f.dtype == torch.float64
        assert np.array_equal(f.cpu().numpy()[:, 0], got[rec][0, -1, :, -1, c], equal_nan=True)
    f2 = E.sort_factors(ds, "b")
    al2 = E.portfolio_alphas(ds.by_b, f2, models=[[0]])     # the factor series is accepted as ``factors``
    torch.cuda.synchronize()
    assert np.isfinite(al2.coef.cpu().numpy()[:5, :, :, 0, 0]).all()


# ---------------------------------------------------------------- 6. pipeline
def test_pipeline_equals_double_sort_by_hand(E):
    import pipe_port_oracle as PPO
    from fmcore import lewellen as LW
    fx = PPO.pipeline_fixture()
    a, c = fx["arrays"], PPO.PIPE
    panel = E.panel_from_arrays(fx["cols"], fx["names"], a["month"], me=a["me"], nyse=a["nyse"], layout="f64")
    base = dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"], portfolios=c["nport"])
    off = LW.run_pipeline(panel, LW.PipelineConfig(**base), model_cols=fx["model_cols"])
    out = LW.run_pipeline(panel, LW.PipelineConfig(double_sort="log_size", double_sort_shape=(3, 4),
                                                   double_sort_conditional=True, **base), model_cols=fx["model_cols"])
    torch.cuda.synchronize()
    assert off.double_sort is None and off.portfolios.forecast is None
    for k in ("bp", "port", "rec", "cnt", "status"):   # the portfolio stage itself is what it was
        assert getattr(out.portfolios, k).cpu().numpy().tobytes() == getattr(off.portfolios, k).cpu().numpy().tobytes(), k
    ds, F = out.double_sort, out.portfolios.forecast
    nsort = len(out.portfolio_problems)
    assert tuple(F.shape) == (nsort, panel.nrows) and tuple(ds.status.shape) == (nsort, panel.nseg) and nsort == 9
    got = _host(ds)
    assert got["status"].any(axis=1).all()
    size = E.column_vector(panel, "log_size")
    for j, k in enumerate(out.portfolio_problems):
        lv = out.res.problems[k].level
        one = E.double_sort(panel.seg_off, size, F[j].contiguous(), E.column_vector(panel, "retx"), weight=panel.me,
                            level=out.level, nyse=panel.nyse, na=3, nb=4, conditional=True, min_level=lv)
        h = _host(one)
        for key in OUTS:
            assert h[key][0].tobytes() == got[key][j].tobytes(), (j, key)
    sb, sa = out.double_sort_summary
    assert tuple(sb.mean.shape) == (nsort, 4, 5, 4) and tuple(sa.mean.shape) == (nsort, 5, 4, 4)
    mean, _, _, nobs = PO.portfolio_summary(got["rec_b"][2, 3], got["status"][2], 4)
    assert np.array_equal(sb.nobs[2, 3].cpu().numpy(), nobs)
    assert_series_close(sb.mean[2, 3].cpu().numpy().ravel(), mean.ravel(), "pipeline double-sort summary")


# ---------------------------------------------------------------- 7. drop-in
def _frame(seed=4, T=14, N=160):
    import pandas as pd
    rng = np.random.default_rng(seed)
    n = T * N
    months = np.repeat((np.datetime64("2001-01") + np.arange(T)).astype("datetime64[ns]"), N)
    df = pd.DataFrame({"mthcaldt": months, "permno": np.tile(np.arange(N) + 10000, T),
                       "retx": rng.normal(0.01, 0.1, n), "me": np.exp(rng.normal(5, 2, n)),
                       "primaryexch": rng.choice(["N", "Q", "A"], n, p=[0.5, 0.4, 0.1]),
                       "bm": rng.normal(size=n), "mom": rng.normal(size=n), "sig": rng.normal(0.01, 0.02, n)})
    df.loc[rng.random(n) < 0.03, "bm"] = np.nan
    df.loc[rng.random(n) < 0.03, "retx"] = np.nan
    return df.sample(frac=1.0, random_state=1).sort_values("mthcaldt", kind="stable").reset_index(drop=True)


def test_drop_in_double_sorted_portfolios(E):
    from fmdrop import calc_Lewellen_2014 as CL
    df = _frame()
    seg = np.concatenate([[0], np.cumsum(df.groupby("mthcaldt", sort=True).size().to_numpy())])
    nyse = (df["primaryexch"] == "N").to_numpy().astype(np.uint8)
    kw = dict(na=3, nb=4, conditional=True, nyse_breakpoints=True)
    exp = DO.double_sort(seg, df["me"].to_numpy(), df["bm"].to_numpy(), df["retx"].to_numpy(), W=df["me"].to_numpy(),
                         nyse=nyse, **kw)
    assert exp["status"].all() and (exp["cnt"] > 0).all()
    monthly, summary = CL.double_sorted_portfolios(df, "me", df["bm"].to_numpy(), weight_col="me", **kw)
    months = np.sort(df["mthcaldt"].unique())
    assert monthly.index.get_level_values(0).unique().tolist() == list(months) and len(monthly) == len(months) * 5 * 6
    for t in (0, 5, 13):
        m = monthly.loc[months[t]]
        for i in range(3):
            for j in range(4):
                row = m.loc[(i, j)]
                assert row["n"] == exp["cnt"][t, i, j]
                assert_series_close(row[["ew_ret", "ew_b", "vw_ret"]].to_numpy(float), exp["rec_b"][i, t, j, :3], f"cell {t} {i} {j}")
                assert_series_close(row[["ew_a"]].to_numpy(float), exp["rec_a"][j, t, i, 1:2], f"cell a {t} {i} {j}")
    got = monthly["vw_ret"].unstack(["a_bin", "b_bin"])
    assert_series_close(got[("avg", "H-L")].to_numpy(), exp["rec_b"][3, :, 4, 2], "a-neutral H-L of b")
    assert_series_close(got[("H-L", "avg")].to_numpy(), exp["rec_a"][4, :, 3, 2], "b-neutral H-L of a")
    assert_series_close(got[(1, "H-L")].to_numpy(), exp["rec_b"][1, :, 4, 2], "row 1 H-L")
    mean, se, t, nobs = PO.portfolio_summary(exp["rec_b"][3], exp["status"], 4)
    assert summary.loc[("avg", "H-L"), ("vw_ret", "nobs")] == nobs[4, 2]
    assert_series_close(summary.loc[[("avg", j) for j in (0, 1, 2, 3, "H-L")], ("ew_ret", "mean")].to_numpy(float), mean[:, 0],
                        "summary of the a-neutral b portfolios")
    assert_series_close(summary.loc[[("avg", "H-L")], ("ew_ret", "tstat")].to_numpy(float), t[4:, 0], "its t")


def test_drop_in_characteristic_factors(E):
    from fmdrop import calc_Lewellen_2014 as CL
    df = _frame()
    seg = np.concatenate([[0], np.cumsum(df.groupby("mthcaldt", sort=True).size().to_numpy())])
    nyse = (df["primaryexch"] == "N").to_numpy().astype(np.uint8)
    chars = ["bm", "mom"]
    fac = CL.characteristic_factors(df, chars)
    assert list(fac.columns) == chars + ["SMB"] and len(fac) == 14 and fac.index.name == "mthcaldt"
    smb = []
    for c in chars:
        exp = DO.double_sort(seg, df["me"].to_numpy(), df[c].to_numpy(), df["retx"].to_numpy(), W=df["me"].to_numpy(),
                             nyse=nyse, na=2, nb=3, qa=(0.5,), qb=(0.3, 0.7), nyse_breakpoints=True)
        assert exp["status"].all() and np.isfinite(exp["rec_b"][2, :, 3, 2]).all()
        assert_series_close(fac[c].to_numpy(), exp["rec_b"][2, :, 3, 2], f"factor {c}")
        smb.append(exp["rec_a"][3, :, 2, 2])
    assert_series_close(fac["SMB"].to_numpy(), -(smb[0] + smb[1]) / 2, "SMB")


def test_build_tables_accept_the_factors(E):
    """build_table_alphas takes characteristic_factors' frame, and build_table_double_sort's frames are the
    pipeline's own summary."""
    import pipe_port_oracle as PPO
    from fmcore import lewellen as LW
    from fmcore import synth
    from fmdrop import calc_Lewellen_2014 as CL
    c = PPO.PIPE
    df = synth.synth_frame(c["T"], c["N"], c["seed"], nan_rate=c["nan_rate"], present_rate=c["present_rate"])
    base = dict(window=c["window"], min_periods=c["min_periods"], lag=c["lag"])
    fac = CL.characteristic_factors(df, ["log_bm", "return_12_2"])
    assert np.isfinite(fac.to_numpy()).all() and len(fac) == c["T"]
    tabs = CL.build_table_alphas(df, fac, nport=c["nport"], **base)
    assert len(tabs) == 9
    t = tabs[("Model 1: Three Predictors", "All stocks")]
    assert np.isfinite(t[("vw", "FF", "alpha")].to_numpy(float)).all() and (t[("vw", "FF", "nobs")] > 3).all()
    ds = CL.build_table_double_sort(df, by="log_size", shape=(2, 3), portfolios=c["nport"], **base)
    assert len(ds) == 9
    panel, mc = CL._pipeline_panel(df)
    out = LW.run_pipeline(panel, LW.PipelineConfig(portfolios=c["nport"], double_sort="log_size", double_sort_shape=(2, 3), **base),
                          model_cols=mc)
    sb = out.double_sort_summary[0]
    j = 4
    prob = out.res.problems[out.portfolio_problems[j]]
    t = ds[(out.model_names[prob.model], LW.SUBSET_NAMES[prob.level])]
    assert list(t.index) == [0, 1, "avg"] and list(t.columns)[:5] == [("ew", 0), ("ew", 1), ("ew", 2), ("ew", "H-L"), ("ew", "t(H-L)")]
    assert np.array_equal(t[("vw", "H-L")].to_numpy(float), sb.mean[j, :, 3, 2].cpu().numpy(), equal_nan=True)
    assert np.array_equal(t[("ew", 1)].to_numpy(float), sb.mean[j, :, 1, 0].cpu().numpy(), equal_nan=True)
    assert np.isfinite(t.drop(columns=[("ew", "t(H-L)"), ("vw", "t(H-L)")]).to_numpy(float)).all()   # (a Newey-West variance
    # of 24 months can come out negative, and its t NaN, here as in portfolio_summary's own tests' oracle)
    assert np.array_equal(t[("ew", "t(H-L)")].to_numpy(float), sb.tstat[j, :, 3, 0].cpu().numpy(), equal_nan=True)
