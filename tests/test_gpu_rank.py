"""GPU tests of the per-month rank transform (A13; fm_rank_transform) against pandas
(tests/rank_oracle.py).  Every rank comparison is bit-exact: equal NaN masks and equal int64
views of the non-NaN outputs.

The kernel's internal thresholds (fm_rank.hip): a wave sorts a run of 64 R keys, R = 8 for
panels whose longest month has <= 8,192 rows and R = 16 above, so
  * the panel's longest month 8,192 | 8,193 switches R (and the run length 512 | 1,024);
  * a month's run count changes at every multiple of the run length: 512 k | 512 k + 1
    (R = 8), 1,024 k | 1,024 k + 1 (R = 16);
  * the merge depth changes where the run count passes a power of two (512, 1,024, 2,048,
    4,096 rows for R = 8; 1,024 .. 8,192 for R = 16), and a run count that is no power of
    two (3 and 5 runs: 1,536 / 2,560 and 3,072 / 5,120 rows) merges against a virtual tail.
EDGE_LENS (R = 16, the issue's lengths) and SHORT_LENS (R = 8) put a month on either side of
each."""
import numpy as np
import pandas as pd
import pytest
import torch

import rank_oracle as RO
from fmtol import assert_series_close

pytestmark = pytest.mark.gpu

EDGE_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096,
             4097, 5119, 5120, 5121, 8191, 8193]
SHORT_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048,
              2049, 2559, 2560, 2561, 4095, 4096, 4097, 8191, 8192]


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _seg(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _panel(E, X, seg_off, names=None):
    """A DevicePanel straight from host columns X [C, n] already in month order."""
    dev = E.require_device()
    X = np.ascontiguousarray(X, dtype=np.float64)
    names = names or [f"c{i}" for i in range(X.shape[0])]
    return E.DevicePanel(cols=torch.from_numpy(X).to(dev), names=list(names),
                         seg_off=torch.from_numpy(seg_off).to(dev), seg_off_h=seg_off,
                         months=np.arange(len(seg_off) - 1))


def _rank(E, panel, **kw):
    out = E.rank_transform(panel, **kw)
    torch.cuda.synchronize()
    return out, out.cols.cpu().numpy(), out.rank_nvalid.cpu().numpy()


def _grid7(n, rng):
    return np.linspace(-0.02, 0.04, 7)[rng.integers(0, 7, n)]


def _length_panel(lens, seed):
    rng = np.random.default_rng(seed)
    seg_off = _seg(lens)
    n = int(seg_off[-1])
    a = rng.normal(size=n)
    a[rng.random(n) < 0.05] = np.nan
    return seg_off, np.stack([a, rng.normal(size=n), _grid7(n, rng), RO.tie_heavy(n, rng)])


@pytest.fixture(scope="module")
def length_panels():
    """The two length panels and pandas' ranks of their columns 0, 2, 3 for every combination,
    computed once."""
    out = {}
    for name, lens, seed in (("edge", EDGE_LENS, 21), ("short", SHORT_LENS, 22)):
        seg_off, X = _length_panel(lens, seed)
        exp = {c: np.stack([RO.pandas_rank(X[i], seg_off, *c) for i in (0, 2, 3)]) for c in RO.COMBOS}
        nv = np.stack([RO.pandas_nvalid(X[i], seg_off) for i in (0, 2, 3)])
        out[name] = (seg_off, X, exp, nv)
    return out


# ---------------------------------------------------------------- 1. edge month lengths
@pytest.mark.parametrize("which", ["edge", "short"])
@pytest.mark.parametrize("method,scale", RO.COMBOS)
def test_month_lengths(E, length_panels, which, method, scale):
    seg_off, X, exp, nv = length_panels[which]
    assert (np.diff(seg_off).max() > 8192) == (which == "edge")   # R = 16 and R = 8
    panel = _panel(E, X, seg_off)
    _, got, gnv = _rank(E, panel, cols=["c0", 2, 3], method=method, scale=scale)
    RO.assert_same_bits(got[[0, 2, 3]], exp[(method, scale)], f"{which} {method}/{scale}")
    assert got[1].tobytes() == X[1].tobytes()   # the column not chosen is copied unchanged
    assert np.array_equal(gnv, nv)


# ---------------------------------------------------------------- 2. edge data
def _edge_data():
    rng = np.random.default_rng(31)
    months = []
    months.append(np.full(700, np.nan))                                    # all NaN
    months.append(np.full(1300, 0.0125))                                   # all equal: one tie run over every run
    months.append(_grid7(3000, rng))                                       # runs of ~430 equal values
    # tie runs of 200 equal values across every multiple of 512 and of 1,024 in sorted order,
    # once with the rows in sorted order (the ties also straddle the waves' row blocks), once shuffled
    v = np.arange(3000, dtype=np.float64)
    for b in range(512, 3000, 512):
        v[b - 100:b + 100] = b - 100
    months.append(v.copy())
    months.append(rng.permutation(v))
    e = rng.normal(size=600)
    e[:5], e[5:9] = np.inf, -np.inf
    months.append(rng.permutation(e))                                      # +-inf at both ends
    z = np.concatenate([-rng.random(30), np.full(20, -0.0), np.full(20, 0.0), rng.random(30)])
    months.append(rng.permutation(z))                                      # -0.0 / +0.0 mixed: they tie
    months.append(1.0 + rng.integers(0, 1 << 20, 900) * 2.0 ** -52)        # differ only in the low 32 bits
    p = rng.normal(size=500)
    pi = p.view(np.uint64)
    pi[::7] = np.uint64(0x7FF0000000000001)                                # NaNs with the payload in the low word:
    pi[3::7] = np.uint64(0xFFF0000000000400)                               # +-inf's high word
    p[1::7] = np.inf
    months.append(p)
    one = np.full(300, np.nan)
    one[137] = -3.5
    months.append(one)                                                     # exactly one eligible row
    months.append(RO.tie_heavy(2100, rng))
    seg_off = _seg([len(m) for m in months])
    return seg_off, np.concatenate(months)[None, :]


@pytest.mark.parametrize("method,scale", RO.COMBOS)
def test_edge_data(E, method, scale):
    seg_off, X = _edge_data()
    exp = RO.pandas_rank(X[0], seg_off, method, scale)
    _, got, gnv = _rank(E, _panel(E, X, seg_off), method=method, scale=scale)
    RO.assert_same_bits(got[0], exp, f"{method}/{scale}")
    assert np.array_equal(gnv[0], RO.pandas_nvalid(X[0], seg_off))
    assert gnv[0][0] == 0 and np.isnan(got[0][:700]).all()
    row = got[0][seg_off[9] + 137]   # the lone eligible row: rank 1, pct 1.0, uniform 0.0
    assert gnv[0][9] == 1 and row == {"raw": 1.0, "pct": 1.0, "uniform": 0.0}[scale]
    zs = X[0][seg_off[6]:seg_off[7]] == 0
    assert len(np.unique(got[0][seg_off[6]:seg_off[7]][zs])) == 1   # the signed zeros tie


# ---------------------------------------------------------------- 3. universe mask
@pytest.mark.parametrize("min_level", [1, 2])
@pytest.mark.parametrize("method,scale", [("average", "pct"), ("min", "raw"), ("max", "uniform")])
def test_universe_mask(E, min_level, method, scale):
    rng = np.random.default_rng(41)
    seg_off = _seg([300, 900, 64, 1500, 10])
    n = int(seg_off[-1])
    X = np.stack([RO.tie_heavy(n, rng), rng.normal(size=n)])
    level = rng.integers(0, 3, n).astype(np.uint8)
    level[seg_off[2]:seg_off[3]] = 0          # a month where no row is eligible
    level[seg_off[4]:seg_off[5]] = 1          # eligible at min_level 1 only
    panel = _panel(E, X, seg_off)
    _, got, gnv = _rank(E, panel, method=method, scale=scale, level=torch.from_numpy(level).to(panel.device),
                        min_level=min_level)
    for i in range(2):
        RO.assert_same_bits(got[i], RO.pandas_rank(X[i], seg_off, method, scale, level, min_level), f"col {i}")
        assert np.array_equal(gnv[i], RO.pandas_nvalid(X[i], seg_off, level, min_level))
    assert (gnv[:, 2] == 0).all() and ((gnv[:, 4] == 0).all() == (min_level == 2))


# ---------------------------------------------------------------- 4. the limit, dst == src
def test_limit(E):
    from fmcore import _lib as L
    rng = np.random.default_rng(51)
    n = E.RANK_MAX_ROWS
    x = rng.normal(size=n + 1)
    x[rng.random(n + 1) < 0.02] = np.nan
    seg_off = _seg([n])
    _, got, gnv = _rank(E, _panel(E, x[None, :n], seg_off), method="average", scale="uniform")
    RO.assert_same_bits(got[0], RO.pandas_rank(x[:n], seg_off, "average", "uniform"), "RANK_MAX_ROWS")
    assert gnv[0, 0] == np.count_nonzero(~np.isnan(x[:n]))
    # one row more: refused before any launch, dst untouched
    big = _panel(E, x[None, :], _seg([n + 1]))
    out = torch.full((1, n + 1), 7.0, dtype=torch.float64, device=big.device)
    with pytest.raises(L.FMError, match=r"\(-3\)"):
        E.rank_transform(big, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_dst_equals_src_refused(E):
    from fmcore import _lib as L
    panel = _panel(E, np.arange(10.0)[None, :], _seg([10]))
    with pytest.raises(ValueError):
        E.rank_transform(panel, out=panel.cols)
    a = L.RankArgs()
    a.src = a.dst = panel.cols.data_ptr()
    a.src_stride = a.dst_stride = 10
    a.ncols, a.nseg, a.max_seg_len, a.seg_off = 1, 1, 10, panel.seg_off.data_ptr()
    with pytest.raises(L.FMError, match=r"\(-1\)"):
        L.call("fm_rank_transform", L.C.byref(a), None)
    torch.cuda.synchronize()
    assert panel.cols.cpu().numpy().tolist() == [list(np.arange(10.0))]


# ---------------------------------------------------------------- 5. random ragged panel
@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(61)
    lens = rng.integers(300, 5201, 24)
    seg_off = _seg(lens)
    n = int(seg_off[-1])
    X = rng.normal(size=(4, n))
    X[1] = np.round(X[1], 2)        # ties
    X[rng.random((4, n)) < 0.05] = np.nan
    return seg_off, X


@pytest.mark.parametrize("method,scale", RO.COMBOS)
def test_random_panel(E, ragged, method, scale):
    seg_off, X = ragged
    _, got, gnv = _rank(E, _panel(E, X, seg_off), method=method, scale=scale)
    for i in range(4):
        RO.assert_same_bits(got[i], RO.pandas_rank(X[i], seg_off, method, scale), f"col {i} {method}/{scale}")
        assert np.array_equal(gnv[i], RO.pandas_nvalid(X[i], seg_off))   # nvalid = pandas' group counts


def test_planes_only_input(E, ragged):
    seg_off, X = ragged
    labels = RO.month_codes(seg_off)
    names = ["a", "b", "c", "d"]
    f64 = E.panel_from_arrays(list(X), names, labels, layout="f64")
    pl = E.panel_from_arrays(list(X), names, labels, layout="planes")
    assert pl.cols is None
    _, a, na = _rank(E, f64, cols=["b", "d"], method="average", scale="uniform")
    out, b, nb = _rank(E, pl, cols=["b", "d"], method="average", scale="uniform")
    assert a.tobytes() == b.tobytes() and na.tobytes() == nb.tobytes()
    assert out.cols is not None and out.planes is None and out.seg_off is pl.seg_off and out.order is pl.order
    E.split_planes(out)   # the caller may split the result


def test_month_locality(E, ragged):
    seg_off, X = ragged
    _, full, nfull = _rank(E, _panel(E, X, seg_off), method="max", scale="pct")
    r0, r1 = int(seg_off[8]), int(seg_off[16])
    _, sub, nsub = _rank(E, _panel(E, X[:, r0:r1], seg_off[8:17] - r0), method="max", scale="pct")
    assert sub.tobytes() == np.ascontiguousarray(full[:, r0:r1]).tobytes()
    assert np.array_equal(nsub, nfull[:, 8:16])


# ---------------------------------------------------------------- 6. drop-in
def test_drop_in(E):
    from fmdrop import calc_Lewellen_2014 as CL
    rng = np.random.default_rng(71)
    T, N = 12, 180
    df = pd.DataFrame({"mthcaldt": np.repeat(pd.date_range("2001-01-31", periods=T, freq="ME"), N),
                       "permno": np.tile(np.arange(N), T), "x": RO.tie_heavy(T * N, rng),
                       "y": rng.normal(size=T * N), "me": np.exp(rng.normal(5, 2, T * N)),
                       "primaryexch": np.where(rng.random(T * N) < 0.4, "N", "Q")})
    df.loc[rng.random(len(df)) < 0.03, "me"] = np.nan
    df.loc[rng.random(len(df)) < 0.02, "mthcaldt"] = pd.NaT
    df.loc[df["mthcaldt"] == df["mthcaldt"].max(), "primaryexch"] = "Q"   # a month without NYSE rows
    df = df.sample(frac=1.0, random_state=3)                              # shuffled, its own index labels
    g = df[df["primaryexch"] == "N"].groupby("mthcaldt")["me"]
    lvl = (df["me"] >= df["mthcaldt"].map(g.quantile(0.2))).astype(int) + \
        (df["me"] >= df["mthcaldt"].map(g.quantile(0.5))).astype(int)
    for universe, ml in ((None, 0), ("all_but_tiny", 1), ("large", 2)):
        got = CL.rank_transform(df, ["x", "y"], method="min", scale="pct", universe=universe)
        assert got.index.equals(df.index) and list(got.columns) == list(df.columns)
        for v in ("x", "y"):
            exp = df[v].where(lvl >= ml).groupby(df["mthcaldt"]).rank(method="min", pct=True)
            RO.assert_same_bits(got[v].to_numpy(), exp.to_numpy(dtype=np.float64), f"{v} {universe}")
        assert got.loc[df["mthcaldt"].isna(), ["x", "y"]].isna().all().all()
    uni = CL.rank_transform(df, ["y"], scale="uniform")
    gy = df["y"].groupby(df["mthcaldt"])
    RO.assert_same_bits(uni["y"].to_numpy(), (gy.rank() / (gy.transform("count") + 1) - 0.5).to_numpy(), "uniform")


# ---------------------------------------------------------------- 7. pipeline
def _pipe_inputs():
    from fmcore import lewellen as LW, synth
    a = synth.synth_arrays(80, 600, 23, nan_rate=0.03)
    mc = LW.table2_models()
    cols = list(dict.fromkeys(["retx"] + [c for xs in mc.values() for c in xs] + LW.FIG1_VARS))
    return a, mc, cols


def _ranked_by_pandas(a, cols, y=None):
    """The host arrays with every predictor replaced by pandas' average / uniform rank."""
    month = pd.Series(a["month"])
    out = {}
    for c in cols:
        if c == "retx":
            out[c] = a[c] if y is None else y
        else:
            g = pd.Series(a[c]).groupby(month)
            out[c] = (g.rank() / (g.transform("count") + 1) - 0.5).to_numpy()
    return out


def _bits_equal(x, y, what):
    x, y = x.cpu().numpy(), y.cpu().numpy()
    assert x.shape == y.shape and x.tobytes() == y.tobytes(), what


def test_pipeline_bit_identical(E):
    from fmcore import lewellen as LW
    a, mc, cols = _pipe_inputs()
    mk = lambda d: E.panel_from_arrays([d[c] for c in cols], cols, a["month"], me=a["me"], nyse=a["nyse"])
    got = LW.run_pipeline(mk(a), LW.PipelineConfig(rank="uniform", winsorize=False), model_cols=mc)
    exp = LW.run_pipeline(mk(_ranked_by_pandas(a, cols)), LW.PipelineConfig(winsorize=False), model_cols=mc)
    assert (exp.res.status.cpu().numpy() & 1).any()
    _bits_equal(got.res.rec, exp.res.rec, "records")
    _bits_equal(got.res.status, exp.res.status, "status")
    for k in ("mean", "se", "tstat", "nobs"):
        _bits_equal(getattr(got.summary, k), getattr(exp.summary, k), f"summary {k}")
        _bits_equal(getattr(got.pred_summary, k), getattr(exp.pred_summary, k), f"predictive summary {k}")
    _bits_equal(got.rolling, exp.rolling, "rolling means")
    _bits_equal(got.pred, exp.pred, "predictive records")
    _bits_equal(got.pred_status, exp.pred_status, "predictive status")
    with pytest.raises(ValueError):
        LW.run_pipeline(mk(a), LW.PipelineConfig(rank="uniform", standardize=True), model_cols=mc)


def test_pipeline_winsorized(E):
    """winsorize=True: the ranked columns carry no cuts, y keeps the unranked run's cuts, and
    the records equal those of pandas-ranked predictors with a pre-clipped y (no select, so no
    Gram pivot) within the project's tolerance."""
    from fmcore import lewellen as LW
    a, mc, cols = _pipe_inputs()
    mk = lambda d: E.panel_from_arrays([d[c] for c in cols], cols, a["month"], me=a["me"], nyse=a["nyse"])
    got = LW.run_pipeline(mk(a), LW.PipelineConfig(rank="uniform"), model_cols=mc)
    plain = LW.run_pipeline(mk(a), LW.PipelineConfig(), model_cols=mc)
    yi = cols.index("retx")
    lo, hi = got.cuts.lo.cpu().numpy(), got.cuts.hi.cpu().numpy()
    rest = [i for i in range(len(cols)) if i != yi]
    assert np.isnan(lo[rest]).all() and np.isnan(hi[rest]).all()
    assert lo[yi].tobytes() == plain.cuts.lo[yi].cpu().numpy().tobytes()
    assert hi[yi].tobytes() == plain.cuts.hi[yi].cpu().numpy().tobytes()
    assert np.isfinite(lo[yi]).all()
    # y clipped on the host at the device's own cuts (months in label order = segment order)
    codes = pd.factorize(a["month"], sort=True)[0]
    yc = np.clip(a["retx"], lo[yi][codes], hi[yi][codes])
    exp = LW.run_pipeline(mk(_ranked_by_pandas(a, cols, y=yc)), LW.PipelineConfig(winsorize=False), model_cols=mc)
    assert np.array_equal(got.res.status.cpu().numpy(), exp.res.status.cpu().numpy())
    g, e = got.res.rec.cpu().numpy(), exp.res.rec.cpu().numpy()
    for p in range(g.shape[1]):
        for k in range(g.shape[2]):
            assert_series_close(g[:, p, k], e[:, p, k], f"problem {p} rec[{k}]")
