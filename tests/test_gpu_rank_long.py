"""GPU tests of the rank transform's long-month path (fm_rank.hip, rank_long_kernel: months of
more than 16,384 rows, up to 65,536) against pandas (tests/rank_oracle.py), bit for bit.

The kernel's internal sizes: a month is visited in parts of 16,384 rows (parts start at
multiples of 16,384), each sorted by one workgroup as the short path does, and the rows a
workgroup ranks are one such part, so a month of L rows takes ceil(L / 16,384) workgroups of
as many part-sorts each.  LONG_LENS puts a month on either side of every part boundary, beside
short months (one part, the later slices' workgroups return at once) and last parts that are
a whole number of runs (20,480) or not (20,000)."""
import numpy as np
import pandas as pd
import pytest
import torch

import rank_oracle as RO
import test_gpu_rank as TR

pytestmark = pytest.mark.gpu

PART = 16384
LONG_LENS = [0, 1, 5000, 16383, 16384, 16385, 20000, 20480, 32767, 32768, 32769, 49152, 49153, 65535, 65536]
LOCAL_MONTH = 6   # the 20,000-row month of LONG_LENS


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module")
def long_panel():
    """The length panel and pandas' ranks of its columns 0, 2, 3 for every combination,
    computed once."""
    seg_off, X = TR._length_panel(LONG_LENS, 81)
    exp = {c: np.stack([RO.pandas_rank(X[i], seg_off, *c) for i in (0, 2, 3)]) for c in RO.COMBOS}
    nv = np.stack([RO.pandas_nvalid(X[i], seg_off) for i in (0, 2, 3)])
    return seg_off, X, exp, nv


# ---------------------------------------------------------------- 1. month lengths
@pytest.mark.parametrize("method,scale", RO.COMBOS)
def test_month_lengths(E, long_panel, method, scale):
    seg_off, X, exp, nv = long_panel
    assert LONG_LENS[LOCAL_MONTH] == 20000 and np.diff(seg_off).max() == E.RANK_MAX_ROWS
    _, got, gnv = TR._rank(E, TR._panel(E, X, seg_off), cols=["c0", 2, 3], method=method, scale=scale)
    RO.assert_same_bits(got[[0, 2, 3]], exp[(method, scale)], f"{method}/{scale}")
    assert got[1].tobytes() == X[1].tobytes()   # the column not chosen is copied unchanged
    assert np.array_equal(gnv, nv)


# ---------------------------------------------------------------- 2. data that crosses parts
def _cross_data():
    rng = np.random.default_rng(82)
    months = []
    months.append(np.full(40000, 0.0125))                                  # 0: eq spans every part
    # tie-free except for runs of 200 equal values across every multiple of 16,384 in sorted
    # order: rows in sorted order (the runs straddle the parts' row blocks too), then shuffled
    v = np.arange(40000, dtype=np.float64)
    for b in range(PART, 40000, PART):
        v[b - 100:b + 100] = b - 100
    months.append(v.copy())                                                # 1
    months.append(rng.permutation(v))                                      # 2
    h = rng.normal(size=34000)
    h[:PART] = np.nan
    months.append(h)                                                       # 3: a part with no eligible row
    one = np.full(34000, np.nan)
    one[33000] = -3.5
    months.append(one)                                                     # 4: one eligible row, in the last part
    months.append(RO.tie_heavy(20000, rng))                                # 5
    months.append(1.0 + rng.integers(0, 1 << 20, 20000) * 2.0 ** -52)      # 6: differ only in the low 32 bits
    seg_off = TR._seg([len(m) for m in months])
    return seg_off, np.concatenate(months)[None, :]


@pytest.fixture(scope="module")
def cross_data():
    return _cross_data()


@pytest.mark.parametrize("method,scale", RO.COMBOS)
def test_data_across_parts(E, cross_data, method, scale):
    seg_off, X = cross_data
    exp = RO.pandas_rank(X[0], seg_off, method, scale)
    _, got, gnv = TR._rank(E, TR._panel(E, X, seg_off), method=method, scale=scale)
    RO.assert_same_bits(got[0], exp, f"{method}/{scale}")
    assert np.array_equal(gnv[0], RO.pandas_nvalid(X[0], seg_off))
    assert len(np.unique(got[0][:40000])) == 1                      # one tie run over three parts
    assert gnv[0][3] == 34000 - PART and np.isnan(got[0][seg_off[3]:seg_off[3] + PART]).all()
    row = got[0][seg_off[4] + 33000]   # the lone eligible row: rank 1, pct 1.0, uniform 0.0
    assert gnv[0][4] == 1 and row == {"raw": 1.0, "pct": 1.0, "uniform": 0.0}[scale]


# ---------------------------------------------------------------- 3. universe mask
@pytest.mark.parametrize("min_level", [1, 2])
@pytest.mark.parametrize("method,scale", [("average", "pct"), ("min", "raw"), ("max", "uniform")])
def test_universe_mask(E, min_level, method, scale):
    rng = np.random.default_rng(83)
    seg_off = TR._seg([20000, 33000])
    n = int(seg_off[-1])
    X = np.stack([RO.tie_heavy(n, rng), rng.normal(size=n)])
    level = rng.integers(0, 3, n).astype(np.uint8)
    level[seg_off[1] + PART:seg_off[1] + 2 * PART] = 0   # the second month's middle part: no eligible row
    panel = TR._panel(E, X, seg_off)
    _, got, gnv = TR._rank(E, panel, method=method, scale=scale, level=torch.from_numpy(level).to(panel.device),
                           min_level=min_level)
    for i in range(2):
        RO.assert_same_bits(got[i], RO.pandas_rank(X[i], seg_off, method, scale, level, min_level), f"col {i}")
        assert np.array_equal(gnv[i], RO.pandas_nvalid(X[i], seg_off, level, min_level))
    assert np.isnan(got[:, seg_off[1] + PART:seg_off[1] + 2 * PART]).all() and (gnv > 0).all()


# ---------------------------------------------------------------- 4. locality
def test_long_month_alone(E, long_panel):
    """A long month gives the same bytes ranked alone and inside the length panel."""
    seg_off, X, _, _ = long_panel
    _, full, nfull = TR._rank(E, TR._panel(E, X, seg_off), method="max", scale="pct")
    for t in (LOCAL_MONTH, len(LONG_LENS) - 1):
        r0, r1 = int(seg_off[t]), int(seg_off[t + 1])
        _, sub, nsub = TR._rank(E, TR._panel(E, X[:, r0:r1], TR._seg([r1 - r0])), method="max", scale="pct")
        assert sub.tobytes() == np.ascontiguousarray(full[:, r0:r1]).tobytes()
        assert np.array_equal(nsub[:, 0], nfull[:, t])


def test_short_months_beside_a_long_one(E):
    """The short months of a panel that also holds one 20,000-row month (the long kernel, one
    part each) give the same bytes as a call on the short months alone (the short kernels)."""
    lens = [0, 1, 700, 8192, 8193, 16384, 20000, 3000, 16383]
    seg_off, X = TR._length_panel(lens, 84)
    _, full, nfull = TR._rank(E, TR._panel(E, X, seg_off), method="average", scale="uniform")
    r0, r1 = int(seg_off[6]), int(seg_off[7])
    keep = np.r_[0:r0, r1:int(seg_off[-1])]
    short_lens = lens[:6] + lens[7:]
    assert max(short_lens) <= PART
    _, sub, nsub = TR._rank(E, TR._panel(E, X[:, keep], TR._seg(short_lens)), method="average", scale="uniform")
    assert sub.tobytes() == np.ascontiguousarray(full[:, keep]).tobytes()
    assert np.array_equal(nsub, np.delete(nfull, 6, axis=1))


# ---------------------------------------------------------------- 5. pipeline
def test_pipeline_bit_identical(E):
    from fmcore import lewellen as LW, synth
    a = synth.synth_arrays(12, 20000, 29, nan_rate=0.03)
    mc = LW.table2_models()
    cols = list(dict.fromkeys(["retx"] + [c for xs in mc.values() for c in xs] + LW.FIG1_VARS))
    mk = lambda d: E.panel_from_arrays([d[c] for c in cols], cols, a["month"], me=a["me"], nyse=a["nyse"])
    panel = mk(a)
    assert panel.max_seg_len > PART
    got = LW.run_pipeline(panel, LW.PipelineConfig(rank="uniform", winsorize=False), model_cols=mc)
    exp = LW.run_pipeline(mk(TR._ranked_by_pandas(a, cols)), LW.PipelineConfig(winsorize=False), model_cols=mc)
    assert (exp.res.status.cpu().numpy() & 1).any()   # at least one month is fitted
    TR._bits_equal(got.res.rec, exp.res.rec, "records")
    TR._bits_equal(got.res.status, exp.res.status, "status")
    for k in ("mean", "se", "tstat", "nobs"):
        TR._bits_equal(getattr(got.summary, k), getattr(exp.summary, k), f"summary {k}")
        TR._bits_equal(getattr(got.pred_summary, k), getattr(exp.pred_summary, k), f"predictive summary {k}")


# ---------------------------------------------------------------- 6. drop-in
def test_drop_in(E):
    from fmdrop import calc_Lewellen_2014 as CL
    rng = np.random.default_rng(85)
    dates = pd.to_datetime(["2001-01-31", "2001-02-28", "2001-03-31"])
    lens = [300, 17000, 45]
    n = sum(lens)
    df = pd.DataFrame({"mthcaldt": np.repeat(dates, lens), "permno": np.concatenate([np.arange(k) for k in lens]),
                       "x": RO.tie_heavy(n, rng), "y": rng.normal(size=n)})
    df = df.sample(frac=1.0, random_state=5)   # shuffled, its own index labels
    for method, scale in (("average", "pct"), ("max", "raw")):
        got = CL.rank_transform(df, ["x", "y"], method=method, scale=scale)
        assert got.index.equals(df.index) and list(got.columns) == list(df.columns)
        for v in ("x", "y"):
            exp = df[v].groupby(df["mthcaldt"]).rank(method=method, pct=scale == "pct")
            RO.assert_same_bits(got[v].to_numpy(), exp.to_numpy(dtype=np.float64), f"{v} {method}/{scale}")
