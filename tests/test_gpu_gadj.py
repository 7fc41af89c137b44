"""GPU tests of the within-group adjustment (fm_group_adjust, engine.group_adjust_columns,
engine.group_adjust, PipelineConfig(group_adjust=...), the drop-in's group_adjust and group_col=;
build-defined A20) against the numpy restatement tests/gadj_oracle.py.

Integer-valued fixture: every sum is exact in any order, so dst, gmean and gcount are the oracle's
bits.  Real values, DEMEAN and MEAN (U = 2^-53, n and A = sum|x| / n of the row's group, ref the
oracle's value): |got - ref| <= 1.01 U ((n + 2) A + 2 |ref|), the forward bound of an n-term sum in
any order plus the division and the subtraction on either side (tests/test_gadj_host.py: plain
float64 sums in three orders stay below half of it).  ZSCORE and gsd: fmtol.assert_series_close at
RTOL = 1e-9, the project's contract.

The widest call has 17 columns: the kernel bins fm_group_adjust_batch(ngroups) columns per workgroup
-- 8 up to 128 groups, 4 at 256 -- so it runs 3 (6 + 6 + 5 columns) and 5 batches there."""
import dataclasses
import gc

import numpy as np
import pytest
import torch

import fmtol
import gadj_oracle as GO

pytestmark = pytest.mark.gpu

GUARD = 64
SENT_F, SENT_I = 1e300, -77
TABLES = ("gcount", "gmean", "gsd")


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks(E):
    yield
    E.LAST_LAUNCH.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _dev(E, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(E.require_device())


def _raw(E, seg_off, X, group, G, mode, min_count=1, level=None, min_level=0):
    """fm_group_adjust through the binding on the months ``seg_off`` of the [C, n] block ``X``: every
    output pre-filled with a sentinel inside a buffer with GUARD more elements either side, which must
    come back untouched, as must the dst rows outside the call's months; every other element must have
    been written -> host dict."""
    L = E.L
    X = np.ascontiguousarray(X, dtype=np.float64)
    C, n = X.shape
    T = len(seg_off) - 1
    ins = [_dev(E, x) for x in (np.asarray(seg_off, dtype=np.int64), X, np.asarray(group, dtype=np.int32), level)]
    shapes = dict(dst=(C, n), gcount=(C, T, G), gmean=(C, T, G))
    if mode == "zscore":
        shapes["gsd"] = (C, T, G)
    bufs = {}
    for name, sh in shapes.items():
        i32 = name == "gcount"
        bufs[name] = torch.full((int(np.prod(sh)) + 2 * GUARD,), SENT_I if i32 else SENT_F,
                                dtype=torch.int32 if i32 else torch.float64, device=ins[0].device)
    ptr = {name: b[GUARD:].data_ptr() for name, b in bufs.items()}
    a = L.GroupAdjArgs(src=ins[1].data_ptr(), src_stride=n, dst=ptr["dst"], dst_stride=n, seg_off=ins[0].data_ptr(),
                       group=ins[2].data_ptr(), level=None if level is None else ins[3].data_ptr(), nrows=n, ncols=C,
                       nseg=T, ngroups=G, mode=E.GADJ_MODES[mode], min_count=min_count, min_level=min_level,
                       gcount=ptr["gcount"], gmean=ptr["gmean"], gsd=ptr.get("gsd"))
    L.call("fm_group_adjust", L.C.byref(a), E._stream())
    torch.cuda.synchronize()
    out = {}
    for name, sh in shapes.items():
        h = bufs[name].cpu().numpy()
        sent = SENT_I if name == "gcount" else SENT_F
        assert np.all(h[:GUARD] == sent) and np.all(h[-GUARD:] == sent), f"{name}: a guard element was written"
        body = h[GUARD:-GUARD].reshape(sh).copy()
        if name == "dst":
            r0, r1 = int(seg_off[0]), int(seg_off[-1])
            assert np.all(body[:, :r0] == sent) and np.all(body[:, r1:] == sent), "dst: a row outside the months was written"
            assert not np.any(body[:, r0:r1] == sent), "dst: a row was not written"
        else:
            assert not np.any(body == sent), f"{name}: an element was not written"
        out[name] = body
    return out


def _same_tables(got, exp, what, C=slice(None)):
    assert got["gcount"].dtype == np.int32 and np.array_equal(got["gcount"], exp["gcount"][C]), (what, "gcount")
    GO.assert_same_bits(got["gmean"], exp["gmean"][C], f"{what} gmean")


# ---------------------------------------------------------------- 1. to the bit
@pytest.mark.parametrize("G", GO.NGROUPS)
def test_integer_fixture_to_the_bit(E, G):
    X, g, exp = GO.int_values(), GO.codes(G), GO.int_expected(G)
    B = E.L.load().fm_group_adjust_batch(G)
    assert B == (4 if G == 256 else 8) and max(GO.NCOLS) > 2 * B   # the widest call: three batches or more
    for C in GO.NCOLS:
        for mode in ("demean", "mean"):
            got = _raw(E, GO.SEG_OFF, X[:C], g, G, mode)
            GO.assert_same_bits(got["dst"], exp[mode][:C], f"G={G} C={C} {mode}")
            _same_tables(got, exp, f"G={G} C={C} {mode}", slice(0, C))
    # what the fixture is there for (tests/test_gadj_host.py checks the oracle's side of it)
    assert np.isnan(got["dst"][GO.NAN_COL]).all() and got["gcount"][GO.NAN_COL].sum() == 0
    assert np.isnan(got["gmean"][GO.INF_COL, -1, 0])
    if G >= 2:
        assert got["gmean"][GO.INF_COL, -1, 1] == np.inf
        assert got["gcount"][0, 8, G - 1] >= 1      # the group of the 1000-row month's last tile alone
    # the z-score of the same call: the counts again to the bit, the values at the project's tolerance
    got = _raw(E, GO.SEG_OFF, X[:3], g, G, "zscore")
    _same_tables(got, exp, f"G={G} zscore", slice(0, 3))
    fmtol.assert_series_close(got["dst"], exp["zscore"][:3], f"G={G} zscore")
    fmtol.assert_series_close(got["gsd"], exp["gsd"][:3], f"G={G} gsd")


# ---------------------------------------------------------------- 2. real values
def test_real_values_within_the_bound(E):
    X, g, G, exp = GO.real_values(), GO.codes(GO.REAL_G), GO.REAL_G, GO.real_expected()
    for mode in ("demean", "mean"):
        got = _raw(E, GO.SEG_OFF, X, g, G, mode)
        assert np.array_equal(got["gcount"], exp["gcount"])
        GO.assert_within(got["dst"], exp[mode], GO.sum_bound(GO.SEG_OFF, g, G, exp, exp[mode]), f"real {mode}")
        GO.assert_within(got["gmean"], exp["gmean"], GO.table_bound(exp), f"real {mode} gmean")
    got = _raw(E, GO.SEG_OFF, X, g, G, "zscore")
    assert np.array_equal(got["gcount"], exp["gcount"])
    fmtol.assert_series_close(got["dst"], exp["zscore"], "real zscore")
    fmtol.assert_series_close(got["gsd"], exp["gsd"], "real gsd")
    # groups of one row and the constant group are NaN (NaN positions equal, checked above), sd NaN / 0
    rows = GO.OFF_1000 + np.flatnonzero(g[GO.OFF_1000:GO.OFF_5000] == GO.CONST_GROUP)
    assert np.isnan(got["dst"][0, rows]).all() and got["gsd"][0, 8, GO.CONST_GROUP] == 0.0
    assert np.isnan(got["gsd"][exp["gcount"] == 1]).all() and (exp["gcount"] == 1).sum() >= 10


# ---------------------------------------------------------------- 3. locality
def test_same_bits_from_any_call(E):
    X, G = GO.real_values(), GO.REAL_G
    g = GO.codes(G, foreign=256)      # "no group" at 49 groups and at 256
    for mode in GO.MODES:
        names = ("dst", "gcount", "gmean") + (("gsd",) if mode == "zscore" else ())
        full = _raw(E, GO.SEG_OFF, X, g, G, mode)
        again = _raw(E, GO.SEG_OFF, X, g, G, mode)
        for name in names:
            assert again[name].tobytes() == full[name].tobytes(), (mode, "repeat", name)
        part = _raw(E, GO.SEG_OFF[3:8], X, g, G, mode)          # months [3, 7)
        r0, r1 = int(GO.SEG_OFF[3]), int(GO.SEG_OFF[7])
        assert part["dst"][:, r0:r1].tobytes() == full["dst"][:, r0:r1].tobytes(), (mode, "months")
        for name in names[1:]:
            assert part[name].tobytes() == full[name][:, 3:7].tobytes(), (mode, "months", name)
        two = _raw(E, GO.SEG_OFF, X[[0, 2]], g, G, mode)        # columns {0, 2} alone
        for name in names:
            assert two[name].tobytes() == full[name][[0, 2]].tobytes(), (mode, "columns", name)
        wide = _raw(E, GO.SEG_OFF, X, g, 256, mode)             # the same codes among 256 groups (another batch size)
        assert wide["dst"].tobytes() == full["dst"].tobytes(), (mode, "ngroups")
        for name in names[1:]:
            assert wide[name][:, :, :G].tobytes() == full[name].tobytes(), (mode, "ngroups", name)
        assert wide["gcount"][:, :, G:].sum() == 0 and np.isnan(wide["gmean"][:, :, G:]).all()


# ---------------------------------------------------------------- 4. universe and min_count
@pytest.mark.parametrize("min_count", [0, 1, 5, 10 ** 6])
def test_level_and_min_count(E, min_count):
    X, g, lv = GO.int_values()[:3], GO.codes(49), GO.levels()
    for leveled in (False, True):
        exp = GO.int_expected(49, min_count, leveled, 3)
        for mode in ("demean", "mean"):
            got = _raw(E, GO.SEG_OFF, X, g, 49, mode, min_count=min_count, level=lv if leveled else None, min_level=1)
            GO.assert_same_bits(got["dst"], exp[mode][:3], f"min_count={min_count} level={leveled} {mode}")
            _same_tables(got, exp, f"min_count={min_count} level={leveled} {mode}", slice(0, 3))
        if leveled:
            assert np.isnan(got["dst"][:, lv < 1]).all()
    if min_count == 10 ** 6:
        assert np.isnan(got["dst"]).all() and np.isnan(got["gmean"]).all() and got["gcount"].sum() > 0
    if min_count == 5:
        small = (exp["gcount"] > 0) & (exp["gcount"] < 5)
        assert small.sum() >= 10 and np.isnan(got["gmean"][small[:3]]).all()
    if min_count == 0:
        GO.assert_same_bits(got["dst"], GO.int_expected(49, 1, True, 3)["mean"], "min_count 0 is 1")


# ---------------------------------------------------------------- 5. the engine
@pytest.fixture(scope="module")
def small(E):
    from fmcore import synth
    a = synth.synth_arrays(12, 100, 3, nan_rate=0.03, present_rate=0.9)
    names = ["retx", "log_size", "log_bm", "return_12_2"]
    group = ((a["permno"] * 7) % 13 - 1).astype(np.int64)        # -1: no group; 12 groups
    panel = E.panel_from_arrays([a[c] for c in names], names, a["month"], me=a["me"], nyse=a["nyse"], ids=a["permno"],
                                group=group)
    X = np.stack([a[c] for c in names])[:, panel.order]
    return dict(panel=panel, X=X, group=group[panel.order], names=names)


def test_engine_group_adjust(E, small):
    panel, X, g = small["panel"], small["X"], small["group"]
    assert panel.ngroups == 12 and panel.group.dtype == torch.int32
    assert np.array_equal(panel.group.cpu().numpy(), g)
    E.month_links(panel, 1)
    exp = GO.group_adjust(panel.seg_off_h, X, g, 12)
    res = E.group_adjust(panel, cols=["log_bm", "log_size"], mode="demean", stats=True)
    got = res.cols.cpu().numpy()
    for i in (0, 3):                                             # untouched columns are copies
        assert got[i].tobytes() == X[i].tobytes() and res.cols[i].data_ptr() != panel.cols[i].data_ptr()
    for i in (1, 2):
        GO.assert_within(got[i:i + 1], exp["demean"][i:i + 1],
                         GO.sum_bound(panel.seg_off_h, g, 12, exp, exp["demean"])[i:i + 1], f"engine column {i}")
    st = res.group_stats
    assert st.sd is None and tuple(st.mean.shape) == (2, panel.nseg, 12) and st.count.dtype == torch.int32
    assert np.array_equal(st.count.cpu().numpy(), exp["gcount"][[2, 1]])     # in the order of ``cols``
    for name in ("seg_off", "me", "nyse", "group", "ids"):
        assert getattr(res, name) is getattr(panel, name), name
    assert res.ngroups == 12 and res.order is panel.order and res.month_index is panel.month_index
    assert res.months is panel.months and res.names == panel.names and res.names is not panel.names
    assert res.__dict__["_links"] is panel.__dict__["_links"]
    # all columns, z-scores, with the sd table; the default has no group_stats
    z = E.group_adjust(panel, mode="zscore", stats=True)
    fmtol.assert_series_close(z.cols.cpu().numpy(), exp["zscore"], "engine zscore")
    fmtol.assert_series_close(z.group_stats.sd.cpu().numpy(), exp["gsd"], "engine gsd")
    assert not hasattr(E.group_adjust(panel, cols=[0]), "group_stats")
    # the panels made from this one keep the codes
    r = E.rank_transform(res, cols=["log_bm"])
    h = E.horizon_panel(panel, 3)
    assert r.group is panel.group and r.ngroups == 12 and h.group is panel.group and h.ngroups == 12
    # plain tensors: the same launch
    m = E.group_adjust_columns(panel.seg_off, panel.cols[1:3], panel.group, 12, mode="demean")
    assert m.cpu().numpy().tobytes() == got[1:3].tobytes()
    # out: the caller's block, validated
    out = torch.full_like(panel.cols, 5.0)
    assert E.group_adjust(panel, cols=[2], out=out).cols is out and out[2].cpu().numpy().tobytes() == got[2].tobytes()
    for bad in (panel.cols, out[:, :-1], out.to(torch.float32), out[:2]):
        with pytest.raises(ValueError, match="group_adjust: out must"):
            E.group_adjust(panel, out=bad)
    with pytest.raises(ValueError, match="cols must be distinct columns"):
        E.group_adjust(panel, cols=[1, 1])
    with pytest.raises(ValueError, match="min_count must be an integer >= 0"):
        E.group_adjust(panel, min_count=-1)
    with pytest.raises(E.L.FMError, match="dst must not overlap src"):
        E.group_adjust_columns(panel.seg_off, panel.cols[0:2], panel.group, 12, out=panel.cols[1:3])
    with pytest.raises(ValueError, match="carries no group codes"):
        E.group_adjust(dataclasses.replace(panel, group=None, ngroups=0))


# ---------------------------------------------------------------- 6. the pipeline
PIPE = dict(T=90, N=300, seed=31, window=24, min_periods=12, nport=10, G=12)


@pytest.fixture(scope="module")
def pipe(E):
    import pipe_port_oracle as PPO
    from fmcore import synth
    a = synth.synth_arrays(PIPE["T"], PIPE["N"], PIPE["seed"], nan_rate=0.02, present_rate=0.9)
    names, mc = PPO.pipeline_columns()
    of_firm = np.random.default_rng(9).integers(-1, PIPE["G"], PIPE["N"])       # a firm's industry; -1: none
    panel = E.panel_from_arrays([a[c] for c in names], names, a["month"], me=a["me"], nyse=a["nyse"], ids=a["permno"],
                                group=of_firm[a["firm"]], ngroups=PIPE["G"])
    return dict(panel=panel, mc=mc, kw=dict(window=PIPE["window"], min_periods=PIPE["min_periods"],
                                            portfolios=PIPE["nport"]))


def _same_run(a, b, what):
    GO.assert_same_bits(a.res.rec.cpu().numpy(), b.res.rec.cpu().numpy(), f"{what} coefficients")
    assert np.array_equal(a.res.status.cpu().numpy(), b.res.status.cpu().numpy()), what
    for s, t in ((a.summary, b.summary), (a.pred_summary, b.pred_summary), (a.portfolio_summary, b.portfolio_summary)):
        for x in ("mean", "se", "tstat", "nobs"):
            GO.assert_same_bits(getattr(s, x).cpu().numpy(), getattr(t, x).cpu().numpy(), f"{what} summary {x}")
    GO.assert_same_bits(a.portfolios.rec.cpu().numpy(), b.portfolios.rec.cpu().numpy(), f"{what} portfolio records")
    for x in ("port", "cnt", "status"):
        assert np.array_equal(getattr(a.portfolios, x).cpu().numpy(), getattr(b.portfolios, x).cpu().numpy()), (what, x)


@pytest.mark.parametrize("extra", [dict(), dict(rank="uniform"), dict(group_adjust_cols=["log_bm", "return_12_2"])],
                         ids=["demean", "ranked", "two-columns"])
def test_pipeline_is_the_adjustment_beforehand(E, pipe, extra):
    from fmcore import lewellen as LW
    panel, mc, kw = pipe["panel"], pipe["mc"], pipe["kw"]
    on = LW.run_pipeline(panel, LW.PipelineConfig(group_adjust="demean", **kw, **extra), model_cols=mc)
    cols = extra.get("group_adjust_cols") or [c for c in panel.names if c != "retx"]
    assert on.group_adjusted == [c for c in panel.names if c in cols] and "retx" not in on.group_adjusted
    before = E.group_adjust(panel, cols=on.group_adjusted, mode="demean", stats=True)
    rest = {k: v for k, v in extra.items() if k != "group_adjust_cols"}
    off = LW.run_pipeline(before, LW.PipelineConfig(**kw, **rest), model_cols=mc)
    plain = LW.run_pipeline(panel, LW.PipelineConfig(**kw, **rest), model_cols=mc)
    torch.cuda.synchronize()
    _same_run(on, off, "adjusted in the pipeline / beforehand")
    assert off.group_stats is None and off.group_adjusted is None
    st = on.group_stats
    assert tuple(st.mean.shape) == (len(on.group_adjusted), panel.nseg, PIPE["G"]) and st.sd is None
    assert st.mean.cpu().numpy().tobytes() == before.group_stats.mean.cpu().numpy().tobytes()
    assert np.array_equal(st.count.cpu().numpy(), before.group_stats.count.cpu().numpy())
    # the run means something (fitted months, sorted months) and differs from the unadjusted one
    assert (on.res.status.cpu().numpy() & 1).sum() > 0.9 * on.res.status.numel()
    assert on.portfolios.status.cpu().numpy().sum() > 0
    assert on.res.rec.cpu().numpy().tobytes() != plain.res.rec.cpu().numpy().tobytes()


def test_pipeline_refuses_a_panel_without_groups(E, pipe):
    from fmcore import lewellen as LW
    bare = dataclasses.replace(pipe["panel"], group=None, ngroups=0)
    with pytest.raises(ValueError, match="group_adjust needs a panel with group codes"):
        LW.run_pipeline(bare, LW.PipelineConfig(group_adjust="demean"))


# ---------------------------------------------------------------- 7. the drop-in and the ingest
@pytest.fixture(scope="module")
def frame():
    from fmcore import synth
    import pandas as pd
    df = synth.synth_frame(40, 300, 17, nan_rate=0.03, present_rate=0.9, shuffle=True)
    rng = np.random.default_rng(3)
    labels = np.array(["autos", "banks", "chips", "drugs", "oil", "rail", "steel", None], dtype=object)
    firm = pd.factorize(df["permno"])[0]
    df["ind"] = labels[rng.integers(0, len(labels), firm.max() + 1)][firm]      # a firm's industry; None: unknown
    return df


def test_drop_in_group_adjust(E, frame):
    from fmdrop import calc_Lewellen_2014 as CL
    df, cols = frame, ["log_bm", "return_12_2"]
    order = np.lexsort((df["permno"].to_numpy(), df["mthcaldt"].to_numpy()))
    d = df.iloc[order]
    _, counts = np.unique(d["mthcaldt"].to_numpy(), return_counts=True)
    so = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    codes, uniq = E.group_codes(d["ind"])
    assert list(uniq) == ["autos", "banks", "chips", "drugs", "oil", "rail", "steel"] and (codes == -1).sum() > 100
    X = d[cols].to_numpy().T
    exp = GO.group_adjust(so, X, codes, 7)
    for mode in ("demean", "mean", "zscore"):
        out = CL.group_adjust(df, cols, group_col="ind", mode=mode)
        assert out.index.equals(df.index) and list(out.columns) == list(df.columns)
        assert out["permno"].equals(df["permno"]) and out["retx"].equals(df["retx"])      # the caller's row order
        got = out[cols].to_numpy()[order].T
        alt = GO.pandas_adjust(so, X, codes, 7, mode)
        if mode == "zscore":
            fmtol.assert_series_close(got, alt, "drop-in zscore")
        else:
            bound = GO.sum_bound(so, codes, 7, exp, exp[mode])
            GO.assert_within(got, alt, bound, f"drop-in {mode} against pandas")
            GO.assert_within(got, exp[mode], bound, f"drop-in {mode}")
    assert np.isnan(out.loc[df["ind"].isna(), cols].to_numpy()).all()
    big = CL.group_adjust(df, cols, group_col="ind", min_count=10 ** 6)
    assert np.isnan(big[cols].to_numpy()).all()
    with pytest.raises(ValueError, match="mode must be one of"):
        CL.group_adjust(df, cols, group_col="ind", mode="median")


def test_drop_in_pipeline_takes_group_col(E, frame):
    from fmdrop import calc_Lewellen_2014 as CL
    kw = dict(window=12, min_periods=6)
    on = CL.lewellen_pipeline(frame, group_col="ind", group_adjust="demean", **kw)
    off = CL.lewellen_pipeline(frame, **kw)
    also = CL.lewellen_pipeline(frame, group_col="ind", **kw)          # the codes alone change nothing
    torch.cuda.synchronize()
    assert on.group_adjusted is not None and "retx" not in on.group_adjusted and len(on.group_adjusted) == 14
    assert tuple(on.group_stats.count.shape) == (14, 40, 7)
    assert (on.res.status.cpu().numpy() & 1).sum() > 0
    assert on.res.rec.cpu().numpy().tobytes() != off.res.rec.cpu().numpy().tobytes()
    GO.assert_same_bits(also.res.rec.cpu().numpy(), off.res.rec.cpu().numpy(), "group_col without group_adjust")
    t5 = CL.build_table_5(frame, nport=5, group_col="ind", group_adjust="demean", **kw)
    assert len(t5) == 9
    with pytest.raises(ValueError, match="group_adjust needs a panel with group codes"):
        CL.lewellen_pipeline(frame, group_adjust="demean", **kw)


def test_arrow_ingest_carries_the_codes(E, frame):
    import pyarrow as pa
    from fmcore import ingest as IN
    cols = ["retx", "log_bm"]
    tab = pa.Table.from_pandas(frame[["mthcaldt", "ind", "permno"] + cols], preserve_index=False)
    p = IN.panel_from_arrow(tab, cols, group_col="ind")
    q = E.panel_from_arrays([frame[c].to_numpy() for c in cols], cols, frame["mthcaldt"].values,
                            group=E.group_codes(frame["ind"])[0], ngroups=7)
    assert p.ngroups == 7 and list(p.group_labels) == ["autos", "banks", "chips", "drugs", "oil", "rail", "steel"]
    assert np.array_equal(p.group.cpu().numpy(), q.group.cpu().numpy()) and (p.group == -1).sum().item() > 100
    a, b = E.group_adjust(p, cols=["log_bm"]), E.group_adjust(q, cols=["log_bm"])
    assert a.cols.cpu().numpy().tobytes() == b.cols.cpu().numpy().tobytes()
    by_permno = pa.Table.from_pandas(frame[["mthcaldt", "permno"] + cols], preserve_index=False)
    assert IN.panel_from_arrow(by_permno, cols).group is None
    with pytest.raises(ValueError, match="panel_from_arrow: ngroups must be 1..256"):
        IN.panel_from_arrow(by_permno, cols, group_col="permno")
