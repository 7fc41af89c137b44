"""Host-side checks of the double-sorted portfolios (A21): the numpy restatement against months
worked by hand and against two single sorts, the binding's ABI, and every refusal that needs no
device (engine.double_sort, PipelineConfig, ShardedStep)."""
import ctypes
import dataclasses
import inspect

import numpy as np
import pytest
import torch

import dsort_oracle as DO
import port_oracle as PO


def test_oracle_two_by_two_month_by_hand():
    # medians: a 2.5, b 25; two rows per cell; weights 1 (first four rows) and 3
    a = np.array([1, 2, 3, 4, 1, 2, 3, 4], dtype=float)
    b = np.array([10, 40, 20, 30, 10, 40, 20, 30], dtype=float)
    r = np.array([1, 2, 3, 4, 3, 4, 5, 6], dtype=float)
    w = np.array([1, 1, 1, 1, 3, 3, 3, 3], dtype=float)
    o = DO.double_sort([0, 8], a, b, r, W=w, na=2, nb=2)
    assert o["status"].tolist() == [1] and o["bpa"].tolist() == [[2.5]] and o["bpb"].tolist() == [[[25.0], [25.0]]]
    assert o["cell"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3] and o["cnt"].tolist() == [[[2, 2], [2, 2]]]
    rb, ra = o["rec_b"][:, 0], o["rec_a"][:, 0]     # [slab, row, 4]
    assert rb[:2, :2, 0].tolist() == [[2, 3], [4, 5]] and rb[:2, :2, 2].tolist() == [[2.5, 3.5], [4.5, 5.5]]
    assert rb[:2, :2, 1].tolist() == [[10, 40], [20, 30]]                # mean b of the cells
    assert rb[:, 2, 0].tolist() == [1, 1, 1] and rb[2, :2, 0].tolist() == [3, 4]   # spreads; the a-neutral b portfolios
    assert rb[2, :, 1].tolist() == [15, 35, 20]
    assert ra[:2, :2, 0].tolist() == [[2, 4], [3, 5]] and ra[:2, :2, 1].tolist() == [[1, 3], [2, 4]]
    assert ra[:, 2, 0].tolist() == [2, 2, 2] and ra[2, :2, 0].tolist() == [2.5, 4.5] and ra[2, :, 2].tolist() == [3, 5, 2]
    # a NaN return leaves the count and the return sums, not the cell; a zero weight leaves the weighted sums
    r2, w2 = r.copy(), w.copy()
    r2[4], w2[1] = np.nan, 0.0
    o2 = DO.double_sort([0, 8], a, b, r2, W=w2, na=2, nb=2)
    assert o2["cell"].tolist() == o["cell"].tolist() and o2["cnt"].tolist() == [[[1, 2], [2, 2]]]
    assert o2["rec_b"][0, 0, 0, 0] == 1 and o2["rec_b"][0, 0, 1, 2] == 4   # cell (0, 1) value-weighted: row 5 alone
    # one row short of min_count: unsorted
    o3 = DO.double_sort([0, 8], a, b, r, na=2, nb=2, min_count=9)
    assert o3["status"].tolist() == [0] and (o3["cell"] == 255).all() and np.isnan(o3["rec_b"]).all()
    assert np.isnan(o3["bpa"]).all() and np.isnan(o3["bpb"]).all() and (o3["cnt"] == 0).all()


def test_oracle_conditional_breakpoints_differ_per_bin():
    a = np.arange(1, 9, dtype=float)
    b = np.array([1, 2, 3, 4, 10, 20, 30, 40], dtype=float)
    r = np.ones(8)
    ind = DO.double_sort([0, 8], a, b, r, na=2, nb=2)
    con = DO.double_sort([0, 8], a, b, r, na=2, nb=2, conditional=True)
    assert ind["bpa"].tolist() == con["bpa"].tolist() == [[4.5]]
    assert ind["bpb"].tolist() == [[[7.0], [7.0]]] and con["bpb"].tolist() == [[[2.5], [25.0]]]
    assert ind["cell"].tolist() == [0, 0, 0, 0, 3, 3, 3, 3] and con["cell"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert ind["cnt"].tolist() == [[[4, 0], [0, 4]]] and np.isnan(ind["rec_b"][0, 0, 1]).all()
    assert np.isnan(ind["rec_b"][2, 0, :, 0]).all()        # a neutral average over an empty cell is NaN
    assert con["rec_b"][2, 0, :, 1].tolist() == [(1.5 + 15) / 2, (3.5 + 35) / 2, (2 + 20) / 2]
    # an a-bin below min_count_bin: NaN breakpoints, its rows in no cell
    few = DO.double_sort([0, 8], a, b, r, na=2, nb=2, qa=(0.75,), conditional=True, min_count_bin=3)
    assert few["bpa"].tolist() == [[6.25]] and np.isnan(few["bpb"][0, 1]).all() and few["bpb"][0, 0].tolist() == [3.5]
    assert few["cell"].tolist() == [0, 0, 0, 1, 1, 1, 255, 255] and few["cnt"][0].tolist() == [[3, 3], [0, 0]]


def test_oracle_independent_equals_two_single_sorts():
    pan = DO.ragged_panel(seed=9, T=8)
    A, B = pan["A"], pan["B"]
    for kw in (dict(), dict(min_level=1, nyse_breakpoints=True)):
        o = DO.double_sort(pan["seg_off"], A, B, pan["R"], W=pan["W"], level=pan["level"], nyse=pan["nyse"], na=4, nb=3, **kw)
        pa = PO.portfolio_sort(pan["seg_off"], np.where(np.isfinite(B), A, np.nan), pan["R"], level=pan["level"],
                               nyse=pan["nyse"], nport=4, min_count=12, **kw)
        pb = PO.portfolio_sort(pan["seg_off"], np.where(np.isfinite(A), B, np.nan), pan["R"], level=pan["level"],
                               nyse=pan["nyse"], nport=3, min_count=12, **kw)
        assert o["status"].all() and np.array_equal(o["status"], pa["status"])
        assert np.array_equal(o["bpa"], pa["bp"]) and np.array_equal(o["bpb"][:, 0], pb["bp"])
        ok = o["cell"] != 255
        assert np.array_equal(ok, pa["port"] != 255) and np.array_equal(ok, pb["port"] != 255)
        assert np.array_equal(o["cell"][ok], pa["port"][ok] * 3 + pb["port"][ok])
        # the marginal counts are the single sorts' counts
        assert np.array_equal(o["cnt"].sum(axis=2), pa["cnt"]) and np.array_equal(o["cnt"].sum(axis=1), pb["cnt"])


def test_binding_has_double_sort():
    from fmcore import _lib as L
    assert "fm_portfolio_double_sort" in L.EXPORTED and L.FM_MAX_DSORT == 10
    lib = L.load()
    assert hasattr(lib, "fm_portfolio_double_sort")
    assert lib.fm_struct_size(b"fm_dsort_args") == ctypes.sizeof(L.DsortArgs) == 320
    assert L._STRUCTS["fm_dsort_args"] is L.DsortArgs
    assert L.DsortArgs.qa.size == L.DsortArgs.qb.size == 8 * (L.FM_MAX_DSORT - 1)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fm_hip.h")).read()
    assert "X(fm_dsort_args)" in header and "#define FM_MAX_DSORT 10" in header


def test_library_refuses_bad_arguments_without_a_device():
    from fmcore import _lib as L
    lib = L.load()

    def rc(**kw):
        a = L.DsortArgs(**dict(dict(na=5, nb=5, nseg=1, nsel=1, min_count=25, min_count_bin=5), **kw))
        for j in range(9):
            a.qa[j] = a.qb[j] = (j + 1) / 10
        return lib.fm_portfolio_double_sort(ctypes.byref(a), None), lib.fm_last_error().decode()

    assert lib.fm_portfolio_double_sort(None, None) == -1
    for kw, msg in ((dict(na=1), "na must be 2..10"), (dict(nb=11), "nb must be 2..10"), (dict(min_count=0), "min_count"),
                    (dict(conditional=1, min_count_bin=0), "min_count_bin"), (dict(min_level=256), "min_level"),
                    (dict(nyse_breakpoints=1), "nyse_breakpoints needs nyse"), (dict(nsel=-1), "nsel"),
                    (dict(a_sort_stride=-1), "stride"), (dict(nseg=-1), "bad sizes")):
        code, err = rc(**kw)
        assert code == -1 and msg in err, (kw, err)
    code, err = rc(max_seg_len=16385)
    assert code == -3 and "16385-row months exceed 16384" in err       # FM_ETOOBIG, before any launch
    assert rc(nseg=0)[0] == 0 and rc(nsel=0)[0] == 0                    # valid empty calls: no pointer is read
    code, err = rc()
    assert code == -1 and "null pointer" in err


def test_engine_double_sort_refusals():
    from fmcore import engine as E
    n = 40
    seg = torch.tensor([0, 20, 40], dtype=torch.int64)
    x = torch.arange(n, dtype=torch.float64)
    good = dict(seg_off=seg, a=x, b=x, ret=x)

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            E.double_sort(**dict(good, **kw))

    bad("a must be a float64", a=x.float())
    bad("b must be a float64", b=x.view(2, 4, 5))
    bad("same rows", b=x[:10])
    bad("holds 2 sorts, the other signal 3", a=x.repeat(2, 1), b=x.repeat(3, 1))
    bad("seg_off must be an int64", seg_off=seg.int())
    bad("ret must be", ret=x[:5])
    bad("weight must be", weight=x.float())
    bad("level must be", level=x)
    bad("nyse must be", nyse=torch.zeros(n, dtype=torch.int32))
    bad("na must be 2..10", na=1)
    bad("nb must be 2..10", nb=11)
    bad("qa must hold na - 1 = 4 levels", qa=(0.5,))
    bad("qb must be strictly ascending", qb=(0.2, 0.2, 0.6, 0.8))
    bad("qa must be strictly ascending", qa=(0.2, 0.4, 0.6, 1.0))
    bad("min_count and min_count_bin must be >= 1", min_count=0)
    bad("min_count and min_count_bin must be >= 1", min_count_bin=0)
    bad("min_level must be 0..255", min_level=256)
    bad("nyse_breakpoints needs nyse", nyse_breakpoints=True)
    with pytest.raises(ValueError, match="axis must be 'a' or 'b'"):
        E.sort_factors(None, axis="c")
    p = inspect.signature(E.double_sort).parameters
    assert list(p) == ["seg_off", "a", "b", "ret", "weight", "level", "nyse", "na", "nb", "qa", "qb", "conditional",
                       "min_level", "nyse_breakpoints", "min_count", "min_count_bin", "max_seg_len"]
    assert (p["na"].default, p["nb"].default, p["conditional"].default, p["min_count"].default) == (5, 5, False, None)
    assert list(inspect.signature(E.double_sort_panel).parameters)[:5] == ["panel", "a_col", "b_cols", "ret", "weight"]
    assert list(inspect.signature(E.sort_factors).parameters) == ["ds", "axis", "weighted"]
    assert isinstance(E.DoubleSort.by_b, property) and isinstance(E.DoubleSort.by_a, property)
    # the views on host tensors: shapes, and a status row per slab
    S, T, na, nb = 2, 3, 2, 3
    ds = E.DoubleSort(rec_b=torch.zeros(S, na + 1, T, nb + 1, 4, dtype=torch.float64),
                      rec_a=torch.zeros(S, nb + 1, T, na + 1, 4, dtype=torch.float64), cnt=None, cell=None, bpa=None, bpb=None,
                      status=torch.tensor([[1, 0, 1], [0, 1, 1]], dtype=torch.int32), na=na, nb=nb)
    ds.rec_b[1, 2, :, 3, 2] = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    assert tuple(ds.by_b.rec.shape) == (6, 3, 4, 4) and tuple(ds.by_a.rec.shape) == (8, 3, 3, 4)
    assert ds.by_b.status.tolist() == [[1, 0, 1]] * 3 + [[0, 1, 1]] * 3 and ds.by_b.status.is_contiguous()
    assert ds.by_a.status.shape == (8, 3) and ds.by_a.status.dtype == torch.int32
    assert E.sort_factors(ds, "b").tolist() == [[0.0, 1.0], [0.0, 2.0], [0.0, 3.0]]


def test_pipeline_config_and_sharded_step():
    from fmcore import lewellen as LW
    from fmcore import step as ST
    f = {x.name: x for x in dataclasses.fields(LW.PipelineConfig)}
    for name, default in (("double_sort", None), ("double_sort_shape", (5, 5)), ("double_sort_conditional", False)):
        assert f[name].kw_only and f[name].default == default
    res = {x.name: x for x in dataclasses.fields(LW.PipelineResult)}
    assert res["double_sort"].default is None and res["double_sort_summary"].default is None

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            LW.run_pipeline(None, LW.PipelineConfig(**kw))

    bad("double_sort needs portfolios", double_sort="log_size")
    bad("double_sort must name a panel column", double_sort=3, portfolios=10)
    bad("double_sort_shape must be", double_sort="log_size", portfolios=10, double_sort_shape=(5, 11))
    bad("double_sort_shape must be", double_sort="log_size", portfolios=10, double_sort_shape=(5,))
    bad("double_sort_shape must be", double_sort="log_size", portfolios=10, double_sort_shape=(2.5, 5))
    bad("double_sort excludes horizon=3", double_sort="log_size", portfolios=10, horizon=3, lag=3)
    bad("double_sort excludes extrapolate", double_sort="log_size", portfolios=10, extrapolate=6)
    bad("double_sort excludes portfolio_hold", double_sort="log_size", portfolios=10, portfolio_hold=3)
    with pytest.raises(ValueError, match="ShardedStep: cfg.double_sort must be None"):
        ST.ShardedStep(None, LW.PipelineConfig(double_sort="log_size", portfolios=10), None)


def test_drop_in_signatures():
    from fmdrop import bind
    from fmdrop import calc_Lewellen_2014 as CL
    p = inspect.signature(CL.double_sorted_portfolios).parameters
    assert list(p) == ["df", "a", "b", "return_col", "weight_col", "na", "nb", "breakpoints_a", "breakpoints_b",
                       "conditional", "universe", "nyse_breakpoints", "date_col", "nw_lags"]
    assert (p["return_col"].default, p["na"].default, p["nb"].default, p["nw_lags"].default) == ("retx", 5, 5, 4)
    p = inspect.signature(CL.build_table_double_sort).parameters
    assert list(p) == ["crsp_comp", "by", "variables_dict", "shape", "cfg"] and p["by"].default == "log_size"
    p = inspect.signature(CL.characteristic_factors).parameters
    assert list(p)[:7] == ["df", "char_cols", "size_col", "weight_col", "breakpoints_size", "breakpoints_char",
                           "nyse_breakpoints"]
    assert (p["size_col"].default, p["weight_col"].default, p["breakpoints_size"].default,
            p["breakpoints_char"].default, p["nyse_breakpoints"].default) == ("me", "me", (0.5,), (0.3, 0.7), True)
    src = inspect.getsource(bind)     # extensions, like Tables 3 to 5: not bound into the reference's namespace
    for name in ("double_sorted_portfolios", "build_table_double_sort", "characteristic_factors"):
        assert name not in src
    # the frame builder on hand-made records: labels, margins and the undefined corners
    na, nb, T = 2, 2, 2
    rb = np.arange((na + 1) * T * (nb + 1) * 4, dtype=float).reshape(na + 1, T, nb + 1, 4)
    ra = 1000 + np.arange((nb + 1) * T * (na + 1) * 4, dtype=float).reshape(nb + 1, T, na + 1, 4)
    cnt = np.arange(T * na * nb).reshape(T, na, nb) + 1
    z = lambda n1, n2: [np.zeros((n1, n2, 4))] * 3
    monthly, summary = CL._dsort_frames(np.array([1, 1]), rb, ra, cnt, z(na + 1, nb + 1), z(nb + 1, na + 1), np.array([7, 8]), na, nb)
    assert list(monthly.columns) == ["ew_ret", "vw_ret", "ew_a", "ew_b", "n"] and len(monthly) == T * 16
    assert monthly.index.names == ["mthcaldt", "a_bin", "b_bin"] and len(summary) == 16
    assert monthly.loc[(8, 1, 0), ["ew_ret", "ew_b", "vw_ret"]].tolist() == rb[1, 1, 0, :3].tolist()
    assert monthly.loc[(8, 1, 0), "ew_a"] == ra[0, 1, 1, 1]
    assert monthly.loc[(7, "avg", "H-L"), "vw_ret"] == rb[na, 0, nb, 2] and monthly.loc[(7, "H-L", "avg"), "ew_ret"] == ra[nb, 0, na, 0]
    assert monthly.loc[(7, 0, "H-L"), "n"] == cnt[0, 0, 0] + cnt[0, 0, 1] and monthly.loc[(7, "avg", 1), "n"] == cnt[0, :, 1].sum()
    assert np.isnan(monthly.loc[(7, "H-L", "H-L"), "ew_ret"]) and np.isnan(monthly.loc[(7, "avg", "avg"), "vw_ret"])
