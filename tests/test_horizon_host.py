"""Host-side checks of the multi-month return horizons (A16): the numpy restatement against an
independent pandas formulation, the calendar month numbers, the argument checks of fm_month_links
and fm_horizon_return (each returns before any launch) and the PipelineConfig rules."""
import ctypes
import dataclasses

import numpy as np
import pytest

import horizon_oracle as HO


def _synth_panel(seed=5):
    """synth_arrays(40, 300, seed, present_rate=0.9): ids, seg_off, month numbers, returns."""
    from fmcore import synth
    a = synth.synth_arrays(40, 300, seed, present_rate=0.9)
    months = np.unique(a["month"])
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(a["month"] - months[0], minlength=len(months)))]).astype(np.int64)
    return a, seg_off, months.astype(np.int32)


@pytest.mark.parametrize("h", [1, 3, 12])
def test_oracle_matches_pandas_formulation(h):
    a, seg_off, mi = _synth_panel()
    link = HO.month_links(a["permno"], seg_off, mi, 1)
    HO.assert_same_bits(HO.horizon_return(a["retx"], link, seg_off, h),
                        HO.pandas_horizon(a["permno"], a["month"], a["retx"], h), f"h={h}")


def test_oracle_matches_pandas_on_the_edge_panel():
    """Gaps in the calendar, an empty month, NaN / inf / -1 / -0.0 returns."""
    p = HO.edge_panel()
    assert HO.count_bad(p["ids"], p["seg_off"]) == 0
    month = np.repeat(p["month_index"].astype(np.int64), np.diff(p["seg_off"]))
    fwd = HO.month_links(p["ids"], p["seg_off"], p["month_index"], 1)
    bwd = HO.month_links(p["ids"], p["seg_off"], p["month_index"], -1)
    # no link across the two gaps, links across every other boundary, and -1 inverts +1
    seg = np.searchsorted(p["seg_off"], np.arange(len(fwd)), side="right") - 1
    for s, gap in HO.EDGE_GAPS.items():
        assert gap > 1 and np.all(fwd[seg == s - 1] == -1) and np.all(bwd[seg == s] == -1)
    assert (fwd[seg == 12] >= 0).sum() > 4000
    rows = np.nonzero(fwd >= 0)[0]
    there = p["seg_off"][seg[rows] + 1] + fwd[rows]
    assert np.array_equal(p["seg_off"][seg[rows]] + bwd[there], rows) and (bwd >= 0).sum() == len(rows)
    # ids that differ only above bit 32 are different firms
    x = np.nonzero(p["ids"] == HO.ID_X)[0]
    assert seg[x[0]] == HO.SEG_X and fwd[x[0]] == -1
    for h in (2, 3, 6):
        HO.assert_same_bits(HO.horizon_return(p["ret"], fwd, p["seg_off"], h),
                            HO.pandas_horizon(p["ids"], month, p["ret"], h), f"h={h}")


def test_pipeline_fixture_keeps_enough_three_month_returns():
    """The input condition of the pipeline test (tests/test_gpu_horizon.py): at seed 5 each of the
    first 38 months keeps at least 182 rows with a valid 3-month return, before predictor NaNs."""
    a, seg_off, mi = _synth_panel(5)
    r3 = HO.horizon_return(a["retx"], HO.month_links(a["permno"], seg_off, mi, 1), seg_off, 3)
    per_month = np.add.reduceat(np.isfinite(r3).astype(np.int64), seg_off[:-1])
    assert per_month[:38].min() >= 182 and np.all(per_month[38:] == 0)


def test_month_index():
    from fmcore import engine as E
    d = np.array(["1999-11-30", "1999-12-31", "2000-02-29", "2000-03-15"], dtype="datetime64[D]")
    assert E.month_index(d).tolist() == [1999 * 12 + 10, 1999 * 12 + 11, 2000 * 12 + 1, 2000 * 12 + 2]
    assert E.month_index(d.astype("datetime64[ns]")).dtype == np.int32
    import pandas as pd
    assert E.month_index(pd.DatetimeIndex(d)).tolist() == E.month_index(d).tolist()
    assert E.month_index(np.array([3, 4, 7], dtype=np.int64)).tolist() == [3, 4, 7]
    assert E.month_index(np.array([], dtype=np.int64)).shape == (0,)
    for bad, text in ((np.array(["a", "b"]), "datetime64 or integers"),
                      (np.array([1.0, 2.0]), "datetime64 or integers"),
                      (np.array(["2000-01-03", "2000-01-31"], dtype="datetime64[D]"), "same calendar month"),
                      (np.array([5, 5]), "same calendar month"),
                      (np.array([6, 5]), "do not ascend"),
                      (np.array(["2000-01-03", "NaT"], dtype="datetime64[D]"), "NaT"),
                      (np.array([1, 1 << 40]), "32 bits")):
        with pytest.raises(ValueError, match=text):
            E.month_index(bad)


def test_binding_has_the_horizon_entry_points():
    from fmcore import _lib as L
    lib = L.load()
    for f in ("fm_month_links", "fm_horizon_return"):
        assert f in L.EXPORTED and hasattr(lib, f)
    assert lib.fm_struct_size(b"fm_links_args") == ctypes.sizeof(L.LinksArgs)
    assert lib.fm_struct_size(b"fm_horizon_args") == ctypes.sizeof(L.HorizonArgs)
    assert L.FM_MAX_HORIZON == 60


FAKE = 4096   # never dereferenced: every call below returns before a launch


def _links_args(L, **kw):
    a = L.LinksArgs(ids=FAKE, seg_off=FAKE, month_index=FAKE, nrows=100, nseg=3, step=1, link=FAKE, bad=FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _horizon_args(L, **kw):
    a = L.HorizonArgs(ret=FAKE, link=FAKE + (1 << 20), seg_off=FAKE, nrows=100, nseg=3, horizon=3, out=FAKE + (2 << 20))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_month_links_refuses_bad_arguments_before_any_launch():
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_month_links(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    for a, text in ((None, "null args"), (_links_args(L, step=0), "step"), (_links_args(L, step=2), "step"),
                    (_links_args(L, step=-2), "step"), (_links_args(L, nseg=-1), "nseg"),
                    (_links_args(L, nrows=-1), "nrows"), (_links_args(L, ids=None), "ids"),
                    (_links_args(L, seg_off=None), "seg_off"), (_links_args(L, month_index=None), "month_index"),
                    (_links_args(L, link=None), "link"), (_links_args(L, bad=None), "bad")):
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_month_links: ") and text in msg, (text, r, msg)
    # empty calls are valid and launch nothing
    assert rc(_links_args(L, nseg=0, nrows=0))[0] == 0 and rc(_links_args(L, nrows=0))[0] == 0
    assert rc(_links_args(L, nseg=0, nrows=0, step=-1, ids=None, month_index=None, link=None))[0] == 0


def test_horizon_return_refuses_bad_arguments_before_any_launch():
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_horizon_return(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    for a, text in ((None, "null args"), (_horizon_args(L, horizon=0), "horizon"),
                    (_horizon_args(L, horizon=61), "horizon"), (_horizon_args(L, horizon=-3), "horizon"),
                    (_horizon_args(L, nseg=-1), "nseg"), (_horizon_args(L, nrows=-5), "nrows"),
                    (_horizon_args(L, ret=None), "ret"), (_horizon_args(L, link=None), "link"),
                    (_horizon_args(L, seg_off=None), "seg_off"), (_horizon_args(L, out=None), "out"),
                    (_horizon_args(L, out=FAKE), "overlap ret"),                     # out == ret
                    (_horizon_args(L, out=FAKE + 8 * 99), "overlap ret"),            # the last element of ret
                    (_horizon_args(L, out=FAKE - 8 * 99), "overlap ret"),            # the first one
                    (_horizon_args(L, out=FAKE + (1 << 20) + 4 * 99), "overlap link")):
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_horizon_return: ") and text in msg, (text, r, msg)
    # adjacent buffers do not overlap; empty calls are valid: nothing is launched either way
    assert rc(_horizon_args(L, out=FAKE + 8 * 100, nseg=0))[0] == 0
    assert rc(_horizon_args(L, nseg=0))[0] == 0 and rc(_horizon_args(L, nrows=0, horizon=60))[0] == 0


def test_pipeline_config_rules_need_no_device():
    from fmcore import lewellen as LW
    from fmcore import step as ST
    assert LW.PipelineConfig().horizon == 1
    names = [f.name for f in dataclasses.fields(LW.PipelineConfig)]
    assert names[-1] == "rank" and "horizon" in names[:-1]     # rank is still the trailing field
    f = {f.name: f for f in dataclasses.fields(LW.PipelineConfig)}["horizon"]
    assert f.kw_only
    for h in (0, -1, 61, 2.5, True):
        with pytest.raises(ValueError, match="horizon must be an integer in 1..60"):
            LW.run_pipeline(None, LW.PipelineConfig(horizon=h, lag=60))
    with pytest.raises(ValueError, match=r"horizon=3 needs lag >= horizon, got lag=1"):
        LW.run_pipeline(None, LW.PipelineConfig(horizon=3))
    with pytest.raises(ValueError, match=r"horizon=12 needs lag >= horizon, got lag=11"):
        LW.run_pipeline(None, LW.PipelineConfig(horizon=12, lag=11))
    LW.check_horizon(LW.PipelineConfig(horizon=12, lag=12))
    LW.check_horizon(LW.PipelineConfig(horizon=60, lag=60))
    assert LW.horizon_column("panel", LW.PipelineConfig(), "retx") == ("panel", "retx")
    assert "y_col" in [f.name for f in dataclasses.fields(LW.PipelineResult)]
    with pytest.raises(ValueError, match="ShardedStep: cfg.horizon must be 1"):
        ST.ShardedStep(None, LW.PipelineConfig(horizon=3, lag=3), None)


def test_engine_and_dropin_signatures():
    import inspect
    from fmcore import engine as E
    from fmdrop import calc_Lewellen_2014 as CL
    names = [f.name for f in dataclasses.fields(E.DevicePanel)]
    assert names[-2:] == ["ids", "month_index"]
    assert list(inspect.signature(E.horizon_panel).parameters) == ["panel", "h", "ret", "name"]
    assert inspect.signature(E.month_links).parameters["step"].default == 1
    assert inspect.signature(E.panel_from_arrays).parameters["ids"].default is None
    p = inspect.signature(CL.horizon_returns).parameters
    assert list(p) == ["df", "h", "return_col", "date_col", "id_col"]
    assert (p["return_col"].default, p["date_col"].default, p["id_col"].default) == ("retx", "mthcaldt", "permno")
    assert hasattr(CL, "build_table_2_horizon")
    with pytest.raises(ValueError, match="step must be"):
        E.month_links(None, step=2)
