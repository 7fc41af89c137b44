"""Host-side checks of the k-month holding of the sorted portfolios (A19): the ABI and the argument
checks of fm_portfolio_hold (each returns before any launch), the numpy restatement against an
independent formulation without links and, at k = 1, against the sort's own oracle, the conditions
the GPU tests rely on in the committed fixture, and the PipelineConfig rules."""
import ctypes
import dataclasses
import functools
import inspect
import os
import types

import numpy as np
import pytest

import hold_oracle as HO
import horizon_oracle as HZ
import port_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLDS = (1, 3, 6, 12)


@functools.lru_cache(maxsize=None)
def _panel():
    return HO.hold_panel()


@functools.lru_cache(maxsize=None)
def _oracle(k):
    p = _panel()
    return HO.portfolio_hold(p["seg_off"], p["month_index"], p["link_prev"], p["port"], p["status"], p["ret"],
                             p["weight"], HO.HOLD_NPORT, k, p["sort_rec"])


def _same(got, exp, what):
    for name in ("members", "stay", "cohort_n", "status"):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], exp[name]), (what, name)
    for name in ("cohort", "rec", "turnover"):
        HZ.assert_same_bits(got[name], exp[name], f"{what} {name}")


# ---------------------------------------------------------------- the ABI
def test_binding_and_header():
    from fmcore import _lib as L
    lib = L.load()
    assert "fm_portfolio_hold" in L.EXPORTED and hasattr(lib, "fm_portfolio_hold")
    assert lib.fm_struct_size(b"fm_hold_args") == ctypes.sizeof(L.HoldArgs) == 144
    assert L._STRUCTS["fm_hold_args"] is L.HoldArgs and L.FM_MAX_HOLD == 36
    with open(os.path.join(ROOT, "include", "fm_hip.h")) as f:
        header = f.read()
    assert "fm_portfolio_hold <- build-defined extension A19; no reference line" in header
    assert "X(fm_hold_args)" in header and "#define FM_MAX_HOLD 36" in header
    names = [n for n, _ in L.HoldArgs._fields_]
    assert names[:8] == ["seg_off", "month_index", "link_prev", "port", "status", "ret", "weight", "sort_rec"]
    assert names[-7:] == ["members", "stay", "cohort_n", "cohort", "status_out", "rec", "turnover"]


FAKE = 1 << 24   # never dereferenced: every call below returns before a launch
INPUTS = ("seg_off", "month_index", "link_prev", "port", "status", "ret", "weight", "sort_rec")
OUTPUTS = ("members", "stay", "cohort_n", "cohort", "status_out", "rec", "turnover")


def _args(L, **kw):
    a = L.HoldArgs(nrows=100, nseg=3, nsel=2, nport=5, hold=3)
    for i, name in enumerate(INPUTS + OUTPUTS):
        setattr(a, name, FAKE * (i + 1))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refuses_bad_arguments_before_any_launch():
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_portfolio_hold(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    at = {name: FAKE * (i + 1) for i, name in enumerate(INPUTS + OUTPUTS)}
    cases = [(None, "null args")]
    cases += [(_args(L, nport=v), "nport") for v in (1, 0, -1, 21)]
    cases += [(_args(L, hold=v), "hold") for v in (0, -2, 37)]
    cases += [(_args(L, nsel=v), "nsel") for v in (-1, 17)]
    cases += [(_args(L, nseg=-1), "nseg"), (_args(L, nrows=-1), "nrows")]
    cases += [(_args(L, **{name: None}), f"{name} is NULL") for name in INPUTS[:6] + OUTPUTS]
    # an output that shares a byte with an input: the first, the last, and one inside
    cases += [(_args(L, rec=at["ret"]), "rec must not overlap ret"),
              (_args(L, cohort=at["ret"] + 8 * 99), "cohort must not overlap ret"),
              (_args(L, members=at["port"] + 2 * 100 - 1), "members must not overlap port"),
              (_args(L, turnover=at["seg_off"] - 8 * 2 * 3 * 5 + 1), "turnover must not overlap seg_off"),
              (_args(L, stay=at["link_prev"] + 4 * 99), "stay must not overlap link_prev"),
              (_args(L, cohort_n=at["month_index"] + 8), "cohort_n must not overlap month_index"),
              (_args(L, status_out=at["status"]), "status_out must not overlap status"),
              (_args(L, rec=at["weight"] + 16), "rec must not overlap weight"),
              (_args(L, turnover=at["sort_rec"] + 8 * (2 * 3 * 6 * 4 - 1)), "turnover must not overlap sort_rec")]
    for a, text in cases:
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_portfolio_hold: ") and text in msg, (text, r, msg)
    # the empty calls are valid and launch nothing, whatever their pointers
    for kw in (dict(nseg=0), dict(nrows=0), dict(nsel=0), dict(nseg=0, nrows=0, nsel=0, seg_off=None, rec=None)):
        assert rc(_args(L, **kw))[0] == 0, kw


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("k", HOLDS)
def test_oracle_matches_the_formulation_without_links(k):
    p = _panel()
    alt = HO.pivot_hold(p["ids"], p["seg_off"], p["month_index"], p["port"], p["status"], p["ret"], p["weight"],
                        HO.HOLD_NPORT, k, p["sort_rec"])
    _same(_oracle(k), alt, f"k={k}")


def test_oracle_at_one_month_is_the_sort():
    """The cohort of age 0 is the portfolio itself: with the port bytes of the sort's oracle, the
    cohort means and counts at k = 1 are the sort's records and counts."""
    p = _panel()
    rng = np.random.default_rng(2)
    n, P = len(p["ret"]), HO.HOLD_NPORT
    F = rng.integers(-50, 51, n) / 8.0
    F[rng.random(n) < 0.05] = np.nan
    s = PO.portfolio_sort(p["seg_off"], F, p["ret"], p["weight"], nport=P)
    assert s["status"].sum() == 29
    o = HO.portfolio_hold(p["seg_off"], p["month_index"], p["link_prev"], s["port"][None], s["status"][None],
                          p["ret"], p["weight"], P, 1, s["rec"][None])
    assert np.array_equal(o["cohort_n"][0, :, 0, :, 0], s["cnt"])
    srt = s["status"] == 1
    HZ.assert_same_bits(o["cohort"][0, srt, 0, :, 0], s["rec"][srt, :P, 0], "ew")
    HZ.assert_same_bits(o["cohort"][0, srt, 0, :, 1], s["rec"][srt, :P, 2], "vw")
    assert np.array_equal(o["status"][0], s["status"])
    HZ.assert_same_bits(o["rec"][0, srt], s["rec"][srt], "rec")     # one cohort: the average is the cohort
    assert np.array_equal(o["stay"][0, :, 0], o["members"][0, :, 0])


def test_fixture_conditions():
    p = _panel()
    assert list(np.diff(p["seg_off"])) == HO.HOLD_LENS and len(p["ret"]) == 11276
    assert HZ.count_bad(p["ids"], p["seg_off"]) == 0 and p["ids"].max() > 1 << 40
    assert np.diff(p["month_index"]).tolist() == [2 if s == HO.HOLD_GAP_SEG else 1 for s in range(1, 32)]
    assert abs(np.mean(p["port"] == 255) - 0.08) < 0.02
    assert np.all(p["ret"][np.isfinite(p["ret"])] * 64 == np.round(p["ret"][np.isfinite(p["ret"])] * 64))
    for k, need in zip(HOLDS, (26, 17, 11, 4)):
        o = _oracle(k)
        assert np.all(o["status"].sum(axis=1) >= need), k
        assert o["stay"][:, :, k].any(), k
        assert np.array_equal(o["stay"][:, :, 0], o["members"][:, :, 0])
    o = _oracle(3)
    full = (o["cohort_n"][..., 0] > 0).all(axis=(2, 3))
    assert np.all(((o["status"] == 1) & full).sum(axis=1) >= 15)
    assert ((o["status"] == 1) & ~full).sum() >= 1            # the NaN path of a complete month
    o = _oracle(12)
    assert np.all((np.isfinite(o["rec"][:, :, HO.HOLD_NPORT, 0]) & (o["status"] == 1)).any(axis=1))
    assert np.isfinite(o["turnover"]).any()


# ---------------------------------------------------------------- the Python layers
def test_signatures_and_fields():
    from fmcore import engine as E
    from fmcore import lewellen as LW
    from fmdrop import bind
    from fmdrop import calc_Lewellen_2014 as CL
    assert [f.name for f in dataclasses.fields(E.HeldPortfolios)] == \
        ["rec", "status", "cohort", "cohort_n", "members", "stay", "turnover", "hold"]
    assert list(inspect.signature(E.portfolio_hold).parameters) == \
        ["seg_off", "month_index", "link_prev", "port", "status", "ret", "weight", "nport", "hold", "sort_rec"]
    assert list(inspect.signature(E.held_portfolios).parameters) == ["panel", "ports", "hold", "ret", "weight"]
    assert E.MAX_HOLD == 36
    f = {f.name: f for f in dataclasses.fields(LW.PipelineConfig)}["portfolio_hold"]
    assert f.kw_only and f.default is None
    res = {f.name: f for f in dataclasses.fields(LW.PipelineResult)}
    for name in ("held", "held_summary", "held_alphas"):
        assert res[name].default is None
    p = inspect.signature(CL.held_sorted_portfolios).parameters
    q = inspect.signature(CL.forecast_sorted_portfolios).parameters
    assert list(p) == ["df", "forecast", "hold"] + list(q)[2:] + ["id_col"] and p["id_col"].default == "permno"
    assert all(p[n].default == q[n].default for n in list(q)[2:])
    p = inspect.signature(CL.build_table_5_held).parameters
    assert list(p) == ["crsp_comp", "hold", "nport", "nyse_breakpoints", "cfg"]
    assert (p["nport"].default, p["nyse_breakpoints"].default) == (10, False)
    src = inspect.getsource(bind)   # extensions, like Tables 3 to 5: not bound into the reference's namespace
    assert "held_sorted_portfolios" not in src and "build_table_5_held" not in src


def test_pipeline_config_rules_need_no_device():
    from fmcore import lewellen as LW
    from fmcore import step as ST
    for k in (0, -1, 37, 2.5, True, "3"):
        with pytest.raises(ValueError, match="portfolio_hold must be an integer in 1..36"):
            LW.run_pipeline(None, LW.PipelineConfig(portfolio_hold=k, portfolios=10))
    with pytest.raises(ValueError, match="portfolio_hold needs portfolios"):
        LW.run_pipeline(None, LW.PipelineConfig(portfolio_hold=6))
    with pytest.raises(ValueError, match="portfolio_hold=6 excludes horizon=3"):
        LW.run_pipeline(None, LW.PipelineConfig(portfolio_hold=6, portfolios=10, horizon=3, lag=3))
    no_ids = types.SimpleNamespace(ids=None, month_index=None, nseg=40)
    with pytest.raises(ValueError, match="portfolio_hold needs a panel with firm ids"):
        LW.run_pipeline(no_ids, LW.PipelineConfig(portfolio_hold=6, portfolios=10))
    LW.check_hold(LW.PipelineConfig())
    LW.check_hold(LW.PipelineConfig(portfolio_hold=36, portfolios=5))
    LW.check_hold(LW.PipelineConfig(portfolio_hold=1, portfolios=5), types.SimpleNamespace(ids=0, month_index=0))
    with pytest.raises(ValueError, match="ShardedStep: cfg.portfolio_hold must be None"):
        ST.ShardedStep(None, LW.PipelineConfig(portfolio_hold=3, portfolios=10), None)
    with pytest.raises(ValueError, match="held_portfolios: the panel carries no firm ids"):
        from fmcore import engine as E
        E.held_portfolios(no_ids, None, 3)
