"""Host-side checks of the within-group adjustment (A20): the ABI and the argument checks of
fm_group_adjust (each returns before any launch), the two restatements of the definition against
each other, the conditions the GPU tests rely on in the fixtures (among them: every float64
summation order gives the oracle's bits on the integer fixture, and stays inside the GPU test's
bound on the real-valued one), and the rules of the Python layers that need no device."""
import ctypes
import dataclasses
import inspect
import os
import re
import types

import numpy as np
import pytest

import fmtol
import gadj_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "fm_hip.h")) as f:
        return f.read()


# ---------------------------------------------------------------- the ABI
def test_binding_and_header():
    from fmcore import _lib as L
    from fmcore import engine as E
    lib = L.load()
    for f in ("fm_group_adjust", "fm_group_adjust_batch"):
        assert f in L.EXPORTED and hasattr(lib, f)
    assert lib.fm_struct_size(b"fm_gadj_args") == ctypes.sizeof(L.GroupAdjArgs) == 112
    assert L._STRUCTS["fm_gadj_args"] is L.GroupAdjArgs
    header = _header()
    assert "fm_group_adjust <- build-defined extension A20; no reference line" in header
    assert "X(fm_gadj_args)" in header
    for name, value in (("FM_MAX_GROUPS", 256), ("FM_GADJ_DEMEAN", 0), ("FM_GADJ_MEAN", 1), ("FM_GADJ_ZSCORE", 2)):
        assert f"#define {name} {value}\n" in header and getattr(L, name) == value
    assert E.MAX_GROUPS == 256
    assert E.GADJ_MODES == {"demean": L.FM_GADJ_DEMEAN, "mean": L.FM_GADJ_MEAN, "zscore": L.FM_GADJ_ZSCORE}
    assert tuple(E.GADJ_MODES) == GO.MODES
    # the struct's field order is the header's
    body = header[header.index("typedef struct fm_gadj_args {"):header.index("} fm_gadj_args;")]
    fields = re.findall(r"^\s+(?:const\s+)?\w+\*?\s+(\w+);", body, flags=re.M)
    assert fields == [n for n, _ in L.GroupAdjArgs._fields_] and len(fields) == 17
    # the columns that share a workgroup: bounded by the LDS bins, fewer at more groups
    batch = [lib.fm_group_adjust_batch(g) for g in (1, 2, 49, 64, 65, 128, 256)]
    assert batch == [8, 8, 8, 8, 8, 8, 4] and lib.fm_group_adjust_batch(0) == lib.fm_group_adjust_batch(257) == 0
    assert max(GO.NCOLS) > max(batch)   # the GPU test's widest call needs more than one batch


FAKE = 1 << 24   # never dereferenced: every call below returns before a launch
INPUTS = ("src", "seg_off", "group", "level")
OUTPUTS = ("dst", "gcount", "gmean", "gsd")


def _args(L, **kw):
    a = L.GroupAdjArgs(src_stride=100, dst_stride=100, nrows=100, ncols=3, nseg=4, ngroups=7, mode=L.FM_GADJ_ZSCORE,
                       min_count=1)
    for i, name in enumerate(INPUTS + OUTPUTS):
        setattr(a, name, FAKE * (i + 1))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refuses_bad_arguments_before_any_launch():
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_group_adjust(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    at = {name: FAKE * (i + 1) for i, name in enumerate(INPUTS + OUTPUTS)}
    cases = [(None, "null args")]
    cases += [(_args(L, ngroups=v), "ngroups must be 1..256") for v in (0, -1, 257, 2 ** 31 - 1)]
    cases += [(_args(L, mode=v), "unknown mode") for v in (-1, 3, 99)]
    cases += [(_args(L, min_count=-1), "min_count")]
    cases += [(_args(L, mode=m), "gsd needs FM_GADJ_ZSCORE") for m in (L.FM_GADJ_DEMEAN, L.FM_GADJ_MEAN)]
    cases += [(_args(L, nseg=-1), "nseg"), (_args(L, nrows=-1), "nrows"), (_args(L, ncols=-1), "ncols")]
    cases += [(_args(L, src_stride=99), "stride"), (_args(L, dst_stride=0), "stride")]
    cases += [(_args(L, **{name: None}), f"{name} is NULL") for name in ("src", "seg_off", "group", "dst")]
    # dst on src, and an output that shares a byte with an input: the first, the last, and one inside
    cases += [(_args(L, dst=at["src"]), "dst must not overlap src"),
              (_args(L, dst=at["src"] + 8 * 299), "dst must not overlap src"),
              (_args(L, dst=at["src"] - 8 * 299), "dst must not overlap src"),
              (_args(L, dst=at["group"] + 4 * 99), "dst must not overlap group"),
              (_args(L, dst=at["seg_off"] + 8 * 4), "dst must not overlap seg_off"),
              (_args(L, dst=at["level"] + 99), "dst must not overlap level"),
              (_args(L, gcount=at["src"] + 8), "gcount must not overlap src"),
              (_args(L, gmean=at["group"] - 8 * 3 * 4 * 7 + 1), "gmean must not overlap group"),
              (_args(L, gsd=at["seg_off"]), "gsd must not overlap seg_off"),
              (_args(L, gcount=at["level"] + 50), "gcount must not overlap level")]
    for a, text in cases:
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_group_adjust: ") and text in msg, (text, r, msg)
    # just past the end is no overlap, and the optional pointers may be NULL: these would launch, so
    # only the refusal's absence is checked through the empty calls below
    for kw in (dict(nseg=0), dict(nrows=0), dict(ncols=0),
               dict(nseg=0, nrows=0, ncols=0, src=None, dst=None, seg_off=None, group=None)):
        assert rc(_args(L, **kw))[0] == 0, kw


# ---------------------------------------------------------------- the oracle
def test_the_two_restatements_agree():
    """On the real-valued fixture, plain case: DEMEAN and MEAN within the GPU test's bound (pandas adds
    in its own order), ZSCORE at the project's tolerance."""
    X, g, G = GO.real_values(), GO.codes(GO.REAL_G), GO.REAL_G
    exp = GO.real_expected()
    for mode in ("demean", "mean"):
        alt = GO.pandas_adjust(GO.SEG_OFF, X, g, G, mode)
        GO.assert_within(alt, exp[mode], GO.sum_bound(GO.SEG_OFF, g, G, exp, exp[mode]), f"pandas {mode}")
    fmtol.assert_series_close(GO.pandas_adjust(GO.SEG_OFF, X, g, G, "zscore"), exp["zscore"], "pandas zscore")
    # and on the integer fixture the means are the same bits
    # (columns without an infinity: pandas' compensated group sums treat those in their own way)
    Xi, gi = GO.int_values()[[0, 3]], GO.codes(49)
    ei = GO.int_expected(49)
    for mode in ("demean", "mean"):
        alt = GO.pandas_adjust(GO.SEG_OFF, Xi, gi, 49, mode)
        GO.assert_same_bits(alt, ei[mode][[0, 3]], f"pandas integer {mode}")


def _ordered_means(X, g, G, perm_seed):
    """gmean with plain float64 additions: in row order (perm_seed None), reversed (-1) or permuted."""
    C = X.shape[0]
    T = len(GO.SEG_OFF) - 1
    out = np.full((C, T, G), np.nan)
    rng = np.random.default_rng(0 if perm_seed in (None, -1) else perm_seed)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            a, b = GO.SEG_OFF[t], GO.SEG_OFF[t + 1]
            for c in range(C):
                for k in range(G):
                    x = X[c, a:b][(g[a:b] == k) & ~np.isnan(X[c, a:b])]
                    if len(x) == 0:
                        continue
                    if perm_seed == -1:
                        x = x[::-1]
                    elif perm_seed is not None:
                        x = x[rng.permutation(len(x))]
                    out[c, t, k] = np.cumsum(x)[-1] / np.float64(len(x))   # cumsum adds one by one
    return out


def test_fixture_conditions():
    assert list(np.diff(GO.SEG_OFF)) == GO.LENS and GO.NROWS == 6961 + 0
    X = GO.int_values()
    fin = np.isfinite(X)
    assert np.all(X[fin] == np.round(X[fin])) and np.abs(X[fin]).max() <= 2 ** 20
    assert np.isnan(X[GO.NAN_COL]).all() and abs(np.isnan(X[0]).mean() - 0.05) < 0.01
    assert np.isinf(X).sum() == 3 and np.isinf(X[GO.INF_COL]).sum() == 3
    for G in GO.NGROUPS:
        c = GO.codes(G).astype(np.int64)
        for v in (-1, G, GO.I32_MIN, GO.I32_MAX):
            assert (c == v).sum() >= 10, (G, v)
        assert np.all(c[GO.ONE_GROUP_TILE:GO.ONE_GROUP_TILE + 64] == 0)
        assert len(set(c[GO.DISTINCT_TILE:GO.DISTINCT_TILE + 64])) == min(G, 64)
        assert (GO.ONE_GROUP_TILE - GO.OFF_5000) % 64 == 0 and (GO.DISTINCT_TILE - GO.OFF_5000) % 64 == 0
        if G >= 2:
            m = c[GO.OFF_1000:GO.OFF_5000]
            assert (m[:960] == G - 1).sum() == 0 and (m[960:] == G - 1).sum() >= 2
        e = GO.int_expected(G)
        # +inf alone: -inf for the group's finite rows, NaN for the row itself; both: all NaN
        t9 = len(GO.LENS) - 1
        both = np.flatnonzero(c[GO.OFF_5000:] == 0) + GO.OFF_5000
        both = both[~np.isnan(X[GO.INF_COL, both])]
        assert np.isnan(e["demean"][GO.INF_COL, both]).all() and np.isnan(e["gmean"][GO.INF_COL, t9, 0])
        if G >= 2:
            one = np.flatnonzero(c[GO.OFF_5000:] == 1) + GO.OFF_5000
            one = one[np.isfinite(X[GO.INF_COL, one])]
            assert len(one) >= 5 and np.all(e["demean"][GO.INF_COL, one] == -np.inf)
            assert np.isnan(e["demean"][GO.INF_COL, GO.ROW_PINF]) and e["gmean"][GO.INF_COL, t9, 1] == np.inf
        assert e["gcount"][GO.NAN_COL].sum() == 0 and np.isnan(e["demean"][GO.NAN_COL]).all()
    # every float64 summation order gives the oracle's bits on the integer fixture
    e = GO.int_expected(49)
    X3, g = np.where(np.isinf(X[:3]), np.nan, X[:3]), GO.codes(49)
    ref = GO.group_adjust(GO.SEG_OFF, X3, g, 49)["gmean"]
    for seed in (None, -1, 11):
        GO.assert_same_bits(_ordered_means(X3, g, 49, seed), ref, f"order {seed}")
    assert np.array_equal(e["gcount"][0], GO.group_adjust(GO.SEG_OFF, X3, g, 49)["gcount"][0])


def test_real_fixture_orders_stay_inside_the_bound():
    """Sequential, reversed and permuted float64 sums of the real-valued fixture stay inside the bound
    the GPU test holds the kernel to: below half of it here, so the bound has room for any order."""
    X, g, G = GO.real_values(), GO.codes(GO.REAL_G), GO.REAL_G
    exp = GO.real_expected()
    bound = GO.table_bound(exp)
    worst = 0.0
    for seed in (None, -1, 12):
        got = _ordered_means(X, g, G, seed)
        ok = ~np.isnan(exp["gmean"])
        assert np.array_equal(np.isnan(got), ~ok)
        worst = max(worst, float(np.max(np.abs(got[ok] - exp["gmean"][ok]) / bound[ok])))
    assert worst <= 0.5, worst
    # the z-score fixture has its NaN cases: a constant group and groups of one row
    t8 = 8
    assert exp["gcount"][0, t8, GO.CONST_GROUP] >= 5 and exp["gsd"][0, t8, GO.CONST_GROUP] == 0.0
    rows = GO.OFF_1000 + np.flatnonzero(g[GO.OFF_1000:GO.OFF_5000] == GO.CONST_GROUP)
    assert np.isnan(exp["zscore"][0, rows]).all() and np.all(exp["demean"][0, rows] == 0.0)
    assert (exp["gcount"] == 1).sum() >= 10
    assert np.isnan(exp["gsd"][exp["gcount"] == 1]).all()
    assert np.isfinite(exp["zscore"]).mean() > 0.8


# ---------------------------------------------------------------- the Python layers
def test_signatures_and_fields():
    from fmcore import engine as E
    from fmcore import ingest as IN
    from fmcore import lewellen as LW
    from fmdrop import bind
    from fmdrop import calc_Lewellen_2014 as CL
    names = [f.name for f in dataclasses.fields(E.DevicePanel)]
    assert names[-4:] == ["group", "ngroups", "ids", "month_index"]
    d = {f.name: f.default for f in dataclasses.fields(E.DevicePanel)}
    assert d["group"] is None and d["ngroups"] == 0
    assert [f.name for f in dataclasses.fields(E.GroupStats)] == ["mean", "sd", "count"]
    p = inspect.signature(E.panel_from_arrays).parameters
    assert list(p)[-3:] == ["ids", "group", "ngroups"] and p["group"].default is None and p["ngroups"].default is None
    assert list(inspect.signature(E.group_adjust_columns).parameters) == \
        ["seg_off", "x", "group", "ngroups", "mode", "min_count", "level", "min_level", "out", "stats"]
    p = inspect.signature(E.group_adjust).parameters
    assert list(p) == ["panel", "cols", "mode", "min_count", "level", "min_level", "out", "stats"]
    assert (p["cols"].default, p["mode"].default, p["min_count"].default, p["level"].default, p["min_level"].default,
            p["out"].default, p["stats"].default) == (None, "demean", 1, None, 0, None, False)
    p = inspect.signature(IN.panel_from_arrow).parameters
    assert list(p)[-1] == "group_col" and p["group_col"].default is None
    # PipelineConfig: three keyword-only fields directly in front of alpha_factors
    fields = dataclasses.fields(LW.PipelineConfig)
    names = [f.name for f in fields]
    i = names.index("alpha_factors")
    assert names[i - 3:i] == ["group_adjust", "group_adjust_cols", "group_min_count"]
    assert all(f.kw_only for f in fields[i - 3:i])
    assert [f.default for f in fields[i - 3:i]] == [None, None, 1]
    assert names[-1] == "rank"
    rn = [f.name for f in dataclasses.fields(LW.PipelineResult)]
    i = rn.index("y_col")
    assert rn[i + 1:i + 3] == ["group_stats", "group_adjusted"]
    res = {f.name: f for f in dataclasses.fields(LW.PipelineResult)}
    assert res["group_stats"].default is None and res["group_adjusted"].default is None
    # the drop-in
    p = inspect.signature(CL.group_adjust).parameters
    assert list(p) == ["crsp_comp", "varlist", "group_col", "date_col", "mode", "min_count", "universe"]
    assert [p[n].default for n in list(p)[2:]] == ["siccd", "mthcaldt", "demean", 1, None]
    p = inspect.signature(CL._pipeline_panel).parameters
    assert list(p) == ["crsp_comp", "variables_dict", "group_col"] and p["group_col"].default is None
    assert list(inspect.signature(CL.lewellen_pipeline).parameters) == ["crsp_comp", "variables_dict", "cfg"]
    for f in (CL.lewellen_pipeline, CL.build_table_5, CL.build_table_5_held, CL.build_table_alphas, CL.build_table_3,
              CL.build_table_3_extrapolated, CL.build_table_4, CL.build_table_2_horizon):
        assert 'cfg.pop("group_col", None)' in inspect.getsource(f), f.__name__
    src = inspect.getsource(bind)   # an extension: not bound into the reference's namespace
    assert "group_adjust" not in src


def test_group_codes():
    from fmcore import engine as E
    codes, uniq = E.group_codes(["oil", None, "banks", "oil", "autos"])
    assert codes.dtype == np.int32 and codes.tolist() == [2, -1, 1, 2, 0] and list(uniq) == ["autos", "banks", "oil"]
    codes, uniq = E.group_codes(np.array([3711.0, np.nan, 1311.0, 3711.0]))
    assert codes.tolist() == [1, -1, 0, 1] and uniq.tolist() == [1311.0, 3711.0]
    import pandas as pd
    codes, uniq = E.group_codes(pd.Series([49, 1, 1, 13], dtype="int64"))
    assert codes.tolist() == [2, 0, 0, 1] and uniq.tolist() == [1, 13, 49]
    codes, uniq = E.group_codes(np.array([], dtype=np.int64))
    assert codes.dtype == np.int32 and len(codes) == 0 and len(uniq) == 0


def test_rules_that_need_no_device():
    from fmcore import engine as E
    from fmcore import lewellen as LW
    from fmcore import step as ST
    with pytest.raises(ValueError, match=r"PipelineConfig: group_adjust must be one of \['demean', 'mean', 'zscore'\], "
                                         r"got 'median'"):
        LW.run_pipeline(None, LW.PipelineConfig(group_adjust="median"))
    bare = types.SimpleNamespace(group=None, ngroups=0, ids=None, month_index=None, nseg=40)
    with pytest.raises(ValueError, match="PipelineConfig: group_adjust needs a panel with group codes"):
        LW.run_pipeline(bare, LW.PipelineConfig(group_adjust="demean"))
    with pytest.raises(ValueError, match="PipelineConfig: group_adjust excludes standardize"):
        LW.run_pipeline(bare, LW.PipelineConfig(group_adjust="zscore", standardize=True))
    with pytest.raises(ValueError, match=r"PipelineConfig: group_adjust_cols must name predictors of the models, "
                                         r"not \['retx', 'nope'\]"):
        LW.run_pipeline(bare, LW.PipelineConfig(group_adjust="mean", group_adjust_cols=["log_bm", "retx", "nope"]))
    with pytest.raises(ValueError, match="PipelineConfig: group_adjust_cols needs group_adjust"):
        LW.run_pipeline(None, LW.PipelineConfig(group_adjust_cols=["log_bm"]))
    for k in (-1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="PipelineConfig: group_min_count must be an integer >= 0"):
            LW.run_pipeline(None, LW.PipelineConfig(group_adjust="demean", group_min_count=k))
    # a configuration without group_adjust never touches panel.group
    LW.check_group_adjust(LW.PipelineConfig(), types.SimpleNamespace())
    LW.check_group_adjust(LW.PipelineConfig(group_adjust="demean", group_adjust_cols=["log_bm", "roa"]),
                          types.SimpleNamespace(group=0))
    with pytest.raises(ValueError, match="ShardedStep: cfg.group_adjust must be None"):
        ST.ShardedStep(None, LW.PipelineConfig(group_adjust="demean"), None)
    with pytest.raises(ValueError, match="group_adjust: the panel carries no group codes"):
        E.group_adjust(bare)
    with pytest.raises(ValueError, match="group_adjust: mode must be one of"):
        E.group_adjust(bare, mode="median")
    # more than 256 groups, or codes that are no integers: refused before any upload
    lab = np.zeros(300, dtype=np.int64)
    with pytest.raises(ValueError, match="panel_from_arrays: ngroups must be 1..256, got 257"):
        E.panel_from_arrays([np.zeros(300)], ["x"], lab, group=np.arange(300) % 257)
    with pytest.raises(ValueError, match="panel_from_arrays: ngroups must be 1..256, got 300"):
        E.panel_from_arrays([np.zeros(300)], ["x"], lab, group=lab, ngroups=300)
    with pytest.raises(ValueError, match="panel_from_arrays: group must hold one integer code per input row"):
        E.panel_from_arrays([np.zeros(300)], ["x"], lab, group=np.zeros(300))
    with pytest.raises(ValueError, match="panel_from_arrays: group must hold one integer code per input row"):
        E.panel_from_arrays([np.zeros(300)], ["x"], lab, group=lab[:299])
