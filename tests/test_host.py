"""CPU-only tests: the C-ABI library loads and exports every symbol include/fm_hip.h
declares (no compute call), struct layouts match, and the host-side planning logic
(validity patterns, chunking, month sharding, Table-2 formatting, synthetic generator)
behaves as the kernels assume."""
import os
import re

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "fm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(fm_\w+)\s*\(", txt, flags=re.M)))


def test_library_exports_header_symbols():
    import ctypes
    from fmcore import _lib as L
    lib = L.load()
    funcs = _header_functions()
    assert len(funcs) >= 18
    for f in funcs:
        assert hasattr(lib, f), f
        assert f in L.EXPORTED, f"ctypes signature missing for {f}"
    assert L.version().startswith("libfm_hip")
    assert {"fm_gram_args", "fm_solve_args", "fm_forecast_src"} <= set(L._STRUCTS)
    for name, cls in L._STRUCTS.items():
        assert lib.fm_struct_size(name.encode()) == ctypes.sizeof(cls), name
    # every struct the header lists has a binding class, and no other name is known
    hdr = open(os.path.join(ROOT, "include", "fm_hip.h")).read()
    listed = re.findall(r"X\((fm_\w+)\)", hdr[hdr.index("#define FM_ARG_STRUCTS"):hdr.index("int64_t fm_struct_size")])
    assert sorted(listed) == sorted(L._STRUCTS)
    assert lib.fm_struct_size(b"fm_no_such_args") == -1


def _fixup_args(L, **kw):
    """An fm_solve_fixup call that is valid on its arguments (3 months x 2 problems of up to 15
    columns); the pointers are never dereferenced: each call below returns before any launch."""
    fake = 4096
    a = L.SolveArgs(nseg=3, nprob=2, zw=32, pmax=16, mom_stride=300, prob_level=fake, prob_z=fake, prob_nz=fake,
                    rec=fake, status=fake, moments=fake, fix_cols=fake, fix_stride=100, fix_seg_off=fake,
                    fix_check_const=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_solve_fixup_refuses_on_arguments_alone():
    import ctypes
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_solve_fixup(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    fake = 4096
    bad = [(None, "null args"),
           (_fixup_args(L, fix_cols=None), "null pointer"),
           (_fixup_args(L, fix_hi_plane=fake, fix_lo_plane=fake), "plane"),
           (_fixup_args(L, fix_cols=None, fix_hi_plane=fake, fix_lo_plane=fake), "plane"),
           (_fixup_args(L, fix_hi_plane=fake), "plane"),
           (_fixup_args(L, fix_lo=fake), "fix_lo and fix_hi"),
           (_fixup_args(L, fix_hi=fake), "fix_lo and fix_hi"),
           (_fixup_args(L, fix_inv_scale=fake), "fix_inv_scale needs fix_shift"),
           (_fixup_args(L, moments=None), "moments"),
           (_fixup_args(L, fix_seg_off=None), "fix_seg_off"),
           (_fixup_args(L, pmax=1), "pmax"),
           (_fixup_args(L, pmax=33), "pmax")]
    for a, text in bad:
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_solve_fixup: ") and text in msg, (text, r, msg)
    # the same conditions refuse fm_solve's inline fix-ups, in the same words after the prefix
    for kw in (dict(fix_lo=fake), dict(fix_inv_scale=fake), dict(moments=None), dict(fix_seg_off=None)):
        a = _fixup_args(L, zw=16, pmax=15, partial=fake, seg_chunk_off=fake, pattern_models=fake, prob_model=fake,
                        prob_flags=fake, npatterns=1, nlevels=1, **kw)
        r1, m1 = rc(a)
        r2 = lib.fm_solve(ctypes.byref(a), None)
        m2 = lib.fm_last_error().decode()
        assert r1 == r2 == -1 and m1.split(": ", 1)[1] == m2.split(": ", 1)[1] and m2.startswith("fm_solve: "), (kw, m1, m2)
    # and fm_solve still refuses the fix-ups with the 32-wide solve
    a = _fixup_args(L, partial=fake, seg_chunk_off=fake, pattern_models=fake, prob_model=fake, prob_flags=fake,
                    npatterns=1, nlevels=1)
    assert lib.fm_solve(ctypes.byref(a), None) == -1 and "zw 16" in lib.fm_last_error().decode()
    # nothing to scan: valid, nothing launched
    assert rc(_fixup_args(L, nseg=0))[0] == 0 and rc(_fixup_args(L, nprob=0))[0] == 0
    # with every condition met the struct passes the checks of both entry points' shared helper:
    # lo with hi and inv_scale with shift are accepted (nseg = 0, so still no launch)
    assert rc(_fixup_args(L, nseg=0, fix_lo=fake, fix_hi=fake, fix_shift=fake, fix_inv_scale=fake))[0] == 0


def test_library_is_gfx950_code_object(tmp_path):
    import shutil
    import subprocess
    from fmcore import _lib as L
    lib = tmp_path / "libfm_hip.so"
    shutil.copy(L.LIB_PATH, lib)   # --offloading extracts the code objects next to its input
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(lib)],
                         capture_output=True, text=True, cwd=tmp_path)
    if out.returncode != 0:
        pytest.skip("llvm-objdump --offloading unavailable")
    assert "gfx950" in out.stdout + out.stderr


def test_compute_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from fmcore import engine
    with pytest.raises(RuntimeError):
        engine.require_device()


def test_plan_patterns_nested_lewellen_models():
    from fmcore.engine import Model, plan_patterns
    cols = list(range(16))
    m1 = Model("m1", 0, [1, 2, 3])
    m2 = Model("m2", 0, [1, 2, 3, 4, 5, 6, 7])
    m3 = Model("m3", 0, list(range(1, 15)))
    f1 = Model("f1", 0, [2, 3, 4, 5, 7])
    lut, pats = plan_patterns([m1, m2, m3, f1])
    # M3 valid => M2 valid => M1, F1 valid: 5 non-empty consistent patterns
    assert sorted(pats) == sorted([0b0001, 0b1000, 0b1001, 0b1011, 0b1111])
    assert lut[0] == 255 and all(lut[p] != 255 for p in pats)
    assert cols  # silence


def test_make_chunks_cover_segments_exactly():
    from fmcore.engine import default_chunk_rows, make_chunks
    seg_off = np.array([0, 0, 5000, 5003, 20000, 20001], dtype=np.int64)
    ch = default_chunk_rows(20001, 5, 15000, target_chunks=8)
    seg, rows, off = make_chunks(seg_off, ch)
    rows = rows.reshape(-1, 2)
    for s in range(len(seg_off) - 1):
        mine = rows[off[s]:off[s + 1]]
        assert (seg[off[s]:off[s + 1]] == s).all()
        assert mine[0, 0] == seg_off[s] and mine[-1, 1] == seg_off[s + 1]
        assert (mine[1:, 0] == mine[:-1, 1]).all()
        assert (mine[:, 1] - mine[:, 0] <= ch).all()
    # a month is chunked the same way whatever else is in the panel (shard independence)
    s2, r2, o2 = make_chunks(seg_off[2:5] - seg_off[2], ch)
    assert np.array_equal(r2.reshape(-1, 2) + seg_off[2], rows.reshape(-1, 2)[off[2]:off[4]])


def test_shard_bounds_balanced_and_contiguous():
    from fmcore.dist import shard_bounds
    rows = np.r_[np.full(50, 100), np.full(50, 300)]
    b = shard_bounds(rows, 4)
    assert b[0][0] == 0 and b[-1][1] == 100
    assert all(b[i][1] == b[i + 1][0] for i in range(3))
    loads = [rows[s:e].sum() for s, e in b]
    assert max(loads) - min(loads) <= 300


def test_synth_deterministic_and_month_major():
    from fmcore import synth
    a = synth.synth_arrays(5, 40, 3, nan_rate=0.1, present_rate=0.8)
    b = synth.synth_arrays(5, 40, 3, nan_rate=0.1, present_rate=0.8)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")
    assert (np.diff(a["month"]) >= 0).all()
    c = synth.synth_arrays(3, 40, 3, nan_rate=0.1, month0=2)
    full = synth.synth_arrays(5, 40, 3, nan_rate=0.1)
    assert np.array_equal(c["retx"], full["retx"][2 * 40:], equal_nan=True)   # shards agree


def test_table2_formatting_matches_golden_from_oracle_stats():
    """The host-side Table-2 string layout (no compute) against the reference's strings."""
    import cases
    from fmtol import frame_from, load_json, load_npz
    from oracle import fm_oracle as O
    from fmdrop import calc_Lewellen_2014 as CL
    g = load_npz("fm.npz")
    meta = load_json("fm.json")
    df = frame_from(g, "in_")
    subs = O.get_subsets(O.winsorize(df, cases.WINSOR_VARS))
    stats = {}
    for mname, (label, xs) in zip(cases.MODELS, zip(CL._LW.MODELS_PREDICTORS, cases.MODELS.values())):
        for s in cases.SUBSETS:
            cs = O.run_monthly_cs_regressions(subs[s], "retx", xs)
            sm = O.fama_macbeth_summary(cs, xs)
            stats[(label, s)] = {"coef": [sm[f"{x}_coef"] for x in xs], "tstat": [sm[f"{x}_tstat"] for x in xs],
                                 "mean_R2": sm["mean_R2"], "mean_N": sm["mean_N"]}
    t2 = CL._format_table_2(stats, cases.SUBSETS)
    assert [list(i) for i in t2.index] == meta["table2"]["index"]
    assert [list(c) for c in t2.columns] == meta["table2"]["columns"]
    assert [[str(x) for x in r] for r in t2.values.tolist()] == meta["table2"]["values"]


def test_reference_test_file_collects_nothing():
    """The reference's own test module defines no test_* function."""
    import ast
    src = "/root/reference/src/test_calc_Lewellen_2014.py"
    if not os.path.exists(src):
        pytest.skip("reference not mounted")
    tree = ast.parse(open(src).read())
    assert not [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test")]


def _arrow_frame(n=3000, seed=3):
    rng = np.random.default_rng(seed)
    months = pd.date_range("1964-01-31", periods=12, freq="ME")
    df = pd.DataFrame({
        "mthcaldt": rng.choice(months, n),
        "retx": rng.normal(1, 10, n),
        "log_size": rng.normal(5, 2, n),
        "me": np.exp(rng.normal(5, 2, n)),
        "primaryexch": rng.choice(["N", "Q", "A"], n),
    })
    df.loc[rng.random(n) < 0.05, "retx"] = np.nan
    df.loc[rng.random(n) < 0.02, "mthcaldt"] = pd.NaT
    df.loc[rng.random(n) < 0.02, "primaryexch"] = None
    return df


def test_arrow_host_columns_match_frame_path():
    """§8(f) row 3: Arrow ingest yields the arrays, month segments and NYSE mask the pandas
    path (calc_Lewellen_2014.get_subsets / winsorize -> panel_from_arrays) builds."""
    import pyarrow as pa
    from fmcore import engine, ingest
    df = _arrow_frame()
    tab = pa.Table.from_pandas(df, preserve_index=False)
    arrays, labels, me, nyse = ingest.arrow_host_columns(tab, ["retx", "log_size"], me_col="me",
                                                         exch_col="primaryexch")
    for a, c in zip(arrays, ["retx", "log_size"]):
        np.testing.assert_array_equal(a, df[c].to_numpy(dtype=np.float64))
    np.testing.assert_array_equal(me, df["me"].to_numpy())
    np.testing.assert_array_equal(nyse, (df["primaryexch"] == "N").to_numpy().astype(np.uint8))
    _, u1, o1, s1 = engine.month_segments(labels)
    _, u2, o2, s2 = engine.month_segments(df["mthcaldt"].values)
    np.testing.assert_array_equal(o1, o2)
    np.testing.assert_array_equal(s1, s2)
    assert list(u1) == list(u2)


def test_arrow_host_columns_from_parquet(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from fmcore import ingest
    df = _arrow_frame(500, 4)
    tab = pa.Table.from_pandas(df, preserve_index=False)
    p = tmp_path / "panel.parquet"
    pq.write_table(tab, p, row_group_size=128)      # several chunks per column
    arrays, labels, me, nyse = ingest.arrow_host_columns(str(p), ["retx"], exch_col="primaryexch")
    np.testing.assert_array_equal(arrays[0], df["retx"].to_numpy())
    assert me is None and nyse.dtype == np.uint8 and len(labels) == len(df)


def test_month_segments_radix_order_is_stable_order():
    """engine.month_segments narrows month codes to int16 (numpy's stable radix sort); the
    order must equal the int64 stable sort of the pandas factorize codes."""
    from fmcore import engine
    df = _arrow_frame(5000, 5)
    for labels in (df["mthcaldt"].values, np.arange(40000) % 33000):   # int16 and wide paths
        codes, uniq = pd.factorize(labels, sort=True)
        ref = np.argsort(np.asarray(codes, dtype=np.int64), kind="stable")
        ref = ref[codes[ref] >= 0]
        _, u1, o1, s1 = engine.month_segments(labels)
        np.testing.assert_array_equal(o1, ref)
        assert s1[-1] == len(ref) and len(u1) == len(uniq)


def test_etl_month_codes_round_trip():
    """fmcore.etl's host planning: month codes of month-end and mid-month dates, and the
    month-end dates of codes (the calendar side of fm_ffill_expand)."""
    import pandas as pd
    from fmcore import etl as X
    d = pd.to_datetime(["1964-01-31", "1999-12-31", "2000-02-29", "2013-06-15", "1970-01-01"])
    c = X.month_code(d.to_numpy())
    assert list(c) == [1964 * 12, 1999 * 12 + 11, 2000 * 12 + 1, 2013 * 12 + 5, 1970 * 12]
    back = pd.DatetimeIndex(X.code_to_month_end(c))
    assert list(back.strftime("%Y-%m-%d")) == ["1964-01-31", "1999-12-31", "2000-02-29", "2013-06-30",
                                               "1970-01-31"]


def test_split_month_chunk_plan():
    """make_chunks_split: every month of >= 256 rows as a 3/4 + 1/4 pair (own length only),
    shorter ones whole; chunks tile each month exactly; the launch order is a permutation
    with every big chunk first (last month first)."""
    import numpy as np
    from fmcore.engine import make_chunks_split, split_policy
    lens = np.array([5000, 255, 256, 1, 7919, 0, 300])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seg, rows, coff, order = make_chunks_split(off)
    rows = rows.reshape(-1, 2)
    assert sorted(order.tolist()) == list(range(len(seg)))
    for t in range(len(lens)):
        cs = list(range(coff[t], coff[t + 1]))
        assert all(seg[c] == t for c in cs)
        assert len(cs) == (2 if lens[t] >= 256 else 1)
        assert rows[cs[0], 0] == off[t] and rows[cs[-1], 1] == off[t + 1]
        for a, b in zip(cs, cs[1:]):
            assert rows[a, 1] == rows[b, 0]
        if len(cs) == 2:
            assert rows[cs[0], 1] - rows[cs[0], 0] == lens[t] * 3 // 4
    nbig = len(lens)
    assert list(order[:nbig]) == list(coff[:-1][::-1])
    assert not split_policy(600) and not split_policy(12500)


def test_balanced_chunk_plan():
    """fm_gram's balanced plan: chunks never straddle a month, a month's chunks are
    contiguous and cover it (empty months keep one empty chunk), every workgroup's chunks lie
    in one global R-row block, and the plan of a shard (row_origin) equals the global plan
    restricted to its months -- so a month sums the same rows in the same order at any
    rank count."""
    from fmcore.engine import chunk_policy, make_chunks_balanced
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 9000, 57)
    lens[[3, 4, 20]] = 0
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for R in (997, 3906, 10 ** 6):
        seg, rows, off, wg = make_chunks_balanced(so, R)
        r = rows.reshape(-1, 2)
        assert (np.diff(seg) >= 0).all() and (r[:, 0] <= r[:, 1]).all()
        for m in range(len(so) - 1):
            rr = r[off[m]:off[m + 1]]
            assert len(rr) >= 1 and (seg[off[m]:off[m + 1]] == m).all()
            assert rr[0, 0] == so[m] and rr[-1, 1] == so[m + 1] and (rr[1:, 0] == rr[:-1, 1]).all()
        for b in range(len(wg) - 1):
            nz = r[wg[b]:wg[b + 1]]
            nz = nz[nz[:, 1] > nz[:, 0]]
            assert len(set((nz[:, 0] // R).tolist())) <= 1 and ((nz[:, 1] - 1) // R == nz[:, 0] // R).all()
        # a shard of months [s0, s1) with its global row origin: the same chunks of its months
        s0, s1 = 10, 40
        sub = so[s0:s1 + 1] - so[s0]
        seg2, rows2, off2, _ = make_chunks_balanced(sub, R, row_origin=int(so[s0]))
        for m in range(s1 - s0):
            a = r[off[s0 + m]:off[s0 + m + 1]]
            b = rows2.reshape(-1, 2)[off2[m]:off2[m + 1]] + so[s0]
            assert np.array_equal(a, b)
    assert chunk_policy(3_000_000, 600, 5000, slots=768) == ("balanced", 3907)
    assert chunk_policy(250_000_000, 12500, 20000, slots=768)[0] == "months"
