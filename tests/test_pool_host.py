"""Host-side checks of the pooled panel regressions (A23): the numpy restatement (tests/pool_oracle.py)
against brute force (the dense month-dummy regression, explicit loops over the clusters), the checker
panel's exact numbers, the input conditions the GPU tests rely on, the binding and fm_pool's argument
refusals (each returns before any launch), and the rules of the Python layers that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import pool_oracle as PO
from fmtol import RTOL, assert_series_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement against brute force
def _brute(d, y, xs, u, month_fe, small_sample):
    """float64, no shared code: lstsq on [1, x] (or [month dummies, x]), the meats by Python loops."""
    T = len(d["seg_off"]) - 1
    month = np.repeat(np.arange(T), np.diff(d["seg_off"]))
    use = d["level"] >= u
    for c in list(xs) + [y]:
        use &= ~np.isnan(d["cols"][c])
    X = np.column_stack([d["cols"][c][use] for c in xs])
    Y, mo, fi = d["cols"][y][use], month[use], d["firm"][use]
    N, K = X.shape
    if month_fe:
        months = sorted(set(mo))
        D = np.column_stack([(mo == t).astype(float) for t in months] + [X])
        keep = slice(len(months), None)
    else:
        D = np.column_stack([np.ones(N), X])
        keep = slice(0, None)
    theta = np.linalg.lstsq(D, Y, rcond=None)[0]
    e = Y - D @ theta
    A = np.linalg.inv(D.T @ D)
    sc = D * e[:, None]

    def meat(g):
        M = np.zeros((D.shape[1],) * 2)
        for key in sorted(set(g)):
            s = np.zeros(D.shape[1])
            for i in np.flatnonzero(g == key):
                s += sc[i]
            M += np.outer(s, s)
        return M, len(set(g))
    Mw = sum(np.outer(sc[i], sc[i]) for i in range(N))
    (Mm, Gt), (Mf, Gf) = meat(mo), meat(fi)
    p0 = K + 1
    cw = N / (N - p0) if small_sample else 1.0
    cn = (N - 1) / (N - p0) if small_sample else 1.0
    cm = Gt / (Gt - 1) * cn if small_sample else 1.0
    cf = Gf / (Gf - 1) * cn if small_sample else 1.0
    dof = N - K - Gt if month_fe else N - K - 1
    V = [(e @ e) / dof * A, A @ Mw @ A * cw, A @ Mm @ A * cm, A @ Mf @ A * cf]
    V.append(V[3] + V[2] - V[1])
    return theta[keep], [v[keep, keep] for v in V], e, (N, Gt, Gf)


@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("month_fe", [False, True])
def test_restatement_against_brute_force(seed, month_fe):
    d = PO.parity_panel(seed)
    assert list(np.diff(d["seg_off"])) == PO.PARITY_LENS and d["nfirms"] == 150 and d["ids"].max() > 10 ** 4
    y, xs, levels = PO.PARITY_MODELS[0]
    for u in levels:
        for ss in (True, False):
            ref = PO.pooled(d["cols"], d["seg_off"], d["firm"], y, xs, d["level"], u, month_fe=month_fe, small_sample=ss)
            PO.assert_benign(ref, (seed, month_fe, u))          # what the GPU tests' variance tolerance relies on
            theta, V, e, counts = _brute(d, y, xs, u, month_fe, ss)
            off = int(month_fe)
            assert (ref["N"], ref["Gt"], ref["Gf"]) == counts
            assert_series_close(ref["coef"][off:], theta, "coef", RTOL)
            assert_series_close(ref["resid"][~np.isnan(ref["resid"])], e, "resid", RTOL)
            for k in range(5):
                white = np.diag(V[1])
                for i in range(len(theta)):
                    assert abs(ref["cov"][k][off + i, off + i] - V[k][i, i]) <= RTOL * max(abs(V[k][i, i]), white[i]), \
                        (PO.KINDS[k], i)
            assert np.isnan(ref["se"][:, 0]).all() == month_fe


def test_checker_panel_exact():
    d = PO.checker_panel()
    y, xs, _ = PO.CHECKER_MODELS[0]
    ref = PO.pooled(d["cols"], d["seg_off"], d["firm"], y, xs)
    assert ref["status"] == PO.FITTED | PO.NEG_VAR
    assert list(ref["coef"]) == [1.0, 2.0] and list(ref["stat"][:3]) == [16, 4, 4]
    w = float(np.sqrt(np.float64(1) / np.float64(14)))
    assert list(ref["se"][1]) == [w, w]
    assert list(ref["se"][2]) == [0.0, 0.0] and list(ref["se"][3]) == [0.0, 0.0]
    assert np.isnan(ref["se"][4]).all()
    assert list(np.diag(ref["cov"][4])) == [-1 / 14, -1 / 14]


def test_block_panel_is_what_the_gpu_test_needs():
    from fmcore import _lib as L
    B = L.FM_POOL_FIRM_BLOCK
    for nf in (B - 1, B, B + 1, 2 * B + 1):
        d = PO.block_panel(nf, B)
        f, month = d["firm"], np.repeat(np.arange(5), np.diff(d["seg_off"]))
        assert d["nfirms"] == nf and set(f) == set(range(nf))
        for t in range(5):
            assert (np.diff(f[month == t]) > 0).all()
        assert (month[f == nf - 1] == 0).all() and (f == nf - 1).sum() == 1      # a firm of a single month
        if nf > B:
            assert not (f[month == 2] < B).any()                                  # block 0 has no row in month 2
            assert not (f[month == 1] >= B).any() or nf > 2 * B                   # nor block 1 in month 1
            assert np.isnan(d["cols"][0][(f >= B) & (f < 2 * B)]).all()           # block 1: every row dropped
        for fe in (False, True):
            ref = PO.pooled(d["cols"], d["seg_off"], f, *PO.BLOCK_MODELS[0][:2], month_fe=fe)
            PO.assert_benign(ref, (nf, fe))


# ---------------------------------------------------------------- the ABI
def test_binding_and_header():
    from fmcore import _lib as L
    lib = L.load()
    assert "fm_pool" in L.EXPORTED and "fm_pool_ws_bytes" in L.EXPORTED and hasattr(lib, "fm_pool")
    assert lib.fm_struct_size(b"fm_pool_args") == ctypes.sizeof(L.PoolArgs)
    assert L._STRUCTS["fm_pool_args"] is L.PoolArgs
    with open(os.path.join(ROOT, "include", "fm_hip.h")) as f:
        header = f.read()
    assert "fm_pool         <- build-defined extension A23; no reference line" in header
    assert "X(fm_pool_args)" in header
    assert f"#define FM_POOL_FIRM_BLOCK {L.FM_POOL_FIRM_BLOCK}\n" in header
    assert f"#define FM_POOL_MAX_K {L.FM_POOL_MAX_K}\n" in header
    assert "#define FM_ST_NEG_VAR 0x100u" in header and L.FM_ST_NEG_VAR == 0x100
    for k, name in enumerate(("CLASSICAL", "WHITE", "MONTH", "FIRM", "TWOWAY")):
        assert f"#define FM_POOL_SE_{name} {k}\n" in header and getattr(L, f"FM_POOL_SE_{name}") == k
    body = header[header.index("typedef struct fm_pool_args {"):header.index("} fm_pool_args;")]
    fields = []
    for names in re.findall(r"^\s+(?:const\s+)?\w+\*?\s+([\w, ]+);", body, flags=re.M):
        fields += [n.strip() for n in names.split(",")]
    assert fields == [n for n, _ in L.PoolArgs._fields_]


FAKE = 1 << 24   # never dereferenced: every call below returns before a launch
POINTERS = ("cols", "seg_off", "firm", "bad", "prob_level", "prob_z", "prob_nz", "coef", "se", "stat", "status")


def _args(L, **kw):
    a = L.PoolArgs(col_stride=100, nrows=100, ncols=40, nseg=4, nprob=3, pmax=15, nfirms=300, seg_lo=0, seg_hi=4,
                   ws=FAKE * 20, ws_bytes=1 << 40)
    for i, name in enumerate(POINTERS):
        setattr(a, name, FAKE * (i + 1))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_refuses_bad_arguments_before_any_launch():
    from fmcore import _lib as L
    lib = L.load()

    def rc(a):
        r = lib.fm_pool(None if a is None else ctypes.byref(a), None)
        return r, lib.fm_last_error().decode()

    need = lib.fm_pool_ws_bytes(4, 3, 15, 300)
    assert need > 0 and lib.fm_pool_ws_bytes(4, 3, 15, 257) > lib.fm_pool_ws_bytes(4, 3, 15, 256)
    assert lib.fm_pool_ws_bytes(4, 3, 15, 600) > need                      # a third firm block
    for bad in ((-1, 3, 16, 300), (4, -1, 16, 300), (4, 3, -1, 300), (4, 3, 16, -1)):
        assert lib.fm_pool_ws_bytes(*bad) == -1
    cases = [(None, "null args")]
    cases += [(_args(L, nseg=-1), "negative"), (_args(L, nprob=-1), "negative"), (_args(L, nrows=-1), "negative")]
    cases += [(_args(L, nfirms=-1), "nfirms")]
    cases += [(_args(L, ncols=0), "ncols")]
    cases += [(_args(L, nprob=65536), "65,535")]
    cases += [(_args(L, pmax=v), "pmax must be 2..15") for v in (0, 1, 16)]          # [1, x, y] with K = 15 is 17 wide
    cases += [(_args(L, seg_lo=3, seg_hi=2), "seg_lo"), (_args(L, seg_lo=-1), "seg_lo"), (_args(L, seg_hi=5), "seg_lo")]
    cases += [(_args(L, cols=None), "cols is NULL")]                                   # a planes-only panel
    cases += [(_args(L, **{name: None}), "null pointer") for name in POINTERS if name != "cols"]
    cases += [(_args(L, col_stride=99), "col_stride")]
    cases += [(_args(L, lo=FAKE), "lo and hi"), (_args(L, hi=FAKE), "lo and hi")]
    cases += [(_args(L, stage=-1), "stage"), (_args(L, stage=9), "stage")]
    cases += [(_args(L, ws_bytes=need - 1), "fm_pool_ws_bytes"), (_args(L, ws=None), "fm_pool_ws_bytes")]
    for a, text in cases:
        r, msg = rc(a)
        assert r == -1 and msg.startswith("fm_pool: ") and text in msg, (text, r, msg)
    # a panel wider than 16 columns is no reason to refuse; empty calls are valid
    for kw in (dict(nseg=0, seg_hi=0), dict(nprob=0), dict(seg_lo=2, seg_hi=2), dict(nseg=0, seg_hi=0, cols=None, ws=None)):
        assert rc(_args(L, **kw))[0] == 0, kw


# ---------------------------------------------------------------- the Python layers
def test_check_pooled_rules():
    from fmcore import lewellen as LW

    class P:           # what check_pooled reads of a panel
        ids = None
        cols = object()
    LW.check_pooled(LW.PipelineConfig(), P())                                   # off: nothing to check
    with pytest.raises(ValueError, match="ids"):
        LW.check_pooled(LW.PipelineConfig(pooled=True), P())
    P.ids = object()
    LW.check_pooled(LW.PipelineConfig(pooled=True, pooled_month_fe=True, pooled_small_sample=False), P())
    with pytest.raises(ValueError, match="wls_weights"):
        LW.check_pooled(LW.PipelineConfig(pooled=True, wls_weights="me"), P())
    P.cols = None
    with pytest.raises(ValueError, match="planes-only"):
        LW.check_pooled(LW.PipelineConfig(pooled=True), P())
    cfg = LW.PipelineConfig()
    assert (cfg.pooled, cfg.pooled_month_fe, cfg.pooled_small_sample) == (False, False, True)
    import dataclasses
    kw = {f.name: f.kw_only for f in dataclasses.fields(LW.PipelineConfig)}
    assert kw["pooled"] and kw["pooled_month_fe"] and kw["pooled_small_sample"]
    with pytest.raises(ValueError, match="standardize"):
        LW.check_pooled(LW.PipelineConfig(pooled=True, standardize=True))


def test_sharded_step_refuses_pooled():
    import inspect
    from fmcore import step
    src = inspect.getsource(step)
    assert "cfg.pooled" in src and "ShardedStep: cfg.pooled must be False" in src
