"""GPU tests of the pooled panel regressions (A23): engine.pooled_regressions (fm_pool) against the
numpy restatement (tests/pool_oracle.py), against the monthly kernels' moments, the checker panel's
exact numbers, the firm-block edges, the bit identities of the header's order contract, the status
rules, and PipelineConfig(pooled=True), run_pooled_regression and build_table_2_pooled end to end."""
import numpy as np
import pytest
import torch

import pipe_port_oracle as PPO
import pool_oracle as PO
from fmtol import RTOL, assert_series_close, scalar_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _dev(E, a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(E.require_device())


def _panel(E, d, ids=None):
    seg_off = np.asarray(d["seg_off"], dtype=np.int64)
    return E.DevicePanel(cols=_dev(E, np.stack(d["cols"])), names=[f"c{i}" for i in range(len(d["cols"]))],
                         seg_off=_dev(E, seg_off), seg_off_h=seg_off, ids=_dev(E, d["ids"] if ids is None else ids))


def _models(E, models):
    return [E.Model(f"m{i}", y=y, xs=list(xs), levels=tuple(levels)) for i, (y, xs, levels) in enumerate(models)]


def _host(res):
    torch.cuda.synchronize()
    g = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(coef=g(res.coef), se=g(res.se), cov=g(res.cov), stat=g(res.stat), status=g(res.status),
                resid=g(res.resid))


def _run(E, d, models, cuts=None, panel=None, **kw):
    panel = _panel(E, d) if panel is None else panel
    level = _dev(E, d.get("level"))
    c = None if cuts is None else E.Cuts(_dev(E, cuts[0]), _dev(E, cuts[1]), None)
    kw.setdefault("cov", True)
    kw.setdefault("resid", True)
    res = E.pooled_regressions(panel, _models(E, models), level=level, nlevels=3 if level is not None else 1, cuts=c, **kw)
    return res, _host(res)


def _assert_close(h, refs, what):
    """coef, stat and resid under the project's series tolerance; variances at RTOL with the
    coefficient's White variance as the scale; the counts and the status exact."""
    for k, ref in enumerate(refs):
        w = f"{what}, problem {k}"
        K1 = len(ref["coef"])
        assert int(h["status"][k]) == ref["status"], (w, int(h["status"][k]), ref["status"])
        assert list(h["stat"][k, :3]) == [ref["N"], ref["Gt"], ref["Gf"]] and h["stat"][k, 7] == 0.0, w
        assert_series_close(h["coef"][k, :K1], ref["coef"], f"{w}: coef", RTOL)
        assert np.isnan(h["coef"][k, K1:]).all() and np.isnan(h["se"][k, :, K1:]).all(), w
        for i, name in ((3, "R2"), (4, "SSR"), (5, "s2"), (6, "dof")):
            assert scalar_close(h["stat"][k, i], ref["stat"][i], RTOL), (w, name, h["stat"][k, i], ref["stat"][i])
        assert_series_close(h["resid"][k], ref["resid"], f"{w}: resid", RTOL)
        white = np.diag(ref["cov"][1])
        for kind in range(5):
            got, want = h["se"][k, kind, :K1] ** 2, ref["se"][kind] ** 2
            assert np.array_equal(np.isnan(got), np.isnan(want)), (w, PO.KINDS[kind], got, want)
            covd = np.diag(h["cov"][k, kind, :K1, :K1])
            for i in range(K1):
                if not np.isnan(want[i]):
                    assert abs(got[i] - want[i]) <= RTOL * max(abs(want[i]), white[i]), (w, PO.KINDS[kind], i, got[i], want[i])
                v = ref["cov"][kind][i, i]
                assert (np.isnan(v) and np.isnan(covd[i])) or abs(covd[i] - v) <= RTOL * max(abs(v), white[i]), \
                    (w, "cov", PO.KINDS[kind], i)
            # the whole matrix, every entry scaled by its two White standard errors
            sc = np.sqrt(np.outer(white, white))
            both = ~np.isnan(ref["cov"][kind])
            assert np.array_equal(~np.isnan(h["cov"][k, kind, :K1, :K1]), both), (w, PO.KINDS[kind])
            diff = np.abs(h["cov"][k, kind, :K1, :K1] - ref["cov"][kind])[both]
            assert (diff <= RTOL * np.maximum(np.abs(ref["cov"][kind]), sc)[both]).all(), (w, "cov", PO.KINDS[kind])


# ---------------------------------------------------------------- 1. against the restatement
@pytest.fixture(scope="module")
def parity_data():
    d = PO.parity_panel()
    return d, PPO.winsor_cuts(d["cols"], d["seg_off"])


@pytest.mark.parametrize("small_sample", [True, False])
@pytest.mark.parametrize("with_cuts", [False, True])
@pytest.mark.parametrize("month_fe", [False, True])
def test_against_restatement(E, parity_data, month_fe, with_cuts, small_sample):
    d, (lo, hi) = parity_data
    cuts = (lo, hi) if with_cuts else None
    refs = PO.pooled_all(d, PO.PARITY_MODELS, *(cuts or (None, None)), month_fe=month_fe, small_sample=small_sample)
    for r in refs:
        PO.assert_benign(r)
    res, h = _run(E, d, PO.PARITY_MODELS, cuts=cuts, month_fe=month_fe, small_sample=small_sample)
    assert [(p.model, p.level, p.K) for p in res.problems] == PO.problems(PO.PARITY_MODELS) and res.pmax == 4
    assert len({r["N"] for r in refs}) == 3                       # the three universe levels differ
    _assert_close(h, refs, f"parity fe={month_fe} cuts={with_cuts} ss={small_sample}")
    t = res.tstat("firm").cpu().numpy()
    assert np.array_equal(t, h["coef"] / h["se"][:, 3], equal_nan=True)


# ---------------------------------------------------------------- 2. cross-checks on the existing kernels
def test_fe_slopes_equal_the_months_centred_moments(E):
    d = PO.block_panel(255)
    panel, models = _panel(E, d), _models(E, PO.BLOCK_MODELS)
    res, h = _run(E, d, PO.BLOCK_MODELS, panel=panel, month_fe=True)
    fm = E.fm_pass(panel, models, moments=True)
    torch.cuda.synchronize()
    mom, st = fm.moments.cpu().numpy()[:, 0], fm.status.cpu().numpy()[:, 0]
    assert (st == E.L.FM_ST_FITTED).all()
    K, K1 = 2, 3
    S = mom[:, 1 + K1:1 + K1 + K1 * K1].reshape(-1, K1, K1).astype(np.longdouble).sum(axis=0)
    b = PO._inv(S[:K, :K]) @ S[:K, K]
    assert h["stat"][0, 0] == mom[:, 0].sum()
    assert_series_close(h["coef"][0, 1:K1], b.astype(np.float64), "FE slopes", RTOL)
    assert np.isnan(h["coef"][0, 0])


def test_every_firm_once_makes_the_firm_meat_the_white_meat(E, parity_data):
    d = dict(parity_data[0])
    n = int(d["seg_off"][-1])
    d["ids"] = np.arange(n, dtype=np.int64) * 5 + 11
    for fe in (False, True):
        res, h = _run(E, d, PO.PARITY_MODELS, month_fe=fe, small_sample=False)
        assert (h["status"] == E.L.FM_ST_FITTED).all() and (h["stat"][:, 2] == h["stat"][:, 0]).all()    # G_f = N
        off = int(fe)
        for k in range(3):
            white, firm = h["cov"][k, 1, off:, off:], h["cov"][k, 3, off:, off:]
            sc = np.sqrt(np.outer(np.diag(white), np.diag(white)))
            assert (np.abs(firm - white) <= RTOL * np.maximum(np.abs(white), sc)).all(), (fe, k)


def test_one_month_panel(E, parity_data):
    d0 = parity_data[0]
    a, b = int(d0["seg_off"][3]), int(d0["seg_off"][4])
    d = dict(cols=[c[a:b] for c in d0["cols"]], seg_off=np.array([0, b - a], dtype=np.int64), ids=d0["ids"][a:b],
             level=d0["level"][a:b])
    d["firm"] = PO._codes(d["ids"])
    for fe in (False, True):
        res, h = _run(E, d, PO.PARITY_MODELS, month_fe=fe)
        refs = PO.pooled_all(d, PO.PARITY_MODELS, month_fe=fe)
        off = int(fe)
        for k in range(3):
            assert h["status"][k] == E.L.FM_ST_FITTED == refs[k]["status"] and h["stat"][k, 1] == 1
            assert np.isnan(h["se"][k, 2]).all() and np.isnan(h["se"][k, 4]).all()
            assert np.isfinite(h["se"][k, [0, 1, 3], off:]).all()
            assert_series_close(h["se"][k, [0, 1, 3]].ravel(), refs[k]["se"][[0, 1, 3]].ravel(), "one month: se", RTOL)


EDGE_LENS = (0, 1, 63, 64, 65, 255, 256, 257, 300)               # round the wave tile (64) and the block (256)
EDGE_MODELS = [(14, (0,), (0, 1, 2)), (14, tuple(range(7)), (0, 1, 2)), (14, tuple(range(14)), (0, 1, 2))]


def edge_panel(seed=29):
    """Nine months of EDGE_LENS rows, 15 columns with 5 % NaN, levels 0 .. 2, ascending firm ids."""
    rng = np.random.default_rng(seed)
    n = sum(EDGE_LENS)
    cols = [np.where(rng.random(n) < 0.05, np.nan, rng.normal(size=n)) for _ in range(15)]
    return dict(cols=cols, seg_off=np.concatenate([[0], np.cumsum(EDGE_LENS)]).astype(np.int64),
                ids=np.concatenate([np.arange(m, dtype=np.int64) * 3 + 7 for m in EDGE_LENS]),
                level=rng.integers(0, 3, size=n).astype(np.uint8))


def test_wls_and_pool_count_the_same_rows(E):
    """fm_wls and fm_pool read a problem's width, columns and month rows through the same helpers: with
    unit weights and no cuts both count exactly the rows a numpy mask counts (level >= u and no NaN
    among the problem's columns), per month and in all, at every edge of the 64-row tile and the
    256-row block and for K = 1, 7 and 14."""
    d = edge_panel()
    panel, models = _panel(E, d), _models(E, EDGE_MODELS)
    level = _dev(E, d["level"])
    T, n = len(EDGE_LENS), int(d["seg_off"][-1])
    month = np.repeat(np.arange(T), EDGE_LENS)
    want = []                                                      # [problem][month] used rows
    for mi, u, _ in PO.problems(EDGE_MODELS):
        y, xs, _ = EDGE_MODELS[mi]
        use = d["level"] >= u
        for c in list(xs) + [y]:
            use &= ~np.isnan(d["cols"][c])
        want.append(np.bincount(month[use], minlength=T))
    want = np.array(want, dtype=np.int64)
    assert want.shape == (9, T) and (want[:, 0] == 0).all() and (want[:, 2:].sum(axis=1) > 0).all()
    assert len({tuple(w) for w in want}) == 9                      # every problem counts its own rows
    wls = E.fm_pass_wls(panel, models, weight=torch.ones(n, dtype=torch.float64, device=level.device), level=level,
                        nlevels=3)
    torch.cuda.synchronize()
    assert [(p.model, p.level, p.K) for p in wls.problems] == PO.problems(EDGE_MODELS) and wls.pmax == 15
    nt = wls.rec.cpu().numpy()[:, :, wls.pmax + 1]                 # [T, nprob]
    assert np.array_equal(nt, want.T.astype(np.float64))
    for fe in (False, True):
        res, h = _run(E, d, EDGE_MODELS, panel=panel, month_fe=fe, cov=False, resid=False)
        assert res.pmax == wls.pmax
        for p in range(9):
            w = (fe, p)
            assert int(nt[:, p].sum()) == int(h["stat"][p, 0]) == int(want[p].sum()), w
            assert int((nt[:, p] > 0).sum()) == int(h["stat"][p, 1]) == int((want[p] > 0).sum()), w
            assert h["stat"][p, 0] == np.floor(h["stat"][p, 0]) and h["stat"][p, 1] == np.floor(h["stat"][p, 1]), w


# ---------------------------------------------------------------- 3. the checker panel

def test_checker_panel_exact(E):
    d = PO.checker_panel()
    res, h = _run(E, d, PO.CHECKER_MODELS)
    assert int(h["status"][0]) == E.L.FM_ST_FITTED | E.L.FM_ST_NEG_VAR
    assert h["coef"][0].tobytes() == np.array([1.0, 2.0]).tobytes()
    w = np.sqrt(np.float64(1) / np.float64(14))
    assert h["se"][0, 1].tobytes() == np.array([w, w]).tobytes()
    assert h["se"][0, 2].tobytes() == np.zeros(2).tobytes() and h["se"][0, 3].tobytes() == np.zeros(2).tobytes()
    assert np.isnan(h["se"][0, 4]).all()
    assert list(h["stat"][0, :3]) == [16, 4, 4] and h["stat"][0, 4] == 16.0
    assert list(np.diag(h["cov"][0, 4])) == [-1 / 14, -1 / 14]


# ---------------------------------------------------------------- 4. firm-block edges
@pytest.mark.parametrize("which", ["B-1", "B", "B+1", "2B+1"])
def test_firm_block_edges(E, which):
    B = E.L.FM_POOL_FIRM_BLOCK
    nf = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1}[which]
    d = PO.block_panel(nf, B)
    for fe in (False, True):
        refs = PO.pooled_all(d, PO.BLOCK_MODELS, month_fe=fe)
        PO.assert_benign(refs[0])
        res, h = _run(E, d, PO.BLOCK_MODELS, month_fe=fe)
        _assert_close(h, refs, f"block panel nfirms={nf} fe={fe}")


# ---------------------------------------------------------------- 5. the order contract
def _bits(h, k=slice(None), rows=slice(None)):
    return [h[n][k].tobytes() for n in ("coef", "se", "cov", "stat", "status")] + [h["resid"][k][..., rows].tobytes()]


TWO_MODELS = PO.PARITY_MODELS + [(PO.PARITY_Y, (9, 3), (0, 2))]


@pytest.mark.parametrize("month_fe", [False, True])
def test_bit_identities(E, parity_data, month_fe):
    d, (lo, hi) = parity_data
    kw = dict(cuts=(lo, hi), month_fe=month_fe)
    res, h = _run(E, d, PO.PARITY_MODELS, **kw)
    assert (h["status"] == E.L.FM_ST_FITTED).all()
    # a repeat
    assert _bits(_run(E, d, PO.PARITY_MODELS, **kw)[1]) == _bits(h)
    # a problem alone or in a batch (the batch's pmax is the same: K = 3 is its widest model)
    res2, h2 = _run(E, d, TWO_MODELS, **kw)
    assert res2.nprob == 5 and res2.pmax == res.pmax
    assert _bits(h2, slice(0, 3)) == _bits(h)
    one = [(PO.PARITY_Y, PO.PARITY_XS, (1,))]
    assert _bits(_run(E, d, one, **kw)[1]) == _bits(h, slice(1, 2))
    # firm ids relabelled by an increasing map: the same codes
    ids2 = d["ids"] * 3 + 1000
    p2 = _panel(E, d, ids=ids2)
    assert torch.equal(E.firm_codes(p2)[0].cpu(), torch.from_numpy(d["firm"])) and E.firm_codes(p2)[1] == d["nfirms"]
    assert _bits(_run(E, d, PO.PARITY_MODELS, panel=p2, **kw)[1]) == _bits(h)
    # [seg_lo, seg_hi) of the panel against a panel of those months alone, the firm codes kept
    s0, s1 = 2, 7
    a, b = int(d["seg_off"][s0]), int(d["seg_off"][s1])
    full, hf = _run(E, d, PO.PARITY_MODELS, seg_lo=s0, seg_hi=s1, **kw)
    assert (hf["status"] == E.L.FM_ST_FITTED).all() and np.isnan(hf["resid"][:, :a]).all() and np.isnan(hf["resid"][:, b:]).all()
    sub = dict(cols=[c[a:b] for c in d["cols"]], seg_off=d["seg_off"][s0:s1 + 1] - a, ids=d["ids"][a:b],
               level=d["level"][a:b])
    firm = (_dev(E, d["firm"][a:b]), d["nfirms"])
    hs = _run(E, sub, PO.PARITY_MODELS, cuts=(lo[:, s0:s1], hi[:, s0:s1]), month_fe=month_fe, firm=firm)[1]
    assert _bits(hs) == _bits(hf, rows=slice(a, b))
    assert hf["stat"][0, 0] < h["stat"][0, 0]


# ---------------------------------------------------------------- 6. status
def _small(n_per_month, K, seed=3):
    rng = np.random.default_rng(seed)
    n = sum(n_per_month)
    ids = np.concatenate([np.arange(m, dtype=np.int64) * 2 + 5 for m in n_per_month])
    return dict(cols=[rng.normal(size=n) for _ in range(K + 1)],
                seg_off=np.concatenate([[0], np.cumsum(n_per_month)]).astype(np.int64), ids=ids, level=None)


def _fitted(E, h):
    """FITTED and nothing but, FM_ST_NEG_VAR apart (two month clusters can leave a two-way variance below 0)."""
    return int(h["status"][0]) & ~E.L.FM_ST_NEG_VAR == E.L.FM_ST_FITTED and np.isfinite(h["coef"][0, :4]).all()


def _failed(E, h, st, N):
    assert int(h["status"][0]) == st and h["stat"][0, 0] == N
    assert np.isnan(h["coef"]).all() and np.isnan(h["se"]).all() and np.isnan(h["cov"]).all()


def test_status_rules(E):
    L = E.L
    m3 = [(3, (0, 1, 2), (0,))]
    d = _small([2, 2], 3)                                         # N = K + 1 under the intercept model
    _failed(E, _run(E, d, m3)[1], L.FM_ST_SKIPPED, 4)
    d5 = _small([3, 2], 3)                                        # N = K + 2 is fitted
    assert _fitted(E, _run(E, d5, m3)[1])
    _failed(E, _run(E, d5, m3, month_fe=True)[1], L.FM_ST_SKIPPED, 5)     # dof = 5 - 3 - 2 < 1
    for col, bit in ((1, L.FM_ST_INF_IN_X), (3, L.FM_ST_INF_IN_Y)):
        d = _small([20, 30], 3)
        d["cols"][col][7] = np.inf
        _failed(E, _run(E, d, m3)[1], bit, 50)
        lo, hi = np.full((4, 2), -2.0), np.full((4, 2), 2.0)      # clipped away: fitted
        assert _fitted(E, _run(E, d, m3, cuts=(lo, hi))[1])
    d = _small([20, 30], 3)
    d["cols"][0][-1] = -np.inf
    d["cols"][3][0] = np.inf
    _failed(E, _run(E, d, m3)[1], L.FM_ST_INF_IN_X | L.FM_ST_INF_IN_Y, 50)
    for fe in (False, True):
        d = _small([20, 30], 3)
        d["cols"][1][:] = 4.25                                    # a constant predictor
        _failed(E, _run(E, d, m3, month_fe=fe)[1], L.FM_ST_RANK_DEF, 50)
        d = _small([20, 30], 3)
        d["cols"][2] = 2.0 * d["cols"][0] - 0.5 * d["cols"][1]    # collinear
        _failed(E, _run(E, d, m3, month_fe=fe)[1], L.FM_ST_RANK_DEF, 50)
    d = _small([20, 30], 3)                                       # constant within every month: rank deficient under FE alone
    d["cols"][1][:20], d["cols"][1][20:] = 1.0, 2.0
    assert _fitted(E, _run(E, d, m3)[1])
    _failed(E, _run(E, d, m3, month_fe=True)[1], L.FM_ST_RANK_DEF, 50)


def test_bad_firm_codes_and_empty_range(E):
    d = _small([20, 30], 3)
    m3 = [(3, (0, 1, 2), (0,))]
    panel = _panel(E, d)
    codes = PO._codes(d["ids"])
    for bad in (codes[::-1].copy(), np.where(np.arange(50) == 4, codes[3], codes), codes + 40, codes - 1):
        with pytest.raises(ValueError, match="firm code"):
            _run(E, d, m3, panel=panel, firm=(_dev(E, bad.astype(np.int32)), 30))
        torch.cuda.synchronize()
    with pytest.raises(ValueError, match="firm ids"):
        E.firm_codes(E.DevicePanel(cols=panel.cols, names=panel.names, seg_off=panel.seg_off, seg_off_h=panel.seg_off_h))
    res, h = _run(E, d, m3, panel=panel, seg_lo=1, seg_hi=1)     # an empty month range: nothing is fitted
    assert not int(h["status"][0]) & E.L.FM_ST_FITTED and np.isnan(h["coef"]).all() and np.isnan(h["resid"]).all()
    res, h = _run(E, d, m3, panel=panel)
    assert _fitted(E, h)
    assert E.time_launch("fm_pool", reps=2) > 0.0


# ---------------------------------------------------------------- 7. end to end
@pytest.fixture(scope="module")
def golden_frame():
    import cases
    from fmtol import frame_from, load_npz
    return frame_from(load_npz("fm.npz"), "in_"), cases


def _oracle_of_frame(frame, xs, **kw):
    f = frame.sort_values(["mthcaldt", "permno"])
    seg = np.concatenate([[0], np.cumsum(f.groupby("mthcaldt", sort=True).size().to_numpy())]).astype(np.int64)
    cols = [f[c].to_numpy(dtype=np.float64) for c in list(xs) + ["retx"]]
    return PO.pooled(cols, seg, PO._codes(f["permno"].to_numpy()), len(xs), list(range(len(xs))), **kw)


@pytest.mark.parametrize("month_fe", [False, True])
def test_pipeline_equals_the_direct_call(E, golden_frame, month_fe):
    from fmcore import lewellen as LW
    from fmdrop import calc_Lewellen_2014 as CL
    df, cases = golden_frame
    panel, model_cols = CL._pipeline_panel(df, cases.VARIABLES_DICT)
    cfg = LW.PipelineConfig(forecasts=False, pooled=True, pooled_month_fe=month_fe, pooled_small_sample=not month_fe)
    out = LW.run_pipeline(panel, cfg, model_cols=model_cols)
    assert LW.run_pipeline(panel, LW.PipelineConfig(forecasts=False), model_cols=model_cols).pooled is None
    models, _ = LW.build_models(panel, model_cols, fig1=True, universes=True)
    direct = E.pooled_regressions(panel, models, level=out.level, nlevels=3, cuts=out.cuts, month_fe=month_fe,
                                  small_sample=not month_fe)
    torch.cuda.synchronize()
    assert [(p.model, p.level, p.K) for p in out.pooled.problems] == [(p.model, p.level, p.K) for p in out.res.problems]
    assert max(p.K for p in direct.problems) == E.L.FM_POOL_MAX_K          # Model 3: the widest model the tile takes
    for name in ("coef", "se", "stat", "status"):
        assert getattr(out.pooled, name).cpu().numpy().tobytes() == getattr(direct, name).cpu().numpy().tobytes(), name
    assert (out.pooled.status.cpu().numpy() & E.L.FM_ST_FITTED).all()


def test_drop_in_against_restatement(E, golden_frame):
    from fmdrop import calc_Lewellen_2014 as CL
    from fmdrop import regressions as R
    df, cases = golden_frame
    subs = CL.get_subsets(CL.winsorize(df, cases.WINSOR_VARS, 1, 99))
    xs = cases.MODELS["M1"]
    for fe in (False, True):
        frame = subs["Large stocks"].sample(frac=1.0, random_state=2)            # any row order
        got = R.run_pooled_regression(frame, "retx", xs, month_fe=fe)
        ref = _oracle_of_frame(frame, xs, month_fe=fe)
        assert ref["status"] & PO.FITTED and ref["cond"] < 100
        assert list(got.index) == ["const"] + xs
        assert list(got.columns) == ["coef"] + [f"se_{k}" for k in PO.KINDS] + [f"t_{k}" for k in PO.KINDS]
        assert got.attrs["N"] == ref["N"] and got.attrs["n_months"] == ref["Gt"] and got.attrs["n_firms"] == ref["Gf"]
        assert scalar_close(got.attrs["r2"], ref["stat"][3], RTOL)
        assert_series_close(got["coef"].to_numpy(), ref["coef"], "drop-in coef", RTOL)
        white = np.diag(ref["cov"][1])
        for k, kind in enumerate(PO.KINDS):
            v, want = got[f"se_{kind}"].to_numpy() ** 2, ref["se"][k] ** 2
            assert np.array_equal(np.isnan(v), np.isnan(want)), kind
            ok = ~np.isnan(want)
            assert (np.abs(v - want)[ok] <= RTOL * np.maximum(np.abs(want), white)[ok]).all(), kind
            with np.errstate(invalid="ignore"):
                assert np.array_equal(got[f"t_{kind}"].to_numpy(), got["coef"].to_numpy() / got[f"se_{kind}"].to_numpy(),
                                      equal_nan=True)


def test_build_table_2_pooled(E, golden_frame):
    from fmdrop import calc_Lewellen_2014 as CL
    df, cases = golden_frame
    subs = CL.get_subsets(CL.winsorize(df, cases.WINSOR_VARS, 1, 99))
    t2 = CL.build_table_2(subs, cases.VARIABLES_DICT)
    tp = CL.build_table_2_pooled(subs, cases.VARIABLES_DICT)
    assert list(tp.index) == [i for i in t2.index if i[1] != "N"]
    fmt = lambda v: "" if np.isnan(v) else f"{v:.3f}"  # noqa: E731  (build_table_2 leaves a NaN cell empty)
    for s in cases.SUBSETS:
        # the FM columns are build_table_2's numbers
        assert [fmt(v) for v in tp[(s, "FM slope")]] == [t2.loc[i, (s, "Slope")] for i in tp.index], s
        assert [fmt(v) for v in tp[(s, "FM t")]] == [t2.loc[i, (s, "t-stat")] for i in tp.index], s
        assert np.isfinite(tp[(s, "Pooled slope")].to_numpy()).all() and np.isfinite(tp[(s, "FM slope")].to_numpy()).sum() > 20
    inv = {v: k for k, v in cases.VARIABLES_DICT.items()}
    names = list(dict.fromkeys(tp.index.get_level_values(0)))
    assert len(names) == 3
    for mname, model in zip(("M1", "M2"), names):
        xs = cases.MODELS[mname]
        for s in ("All stocks", "Large stocks"):
            ref = _oracle_of_frame(subs[s], xs)
            assert ref["status"] & PO.FITTED and ref["cond"] < 1e4
            rows = [(model, inv[x]) for x in xs]
            slope = tp.loc[rows, (s, "Pooled slope")].to_numpy()
            assert_series_close(slope, ref["coef"][1:], f"{mname} {s} slope", RTOL)
            white = np.diag(ref["cov"][1])[1:]
            for kind, k in (("white", 1), ("month", 2), ("firm", 3), ("twoway", 4)):
                t = tp.loc[rows, (s, f"t {kind}")].to_numpy()
                want = ref["se"][k, 1:] ** 2
                assert np.array_equal(np.isnan(t), np.isnan(want)), (mname, s, kind)
                ok = ~np.isnan(want)
                var = (slope / t) ** 2                         # the table's t is its slope over its se
                assert (np.abs(var - want)[ok] <= RTOL * np.maximum(want, white)[ok]).all(), (mname, s, kind)
