"""GPU tests of the k-month holding of the sorted portfolios (fm_portfolio_hold, engine.portfolio_hold,
engine.held_portfolios, PipelineConfig(portfolio_hold=k), the drop-in's held_sorted_portfolios and
build_table_5_held; build-defined A19) against the numpy restatement tests/hold_oracle.py: to the
bit on the integer-valued fixture, within the forward error bound of their own sums on real values.

The bound (U = 2^-53; the device and the oracle add the same float64 terms, the oracle in longdouble):
a sum of n terms carries at most (n - 1) U sum|x|, the oracle's rounding of its sum U |S|, the
division U |S / n| each side, so
  |ew - ew'| <= 1.01 (n + 3) U sum|ret| / n,
and with A = sum(w ret), B = sum(w) > 0 (both carry n U of themselves)
  |vw - vw'| <= 1.01 (2 n + 4) U sum|w ret| / sum(w);
the average of k cohort values adds their bounds / k and (k + 1) U sum|c_a| / k for its own k
operations on either side, the spread its two ends' bounds and U (|high| + |low|)."""
import gc

import numpy as np
import pytest
import torch

import alpha_oracle as AO
import hold_oracle as HO
import horizon_oracle as HZ

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
P = HO.HOLD_NPORT
HOLDS = (1, 3, 6, 12)
INT_OUTS = ("members", "stay", "cohort_n", "status")
F64_OUTS = ("cohort", "rec", "turnover")
GUARD = 64


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


@pytest.fixture(scope="module")
def fx():
    """The fixture, computed once and never written to."""
    p = HO.hold_panel()
    for v in p.values():
        v.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def expected(fx):
    """The oracle on the fixture at every tested k, computed once."""
    return {k: HO.portfolio_hold(fx["seg_off"], fx["month_index"], fx["link_prev"], fx["port"], fx["status"], fx["ret"],
                                 fx["weight"], P, k, fx["sort_rec"]) for k in HOLDS}


def _dev(E, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(E.require_device())


def _raw(E, seg_off, month_index, link, port, status, ret, weight, nport, k, sort_rec):
    """fm_portfolio_hold through the binding, every output pre-filled with a sentinel inside a buffer
    with GUARD more elements either side, which must come back untouched -> host dict."""
    L = E.L
    port = np.asarray(port).reshape(-1, len(ret))
    S, T, n = port.shape[0], len(seg_off) - 1, len(ret)
    ins = [_dev(E, x) for x in (seg_off, month_index, link, port, np.asarray(status, dtype=np.int32).reshape(S, T), ret,
                                weight, sort_rec)]
    shapes = dict(members=(S, T, k + 1, nport), stay=(S, T, k + 1, nport), cohort_n=(S, T, k, nport, 2),
                  cohort=(S, T, k, nport, 2), status=(S, T), rec=(S, T, nport + 1, 4), turnover=(S, T, nport))
    bufs = {}
    for name, sh in shapes.items():
        f64 = name in F64_OUTS
        bufs[name] = torch.full((int(np.prod(sh)) + 2 * GUARD,), 1e300 if f64 else -77,
                                dtype=torch.float64 if f64 else torch.int32, device=ins[0].device)
    ptr = {name: b[GUARD:].data_ptr() for name, b in bufs.items()}
    a = L.HoldArgs(seg_off=ins[0].data_ptr(), month_index=ins[1].data_ptr(), link_prev=ins[2].data_ptr(),
                   port=ins[3].data_ptr(), status=ins[4].data_ptr(), ret=ins[5].data_ptr(),
                   weight=None if ins[6] is None else ins[6].data_ptr(),
                   sort_rec=None if ins[7] is None else ins[7].data_ptr(), nrows=n, nseg=T, nsel=S, nport=nport, hold=k,
                   members=ptr["members"], stay=ptr["stay"], cohort_n=ptr["cohort_n"], cohort=ptr["cohort"],
                   status_out=ptr["status"], rec=ptr["rec"], turnover=ptr["turnover"])
    L.call("fm_portfolio_hold", L.C.byref(a), E._stream())
    torch.cuda.synchronize()
    out = {}
    for name, sh in shapes.items():
        h = bufs[name].cpu().numpy()
        sent = 1e300 if name in F64_OUTS else -77
        assert np.all(h[:GUARD] == sent) and np.all(h[-GUARD:] == sent), f"{name}: a guard element was written"
        body = h[GUARD:-GUARD]
        assert not np.any(body == sent), f"{name}: an element was not written"
        out[name] = body.reshape(sh).copy()
    return out


def _raw_fx(E, fx, k, sorts=slice(None), weight=True, sort_rec=True, link=None, ret=None, w=None):
    return _raw(E, fx["seg_off"], fx["month_index"], fx["link_prev"] if link is None else link, fx["port"][sorts],
                fx["status"][sorts], fx["ret"] if ret is None else ret,
                (fx["weight"] if w is None else w) if weight else None, P, k, fx["sort_rec"][sorts] if sort_rec else None)


def _same(got, exp, what, sorts=slice(None)):
    for name in INT_OUTS:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], exp[name][sorts]), (what, name)
    for name in F64_OUTS:
        HZ.assert_same_bits(got[name], exp[name][sorts], f"{what} {name}")


def _same_bytes(a, b, what):
    for name in INT_OUTS + F64_OUTS:
        assert a[name].tobytes() == b[name].tobytes(), (what, name)


def _within_bounds(got, exp, cnt, mag, k, what):
    """The integer outputs exactly; cohort and rec columns 0 and 2 within the bound of the module docstring."""
    for name in INT_OUTS:
        assert np.array_equal(got[name], exp[name]), (what, name)
    n0, n1 = cnt[..., 0].astype(np.float64), cnt[..., 1].astype(np.float64)
    b = np.zeros(exp["cohort"].shape)
    b[..., 0] = 1.01 * (n0 + 3) * U * mag[..., 0] / np.maximum(n0, 1)
    b[..., 1] = 1.01 * (2 * n1 + 4) * U * mag[..., 1] / np.where(mag[..., 2] > 0, mag[..., 2], 1.0)
    worst = 0.0
    for name, bound in (("cohort", b), ("rec", None)):
        g, e = got[name], exp[name]
        if bound is None:
            bound = np.zeros(e.shape)
            c = np.nan_to_num(np.abs(exp["cohort"]))
            for w in (0, 1):
                rb = b[..., w].sum(axis=2) / k + 1.01 * (k + 1) * U * c[..., w].sum(axis=2) / k      # [S, T, P]
                bound[:, :, :P, 2 * w] = rb
                with np.errstate(invalid="ignore"):
                    ends = np.abs(e[:, :, P - 1, 2 * w]) + np.abs(e[:, :, 0, 2 * w])
                bound[:, :, P, 2 * w] = rb[:, :, P - 1] + rb[:, :, 0] + 1.01 * U * np.nan_to_num(ends)
            g, e, bound = g[..., ::2], e[..., ::2], bound[..., ::2]
        assert np.array_equal(np.isnan(g), np.isnan(e)), (what, name, "NaN masks differ")
        ok = ~np.isnan(e)
        assert ok.sum() > 100 and np.all(np.isfinite(e[ok]))
        err = np.abs(g[ok] - e[ok])
        assert np.all(err <= bound[ok]), (what, name, float((err / np.maximum(bound[ok], 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound[ok], 1e-300)).max()))
    print(f"{what}: worst error / bound = {worst:.3f}")
    HZ.assert_same_bits(got["turnover"], exp["turnover"], f"{what} turnover")
    HZ.assert_same_bits(got["rec"][..., 1::2], exp["rec"][..., 1::2], f"{what} predicted columns")


# ---------------------------------------------------------------- 1. the fixture, to the bit
@pytest.mark.parametrize("k", HOLDS)
def test_fixture_matches_the_oracle_to_the_bit(E, fx, expected, k):
    got = _raw_fx(E, fx, k)
    _same(got, expected[k], f"k={k}")
    _same_bytes(_raw_fx(E, fx, k), got, f"k={k}: a second call")
    _same(_raw_fx(E, fx, k, sorts=slice(1, 2)), expected[k], f"k={k}: sort 1 alone", sorts=slice(1, 2))
    # the engine entry point: the same launch into its own tensors
    h = E.portfolio_hold(*(_dev(E, fx[x]) for x in ("seg_off", "month_index", "link_prev", "port", "status", "ret")),
                         weight=_dev(E, fx["weight"]), nport=P, hold=k, sort_rec=_dev(E, fx["sort_rec"]))
    torch.cuda.synchronize()
    assert h.hold == k and h.status.dtype == torch.int32 and h.rec.shape == (3, 32, P + 1, 4)
    _same_bytes({x: getattr(h, x).cpu().numpy() for x in INT_OUTS + F64_OUTS}, got, f"k={k}: engine")


def test_without_weights_and_without_sort_records(E, fx, expected):
    k = 3
    got = _raw_fx(E, fx, k, weight=False, sort_rec=False)
    exp = HO.portfolio_hold(fx["seg_off"], fx["month_index"], fx["link_prev"], fx["port"], fx["status"], fx["ret"], None,
                            P, k, None)
    _same(got, exp, "no weight, no sort_rec")
    assert np.all(got["cohort_n"][..., 1] == 0) and np.all(np.isnan(got["cohort"][..., 1]))
    assert np.all(np.isnan(got["rec"][..., 1:])) and np.isfinite(got["rec"][..., 0]).sum() > 200
    for name in ("members", "stay", "turnover", "status"):
        assert got[name].tobytes() == expected[k][name].tobytes(), name
    HZ.assert_same_bits(got["cohort"][..., 0], expected[k]["cohort"][..., 0], "ew cohorts")
    # an unbatched call (port [rows], status [T]) returns unbatched tensors
    h = E.portfolio_hold(_dev(E, fx["seg_off"]), _dev(E, fx["month_index"]), _dev(E, fx["link_prev"]),
                         _dev(E, fx["port"][2]), _dev(E, fx["status"][2]), _dev(E, fx["ret"]), nport=P, hold=k)
    torch.cuda.synchronize()
    assert h.rec.shape == (32, P + 1, 4) and h.members.shape == (32, k + 1, P) and h.turnover.shape == (32, P)
    assert h.members.cpu().numpy().tobytes() == got["members"][2].tobytes()
    HZ.assert_same_bits(h.rec.cpu().numpy(), got["rec"][2], "unbatched rec")


@pytest.mark.parametrize("nport,k,nsort", [(20, 36, 2), (2, 2, 16), (7, 13, 5)])
def test_the_ends_of_the_ranges(E, fx, nport, k, nsort):
    """FM_MAX_PORTS x FM_MAX_HOLD (one sort's bins beyond the default LDS limit, a batch per sort), two
    portfolios with FM_MAX_SORTS sorts (eight sorts a wave pass, two passes), and sizes that divide
    nothing; k = 36 has no complete month here, its counts and cohorts are compared all the same."""
    rng = np.random.default_rng(100 * nport + k)
    n, T = len(fx["ret"]), len(fx["seg_off"]) - 1
    port = rng.integers(0, nport, (nsort, n)).astype(np.uint8)
    port[rng.random((nsort, n)) < 0.05] = 255
    port[:, :3] = nport                      # a byte >= nport below 255: in no portfolio either
    status = np.ones((nsort, T), dtype=np.int32)
    status[:, np.diff(fx["seg_off"]) < nport] = 0
    srec = rng.normal(0.01, 0.02, (nsort, T, nport + 1, 4))
    args = (fx["seg_off"], fx["month_index"], fx["link_prev"], port, status, fx["ret"], fx["weight"], nport, k, srec)
    got, exp = _raw(E, *args), HO.portfolio_hold(*args[:7], nport=nport, hold=k, sort_rec=srec)
    _same(got, exp, f"nport={nport} k={k}")
    assert got["members"][:, :, min(k, 12)].sum() > 0 and (exp["status"].sum() > 0) == (k <= 13)


def test_empty_calls(E):
    """No rows (three empty months), and no months: nothing is launched, the outputs are what a launch
    would have written."""
    dev = E.require_device()
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    h = E.portfolio_hold(z(4, torch.int64), _dev(E, np.array([5, 6, 7], dtype=np.int32)), z(0, torch.int32),
                         z((2, 0), torch.uint8), z((2, 3), torch.int32), z(0, torch.float64), nport=P, hold=2)
    torch.cuda.synchronize()
    assert h.rec.shape == (2, 3, P + 1, 4) and bool(torch.isnan(h.rec).all()) and bool(torch.isnan(h.turnover).all())
    assert bool(torch.isnan(h.cohort).all()) and h.cohort.shape == (2, 3, 2, P, 2)
    for t in (h.members, h.stay, h.cohort_n, h.status):
        assert t.dtype == torch.int32 and int(t.abs().sum()) == 0
    h = E.portfolio_hold(z(1, torch.int64), z(0, torch.int32), z(0, torch.int32), z(0, torch.uint8), z(0, torch.int32),
                         z(0, torch.float64), nport=P, hold=2)
    assert h.rec.shape == (0, P + 1, 4) and h.members.shape == (0, 3, P)


def test_engine_refuses_wrong_tensors(E, fx):
    t = {x: _dev(E, fx[x]) for x in ("seg_off", "month_index", "link_prev", "port", "status", "ret", "weight", "sort_rec")}

    def call(**kw):
        a = dict(t, nport=P, hold=3)
        a.update(kw)
        return E.portfolio_hold(a["seg_off"], a["month_index"], a["link_prev"], a["port"], a["status"], a["ret"],
                                weight=a["weight"], nport=a["nport"], hold=a["hold"], sort_rec=a["sort_rec"])

    for kw, text in ((dict(seg_off=t["seg_off"].int()), "seg_off must be"), (dict(month_index=t["month_index"][:-1]), "month_index must be"),
                     (dict(link_prev=t["link_prev"].long()), "link_prev must be"), (dict(port=t["port"][:, :-1]), "port must be"),
                     (dict(status=t["status"][:2]), "status must be"), (dict(weight=t["weight"].float()), "weight must be"),
                     (dict(sort_rec=t["sort_rec"][:, :, :P]), "sort_rec must be"), (dict(ret=t["ret"].cpu()), "must be"),
                     (dict(nport=1), "nport must be 2..20"), (dict(hold=0), "hold must be 1..36"),
                     (dict(hold=37), "hold must be 1..36")):
        with pytest.raises(ValueError, match=text):
            call(**kw)


# ---------------------------------------------------------------- 2. real values, within the bound
@pytest.mark.parametrize("k", [1, 6])
def test_real_values_within_the_forward_error_bound(E, fx, k):
    ret, w = HO.real_values(fx)
    got = _raw_fx(E, fx, k, ret=ret, w=w)
    exp = HO.portfolio_hold(fx["seg_off"], fx["month_index"], fx["link_prev"], fx["port"], fx["status"], ret, w, P, k,
                            fx["sort_rec"])
    cnt, mag = HO.sum_bounds(fx["seg_off"], fx["link_prev"], fx["port"], ret, w, P, k)
    assert np.array_equal(cnt, exp["cohort_n"])
    _within_bounds(got, exp, cnt, mag, k, f"real values k={k}")


def test_months_of_any_length(E):
    """horizon_oracle.edge_panel: a 20,000-row month, an empty month, gaps in the calendar."""
    p = HZ.edge_panel()
    rng = np.random.default_rng(12)
    n, T, k = len(p["ret"]), len(p["seg_off"]) - 1, 3
    link = HZ.month_links(p["ids"], p["seg_off"], p["month_index"], -1)
    port = rng.integers(0, P, (2, n)).astype(np.uint8)
    port[rng.random((2, n)) < 0.1] = 255
    status = np.ones((2, T), dtype=np.int32)
    status[:, np.diff(p["seg_off"]) < P] = 0
    w = np.exp(rng.normal(5.0, 2.0, n))
    w[rng.random(n) < 0.01] = np.nan
    got = _raw(E, p["seg_off"], p["month_index"], link, port, status, p["ret"], w, P, k, None)
    exp = HO.portfolio_hold(p["seg_off"], p["month_index"], link, port, status, p["ret"], w, P, k, None)
    cnt, mag = HO.sum_bounds(p["seg_off"], link, port, p["ret"], w, P, k)
    assert exp["members"][:, 13, 0].min() > 3000 and exp["members"][:, 13, k].min() > 100   # the 20,000-row month
    assert exp["status"].sum() >= 2 * 5
    _within_bounds(got, exp, cnt, mag, k, "edge panel")


def test_stale_links_fault_nothing(E, fx, expected):
    """Links of another panel, with entries far beyond the months' lengths and the int32 range's ends:
    every hop with a bad link is missing, as in the oracle."""
    e = HZ.edge_panel()
    n = len(fx["ret"])
    link = HZ.month_links(e["ids"], e["seg_off"], e["month_index"], -1)[-n:].copy()
    assert (link >= 2100).sum() > 1000            # beyond the fixture's longest month
    link[::97] = np.iinfo(np.int32).max
    link[5::101] = np.iinfo(np.int32).min
    link[7::89] = n
    for k in (1, 6):
        got = _raw_fx(E, fx, k, link=link)
        exp = HO.portfolio_hold(fx["seg_off"], fx["month_index"], link, fx["port"], fx["status"], fx["ret"],
                                fx["weight"], P, k, fx["sort_rec"])
        _same(got, exp, f"stale links k={k}")
        assert got["members"][:, :, 0].tobytes() == expected[k]["members"][:, :, 0].tobytes()
        assert got["members"][:, :, 1:].sum() < expected[k]["members"][:, :, 1:].sum()


# ---------------------------------------------------------------- 3. the sort that exists
def test_one_month_holding_is_the_sort(E, fx):
    rng = np.random.default_rng(2)
    n = len(fx["ret"])
    F = rng.integers(-50, 51, n) / 8.0
    F[rng.random(n) < 0.05] = np.nan
    panel = E.DevicePanel(cols=torch.stack([_dev(E, fx["ret"]), _dev(E, F)]), names=["retx", "forecast"],
                          seg_off=_dev(E, fx["seg_off"]), seg_off_h=np.array(fx["seg_off"]),
                          months=np.array(fx["month_index"]), ids=_dev(E, fx["ids"]),
                          month_index=np.array(fx["month_index"]))
    w = _dev(E, fx["weight"])
    ports = E.portfolio_sort(panel.seg_off, panel.cols[1], panel.cols[0], weight=w, nport=P)
    held = E.held_portfolios(panel, ports, 1, ret="retx", weight=w)
    torch.cuda.synchronize()
    assert np.array_equal(E.month_links(panel, -1).cpu().numpy(), fx["link_prev"])
    rec, hrec = ports.rec.cpu().numpy(), held.rec.cpu().numpy()
    assert ports.status.cpu().numpy().sum() == 29
    assert np.array_equal(held.status.cpu().numpy(), ports.status.cpu().numpy())
    HZ.assert_same_bits(hrec[..., 0], rec[..., 0], "ew return")
    HZ.assert_same_bits(hrec[..., 2], rec[..., 2], "vw return")
    HZ.assert_same_bits(hrec[..., 1::2], rec[..., 1::2], "predicted columns")
    assert np.array_equal(held.cohort_n.cpu().numpy()[:, 0, :, 0], ports.cnt.cpu().numpy())
    Fa = _dev(E, np.random.default_rng(4).normal(0.005, 0.04, (32, 3)))
    a, b = E.portfolio_alphas(held, Fa, nw_lags=2), E.portfolio_alphas(ports, Fa, nw_lags=2)
    torch.cuda.synchronize()
    for name in AO.OUTS:
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    assert np.isfinite(a.coef.cpu().numpy()[..., 0]).sum() >= 2 * (P + 1)
    s, hs = E.portfolio_summary(ports), E.portfolio_summary(held)
    assert s.mean.cpu().numpy()[:, ::2].tobytes() == hs.mean.cpu().numpy()[:, ::2].tobytes()
    with pytest.raises(ValueError, match="carries no firm ids"):
        panel.ids = None
        E.held_portfolios(panel, ports, 1)


# ---------------------------------------------------------------- 4. the pipeline
PIPE = dict(T=100, N=300, seed=21, window=24, min_periods=12, nport=5, hold=3)


@pytest.fixture(scope="module")
def pipe(E):
    import pipe_port_oracle as PPO
    from fmcore import lewellen as LW, synth
    a = synth.synth_arrays(PIPE["T"], PIPE["N"], PIPE["seed"], nan_rate=0.02, present_rate=0.9)
    names, mc = PPO.pipeline_columns()
    panel = E.panel_from_arrays([a[c] for c in names], names, a["month"], me=a["me"], nyse=a["nyse"], ids=a["permno"])
    F = np.random.default_rng(8).normal(0.005, 0.04, (panel.nseg, 3))
    kw = dict(window=PIPE["window"], min_periods=PIPE["min_periods"], portfolios=PIPE["nport"])
    on = LW.run_pipeline(panel, LW.PipelineConfig(portfolio_hold=PIPE["hold"], alpha_factors=F, **kw), model_cols=mc)
    off = LW.run_pipeline(panel, LW.PipelineConfig(**kw), model_cols=mc)
    torch.cuda.synchronize()
    return dict(a=a, panel=panel, on=on, off=off, F=F)


def test_pipeline_against_the_oracle(E, pipe):
    out, panel, k, nport = pipe["on"], pipe["panel"], PIPE["hold"], PIPE["nport"]
    assert pipe["off"].held is None and pipe["off"].held_summary is None and pipe["off"].held_alphas is None
    h = out.held
    got = {x: getattr(h, x).cpu().numpy() for x in INT_OUTS + F64_OUTS}
    assert got["rec"].shape == (9, panel.nseg, nport + 1, 4) and h.hold == k
    # the oracle on the run's own port bytes, status, return column and me
    so, mi = panel.seg_off_h, panel.month_index
    link = HZ.month_links(panel.ids.cpu().numpy(), so, mi, -1)
    port, status = out.portfolios.port.cpu().numpy(), out.portfolios.status.cpu().numpy()
    ret, me = panel.cols[panel.col("retx")].cpu().numpy(), panel.me.cpu().numpy()
    srec = out.portfolios.rec.cpu().numpy()
    exp = HO.portfolio_hold(so, mi, link, port, status, ret, me, nport, k, srec)
    cnt, mag = HO.sum_bounds(so, link, port, ret, me, nport, k)
    assert exp["status"].sum(axis=1).min() >= 50
    assert nport == P
    _within_bounds(got, exp, cnt, mag, k, "pipeline")
    s, again = out.held_summary, E.portfolio_summary(h, 4)
    for x in ("mean", "se", "tstat", "nobs"):
        assert getattr(s, x).cpu().numpy().tobytes() == getattr(again, x).cpu().numpy().tobytes(), x
    assert out.held_alphas is not None and out.held_alphas.coef.shape == (9, nport + 1, 2, 2, 4)
    a2 = E.portfolio_alphas(h, _dev(E, pipe["F"]), nw_lags=4)
    assert out.held_alphas.coef.cpu().numpy().tobytes() == a2.coef.cpu().numpy().tobytes()
    assert np.isfinite(out.held_alphas.coef.cpu().numpy()[..., 0]).all()
    # nothing else moves
    for x in ("port", "rec", "cnt", "status", "bp"):
        assert getattr(out.portfolios, x).cpu().numpy().tobytes() == getattr(pipe["off"].portfolios, x).cpu().numpy().tobytes()
    assert out.portfolio_alphas.coef.cpu().numpy().tobytes() == \
        E.portfolio_alphas(out.portfolios, _dev(E, pipe["F"]), nw_lags=4).coef.cpu().numpy().tobytes()


def test_pipeline_refuses_a_panel_without_ids(E, pipe):
    from fmcore import lewellen as LW
    import dataclasses
    bare = dataclasses.replace(pipe["panel"], ids=None, month_index=None)
    with pytest.raises(ValueError, match="portfolio_hold needs a panel with firm ids"):
        LW.run_pipeline(bare, LW.PipelineConfig(portfolio_hold=3, portfolios=5))


# ---------------------------------------------------------------- 5. the drop-in
def test_held_sorted_portfolios_frame(E):
    import pandas as pd
    import port_oracle as PO
    from fmcore import synth
    from fmdrop import calc_Lewellen_2014 as CL
    df = synth.synth_frame(30, 120, 9, present_rate=0.9, shuffle=True)
    rng = np.random.default_rng(6)
    n, k, nport = len(df), 3, 5
    df["retx"] = rng.integers(-8, 9, n) / 64.0          # integer-valued: the frame is exact to the bit
    df.loc[df.index[rng.choice(n, 20, replace=False)], "retx"] = np.nan
    df["w"] = rng.integers(1, 200, n).astype(np.float64)
    f = rng.integers(-200, 201, n) / 16.0
    monthly, summary = CL.held_sorted_portfolios(df, f, k, weight_col="w", nport=nport)
    order = np.lexsort((df["permno"].to_numpy(), df["mthcaldt"].to_numpy()))
    d = df.iloc[order]
    months, counts = np.unique(d["mthcaldt"].to_numpy(), return_counts=True)
    so = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    mi = E.month_index(months)
    s = PO.portfolio_sort(so, f[order], d["retx"].to_numpy(), d["w"].to_numpy(), nport=nport)
    link = HZ.month_links(d["permno"].to_numpy().astype(np.int64), so, mi, -1)
    exp = HO.portfolio_hold(so, mi, link, s["port"][None], s["status"][None], d["retx"].to_numpy(), d["w"].to_numpy(),
                            nport, k, s["rec"][None])
    ok = exp["status"][0] == 1
    assert ok.sum() == len(months) - (k - 1)
    assert list(monthly.columns) == CL.PORTFOLIO_COLUMNS + ["n", "turnover"]
    assert monthly.index.names == ["mthcaldt", "portfolio"] and len(monthly) == ok.sum() * (nport + 1)
    assert list(monthly.index.get_level_values(0).unique()) == list(pd.DatetimeIndex(months[ok]))
    HZ.assert_same_bits(monthly[CL.PORTFOLIO_COLUMNS].to_numpy().reshape(-1, nport + 1, 4), exp["rec"][0, ok], "rec")
    m0 = exp["members"][0, ok, 0].astype(np.int64)
    assert np.array_equal(monthly["n"].to_numpy().reshape(-1, nport + 1), np.concatenate([m0, m0[:, :1] + m0[:, -1:]], axis=1))
    tv = monthly["turnover"].to_numpy().reshape(-1, nport + 1)
    HZ.assert_same_bits(tv[:, :nport], exp["turnover"][0, ok], "turnover")
    assert np.all(np.isnan(tv[:, nport])) and np.isfinite(tv[:, :nport]).sum() == (ok.sum() - 1) * nport
    assert list(summary.index) == list(range(nport)) + ["H-L"] and summary[("ew_ret", "nobs")].max() == ok.sum()
    with pytest.raises(ValueError, match="whole-number firm ids"):
        CL.held_sorted_portfolios(df.assign(permno=df["permno"] + 0.5), f, k)


def test_build_table_5_held(E):
    from fmcore import lewellen as LW, synth
    from fmdrop import calc_Lewellen_2014 as CL
    df = synth.synth_frame(40, 300, 5, present_rate=0.9, shuffle=True)
    frames = CL.build_table_5_held(df, 3, nport=5, window=12, min_periods=6)
    assert list(frames) == [(m, u) for m in LW.MODELS_PREDICTORS for u in LW.SUBSET_NAMES] and len(frames) == 9
    for monthly, summary in frames.values():
        assert list(monthly.columns) == CL.PORTFOLIO_COLUMNS + ["n", "turnover"]
        assert len(monthly) % 6 == 0 and len(monthly) >= 6 * 20 and np.isfinite(monthly["ew_ret"]).sum() > 100
        assert list(summary.index) == [0, 1, 2, 3, 4, "H-L"]
