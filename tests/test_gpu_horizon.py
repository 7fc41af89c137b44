"""GPU tests of the multi-month return horizons (extension A16; paper Section 4): fm_month_links and
fm_horizon_return against the numpy restatement (tests/horizon_oracle.py), exact to the bit, on a
hand-made panel of every tile shape; engine.horizon_panel; PipelineConfig(horizon=h) against a run on
a panel whose k-month column was built on the host; and the drop-in's horizon_returns."""
import dataclasses

import numpy as np
import pytest
import torch

import horizon_oracle as HO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


@pytest.fixture(scope="module")
def edge():
    """The hand-made panel with its oracle links, computed once and never written to."""
    p = HO.edge_panel()
    p["fwd"] = HO.month_links(p["ids"], p["seg_off"], p["month_index"], 1)
    p["bwd"] = HO.month_links(p["ids"], p["seg_off"], p["month_index"], -1)
    for v in p.values():
        v.setflags(write=False)
    return p


def _dev(E, a):
    return torch.from_numpy(np.array(a)).to(E.require_device())


def _raw_links(E, ids, seg_off, month_index, step):
    """fm_month_links through the binding -> (link, bad) on the host."""
    L = E.L
    t_ids, t_so, t_mi = _dev(E, ids), _dev(E, seg_off), _dev(E, month_index)
    link = torch.full((len(ids),), -77, dtype=torch.int32, device=t_ids.device)
    bad = torch.zeros(1, dtype=torch.int32, device=t_ids.device)
    a = L.LinksArgs(ids=t_ids.data_ptr(), seg_off=t_so.data_ptr(), month_index=t_mi.data_ptr(), nrows=len(ids),
                    nseg=len(seg_off) - 1, step=step, link=link.data_ptr(), bad=bad.data_ptr())
    L.call("fm_month_links", L.C.byref(a), E._stream())
    torch.cuda.synchronize()
    return link.cpu().numpy(), int(bad.item())


def _edge_device_panel(E, p, ids=None):
    return E.DevicePanel(cols=_dev(E, p["ret"]).view(1, -1), names=["retx"], seg_off=_dev(E, p["seg_off"]),
                         seg_off_h=np.array(p["seg_off"]), months=np.array(p["month_index"]),
                         ids=_dev(E, p["ids"] if ids is None else ids), month_index=np.array(p["month_index"]))


# ---------------------------------------------------------------- 1. links
@pytest.mark.parametrize("step", [1, -1])
def test_links_match_the_oracle(E, edge, step):
    link, bad = _raw_links(E, edge["ids"], edge["seg_off"], edge["month_index"], step)
    exp = edge["fwd"] if step == 1 else edge["bwd"]
    assert bad == 0
    assert link.dtype == exp.dtype and np.array_equal(link, exp), np.nonzero(link != exp)[0][:8]
    # the engine entry point gives the same tensor and keeps it
    panel = _edge_device_panel(E, edge)
    t = E.month_links(panel, step)
    assert np.array_equal(t.cpu().numpy(), exp) and E.month_links(panel, step) is t


def test_backward_links_invert_forward_links(E, edge):
    fwd, _ = _raw_links(E, edge["ids"], edge["seg_off"], edge["month_index"], 1)
    bwd, _ = _raw_links(E, edge["ids"], edge["seg_off"], edge["month_index"], -1)
    so = edge["seg_off"]
    seg = np.searchsorted(so, np.arange(len(fwd)), side="right") - 1
    rows = np.nonzero(fwd >= 0)[0]
    assert len(rows) > 7000
    there = so[seg[rows] + 1] + fwd[rows]
    assert np.array_equal(so[seg[rows]] + bwd[there], rows) and (bwd >= 0).sum() == len(rows)
    assert np.array_equal(edge["ids"][there], edge["ids"][rows])
    # 64-bit ids: the firm whose id differs from next month's only above bit 32 has no link
    x = np.nonzero(edge["ids"] == HO.ID_X)[0][0]
    assert seg[x] == HO.SEG_X and fwd[x] == -1
    assert np.any((fwd >= 0) & (edge["ids"] > (1 << 40)))


def test_empty_and_single_month_calls(E):
    link, bad = _raw_links(E, np.array([7, 9, 11], dtype=np.int64), np.array([0, 3], dtype=np.int64),
                           np.array([5], dtype=np.int32), 1)
    assert link.tolist() == [-1, -1, -1] and bad == 0
    link, bad = _raw_links(E, np.zeros(0, dtype=np.int64), np.array([0, 0, 0], dtype=np.int64),
                           np.array([5, 6], dtype=np.int32), -1)
    assert len(link) == 0 and bad == 0


# ---------------------------------------------------------------- 2. the order check
def test_unordered_ids_are_counted_and_refused(E, edge):
    ids = np.array(edge["ids"])
    so = edge["seg_off"]
    ids[so[6] + 100] = ids[so[6] + 99]                           # a duplicate id in the 255-row month
    a = so[12] + 2500
    ids[a], ids[a + 1] = ids[a + 1], ids[a]                      # a descending pair in the 5,000-row month
    want = HO.count_bad(ids, so)
    assert want == 2
    _, bad = _raw_links(E, ids, so, edge["month_index"], 1)
    assert bad == want
    _, bad = _raw_links(E, ids, so, edge["month_index"], -1)
    assert bad == want
    with pytest.raises(ValueError, match="2 rows have a firm id that is not greater"):
        E.month_links(_edge_device_panel(E, edge, ids), 1)
    with pytest.raises(ValueError, match="carries no firm ids"):
        p = _edge_device_panel(E, edge)
        p.ids = None
        E.month_links(p, 1)


# ---------------------------------------------------------------- 3. horizon returns
@pytest.mark.parametrize("h", [1, 2, 3, 6, 12, 20])
def test_horizon_returns_match_the_oracle(E, edge, h):
    assert h != 20 or h > len(edge["seg_off"]) - 1
    out = E.horizon_return(_dev(E, edge["seg_off"]), _dev(E, edge["ret"]), _dev(E, edge["fwd"]), h)
    got = out.cpu().numpy()
    exp = HO.horizon_return(edge["ret"], edge["fwd"], edge["seg_off"], h)
    HO.assert_same_bits(got, exp, f"h={h}")
    if h == 1:
        with np.errstate(all="ignore"):
            HO.assert_same_bits(got, (1.0 + edge["ret"]) - 1.0, "h=1 is (1 + r) - 1")
        assert np.isfinite(got).sum() > 28000 and np.isinf(got).sum() == 80
    if h == 2:
        assert np.isfinite(got).sum() > 7000
    if h == 20:
        assert np.isnan(got).all()


def test_horizon_return_refuses_overlap(E, edge):
    ret = _dev(E, edge["ret"])
    with pytest.raises(E.L.FMError, match="overlap ret"):
        E.horizon_return(_dev(E, edge["seg_off"]), ret, _dev(E, edge["fwd"]), 3, out=ret)


# ---------------------------------------------------------------- 4. a hostile link array
def test_links_beyond_the_next_month_give_nan(E, edge):
    """Positions at and beyond the next segment's length, as a stale or foreign link array holds
    them: the rule makes them missing hops, so the rows are NaN and nothing outside the panel is
    read."""
    so = edge["seg_off"]
    n = len(edge["ids"])
    seg = np.searchsorted(so, np.arange(n), side="right") - 1
    nxt = np.diff(so)[np.minimum(seg + 1, len(so) - 2)]
    link = np.array(edge["fwd"])
    rng = np.random.default_rng(8)
    rows = rng.choice(np.nonzero(seg < len(so) - 2)[0], size=600, replace=False)
    link[rows[:200]] = nxt[rows[:200]]                    # exactly the next month's length
    link[rows[200:400]] = nxt[rows[200:400]] + 1 + rng.integers(0, 100000, 200)
    link[rows[400:500]] = np.iinfo(np.int32).max
    link[rows[500:]] = -7
    for h in (2, 6):
        got = E.horizon_return(_dev(E, so), _dev(E, edge["ret"]), _dev(E, link), h).cpu().numpy()
        assert np.isnan(got[rows]).all()
        HO.assert_same_bits(got, HO.horizon_return(edge["ret"], link, so, h), f"hostile links, h={h}")
    # a link array of another, longer panel: every position past the month's end
    far = np.full(n, 1 << 20, dtype=np.int32)
    got = E.horizon_return(_dev(E, so), _dev(E, edge["ret"]), _dev(E, far), 3).cpu().numpy()
    assert np.isnan(got).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. horizon_panel
def _synth(seed=5):
    from fmcore import synth
    return synth.synth_arrays(40, 300, seed, present_rate=0.9), list(synth.WINSOR_VARS)


def _synth_oracle_column(a, h):
    months = np.unique(a["month"])
    so = np.concatenate([[0], np.cumsum(np.bincount(a["month"] - months[0], minlength=len(months)))]).astype(np.int64)
    link = HO.month_links(a["permno"], so, months.astype(np.int32), 1)
    return HO.horizon_return(a["retx"], link, so, h)


def test_horizon_panel(E):
    a, names = _synth()
    panel = E.panel_from_arrays([a[c] for c in names], names, a["month"], me=a["me"], nyse=a["nyse"], ids=a["permno"])
    assert np.array_equal(panel.ids.cpu().numpy(), a["permno"]) and panel.ids.dtype == torch.int64
    assert np.array_equal(panel.month_index, np.unique(a["month"])) and panel.month_index.dtype == np.int32
    assert np.array_equal(panel.month_index_device().cpu().numpy(), panel.month_index)
    before = panel.cols.clone()
    hp = E.horizon_panel(panel, 3)
    assert hp.names == names + ["retx_3m"] and panel.names == names
    assert hp.cols.shape == (len(names) + 1, panel.nrows) and hp.cols.data_ptr() != panel.cols.data_ptr()
    assert torch.equal(panel.cols.view(torch.int64), before.view(torch.int64))                 # input untouched
    assert torch.equal(hp.cols[:len(names)].view(torch.int64), before.view(torch.int64))       # the other columns
    HO.assert_same_bits(hp.cols[-1].cpu().numpy(), _synth_oracle_column(a, 3), "retx_3m")
    for k in ("seg_off", "me", "nyse", "months", "order", "ids", "month_index"):
        assert getattr(hp, k) is getattr(panel, k), k
    # another column, another name; the rank transform carries the identity too
    hq = E.horizon_panel(hp, 2, ret="log_size", name="ls2")
    assert hq.names[-1] == "ls2" and hq.ncols == len(names) + 2
    rk = E.rank_transform(panel, cols=["log_bm"])
    assert rk.ids is panel.ids and rk.month_index is panel.month_index
    HO.assert_same_bits(E.horizon_panel(rk, 3).cols[-1].cpu().numpy(), hp.cols[-1].cpu().numpy(), "after a rank")
    with pytest.raises(ValueError, match="already has a column 'retx_3m'"):
        E.horizon_panel(hp, 3)
    with pytest.raises(ValueError, match="horizon must be 1..60"):
        E.horizon_panel(panel, 61)
    with pytest.raises(ValueError, match="carries no firm ids"):
        E.horizon_panel(E.panel_from_arrays([a[c] for c in names], names, a["month"]), 3)
    wide = E.panel_from_arrays([a["retx"]] * 31, ["retx"] + [f"c{i}" for i in range(30)], a["month"], ids=a["permno"])
    with pytest.raises(ValueError, match="at most 31 columns"):
        E.horizon_panel(wide, 3)
    # the synthetic generator's panel: ids 10000 + the position in the month
    sp = E.panel_synthetic(3, 50, 1, month0=7)
    assert np.array_equal(sp.ids.cpu().numpy(), np.tile(np.arange(50) + 10000, 3)) and sp.month_index.tolist() == [7, 8, 9]
    assert np.array_equal(E.month_links(sp, 1).cpu().numpy(), np.r_[np.tile(np.arange(50), 2), np.full(50, -1)])


# ---------------------------------------------------------------- 6. the pipeline
def _tensors(out):
    """Every output tensor of a pipeline run as host arrays by name; the tables indexed by
    fitted-month row (ix.idx, rolling, pred, pred_status) up to each problem's count and the
    moments of the fitted months up to each problem's own size: what lies beyond is never written."""
    h = lambda t: t.cpu().numpy()   # noqa: E731
    count = h(out.ix.count)
    rows = np.arange(out.ix.idx.shape[1])[None, :] < count[:, None]
    fitted = (h(out.res.status) & 1) != 0
    mom = h(out.res.moments)
    d = {"res.rec": h(out.res.rec), "res.status": h(out.res.status),
         "ix.count": count, "ix.idx": h(out.ix.idx)[rows], "rolling": h(out.rolling)[rows], "pred": h(out.pred)[rows],
         "pred_status": h(out.pred_status)[rows], "level": h(out.level),
         "breakpoints[0]": h(out.breakpoints[0]), "breakpoints[1]": h(out.breakpoints[1])}
    for k, p in enumerate(out.res.problems):   # n, the K + 1 means, the (K + 1)^2 centered moments
        d[f"res.moments[{k}]"] = mom[fitted[:, k], k, :1 + (p.K + 1) + (p.K + 1) ** 2]
    for name in ("summary", "pred_summary", "portfolio_summary", "forecast_dist_summary", "forecast_compare_summary"):
        for k in ("mean", "se", "tstat", "nobs"):
            d[f"{name}.{k}"] = h(getattr(getattr(out, name), k))
    for k in ("lo", "hi", "nvalid", "center"):
        d[f"cuts.{k}"] = h(getattr(out.cuts, k))
    for name, keys in (("portfolios", ("bp", "port", "rec", "cnt", "status")), ("forecast_dist", ("rec", "cnt", "status")),
                       ("forecast_compare", ("rec", "cnt", "status"))):
        for k in keys:
            d[f"{name}.{k}"] = h(getattr(getattr(out, name), k))
    return d


def test_pipeline_equals_a_run_on_the_host_built_column(E):
    from fmcore import lewellen as LW
    a, names = _synth(5)
    kw = dict(lag=3, window=12, min_periods=6, portfolios=5, forecast_dist=True, forecast_compare=True)
    pa = E.panel_from_arrays([a[c] for c in names], names, a["month"], me=a["me"], nyse=a["nyse"], ids=a["permno"])
    run_a = LW.run_pipeline(pa, LW.PipelineConfig(horizon=3, **kw))
    pb = E.panel_from_arrays([a[c] for c in names] + [_synth_oracle_column(a, 3)], names + ["retx_3m"], a["month"],
                             me=a["me"], nyse=a["nyse"])
    run_b = LW.run_pipeline(pb, LW.PipelineConfig(horizon=1, **kw), y="retx_3m")
    assert run_a.y_col == run_b.y_col == "retx_3m" and pa.names == names
    assert run_a.model_names == run_b.model_names and run_a.portfolio_problems == run_b.portfolio_problems
    assert run_a.forecast_compare_pairs == run_b.forecast_compare_pairs
    ta, tb = _tensors(run_a), _tensors(run_b)
    # the condition on the input: every month but the last two is fitted for every problem
    fitted = (tb["res.status"] & 1) != 0
    assert fitted[:38].all() and not fitted[38:].any()
    assert (tb["portfolios.status"] == 1).any() and np.isfinite(tb["pred_summary.mean"][:, 0]).all()
    assert set(ta) == set(tb)
    for k in tb:
        assert ta[k].shape == tb[k].shape and ta[k].dtype == tb[k].dtype, k
        assert ta[k].tobytes() == tb[k].tobytes(), k
    # a panel that has the column already is used as it is; horizon 1 names the monthly return
    run_c = LW.run_pipeline(E.horizon_panel(pa, 3), LW.PipelineConfig(horizon=3, **kw))
    assert _tensors(run_c)["res.rec"].tobytes() == tb["res.rec"].tobytes()
    assert LW.run_pipeline(pa, LW.PipelineConfig(**kw)).y_col == "retx"
    with pytest.raises(ValueError, match="carries no firm ids"):
        LW.run_pipeline(E.panel_from_arrays([a[c] for c in names], names, a["month"], me=a["me"], nyse=a["nyse"]),
                        LW.PipelineConfig(horizon=3, **kw))


# ---------------------------------------------------------------- 7. the drop-in
def test_dropin_horizon_returns_and_tables(E):
    from fmcore import synth
    from fmdrop import calc_Lewellen_2014 as CL
    df = synth.synth_frame(40, 300, 5, present_rate=0.9, shuffle=True)
    df.index = np.random.default_rng(2).permutation(len(df)) + 1000
    before = df.copy()
    out = CL.horizon_returns(df, 3)
    assert out.index.equals(before.index) and list(out.columns) == list(before.columns) + ["retx_3m"]
    assert out[list(before.columns)].equals(before) and df.equals(before)
    month = df["mthcaldt"].dt.year.to_numpy() * 12 + df["mthcaldt"].dt.month.to_numpy() - 1
    HO.assert_same_bits(out["retx_3m"].to_numpy(), HO.pandas_horizon(df["permno"].to_numpy(), month, df["retx"].to_numpy(), 3),
                        "horizon_returns")
    with pytest.raises(ValueError, match="not greater than the previous"):
        CL.horizon_returns(before.iloc[[0, 0, 1]], 2)
    kw = dict(lag=3, window=12, min_periods=6)
    t3 = CL.build_table_3(df, **kw)
    t9 = CL.build_table_3(df, horizon=3, **kw)
    assert t9.index.equals(t3.index) and list(t9.columns) == list(t3.columns)
    assert np.isfinite(t9["Slope"].to_numpy()).all() and not np.allclose(t9["Slope"].to_numpy(), t3["Slope"].to_numpy())
    assert not np.allclose(t9["Avg"].to_numpy(), t3["Avg"].to_numpy())
    t8 = CL.build_table_2_horizon(df, 3, nw_lags=6)
    assert t8.index.names == ["Model", "Predictor"] and t8.shape == (3 + 7 + 14 + 3, 9)
    assert all(v != "" for v in t8[("All stocks", "Slope")])
    assert dataclasses.is_dataclass(CL.lewellen_pipeline(df, horizon=3, **kw)) and CL.lewellen_pipeline(df, horizon=3, **kw).y_col == "retx_3m"
