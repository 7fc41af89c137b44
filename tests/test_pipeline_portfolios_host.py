"""CPU tests of the fused forecast-and-sort's numpy restatement (tests/pipe_port_oracle.py): the
restatement chain against an independent pandas chain of oracle.fm_oracle, the fixture margin
that the end-to-end GPU test (tests/test_gpu_pipeline_portfolios.py) relies on, and the binding."""
import ctypes

import numpy as np
import pandas as pd

import pipe_port_oracle as PPO
import port_oracle as PO
from fmtol import RTOL, assert_series_close
from oracle import fm_oracle as O


def test_library_exports_fused_sort():
    from fmcore import _lib as L
    lib = L.load()
    for f in ("fm_forecast_portfolio_sort", "fm_lagged_coef"):
        assert f in L.EXPORTED and hasattr(lib, f)
    assert lib.fm_struct_size(b"fm_fport_args") == ctypes.sizeof(L.FPortArgs)
    assert lib.fm_struct_size(b"fm_port_args") == ctypes.sizeof(L.PortArgs)


def test_restatement_chain_vs_pandas_chain():
    """(a) winsor cuts -> clipped sequential forecast with the lagged coefficient table ->
    port_oracle, against winsorize -> monthly_params -> rolling_coefficients ->
    expected_return_forecasts -> pd.qcut + groupby().mean(): one model, level 0, tie-free data;
    the same portfolio membership, means within RTOL."""
    from fmcore import synth
    xs = ["log_size", "log_bm", "return_12_2"]
    window, minp, lag, nport = 8, 4, 1, 5
    df = synth.synth_frame(24, 150, 5, nan_rate=0.03, present_rate=0.9).sort_values(["mthcaldt", "permno"])
    df = df.reset_index(drop=True)
    # --- the pandas chain
    w = O.winsorize(df, xs)
    params = O.monthly_params(w, "retx", xs)
    croll = O.rolling_coefficients(params, window, minp, lag)
    F = O.expected_return_forecasts(w, croll, xs).to_numpy()
    # --- the restatement chain, from the raw columns
    months, counts = np.unique(df["mthcaldt"].values, return_counts=True)
    seg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T = len(months)
    cols = [df[c].to_numpy(dtype=np.float64) for c in ["retx"] + xs]
    lo, hi = PPO.winsor_cuts(cols, seg_off)
    roll = np.full((1, T, 4), np.nan)
    nfit = len(params)
    roll[0, :nfit] = np.column_stack([O.rolling_mean(params[c].values, window, minp) for c in params.columns])
    idx = np.zeros((1, T), dtype=np.int64)
    idx[0, :nfit] = np.searchsorted(months, params.index.values)
    coef = PPO.lagged_coef(roll, idx, np.array([nfit]), [0], lag)
    got = PPO.forecast_portfolio_sort(cols, seg_off, coef, [([1, 2, 3], 0)], lo, hi, ret=0, nport=nport)
    assert np.array_equal(got["F"][0], F, equal_nan=True)   # the same operations in the same order
    fin = np.isfinite(F)
    assert len(np.unique(F[fin])) == fin.sum()              # tie-free
    nsorted = 0
    for t in range(T):
        s = slice(int(seg_off[t]), int(seg_off[t + 1]))
        f, r, ok = F[s], cols[0][s], fin[s]
        if ok.sum() < nport:
            assert got["status"][0, t] == 0
            continue
        nsorted += 1
        assert got["status"][0, t] == 1
        bins = pd.qcut(pd.Series(f[ok]), nport, labels=False).to_numpy()
        assert np.array_equal(got["port"][0, s][ok], bins), t
        assert (got["port"][0, s][~ok] == 255).all()
        g = pd.DataFrame({"p": bins, "r": r[ok], "f": f[ok]}).dropna(subset=["r"]).groupby("p").mean()
        for k in range(nport):
            for c, name in ((0, "r"), (1, "f")):
                e = g[name].get(k, np.nan)
                a = got["rec"][0, t, k, c]
                assert (np.isnan(a) and np.isnan(e)) or abs(a - e) <= RTOL * abs(e), (t, k, name, a, e)
    assert nsorted >= 15   # months 0..minp have no lagged coefficient row: all NaN, unsorted


def test_fixture_margin():
    """(b) The end-to-end GPU test compares portfolio bytes of the device pipeline with the
    oracle's; their coefficients agree to RTOL only, so no eligible row of the fixture may sit
    within that of a breakpoint: whenever F_i != bp_j, |F_i - bp_j| > 1e-9 * RMS(F of the month).
    From oracle numbers alone."""
    keys, exp = PPO.pipeline_expected()
    seg_off = PPO.pipeline_fixture()["seg_off"]
    assert len(keys) == 9
    worst = np.inf
    for j in range(len(keys)):
        srt = np.nonzero(exp["status"][j])[0]
        assert len(srt) >= 20, keys[j]
        for t in srt:
            s = slice(int(seg_off[t]), int(seg_off[t + 1]))
            f = exp["F"][j, s][exp["port"][j, s] != 255]
            rms = float(np.sqrt(np.mean(f * f)))
            d = np.abs(f[:, None] - exp["bp"][j, t][None, :])
            d = d[d != 0.0]
            worst = min(worst, d.min() / rms)
            assert d.min() > 1e-9 * rms, (keys[j], t, d.min(), rms)
    print("smallest |F - bp| / RMS(F):", worst)


def test_batched_summary_oracle_shapes():
    """port_oracle.portfolio_summary per sort of the fixture: the sorted months are the series."""
    keys, exp = PPO.pipeline_expected()
    mean, se, t, nobs = PO.portfolio_summary(exp["rec"][0], exp["status"][0], 4)
    assert mean.shape == (PPO.PIPE["nport"] + 1, 4) and nobs.max() == exp["status"][0].sum()
    assert_series_close(mean[:, 0], np.nanmean(exp["rec"][0][exp["status"][0] == 1][:, :, 0], axis=0), "ew_ret")
