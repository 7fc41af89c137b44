"""Host-side checks of the forecast-sorted portfolios (A12): the binding's ABI, the numpy
restatement against pandas on tie-free data, and the drop-in signature."""
import ctypes
import inspect

import numpy as np
import pandas as pd

import port_oracle as PO


def test_binding_has_portfolio_sort():
    from fmcore import _lib as L
    assert "fm_portfolio_sort" in L.EXPORTED
    lib = L.load()
    assert hasattr(lib, "fm_portfolio_sort")
    assert lib.fm_struct_size(b"fm_port_args") == ctypes.sizeof(L.PortArgs)
    assert L.PortArgs.q.size == 8 * (L.FM_MAX_PORTS - 1)


def test_restatement_equals_qcut_groupby_on_tie_free_frame():
    rng = np.random.default_rng(3)
    T, N, nport = 12, 200, 10
    df = pd.DataFrame({"t": np.repeat(np.arange(T), N), "F": rng.normal(0.01, 0.02, T * N),
                       "R": rng.normal(0.01, 0.1, T * N)})
    assert df.groupby("t")["F"].nunique().eq(N).all()
    seg_off = np.arange(T + 1) * N
    got = PO.portfolio_sort(seg_off, df["F"].values, df["R"].values, nport=nport)
    df["p"] = df.groupby("t")["F"].transform(lambda s: pd.qcut(s, nport, labels=False))
    assert np.array_equal(got["port"], df["p"].to_numpy())
    assert got["status"].tolist() == [1] * T
    g = df.groupby(["t", "p"])
    np.testing.assert_allclose(got["rec"][:, :nport, 0], g["R"].mean().unstack().to_numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["rec"][:, :nport, 1], g["F"].mean().unstack().to_numpy(), rtol=1e-13, atol=0)
    assert np.array_equal(got["cnt"], g["R"].size().unstack().to_numpy())
    assert np.isnan(got["rec"][:, :, 2:]).all()   # no weights
    np.testing.assert_array_equal(got["rec"][:, nport, 0], got["rec"][:, nport - 1, 0] - got["rec"][:, 0, 0])


def test_restatement_small_months_and_ties():
    # months of 9 / 10 / 11 rows: unsorted / sorted / sorted at the default min_count = nport
    rng = np.random.default_rng(5)
    lens = np.array([9, 10, 11])
    seg_off = np.concatenate([[0], np.cumsum(lens)])
    n = int(seg_off[-1])
    got = PO.portfolio_sort(seg_off, rng.normal(size=n), rng.normal(size=n), nport=10)
    assert got["status"].tolist() == [0, 1, 1]
    assert (got["port"][:9] == 255).all() and np.isnan(got["bp"][0]).all() and np.isnan(got["rec"][0]).all()
    # a 7-value forecast grid leaves portfolios empty: NaN records, zero counts
    pan = PO.random_panel()
    grid = np.linspace(-0.02, 0.04, 7)
    F = grid[np.abs(np.nan_to_num(pan["F"], nan=0.0, posinf=0.0)[:, None] - grid[None, :]).argmin(axis=1)]
    tie = PO.portfolio_sort(pan["seg_off"], F, pan["R"], pan["W"], nport=10)
    empty = tie["cnt"] == 0
    assert empty.any() and np.isnan(tie["rec"][:, :10, 0][empty]).all()


def test_drop_in_signature():
    from fmdrop import bind
    from fmdrop import calc_Lewellen_2014 as CL
    sig = inspect.signature(CL.forecast_sorted_portfolios)
    assert list(sig.parameters) == ["df", "forecast", "return_col", "weight_col", "nport", "breakpoints",
                                    "universe", "nyse_breakpoints", "date_col", "nw_lags"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(return_col="retx", weight_col=None, nport=10, breakpoints=None, universe=None,
                     nyse_breakpoints=False, date_col="mthcaldt", nw_lags=4)
    assert "forecast_sorted_portfolios" not in bind.HOT["calc_Lewellen_2014"]   # the reference has no such name
    from fmcore import engine as E
    sig = inspect.signature(E.portfolio_sort)
    assert list(sig.parameters) == ["seg_off", "forecast", "ret", "weight", "level", "nyse", "nport", "q",
                                    "min_level", "nyse_breakpoints", "min_count", "max_seg_len"]
