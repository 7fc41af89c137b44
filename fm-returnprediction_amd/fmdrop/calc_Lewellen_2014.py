"""Drop-in replacement for the hot-path functions of the reference's
src/calc_Lewellen_2014.py, on MI355X.

Mirrored (same names, signatures, return types and row/column/index order):
  winsorize        reference :505-529   per-month 1/99 cuts (fm_select_cuts) + clip (fm_clip)
  get_subsets      reference :44-112    NYSE me breakpoints (fm_select_cuts, pandas lerp)
  build_table_1    reference :577-670   monthly moments + distinct permnos on device (§8(f) row 1)
  build_table_2    reference :674-868   9 FM passes batched into one Gram pass on device
  create_figure_1  reference :871-957   F1 OLS + 120-month rolling means on device
Extensions the north star names (not in the reference; parity unpinned):
  standardize, rank_transform, group_adjust (within-industry adjustment; every lewellen_pipeline /
  build_table_* **cfg also takes group_col=...), monthly_coefficients, rolling_coefficients, expected_return_forecasts,
  predictive_slope_regressions, forecast_sorted_portfolios, forecast_distribution,
  forecast_comparison, lewellen_pipeline, build_table_5, build_table_3, build_table_4,
  horizon_returns, build_table_2_horizon (multi-month returns: paper Tables 8 and 9; every
  build_table_* takes horizon=k, lag>=k, nw_lags=...).
Firm-axis characteristic builders (§8(f) row 2; one fused device pass, fm_firm_chars):
  calc_log_size, calc_log_bm, calc_return_12_2, calc_accruals, calc_roa,
  calc_log_assets_growth, calc_dy, calc_log_return_13_36, calc_log_issues_12,
  calc_log_issues_36, calc_debt_price, calc_sales_price   reference :137-341
  calc_std_12      reference :438-466   252-day rolling std on device (fm_rolling_std)
  calc_characteristics (extension): all twelve monthly characteristics in one launch.
  calculate_rolling_beta reference :344-434  polars 156-week weekly-window beta on device
                   (fm_rolling_beta; parity unpinned: no polars here)
Data pulls and LaTeX output of the reference are outside this drop-in (scope).
"""
import os
from pathlib import Path
from typing import Union

import numpy as np
import pandas as pd

from fmcore import _lib as _L
from fmcore import api as _api
from fmcore import engine as _E
from fmcore import lewellen as _LW

from .regressions import fama_macbeth_summary, run_monthly_cs_regressions  # noqa: F401

OUTPUT_DIR = Path(os.environ.get("OUTPUT_DIR", "_output"))


# ------------------------------------------------------------------------------------------
# Universes
# ------------------------------------------------------------------------------------------
def _nyse_cuts(df):
    """me_20/me_50 per month (device) for a frame already sorted by [mthcaldt, permno]."""
    me = _api.as_f64(df["me"])
    nyse = (df["primaryexch"] == "N").to_numpy().astype(np.uint8)
    panel = _E.panel_from_arrays([me], ["me"], df["mthcaldt"].values, me=me, nyse=nyse)
    a, b, level = _E.universe(panel)
    return panel, a.cpu().numpy(), b.cpu().numpy(), level.cpu().numpy()


def get_subsets(crsp_comp: pd.DataFrame) -> dict:
    """All / All-but-tiny / Large universes from NYSE 20th and 50th `me` percentiles per
    month (reference src/calc_Lewellen_2014.py:44-112).  Returns the same 3-key dict; the
    frames carry me_20, me_50, is_all_but_tiny, is_large and a fresh RangeIndex."""
    df = crsp_comp.sort_values(["mthcaldt", "permno"]).copy()
    panel, me20, me50, level = _nyse_cuts(df)
    codes, _ = pd.factorize(df["mthcaldt"], sort=True)
    codes = np.asarray(codes)
    valid = codes >= 0
    # NYSE-less months (or all-NaN NYSE me) carry NaN breakpoints, as after the left merge
    row20 = np.full(len(df), np.nan)
    row50 = np.full(len(df), np.nan)
    row20[valid] = me20[codes[valid]]
    row50[valid] = me50[codes[valid]]
    out = df.reset_index(drop=True)
    out["me_20"] = row20
    out["me_50"] = row50
    lvl = np.zeros(len(df), dtype=np.uint8)
    lvl[panel.order] = level
    out["is_all_but_tiny"] = lvl >= 1
    out["is_large"] = lvl >= 2
    return {
        "All stocks": out.copy(),
        "All-but-tiny stocks": out.loc[out["is_all_but_tiny"]].copy(),
        "Large stocks": out.loc[out["is_large"]].copy(),
    }


# ------------------------------------------------------------------------------------------
# Winsorize / standardize / rank
# ------------------------------------------------------------------------------------------
def _split_runs(varlist):
    runs, cur = [], []
    for v in varlist:
        if v in cur:
            runs.append(cur)
            cur = []
        cur.append(v)
    if cur:
        runs.append(cur)
    return runs


def winsorize(crsp_comp: pd.DataFrame, varlist: list, lower_percentile=1, upper_percentile=99) -> pd.DataFrame:
    """Clip each variable at its per-month [lower, upper] linear percentiles, months with
    fewer than 5 non-NaN values untouched (reference src/calc_Lewellen_2014.py:505-529).
    Returns the frame sorted by [mthcaldt, permno] with the original index labels."""
    df = crsp_comp.sort_values(["mthcaldt", "permno"]).copy()
    varlist = list(varlist)
    if not varlist:
        return df
    codes, _ = pd.factorize(df["mthcaldt"], sort=True)
    if (np.asarray(codes) < 0).any():
        df = df.loc[np.asarray(codes) >= 0]       # groupby(...).apply drops NaT months
    for run in _split_runs(varlist):
        arrays = [_api.as_f64(df[v]) for v in run]
        panel = _E.panel_from_arrays(arrays, run, df["mthcaldt"].values)
        cuts = _E.select_cuts(panel, lower_percentile / 100, upper_percentile / 100, 5, _E.LERP_NUMPY)
        out = _E.clip(panel, cuts).cpu().numpy()
        inv = np.empty_like(panel.order)
        inv[panel.order] = np.arange(len(panel.order))
        for i, v in enumerate(run):
            df[v] = out[i][inv]
    return df


def standardize(crsp_comp: pd.DataFrame, varlist: list, date_col: str = "mthcaldt") -> pd.DataFrame:
    """Per-month z-scores (x - mean_t) / std_t(ddof=1) over non-NaN values (north-star
    extension A9; the reference has no standardization, so this is OFF on parity paths)."""
    df = crsp_comp.copy()
    varlist = list(varlist)
    arrays = [_api.as_f64(df[v]) for v in varlist]
    panel = _E.panel_from_arrays(arrays, varlist, df[date_col].values)
    mom = _E.select_cuts(panel, 0.0, 1.0, 2 ** 31 - 1, _E.LERP_NUMPY, moments=True)
    z = _E.standardize(panel, mom.mean, mom.sd).cpu().numpy()
    for i, v in enumerate(varlist):
        col = np.full(len(df), np.nan)
        col[panel.order] = z[i]
        df[v] = col
    return df


_UNIVERSE_LEVEL = {None: 0, "all_but_tiny": 1, "large": 2}


def rank_transform(crsp_comp: pd.DataFrame, varlist: list, date_col: str = "mthcaldt", method: str = "average",
                   scale: str = "pct", universe: str = None) -> pd.DataFrame:
    """Per-month cross-sectional ranks of each variable over its non-NaN values (extension A13;
    the reference has no rank transform): pandas' ``groupby(date_col)[v].rank(method=method)``
    for ``scale`` "raw", with ``pct=True`` for "pct", and rank / (count + 1) - 0.5 for
    "uniform", bit for bit, on the device (fm_rank_transform).  ``method`` in {"average", "min",
    "max"}.  ``universe`` in {None, "all_but_tiny", "large"} ranks within that get_subsets
    universe (from ``me`` and ``primaryexch``) and gives NaN outside it.  Returns a copy of the
    frame in the caller's row order; rows with a missing month label get NaN.  A month may
    hold up to 65,536 rows (``FMError`` beyond that); a frame whose longest month has more than
    16,384 rows is ranked by a slower kernel that visits such a month in 16,384-row parts."""
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    df = crsp_comp.copy()
    varlist = list(varlist)
    if not varlist:
        return df
    arrays = [_api.as_f64(df[v]) for v in varlist]
    me = nyse = level = None
    if universe is not None:
        me = _api.as_f64(df["me"])
        nyse = (df["primaryexch"] == "N").to_numpy().astype(np.uint8)
    panel = _E.panel_from_arrays(arrays, varlist, df[date_col].values, me=me, nyse=nyse)
    if universe is not None:
        level = _E.universe(panel)[2]
    r = _E.rank_transform(panel, method=method, scale=scale, level=level,
                          min_level=_UNIVERSE_LEVEL[universe]).cols.cpu().numpy()
    for i, v in enumerate(varlist):
        col = np.full(len(df), np.nan)
        col[panel.order] = r[i]
        df[v] = col
    return df


def group_adjust(crsp_comp: pd.DataFrame, varlist: list, group_col: str = "siccd", date_col: str = "mthcaldt",
                 mode: str = "demean", min_count: int = 1, universe: str = None) -> pd.DataFrame:
    """Each variable adjusted within the groups (industries) ``group_col`` of its month over its
    non-NaN values (extension A20; the reference has no such transform): pandas'
    ``groupby([date_col, group_col])[v].transform`` of x - mean for ``mode`` "demean" (the
    industry-relative characteristic), of the mean for "mean" and of (x - mean) / std(ddof=1) for
    "zscore", on the device (fm_group_adjust; sums in a fixed order, so a repeat gives the same
    bits).  ``group_col`` holds integers or strings (at most 256 distinct values); a row with a
    missing label, or in a group of fewer than ``min_count`` rows, gets NaN.  ``universe`` in {None,
    "all_but_tiny", "large"} takes the groups within that get_subsets universe (from ``me`` and
    ``primaryexch``) and gives NaN outside it.  Works on any column, a materialised forecast
    included.  Returns a copy of the frame in the caller's row order; rows with a missing month
    label get NaN."""
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    if mode not in _E.GADJ_MODES:
        raise ValueError(f"group_adjust: mode must be one of {sorted(_E.GADJ_MODES)}, got {mode!r}")
    df = crsp_comp.copy()
    varlist = list(varlist)
    if not varlist:
        return df
    arrays = [_api.as_f64(df[v]) for v in varlist]
    codes, uniq = _E.group_codes(df[group_col])
    me = nyse = level = None
    if universe is not None:
        me = _api.as_f64(df["me"])
        nyse = (df["primaryexch"] == "N").to_numpy().astype(np.uint8)
    panel = _E.panel_from_arrays(arrays, varlist, df[date_col].values, me=me, nyse=nyse, group=codes,
                                 ngroups=max(len(uniq), 1))
    if universe is not None:
        level = _E.universe(panel)[2]
    r = _E.group_adjust(panel, mode=mode, min_count=min_count, level=level,
                        min_level=_UNIVERSE_LEVEL[universe]).cols.cpu().numpy()
    for i, v in enumerate(varlist):
        col = np.full(len(df), np.nan)
        col[panel.order] = r[i]
        df[v] = col
    return df


# ------------------------------------------------------------------------------------------
# Firm-axis characteristics (reference :137-466)
# ------------------------------------------------------------------------------------------
def _firm_grouping(permno):
    """groupby("permno") row order: each firm's rows contiguous, frame order inside a firm
    (a stable sort by permno; None when the frame is already grouped that way).  pandas'
    groupby drops rows whose permno is missing; such rows are rejected here rather than
    read as a garbage id."""
    p = np.asarray(permno)
    if p.dtype.kind == "f":
        if np.isnan(p).any():
            raise ValueError("permno contains NaN: drop those rows first (groupby would drop them)")
    elif p.dtype.kind not in "iu":
        p = pd.to_numeric(pd.Series(p), errors="raise").to_numpy()
        if np.isnan(p.astype(np.float64)).any():
            raise ValueError("permno contains missing values")
    ids = p.astype(np.int64)
    if len(ids) < 2 or bool(np.all(ids[1:] >= ids[:-1])):
        return ids, None
    order = np.argsort(ids, kind="stable")
    return ids[order], order


def _device_chars(df, names):
    """{name: float64 ndarray in df's row order} for the requested characteristics."""
    import torch
    dev = _E.require_device()
    ids, order = _firm_grouping(df["permno"].to_numpy())
    reads = set()
    for nm in names:
        reads |= _CHAR_READS[nm]
    fields = {}
    for f in reads:
        v = _api.as_f64(df[f])
        fields[f] = torch.from_numpy(np.ascontiguousarray(v if order is None else v[order])).to(dev)
    out = _E.firm_chars(torch.from_numpy(ids).to(dev), fields, names)
    res = {}
    for nm in names:
        v = out[nm].cpu().numpy()
        if order is not None:
            u = np.empty_like(v)
            u[order] = v
            v = u
        res[nm] = v
    return res


_CHAR_READS = {
    "log_size": {"me"}, "log_bm": {"me", "be"}, "return_12_2": {"retx"},
    "accruals_final": {"accruals", "depreciation"}, "roa": {"earnings", "assets"},
    "log_assets_growth": {"assets"}, "dy": {"dvc", "prc"}, "log_return_13_36": {"retx"},
    "log_issues_12": {"shrout"}, "log_issues_36": {"shrout"}, "debt_price": {"me", "total_debt"},
    "sales_price": {"me", "sales"},
}


def _add_char(crsp_comp, name):
    crsp_comp[name] = _device_chars(crsp_comp, [name])[name]
    return crsp_comp


def calc_log_size(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """log(me) of the firm's previous row (reference :137-147)."""
    return _add_char(crsp_comp, "log_size")


def calc_log_bm(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """log(be[t-1]) - log(me[t-1]) (reference :150-163)."""
    return _add_char(crsp_comp, "log_bm")


def calc_return_12_2(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """prod(1 + retx) over the firm's rows t-12..t-2, all 11 present, minus 1 (:166-192)."""
    return _add_char(crsp_comp, "return_12_2")


def calc_accruals(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """accruals - depreciation (reference :195-204)."""
    return _add_char(crsp_comp, "accruals_final")


def calc_roa(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """earnings / assets (reference :241-249)."""
    return _add_char(crsp_comp, "roa")


def calc_log_assets_growth(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """log(assets / assets twelve firm rows back) (reference :252-262)."""
    return _add_char(crsp_comp, "log_assets_growth")


def calc_dy(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """Sum of dvc over the firm's last 12 rows (min_periods=1) / prc[t-1], on a copy sorted by
    [permno, mthcaldt], which is returned (reference :265-287)."""
    df = crsp_comp.sort_values(["permno", "mthcaldt"]).copy()
    return _add_char(df, "dy")


def calc_log_return_13_36(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """Sum of log(1 + retx) over the firm's rows t-36..t-13, all 24 present (:290-313)."""
    return _add_char(crsp_comp, "log_return_13_36")


def calc_log_issues_12(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """log(shrout[t-1]) - log(shrout[t-12]) (reference :224-238)."""
    return _add_char(crsp_comp, "log_issues_12")


def calc_log_issues_36(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """log(shrout[t-1]) - log(shrout[t-36]) (reference :207-221)."""
    return _add_char(crsp_comp, "log_issues_36")


def calc_debt_price(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """total_debt / me[t-1] (reference :316-327)."""
    return _add_char(crsp_comp, "debt_price")


def calc_sales_price(crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """sales / me[t-1] (reference :330-341)."""
    return _add_char(crsp_comp, "sales_price")


def calc_characteristics(crsp_comp: pd.DataFrame, names=None) -> pd.DataFrame:
    """Extension: the twelve monthly characteristics in get_factors order (reference
    :537-547) from ONE device pass; same values as calling the calc_* one by one on a frame
    sorted by [permno, mthcaldt] (calc_dy's re-sort is then a no-op)."""
    names = list(_E.CHAR_NAMES if names is None else names)
    out = _device_chars(crsp_comp, names)
    for nm in names:
        crsp_comp[nm] = out[nm]
    return crsp_comp


def calculate_rolling_beta(crsp_d: pd.DataFrame, crsp_index_d: pd.DataFrame,
                           crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """156-week rolling market beta from daily log returns, merged onto crsp_comp as `beta`
    (reference src/calc_Lewellen_2014.py:344-434).  The reference's polars
    group_by_dynamic(every="1w", period="156w", by="permno") windows, sums and beta formula
    run on device (fm_rolling_beta); the inner join on the date, the (permno, date) sort
    and the final left merge on (permno, jdate) are the reference's pandas steps.  Parity
    unpinned: polars is not installed here (oracle/chars_oracle.py restates its semantics)."""
    import torch
    dev = _E.require_device()
    df = crsp_d[["permno", "dlycaldt", "retx"]].rename(columns={"retx": "Ri", "dlycaldt": "date"})
    mkt = crsp_index_d[["caldt", "vwretx"]].rename(columns={"vwretx": "Rm", "caldt": "date"})
    j = df.merge(mkt, on="date", how="inner").sort_values(["permno", "date"], kind="stable")
    permno = j["permno"].to_numpy()
    days = j["date"].values.astype("datetime64[D]").astype(np.int64)
    if len(days) and (days.min() < -(2 ** 31) or days.max() >= 2 ** 31):
        raise ValueError("calculate_rolling_beta: dates out of range")
    starts = np.flatnonzero(np.r_[True, permno[1:] != permno[:-1]]) if len(permno) else np.zeros(0, np.int64)
    seg_off = np.r_[starts, len(permno)].astype(np.int64)
    uperm = permno[starts]
    keys = crsp_comp[["permno", "jdate"]].drop_duplicates()
    kp = keys["permno"].to_numpy()
    pos = np.searchsorted(uperm, kp) if len(uperm) else np.zeros(len(kp), dtype=np.int64)
    ok = pos < len(uperm)
    ok[ok] = uperm[pos[ok]] == kp[ok]
    kq = keys.loc[ok]
    per = pd.to_datetime(kq["jdate"]).dt.to_period("M")
    d0 = per.dt.start_time.values.astype("datetime64[D]").astype(np.int64)
    d1 = per.dt.end_time.values.astype("datetime64[D]").astype(np.int64)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    beta = _E.rolling_beta(t(days, np.int32), t(j["Ri"].to_numpy(dtype=np.float64), np.float64),
                           t(j["Rm"].to_numpy(dtype=np.float64), np.float64), t(seg_off, np.int64),
                           t(pos[ok], np.int32), t(d0, np.int32), t(d1, np.int32)).cpu().numpy()
    # a (permno, month) without an emitted window is NaN after the merge either way
    right = kq.assign(beta=beta)
    return pd.merge(left=crsp_comp, right=right[["permno", "jdate", "beta"]], on=["permno", "jdate"], how="left")


def calc_std_12(crsp_d: pd.DataFrame, crsp_comp: pd.DataFrame) -> pd.DataFrame:
    """Annualized 252-day rolling std of daily retx per permno (min_periods=100), the last
    day of each (permno, month), left-merged onto crsp_comp on [permno, jdate]
    (reference :438-466).  The rolling std runs on device; the month-end pick and the merge
    are the reference's pandas steps."""
    import torch
    dev = _E.require_device()
    df_std_12 = crsp_d.copy()
    ids, order = _firm_grouping(df_std_12["permno"].to_numpy())
    x = _api.as_f64(df_std_12["retx"])
    xs = torch.from_numpy(np.ascontiguousarray(x if order is None else x[order])).to(dev)
    sd = _E.rolling_std(torch.from_numpy(ids).to(dev), xs, 252, 100, float(np.sqrt(252))).cpu().numpy()
    if order is not None:
        u = np.empty_like(sd)
        u[order] = sd
        sd = u
    df_std_12["rolling_std_252"] = sd
    df_std_12["jdate"] = df_std_12["dlycaldt"].dt.to_period("M").dt.to_timestamp("M")
    df_std_12.drop_duplicates(subset=["permno", "jdate"], keep="last", inplace=True)
    return pd.merge(left=crsp_comp, right=df_std_12[["permno", "jdate", "rolling_std_252"]],
                    on=["permno", "jdate"], how="left")


# ------------------------------------------------------------------------------------------
# Table 1
# ------------------------------------------------------------------------------------------
def build_table_1(subsets_crsp_comp: dict, variables_dict: dict) -> pd.DataFrame:
    """Lewellen Table 1: per universe and variable, the time-series averages of the monthly
    cross-sectional mean and std (ddof=1) after inf->NaN and dropna, and the number of
    distinct permnos (reference src/calc_Lewellen_2014.py:577-670)."""
    import torch
    partial = []
    for subset_name, df_subset in subsets_crsp_comp.items():
        present = list(dict.fromkeys(c for c in variables_dict.values() if c in df_subset.columns))
        stats = {}
        if present:
            arrays = [_api.as_f64(df_subset[c]) for c in present]
            panel = _E.panel_from_arrays(arrays, present, df_subset["mthcaldt"].values)
            cnt, mean, sd = _E.segment_moments(panel, finite_only=True)
            T = panel.nseg
            C = len(present)
            vals = torch.cat([mean, sd], dim=0).t().contiguous()           # [T, 2C]
            if T:
                am, _, _, an = _api.records_summary_device(vals, nw_lags=0)
            else:
                am, an = np.full(2 * C, np.nan), np.zeros(2 * C, dtype=np.int64)
            dev = panel.device
            allv = torch.from_numpy(np.stack(arrays)).to(dev)                # every row, NaT months too
            ids = torch.from_numpy(df_subset["permno"].to_numpy(dtype=np.int64)).to(dev)
            nuniq = _E.distinct_count(ids, allv, finite_only=True).cpu().numpy()
            tot = cnt.sum(dim=1).cpu().numpy()
            for i, c in enumerate(present):
                stats[c] = (tot[i], am[i] if an[i] else np.nan, am[C + i] if an[C + i] else np.nan,
                            int(nuniq[i]))
        rows = []
        for var_label, var_col in variables_dict.items():
            st = stats.get(var_col)
            if st is None or (st[0] == 0 and st[3] == 0):
                rows.append({"Column": var_label, "Avg": np.nan, "Std": np.nan, "N": np.nan})
            else:
                rows.append({"Column": var_label, "Avg": st[1], "Std": st[2], "N": st[3]})
        part = pd.DataFrame(rows).set_index("Column")
        part.columns = pd.MultiIndex.from_product([[subset_name], part.columns])
        partial.append(part)
    return pd.concat(partial, axis=1)


# ------------------------------------------------------------------------------------------
# Table 2
# ------------------------------------------------------------------------------------------
def _batched_subsets(subsets):
    """If the dict is get_subsets' output, all 9 passes run as one levelled pass on the
    All-stocks frame; returns (frame, level) or None."""
    if not all(k in subsets for k in _LW.SUBSET_NAMES):
        return None
    a = subsets["All stocks"]
    if not {"is_all_but_tiny", "is_large"} <= set(a.columns):
        return None
    abt = a["is_all_but_tiny"].to_numpy(dtype=bool)
    lg = a["is_large"].to_numpy(dtype=bool)
    if (lg & ~abt).any():
        return None
    if len(subsets["All-but-tiny stocks"]) != abt.sum() or len(subsets["Large stocks"]) != lg.sum():
        return None
    return a, abt.astype(np.uint8) + lg.astype(np.uint8)


def _fm_summaries(df, model_cols, level=None, nlevels=1, fig1=False, moments=False, weight_col=None):
    """Device FM pass of several models over one frame (optionally levelled); ``weight_col``: the
    weighted cross-sections (fm_wls) with that column of the frame as row weights."""
    cols = []
    for xs in model_cols.values():
        for c in ["retx"] + list(xs):
            if c not in cols:
                cols.append(c)
    if fig1:
        for c in _LW.FIG1_VARS:
            if c not in cols:
                cols.append(c)
    arrays = [_api.as_f64(df[c]) for c in cols]
    panel = _E.panel_from_arrays(arrays, cols, df["mthcaldt"].values,
                                 me=None if weight_col is None else _api.as_f64(df[weight_col]))
    lvl_t = None
    if level is not None:
        import torch
        lvl_t = torch.from_numpy(np.ascontiguousarray(level[panel.order])).to(panel.device)
    levels = tuple(range(nlevels))
    models = [_E.Model(n, y=panel.col("retx"), xs=[panel.col(c) for c in xs], levels=levels)
              for n, xs in model_cols.items()]
    if weight_col is not None:
        res = _E.fm_pass_wls(panel, models, weight="me", level=lvl_t, nlevels=nlevels, moments=moments)
    else:
        res = _E.fm_pass(panel, models, level=lvl_t, nlevels=nlevels, moments=moments)
    return panel, models, res


def _summary_series(res, k, xs, status_h, rec_h, summ_h):
    mean, se, t, nobs = summ_h
    return _api.summary_from_device(mean[k], se[k], t[k], nobs[k], xs, k_slope0=1, k_r2=res.pmax,
                                    k_n=res.pmax + 1)


def _check_errors(res, status_h, models):
    for k, p in enumerate(res.problems):
        _api.raise_like_reference(status_h[:, k], p.K)


def _format_table_2(stats, subset_names):
    """Table-2 layout of the reference (src/calc_Lewellen_2014.py:797-866): rows
    (Model, Predictor) with a trailing N row per model; columns (subset, Slope/t-stat/R^2);
    3-decimal strings, R^2 only on each model's first row, N with thousands separators."""
    subset_order = ["All stocks", "All-but-tiny stocks", "Large stocks"]
    metrics = ["Slope", "t-stat", "R^2"]
    present = [s for s in subset_order if s in subset_names]
    rows, index = [], []
    for model, labels in _LW.MODELS_PREDICTORS.items():
        for r, lbl in enumerate(labels + ["N"]):
            index.append((model, lbl))
            row = []
            for s in present:
                st = stats.get((model, s))
                for mtr in metrics:
                    v = np.nan
                    if st is not None:
                        if lbl == "N":
                            v = st["mean_N"] if mtr == "Slope" else np.nan
                        elif mtr == "Slope":
                            v = st["coef"][r]
                        elif mtr == "t-stat":
                            v = st["tstat"][r]
                        elif r == 0:
                            v = st["mean_R2"]
                    if v is None or (isinstance(v, float) and np.isnan(v)):
                        row.append("")
                    elif lbl == "N":
                        row.append(f"{int(round(float(v))):,.0f}")
                    else:
                        row.append(f"{float(v):.3f}")
            rows.append(row)
    cols = pd.MultiIndex.from_tuples([(s, m) for s in present for m in metrics], names=[None, None])
    idx = pd.MultiIndex.from_tuples(index, names=["Model", "Predictor"])
    return pd.DataFrame(rows, index=idx, columns=cols, dtype=object)


def build_table_2(subsets_comp_crsp: dict, variables_dict: dict, weight_col: str = None) -> pd.DataFrame:
    """Lewellen Table 2: Fama-MacBeth slopes, NW(4) t-stats, mean R^2 and mean N for
    Models 1-3 on each universe (reference src/calc_Lewellen_2014.py:674-868).  ``weight_col``
    (build-defined, A22; no reference line), e.g. "me": the same table from weighted cross-sections
    (run_monthly_cs_regressions' ``weight_col``)."""
    model_cols = _LW.table2_models(variables_dict)
    stats = {}
    batched = _batched_subsets(subsets_comp_crsp)
    jobs = []
    if batched is not None:
        frame, level = batched
        jobs.append((frame, level, 3, {i: s for i, s in enumerate(_LW.SUBSET_NAMES)}))
    else:
        for s, frame in subsets_comp_crsp.items():
            jobs.append((frame, None, 1, {0: s}))
    for frame, level, nlevels, level_names in jobs:
        panel, models, res = _fm_summaries(frame, model_cols, level, nlevels, weight_col=weight_col)
        status_h = res.status.cpu().numpy()
        # the reference loop order is model-major, subset-minor: raise on the first failure
        order = sorted(range(len(res.problems)), key=lambda k: (res.problems[k].model, res.problems[k].level))
        for k in order:
            if weight_col is not None:
                _api.raise_like_reference_wls(status_h[:, k])
            else:
                _api.raise_like_reference(status_h[:, k], res.problems[k].K)
        summ, _ = _E.summarize_result(res)
        mean, se, t, nobs = (summ.mean.cpu().numpy(), summ.se.cpu().numpy(), summ.tstat.cpu().numpy(),
                             summ.nobs.cpu().numpy())
        for k, p in enumerate(res.problems):
            name = models[p.model].name
            xs = model_cols[name]
            ser = _api.summary_from_device(mean[k], se[k], t[k], nobs[k], xs, k_slope0=1,
                                           k_r2=res.pmax, k_n=res.pmax + 1)
            stats[(name, level_names[p.level])] = {
                "coef": [ser[f"{x}_coef"] for x in xs],
                "tstat": [ser[f"{x}_tstat"] for x in xs],
                "mean_R2": ser["mean_R2"], "mean_N": ser["mean_N"]}
    return _format_table_2(stats, list(subsets_comp_crsp.keys()))


def build_table_2_pooled(subsets_comp_crsp: dict, variables_dict: dict, month_fe: bool = False) -> pd.DataFrame:
    """The robustness table beside Table 2 (build-defined, A23; no reference line): for every Table-2
    (model, universe, predictor) the Fama-MacBeth slope and Newey-West(4) t-statistic -- build_table_2's
    pass, unchanged -- and beside them the slope of ONE pooled panel OLS over all months
    (run_pooled_regression; ``month_fe``: with month fixed effects) with its t-statistics from White,
    month-clustered, firm-clustered (permno) and two-way clustered standard errors.  A firm effect that
    Fama-MacBeth ignores shows as a firm-clustered t well below the FM one (Petersen 2009).  Numeric
    frame: rows (Model, Predictor), columns (universe, "FM slope" / "FM t" / "Pooled slope" / "t white" /
    "t month" / "t firm" / "t twoway").  The frames need ``permno`` and datetime64 or integer
    ``mthcaldt``."""
    model_cols = _LW.table2_models(variables_dict)
    metrics = ["FM slope", "FM t", "Pooled slope", "t white", "t month", "t firm", "t twoway"]
    batched = _batched_subsets(subsets_comp_crsp)
    jobs = []
    if batched is not None:
        frame, level = batched
        jobs.append((frame, level, 3, {i: s for i, s in enumerate(_LW.SUBSET_NAMES)}))
    else:
        for s, frame in subsets_comp_crsp.items():
            jobs.append((frame, None, 1, {0: s}))
    cells = {}
    for frame, level, nlevels, level_names in jobs:
        ids = _firm_ids(frame["permno"], frame["mthcaldt"])
        if ids is None:
            raise ValueError("build_table_2_pooled: 'permno' must hold whole-number firm ids and 'mthcaldt' "
                             "datetime64 or integer months")
        # rows by (month, permno): the order the firm codes of a month must ascend in
        order = np.lexsort((ids, frame["mthcaldt"].to_numpy()))
        frame = frame.iloc[order]
        level = None if level is None else level[order]
        panel, models, res = _fm_summaries(frame, model_cols, level, nlevels)
        status_h = res.status.cpu().numpy()
        for k in sorted(range(len(res.problems)), key=lambda k: (res.problems[k].model, res.problems[k].level)):
            _api.raise_like_reference(status_h[:, k], res.problems[k].K)
        summ, _ = _E.summarize_result(res)
        mean, tstat = summ.mean.cpu().numpy(), summ.tstat.cpu().numpy()
        import torch
        panel.ids = torch.from_numpy(ids[order][panel.order].astype(np.int64)).to(panel.device)
        lvl_t = None if level is None else torch.from_numpy(np.ascontiguousarray(level[panel.order])).to(panel.device)
        pool = _E.pooled_regressions(panel, models, level=lvl_t, nlevels=nlevels, month_fe=month_fe)
        coef, pt = pool.coef.cpu().numpy(), [pool.tstat(kind).cpu().numpy() for kind in ("white", "month", "firm", "twoway")]
        for k, p in enumerate(res.problems):
            name = models[p.model].name
            for r in range(p.K):
                cells[(name, r, level_names[p.level])] = [mean[k, 1 + r], tstat[k, 1 + r], coef[k, 1 + r]] + \
                    [t[k, 1 + r] for t in pt]
    present = [s for s in _LW.SUBSET_NAMES if s in subsets_comp_crsp]
    index, rows = [], []
    for model, labels in _LW.MODELS_PREDICTORS.items():
        for r, lbl in enumerate(labels):
            index.append((model, lbl))
            rows.append([v for s in present for v in cells.get((model, r, s), [np.nan] * len(metrics))])
    return pd.DataFrame(rows, index=pd.MultiIndex.from_tuples(index, names=["Model", "Predictor"]),
                        columns=pd.MultiIndex.from_tuples([(s, m) for s in present for m in metrics]), dtype=np.float64)


# ------------------------------------------------------------------------------------------
# Figure 1
# ------------------------------------------------------------------------------------------
def figure_1_coefficients(subsets_comp_crsp: dict, model_vars=None, window=120, min_periods=60):
    """Numerical core of create_figure_1 (reference :882-926): per subset ('All stocks',
    'Large stocks') the monthly OLS params (const + slopes, has_constant='add', months with
    N < K+1 skipped) and their rolling(window, min_periods) means.  Returns
    {subset: (monthly_df, rolling_df)} indexed by mthcaldt."""
    model_vars = list(model_vars or _LW.FIG1_VARS)
    out = {}
    for name in ["All stocks", "Large stocks"]:
        if name not in subsets_comp_crsp:
            continue
        d = subsets_comp_crsp[name]
        cols = model_vars + ["retx"]
        arrays = [_api.as_f64(d[c]) for c in cols]
        panel = _E.panel_from_arrays(arrays, cols, d["mthcaldt"].values)
        if panel.nrows == 0:
            continue
        K = len(model_vars)
        res = _E.fm_pass(panel, [_E.Model("fig1", y=K, xs=list(range(K)), const_check=False)])
        status = res.status[:, 0].cpu().numpy()
        fitted = (status & _L.FM_ST_FITTED) != 0
        if not fitted.any():
            continue
        if (status[fitted] & _L.FM_ST_INF_IN_X).any():
            raise _api.MissingDataError("exog contains inf or nans")
        ix = _E.compact_result(res)
        roll = _E.rolling_result(res, ix, window, min_periods)[0].cpu().numpy()
        rec = res.rec[:, 0, :].cpu().numpy()
        months = pd.Index(np.asarray(panel.months)[fitted], name="mthcaldt")
        names = ["const"] + model_vars
        monthly = pd.DataFrame(rec[fitted][:, :K + 1], index=months, columns=names)
        rolling = pd.DataFrame(roll[:fitted.sum(), :K + 1], index=months, columns=names)
        out[name] = (monthly, rolling)
    return out


def create_figure_1(subsets_comp_crsp: dict, save_plot: bool = True,
                    output_dir: Union[None, Path] = OUTPUT_DIR) -> tuple:
    """Figure 1: ten-year rolling Fama-MacBeth slopes of the 5-variable model for All and
    Large stocks, two stacked panels (reference src/calc_Lewellen_2014.py:871-957)."""
    import matplotlib
    if os.environ.get("DISPLAY") is None:
        matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    labels = {"log_bm": "B/M", "return_12_2": "Ret12", "log_issues_36": "Issue36",
              "accruals_final": "Accruals", "log_assets_growth": "Log AG"}
    coefs = figure_1_coefficients(subsets_comp_crsp)
    fig, axes = plt.subplots(nrows=2, ncols=1, figsize=(14, 10), sharex=True)
    for ax, name, title in ((axes[0], "All stocks", "Panel A: All Stocks (10-Year Rolling Slopes)"),
                            (axes[1], "Large stocks", "Panel B: Large Stocks (10-Year Rolling Slopes)")):
        if name not in coefs:
            continue
        roll = coefs[name][1]
        for v in _LW.FIG1_VARS:
            ax.plot(roll.index, roll[v], label=labels[v])
        ax.set_title(title)
        ax.set_ylabel("Slope Coefficient")
        if name == "Large stocks":
            ax.set_xlabel("Month")
        ax.legend()
        ax.margins(x=0)
    plt.tight_layout()
    return fig, axes


# ------------------------------------------------------------------------------------------
# Forecast extensions (A7/A8; not in the reference — parity unpinned)
# ------------------------------------------------------------------------------------------
def monthly_coefficients(df: pd.DataFrame, return_col: str, predictor_cols: list,
                         date_col: str = "mthcaldt") -> pd.DataFrame:
    """Per-month intercept and slopes on the run_monthly_cs_regressions row set."""
    predictor_cols = list(predictor_cols)
    names = predictor_cols + [return_col]
    arrays = [_api.as_f64(df[c]) for c in names]
    panel = _E.panel_from_arrays(arrays, names, df[date_col].values)
    K = len(predictor_cols)
    res = _E.fm_pass(panel, [_E.Model("m", y=K, xs=list(range(K)))])
    status = res.status[:, 0].cpu().numpy()
    _api.raise_like_reference(status, K)
    fitted = (status & _L.FM_ST_FITTED) != 0
    rec = res.rec[:, 0, :].cpu().numpy()
    return pd.DataFrame(rec[fitted][:, :K + 1], index=pd.Index(np.asarray(panel.months)[fitted], name=date_col),
                        columns=["const"] + predictor_cols)


def rolling_coefficients(params_df: pd.DataFrame, window=120, min_periods=60, lag=1) -> pd.DataFrame:
    """rolling(window, min_periods) means of the coefficient table, shifted by ``lag`` rows
    (the forecast for month t uses coefficients through t-lag)."""
    import torch
    dev = _E.require_device()
    T, k = params_df.shape
    vals = np.ascontiguousarray(params_df.to_numpy(dtype=np.float64))
    rec = torch.from_numpy(vals).to(dev).view(T, 1, k)
    status = torch.full((T, 1), _L.FM_ST_FITTED, dtype=torch.int32, device=dev)
    ix = _E.ts_compact(status, 1, 1, T, 1)
    out = torch.empty((1, T, k), dtype=torch.float64, device=dev)
    _L.call("fm_rolling_mean", rec.data_ptr(), k, k, ix.idx.data_ptr(), ix.count.data_ptr(), T, 1, k,
            int(window), int(min_periods), out.data_ptr(), _E._stream())
    roll = pd.DataFrame(out[0].cpu().numpy(), index=params_df.index, columns=params_df.columns)
    return roll.shift(lag)


def expected_return_forecasts(df: pd.DataFrame, coef_rolling: pd.DataFrame, predictor_cols: list,
                              date_col: str = "mthcaldt") -> pd.Series:
    """Out-of-sample expected returns F_it = a_{t-1} + sum_k b_{k,t-1} x_ikt (A7); NaN for
    months without a lagged rolling coefficient row or rows with a NaN characteristic."""
    import torch
    predictor_cols = list(predictor_cols)
    arrays = [_api.as_f64(df[c]) for c in predictor_cols]
    panel = _E.panel_from_arrays(arrays, predictor_cols, df[date_col].values)
    c = coef_rolling[["const"] + predictor_cols].reindex(pd.Index(panel.months))
    coef = torch.from_numpy(np.ascontiguousarray(c.to_numpy(dtype=np.float64))).to(panel.device)
    f = _E.forecast(panel, coef).cpu().numpy()
    out = np.full(len(df), np.nan)
    out[panel.order] = f
    return pd.Series(out, index=df.index, name="forecast")


def predictive_slope_regressions(df: pd.DataFrame, forecast, return_col: str = "retx",
                                 date_col: str = "mthcaldt", nw_lags: int = 4):
    """A8: monthly OLS of returns on the forecast, then the FM summary with NW(nw_lags).
    Returns (monthly results frame, summary Series)."""
    d = pd.DataFrame({date_col: df[date_col].values, return_col: df[return_col].values,
                      "forecast": np.asarray(forecast, dtype=np.float64)})
    cs = run_monthly_cs_regressions(d, return_col, ["forecast"], date_col)
    return cs, fama_macbeth_summary(cs, ["forecast"], date_col, nw_lags)


PORTFOLIO_COLUMNS = ["ew_ret", "ew_pred", "vw_ret", "vw_pred"]


def forecast_sorted_portfolios(df: pd.DataFrame, forecast, return_col: str = "retx", weight_col: str = None,
                               nport: int = 10, breakpoints=None, universe: str = None,
                               nyse_breakpoints: bool = False, date_col: str = "mthcaldt", nw_lags: int = 4):
    """A12 (paper Table 5): each month, sort the stocks into ``nport`` portfolios by ``forecast``
    (right-closed bins at the np.quantile levels ``breakpoints``, default k / nport; with
    ``nyse_breakpoints`` from the NYSE rows only) and average each portfolio's realised return
    and forecast, equal- and ``weight_col``-weighted (None: no value weights, NaN columns), on
    the device (fm_portfolio_sort).  ``universe`` in {None, "all_but_tiny", "large"} keeps the
    rows of that get_subsets universe (from ``me`` and ``primaryexch``).
    Returns (monthly, summary): ``monthly`` is indexed by (month, portfolio 0..nport-1 and
    "H-L") with columns ew_ret, ew_pred, vw_ret, vw_pred, n (rows with a return; for "H-L" of
    both ends), sorted months only; ``summary`` is indexed by portfolio with columns
    (column, mean / tstat / nobs): the FM mean and its Newey-West(nw_lags) t-statistic."""
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    f = np.asarray(forecast, dtype=np.float64)
    if f.shape != (len(df),):
        raise ValueError("forecast must hold one value per row of df")
    panel, p = _sorted_panel(df, f, return_col, weight_col, nport, breakpoints, universe, nyse_breakpoints, date_col)
    s = _E.portfolio_summary(p, nw_lags)
    return _portfolio_frames(p.status.cpu().numpy(), p.rec.cpu().numpy(), p.cnt.cpu().numpy(), s.mean.cpu().numpy(),
                             s.tstat.cpu().numpy(), s.nobs.cpu().numpy(), panel.months, nport, date_col)


def _sorted_panel(df, f, return_col, weight_col, nport, breakpoints, universe, nyse_breakpoints, date_col, ids=None,
                  id_col="permno"):
    """forecast_sorted_portfolios' device work: the frame's panel (columns forecast, return and, with
    ``weight_col``, weight; rows by (month, ``id_col``); ``ids``: the firm ids it carries) and its
    ``Portfolios``."""
    keys = df[id_col].to_numpy() if ids is None else ids
    order = np.lexsort((keys, df[date_col].to_numpy()))
    d = df.iloc[order]
    names = ["forecast", return_col] + ([weight_col] if weight_col is not None else [])
    arrays = [f[order], _api.as_f64(d[return_col])] + ([_api.as_f64(d[weight_col])] if weight_col is not None else [])
    need_nyse = nyse_breakpoints or universe is not None
    me = _api.as_f64(d["me"]) if universe is not None else None
    nyse = (d["primaryexch"] == "N").to_numpy().astype(np.uint8) if need_nyse else None
    panel = _E.panel_from_arrays(arrays, names, d[date_col].values, me=me, nyse=nyse,
                                 ids=None if ids is None else ids[order])
    level = _E.universe(panel)[2] if universe is not None else None
    p = _E.portfolio_sort(panel.seg_off, panel.cols[0], panel.cols[1],
                          weight=panel.cols[2] if weight_col is not None else None, level=level, nyse=panel.nyse,
                          nport=nport, q=breakpoints, min_level=_UNIVERSE_LEVEL[universe],
                          nyse_breakpoints=nyse_breakpoints, max_seg_len=panel.max_seg_len)
    return panel, p


def _portfolio_frames(status, rec, cnt, mean, tstat, nobs, months, nport, date_col="mthcaldt"):
    """forecast_sorted_portfolios' (monthly, summary) frames of one sort's host arrays."""
    labels = list(range(nport)) + ["H-L"]
    srt = status == 1
    rec = rec[srt]
    cnt = cnt[srt].astype(np.int64)
    n = np.concatenate([cnt, cnt[:, :1] + cnt[:, -1:]], axis=1)
    index = pd.MultiIndex.from_product([np.asarray(months)[srt], labels], names=[date_col, "portfolio"])
    monthly = pd.DataFrame(rec.reshape(-1, 4), index=index, columns=PORTFOLIO_COLUMNS)
    monthly["n"] = n.reshape(-1)
    summary = pd.DataFrame({(c, stat): v[:, j] for j, c in enumerate(PORTFOLIO_COLUMNS)
                            for stat, v in (("mean", mean), ("tstat", tstat), ("nobs", nobs))},
                           index=pd.Index(labels, name="portfolio"))
    return monthly, summary


def _held_frames(status, rec, members, turnover, mean, tstat, nobs, months, nport, date_col="mthcaldt"):
    """held_sorted_portfolios' (monthly, summary) frames of one sort's host arrays: _portfolio_frames'
    with ``n`` = the month's own members and one more column, ``turnover`` (NaN for "H-L")."""
    monthly, summary = _portfolio_frames(status, rec, members[:, 0, :], mean, tstat, nobs, months, nport, date_col)
    tv = np.concatenate([turnover[status == 1], np.full((int((status == 1).sum()), 1), np.nan)], axis=1)
    monthly["turnover"] = tv.reshape(-1)
    return monthly, summary


def held_sorted_portfolios(df: pd.DataFrame, forecast, hold: int, return_col: str = "retx", weight_col: str = None,
                           nport: int = 10, breakpoints=None, universe: str = None, nyse_breakpoints: bool = False,
                           date_col: str = "mthcaldt", nw_lags: int = 4, id_col: str = "permno"):
    """A19: forecast_sorted_portfolios' sorts held for ``hold`` = k months as overlapping cohorts (the
    calendar-time strategy of Jegadeesh and Titman): in month t the strategy holds, per portfolio,
    the k cohorts formed in months t, .., t-k+1, each followed through the firm's rows of the months
    between (a firm with a gap leaves its cohort), equal-weighted among a cohort's survivors or
    weighted by their current ``weight_col``; the strategy's return is the plain average of the k
    cohort returns (fm_portfolio_sort, fm_month_links, fm_portfolio_hold on the device).  The other
    arguments are forecast_sorted_portfolios'; ``id_col`` holds whole-number firm ids and ``date_col``
    datetime64 or integer months, one row per (month, firm): ValueError otherwise.
    Returns (monthly, summary) in forecast_sorted_portfolios' frame format over the complete months
    (k sorted consecutive calendar months end there): ``n`` is the month's own sorted rows of the
    portfolio, ew_pred / vw_pred average the formation months' predicted returns, and one more
    column, ``turnover``, is the share of the strategy's names replaced that month, (1 - the share of
    the portfolio's names that were in it k months earlier) / k (NaN for "H-L", and where month t-k is
    not a sorted neighbour)."""
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    f = np.asarray(forecast, dtype=np.float64)
    if f.shape != (len(df),):
        raise ValueError("forecast must hold one value per row of df")
    ids = _firm_ids(df[id_col], df[date_col])
    if ids is None:
        raise ValueError(f"held_sorted_portfolios: {id_col!r} must hold whole-number firm ids and {date_col!r} "
                         "datetime64 or integer months")
    panel, p = _sorted_panel(df, f, return_col, weight_col, nport, breakpoints, universe, nyse_breakpoints, date_col,
                             ids=ids, id_col=id_col)
    h = _E.held_portfolios(panel, p, hold, ret=1, weight=panel.cols[2] if weight_col is not None else None)
    s = _E.portfolio_summary(h, nw_lags)
    return _held_frames(*(t.cpu().numpy() for t in (h.status, h.rec, h.members, h.turnover, s.mean, s.tstat, s.nobs)),
                        panel.months, nport, date_col)


def _dist_columns(q):
    """Table 3's column names of the quantile levels ``q``: p10, p90, p2.5, ..."""
    return ["p%g" % (100.0 * float(v)) for v in q]


def forecast_distribution(df: pd.DataFrame, forecast, universe: str = None, q=(0.1, 0.9),
                          date_col: str = "mthcaldt", nw_lags: int = 4):
    """A14 (paper Table 3, univariate properties): each month's cross-sectional mean, standard
    deviation (ddof 1) and np.quantile levels ``q`` of ``forecast`` over the rows with a finite
    forecast, on the device (fm_forecast_dist).  ``universe`` in {None, "all_but_tiny", "large"}
    keeps the rows of that get_subsets universe (from ``me`` and ``primaryexch``).
    Returns (monthly, summary): ``monthly`` is indexed by month with columns mean, std, one per
    level (p10, p90) and n, months without an eligible row absent; ``summary`` is indexed by those
    columns (not n) with columns mean / tstat / nobs: the time-series average and its
    Newey-West(nw_lags) t-statistic."""
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    f = np.asarray(forecast, dtype=np.float64)
    if f.shape != (len(df),):
        raise ValueError("forecast must hold one value per row of df")
    order = np.lexsort((df["permno"].to_numpy(), df[date_col].to_numpy()))
    d = df.iloc[order]
    me = _api.as_f64(d["me"]) if universe is not None else None
    nyse = (d["primaryexch"] == "N").to_numpy().astype(np.uint8) if universe is not None else None
    panel = _E.panel_from_arrays([f[order]], ["forecast"], d[date_col].values, me=me, nyse=nyse)
    level = _E.universe(panel)[2] if universe is not None else None
    dist = _E.forecast_dist_vector(panel.seg_off, panel.cols[0], level=level, min_level=_UNIVERSE_LEVEL[universe],
                                   q=q, max_seg_len=panel.max_seg_len)
    s = _E.forecast_dist_summary(dist, nw_lags)
    return _dist_frames(dist.status[0].cpu().numpy(), dist.rec[0].cpu().numpy(), dist.cnt[0].cpu().numpy(),
                        s.mean[0].cpu().numpy(), s.tstat[0].cpu().numpy(), s.nobs[0].cpu().numpy(), panel.months, q,
                        date_col)


def _dist_frames(status, rec, cnt, mean, tstat, nobs, months, q, date_col="mthcaldt"):
    """forecast_distribution's (monthly, summary) frames of one forecast's host arrays."""
    cols = ["mean", "std"] + _dist_columns(q)
    ok = status == 1
    monthly = pd.DataFrame(rec[ok], index=pd.Index(np.asarray(months)[ok], name=date_col), columns=cols)
    monthly["n"] = cnt[ok].astype(np.int64)
    summary = pd.DataFrame({"mean": mean, "tstat": tstat, "nobs": nobs}, index=pd.Index(cols, name="statistic"))
    return monthly, summary


EXTRAPOLATION_COLUMNS = ["mean", "std", "slope", "intercept", "r2", "mean_1m"]


def forecast_extrapolation(df: pd.DataFrame, forecast, horizon: int, decay: float = 0.9, return_col: str = "retx",
                           universe: str = None, q=(0.1, 0.9), date_col: str = "mthcaldt", id_col: str = "permno",
                           nw_lags: int = 4):
    """A17 (the paper's Section 4, second approach): each month, the monthly ``forecast`` scaled to
    ``horizon`` = k months, G = k * m + (1 + decay + ... + decay^(k-1)) (forecast - m) with m the
    month's mean forecast over the rows with a finite forecast; G's cross-sectional mean, standard
    deviation (ddof 1) and np.quantile levels ``q``; and the compounded k-month ``return_col`` (built
    over the same firm links as ``horizon_returns``) regressed on G over the rows that have one
    (slope, intercept, r2), on the device (fm_forecast_horizon).  ``universe`` in {None,
    "all_but_tiny", "large"} keeps the rows of that get_subsets universe (from ``me`` and
    ``primaryexch``).  ``date_col`` and ``id_col`` as ``horizon_returns`` needs them.
    Returns (monthly, summary): ``monthly`` is indexed by month with columns mean, std, slope,
    intercept, r2, mean_1m (m), one per level (p10, p90), n (rows with a forecast) and n_ret (those
    with a k-month return), months without an eligible row absent; ``summary`` is indexed by those
    columns (not n, n_ret) with columns mean / se / tstat / nobs: the time-series average, its
    Newey-West(nw_lags) standard error and t-statistic."""
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    k = int(horizon)
    if k < 1 or k > _E.MAX_HORIZON:
        raise ValueError(f"forecast_extrapolation: horizon must be 1..{_E.MAX_HORIZON}, got {horizon!r}")
    if not 0.0 < float(decay) <= 1.0:
        raise ValueError(f"forecast_extrapolation: decay must lie in (0, 1], got {decay!r}")
    f = np.asarray(forecast, dtype=np.float64)
    if f.shape != (len(df),):
        raise ValueError("forecast must hold one value per row of df")
    ids = _firm_ids(df[id_col], df[date_col])
    if ids is None:
        raise ValueError(f"forecast_extrapolation: {id_col!r} must hold whole-number firm ids and {date_col!r} "
                         "datetime64 or integer months")
    dates = df[date_col].to_numpy()
    order = np.lexsort((ids, dates))
    d = df.iloc[order]
    me = _api.as_f64(d["me"]) if universe is not None else None
    nyse = (d["primaryexch"] == "N").to_numpy().astype(np.uint8) if universe is not None else None
    panel = _E.panel_from_arrays([f[order], _api.as_f64(d[return_col])], ["forecast", return_col], dates[order],
                                 me=me, nyse=nyse, ids=ids[order])
    level = _E.universe(panel)[2] if universe is not None else None
    ret_k = _E.horizon_return(panel.seg_off, panel.cols[1], _E.month_links(panel, 1), k)
    h = _E.forecast_horizon_vector(panel.seg_off, panel.cols[0], ret_k, float(k), _E.extrapolation_gain(k, decay),
                                   level=level, min_level=_UNIVERSE_LEVEL[universe], q=q,
                                   max_seg_len=panel.max_seg_len)
    s = _E.forecast_horizon_summary(h, nw_lags)
    cols = EXTRAPOLATION_COLUMNS + _dist_columns(q)
    ok = h.status[0].cpu().numpy() == 1
    monthly = pd.DataFrame(h.rec[0].cpu().numpy()[ok], index=pd.Index(np.asarray(panel.months)[ok], name=date_col),
                           columns=cols)
    cnt = h.cnt[0].cpu().numpy()[ok].astype(np.int64)
    monthly["n"], monthly["n_ret"] = cnt[:, 0], cnt[:, 1]
    summary = pd.DataFrame({c: getattr(s, c)[0].cpu().numpy() for c in ("mean", "se", "tstat", "nobs")},
                           index=pd.Index(cols, name="statistic"))
    return monthly, summary


COMPARISON_COLUMNS = ["corr", "slope", "intercept", "res_std", "pred_slope", "pred_intercept", "pred_r2"]


def forecast_comparison(df: pd.DataFrame, forecast_a, forecast_b, return_col: str = "retx", universe: str = None,
                        date_col: str = "mthcaldt", nw_lags: int = 4):
    """A15 (paper Table 4, model comparison): each month, ``forecast_b`` regressed on ``forecast_a``
    across the rows where both are finite (corr, slope, intercept and the residual's ddof-1 standard
    deviation res_std), then ``return_col`` regressed on that residual over the rows that also have
    a return (pred_slope, pred_intercept, pred_r2), on the device (fm_forecast_compare).
    ``universe`` in {None, "all_but_tiny", "large"} keeps the rows of that get_subsets universe
    (from ``me`` and ``primaryexch``).
    Returns (monthly, summary): ``monthly`` is indexed by month with those seven columns, n (rows
    with both forecasts) and n_ret (those with a return), months of fewer than two rows absent;
    ``summary`` is indexed by the seven columns with columns mean / se / tstat / nobs: the
    time-series average, its Newey-West(nw_lags) standard error and t-statistic."""
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    fa, fb = (np.asarray(f, dtype=np.float64) for f in (forecast_a, forecast_b))
    if fa.shape != (len(df),) or fb.shape != (len(df),):
        raise ValueError("forecast_a and forecast_b must hold one value per row of df")
    order = np.lexsort((df["permno"].to_numpy(), df[date_col].to_numpy()))
    d = df.iloc[order]
    me = _api.as_f64(d["me"]) if universe is not None else None
    nyse = (d["primaryexch"] == "N").to_numpy().astype(np.uint8) if universe is not None else None
    panel = _E.panel_from_arrays([fa[order], fb[order], _api.as_f64(d[return_col])], ["a", "b", return_col],
                                 d[date_col].values, me=me, nyse=nyse)
    level = _E.universe(panel)[2] if universe is not None else None
    c = _E.forecast_compare_vector(panel.seg_off, panel.cols[:2], panel.cols[2], [(0, 1, _UNIVERSE_LEVEL[universe])],
                                   level=level, max_seg_len=panel.max_seg_len)
    s = _E.forecast_compare_summary(c, nw_lags)
    ok = c.status[0].cpu().numpy() == 1
    monthly = pd.DataFrame(c.rec[0].cpu().numpy()[ok], index=pd.Index(np.asarray(panel.months)[ok], name=date_col),
                           columns=COMPARISON_COLUMNS)
    cnt = c.cnt[0].cpu().numpy()[ok].astype(np.int64)
    monthly["n"], monthly["n_ret"] = cnt[:, 0], cnt[:, 1]
    summary = pd.DataFrame({k: getattr(s, k)[0].cpu().numpy() for k in ("mean", "se", "tstat", "nobs")},
                           index=pd.Index(COMPARISON_COLUMNS, name="statistic"))
    return monthly, summary


def _pipeline_panel(crsp_comp: pd.DataFrame, variables_dict: dict = None, group_col: str = None):
    """The device panel and the Table-2 models of a crsp_comp frame (rows by (month, permno));
    ``group_col``: the frame's column of group (industry) labels, whose sorted factorisation becomes
    the panel's group codes (what ``group_adjust=...`` in a ``**cfg`` reads)."""
    vd = variables_dict or _LW.VARIABLES_DICT
    model_cols = _LW.table2_models(vd)
    cols = list(dict.fromkeys(["retx"] + [c for xs in model_cols.values() for c in xs] + _LW.FIG1_VARS))
    df = crsp_comp.sort_values(["mthcaldt", "permno"])
    me = _api.as_f64(df["me"])
    nyse = (df["primaryexch"] == "N").to_numpy().astype(np.uint8)
    group = ngroups = None
    if group_col is not None:
        group, uniq = _E.group_codes(df[group_col])
        ngroups = max(len(uniq), 1)
    panel = _E.panel_from_arrays([_api.as_f64(df[c]) for c in cols], cols, df["mthcaldt"].values,
                                 me=me, nyse=nyse, ids=_firm_ids(df["permno"], df["mthcaldt"]),
                                 group=group, ngroups=ngroups)
    return panel, model_cols


def _firm_ids(ids, dates):
    """The int64 firm ids a panel can carry, or None where the frame has no firm identity the
    month links could use: ids that are not whole numbers, or dates that are neither datetime64
    nor integer month numbers (such a panel runs everything but the multi-month horizons)."""
    p = np.asarray(ids)
    if np.asarray(dates).dtype.kind not in "Miu":
        return None
    if p.dtype.kind in "iu":
        return p.astype(np.int64)
    if p.dtype.kind == "f" and len(p) and bool(np.all(np.isfinite(p))) and bool(np.all(p == np.floor(p))) \
            and float(np.abs(p).max()) < 2.0 ** 53:
        return p.astype(np.int64)
    return None


def horizon_returns(df: pd.DataFrame, h: int, return_col: str = "retx", date_col: str = "mthcaldt",
                    id_col: str = "permno") -> pd.DataFrame:
    """A16 (paper Section 4): the compounded ``h``-month return (1 + r_t)(1 + r_t+1) ... (1 + r_t+h-1) - 1
    of every row, over the same firm's rows of the following h - 1 calendar months, as the new column
    f"{return_col}_{h}m"; NaN where one of those months is missing for the firm (a gap in its
    history, or the end of the sample).  Each factor and product is rounded on its own, in that
    order, on the device (fm_month_links, fm_horizon_return).  Returns are decimals.  ``date_col``
    must be datetime64 or integer month numbers, with one row per (month, firm): ValueError
    otherwise.  Returns a copy of the frame, index and row order preserved; rows with a missing date
    get NaN."""
    ids = _firm_ids(df[id_col], df[date_col])
    if ids is None:
        raise ValueError(f"horizon_returns: {id_col!r} must hold whole-number firm ids and {date_col!r} "
                         "datetime64 or integer months")
    dates = df[date_col].to_numpy()
    order = np.lexsort((ids, dates))
    panel = _E.panel_from_arrays([_api.as_f64(df[return_col])[order]], [return_col], dates[order], ids=ids[order])
    link = _E.month_links(panel, 1)
    r = _E.horizon_return(panel.seg_off, panel.cols[0], link, h).cpu().numpy()
    col = np.full(len(df), np.nan)
    col[order[panel.order]] = r
    out = df.copy()
    out[f"{return_col}_{h}m"] = col
    return out


def lewellen_pipeline(crsp_comp: pd.DataFrame, variables_dict: dict = None, **cfg):
    """The whole Table-2 / Figure-1 / forecast pass device-resident from one frame
    (winsorize -> universes -> 3 models x 3 universes + Figure 1 -> NW -> rolling ->
    predictive slopes; with ``portfolios=nport`` also the forecast-sorted portfolios of every
    Table-2 problem; with ``horizon=k, lag>=k`` on compounded k-month returns, the paper's
    Section 4, ``nw_lags`` being the caller's choice: the paper takes 10 for 6 and 16 for 12
    months).  Returns fmcore.lewellen.PipelineResult (device tensors)."""
    panel, model_cols = _pipeline_panel(crsp_comp, variables_dict, cfg.pop("group_col", None))
    return _LW.run_pipeline(panel, _LW.PipelineConfig(**cfg), model_cols=model_cols)


def build_table_5(crsp_comp: pd.DataFrame, variables_dict: dict = None, nport: int = 10,
                  nyse_breakpoints: bool = False, **cfg):
    """Paper Table 5 from ONE device pipeline run (build-defined; no reference line): for every
    Table-2 model and universe, the stocks sorted each month into ``nport`` portfolios on the
    out-of-sample forecast from that problem's lagged rolling coefficients and the winsorized
    characteristics, value weights from ``me`` -- what monthly_coefficients ->
    rolling_coefficients -> expected_return_forecasts -> forecast_sorted_portfolios give per
    (model, universe), without their uploads and refits.  ``cfg``: further PipelineConfig
    fields (window, min_periods, lag, nw_lags, ...).  Returns {(model name, universe name):
    (monthly, summary)} in forecast_sorted_portfolios' frame format."""
    panel, model_cols = _pipeline_panel(crsp_comp, variables_dict, cfg.pop("group_col", None))
    pcfg = _LW.PipelineConfig(**dict(cfg, portfolios=int(nport), portfolio_nyse_breakpoints=bool(nyse_breakpoints)))
    out = _LW.run_pipeline(panel, pcfg, model_cols=model_cols)
    p, s = out.portfolios, out.portfolio_summary
    host = [t.cpu().numpy() for t in (p.status, p.rec, p.cnt, s.mean, s.tstat, s.nobs)]
    frames = {}
    for j, k in enumerate(out.portfolio_problems):
        prob = out.res.problems[k]
        key = (out.model_names[prob.model], _LW.SUBSET_NAMES[prob.level])
        frames[key] = _portfolio_frames(*(h[j] for h in host), panel.months, int(nport))
    return frames


def build_table_5_held(crsp_comp: pd.DataFrame, hold: int, nport: int = 10, nyse_breakpoints: bool = False, **cfg):
    """build_table_5's portfolios held for ``hold`` months (build-defined A19; no reference line), from
    the same ONE device pipeline run plus one launch: for every Table-2 model and universe the
    overlapping-cohort strategy of held_sorted_portfolios on that problem's sorts, value weights from
    ``me``.  ``cfg``: further PipelineConfig fields.  Returns {(model name, universe name): (monthly,
    summary)} in held_sorted_portfolios' frame format."""
    panel, model_cols = _pipeline_panel(crsp_comp, None, cfg.pop("group_col", None))
    pcfg = _LW.PipelineConfig(**dict(cfg, portfolios=int(nport), portfolio_nyse_breakpoints=bool(nyse_breakpoints),
                                     portfolio_hold=hold))
    out = _LW.run_pipeline(panel, pcfg, model_cols=model_cols)
    h, s = out.held, out.held_summary
    host = [t.cpu().numpy() for t in (h.status, h.rec, h.members, h.turnover, s.mean, s.tstat, s.nobs)]
    frames = {}
    for j, k in enumerate(out.portfolio_problems):
        prob = out.res.problems[k]
        key = (out.model_names[prob.model], _LW.SUBSET_NAMES[prob.level])
        frames[key] = _held_frames(*(x[j] for x in host), panel.months, int(nport))
    return frames


def _month_rows(index, months, what):
    """Row of ``index`` (dates, or the panel's own month numbers) for each of the panel's
    ``months``, matched by calendar year and month; -1 where the month is absent."""
    months = np.asarray(months)
    if months.dtype.kind == "M":
        have = pd.DatetimeIndex(index).values.astype("datetime64[M]")
        want = months.astype("datetime64[M]")
    else:
        have, want = np.asarray(index), months
    if len(np.unique(have)) != len(have):
        raise ValueError(f"build_table_alphas: {what} holds a month twice")
    at = {v: i for i, v in enumerate(have.tolist())}
    return np.array([at.get(v, -1) for v in want.tolist()], dtype=np.int64)


def _month_aligned(values, index, months, what):
    """``values`` [rows(, K)] re-indexed to the panel's months: NaN rows for the months absent."""
    rows = _month_rows(index, months, what)
    v = np.asarray(values, dtype=np.float64)
    out = np.full((len(rows),) + v.shape[1:], np.nan)
    out[rows >= 0] = v[rows[rows >= 0]]
    return out


ALPHA_COLUMNS = ["alpha", "t", "t_hac", "R2", "nobs"]


def build_table_alphas(crsp_comp: pd.DataFrame, factors: pd.DataFrame, rf=None, models: dict = None, nport: int = 10,
                       **cfg):
    """The factor-model alphas of build_table_5's portfolios from the same ONE device pipeline run
    (build-defined A18; no reference line; the second table of the paper's portfolio section,
    "Alphas for expected-return sorted portfolios" in the 2014 working paper): every portfolio's and
    the high-minus-low spread's monthly return, equal- and value-weighted, regressed on factor returns.
    ``factors``: a DataFrame of monthly factor returns (decimals, like the returns) indexed by date,
    matched to the panel's months by calendar year and month; a month absent from it, or with a NaN
    factor of the model, drops out of that model's regressions.  ``rf``: the risk-free rate as a
    column name of ``factors`` (which is then no factor) or a Series indexed by date; it is
    subtracted from the portfolios' returns, not from the spread.  ``models``: {name: [factor
    columns]}, default {"CAPM": [the first column], "FF": all columns}.  ``cfg``: further
    PipelineConfig fields (window, min_periods, lag, nw_lags, alpha_nw_lags, ...); with
    ``portfolio_hold=k`` among them the regressions are those of the portfolios held for k months
    (build_table_5_held's monthly records) instead of the one-month portfolios.
    Returns {(model name, universe name): DataFrame} with build_table_5's portfolio labels as rows and
    the columns (weighting, "", Avg / Std / Shp) -- the mean and standard deviation of the (excess)
    return over the first model's months and the annualised Sharpe ratio Avg / Std * sqrt(12) -- and
    (weighting, factor model, alpha / t / t_hac / R2 / nobs): the intercept, its classical and
    Newey-West t-statistics, the regression's R2 and the months it used."""
    panel, model_cols = _pipeline_panel(crsp_comp, None, cfg.pop("group_col", None))
    fcols = [c for c in factors.columns if not (isinstance(rf, str) and c == rf)]
    if isinstance(rf, str) and rf not in factors.columns:
        raise ValueError(f"build_table_alphas: factors has no column {rf!r}")
    if models is None:
        models = {"CAPM": fcols[:1]}
        if len(fcols) > 1:
            models["FF"] = list(fcols)
    for name, cols in models.items():
        missing = [c for c in cols if c not in fcols]
        if missing:
            raise ValueError(f"build_table_alphas: model {name!r} names {missing}, not among the factors {fcols}")
    F = _month_aligned(factors[fcols].to_numpy(dtype=np.float64), factors.index, panel.months, "factors")
    if rf is None:
        R = None
    elif isinstance(rf, str):
        R = _month_aligned(factors[rf].to_numpy(dtype=np.float64), factors.index, panel.months, "factors")
    else:
        R = _month_aligned(np.asarray(rf, dtype=np.float64), rf.index, panel.months, "rf")
    pcfg = _LW.PipelineConfig(**dict(cfg, portfolios=int(nport), alpha_factors=F, alpha_rf=R,
                                     alpha_models=[[fcols.index(c) for c in cols] for cols in models.values()]))
    out = _LW.run_pipeline(panel, pcfg, model_cols=model_cols)
    a = out.portfolio_alphas if pcfg.portfolio_hold is None else out.held_alphas
    coef, t, th, stat, nobs = (x.cpu().numpy() for x in (a.coef, a.tstat, a.tstat_hac, a.stat, a.nobs))
    labels = pd.Index(list(range(int(nport))) + ["H-L"], name="portfolio")
    frames = {}
    for j, k in enumerate(out.portfolio_problems):
        prob = out.res.problems[k]
        data = {}
        for w, wn in enumerate(("ew", "vw")):
            avg, std = stat[j, :, w, 0, 2], stat[j, :, w, 0, 3]
            data[(wn, "", "Avg")], data[(wn, "", "Std")] = avg, std
            data[(wn, "", "Shp")] = avg / std * np.sqrt(12.0)
            for m, name in enumerate(models):
                for c, v in zip(ALPHA_COLUMNS, (coef[j, :, w, m, 0], t[j, :, w, m, 0], th[j, :, w, m, 0],
                                                stat[j, :, w, m, 0], nobs[j, :, w, m])):
                    data[(wn, name, c)] = v
        frames[(out.model_names[prob.model], _LW.SUBSET_NAMES[prob.level])] = pd.DataFrame(data, index=labels)
    return frames


DOUBLE_SORT_COLUMNS = ["ew_ret", "vw_ret", "ew_a", "ew_b"]


def _dsort_grid(rb, ra, na, nb):
    """The two record views of one double sort, rb [..., na+1, nb+1, 4] (slab, row) and ra [..., nb+1,
    na+1, 4], as one grid [..., na+2, nb+2, 4] over the labels (0..na-1, "H-L", "avg") x (0..nb-1,
    "H-L", "avg") with DOUBLE_SORT_COLUMNS; NaN where the device holds no such number: a margin has
    the mean of the signal its view sorts on only, and the corners ("H-L", "H-L") and ("avg", "avg")
    are not defined."""
    ra = np.swapaxes(ra, -3, -2)    # [..., i <= na, j <= nb, 4]: i = na the H-L of a, j = nb the b-neutral slab
    g = np.full(rb.shape[:-3] + (na + 2, nb + 2, 4), np.nan)
    g[..., :na, :nb + 1, 0], g[..., :na, :nb + 1, 1], g[..., :na, :nb + 1, 3] = (rb[..., :na, :, c] for c in (0, 2, 1))
    g[..., :na, :nb, 2] = ra[..., :na, :nb, 1]
    g[..., na + 1, :nb + 1, 0], g[..., na + 1, :nb + 1, 1], g[..., na + 1, :nb + 1, 3] = (rb[..., na, :, c] for c in (0, 2, 1))
    g[..., na, :nb, 0], g[..., na, :nb, 1], g[..., na, :nb, 2] = (ra[..., na, :nb, c] for c in (0, 2, 1))
    g[..., :na + 1, nb + 1, 0], g[..., :na + 1, nb + 1, 1], g[..., :na + 1, nb + 1, 2] = (ra[..., :, nb, c] for c in (0, 2, 1))
    return g


def _dsort_counts(cnt):
    """cnt [T, na, nb] -> [T, na+2, nb+2]: the rows behind every entry of _dsort_grid (both ends of a
    spread, all cells of an average; 0 in the two undefined corners)."""
    T, na, nb = cnt.shape
    n = np.zeros((T, na + 2, nb + 2), dtype=np.int64)
    n[:, :na, :nb] = cnt
    n[:, :na, nb] = cnt[:, :, 0] + cnt[:, :, -1]
    n[:, na, :nb] = cnt[:, 0, :] + cnt[:, -1, :]
    n[:, :na, nb + 1] = cnt.sum(axis=2)
    n[:, na + 1, :nb] = cnt.sum(axis=1)
    n[:, na + 1, nb] = n[:, :na, nb].sum(axis=1)
    n[:, na, nb + 1] = n[:, na, :nb].sum(axis=1)
    return n


def _dsort_frames(status, rec_b, rec_a, cnt, sb, sa, months, na, nb, date_col="mthcaldt"):
    """double_sorted_portfolios' (monthly, summary) frames of one sort's host arrays: rec_b [na+1, T,
    nb+1, 4], rec_a [nb+1, T, na+1, 4], cnt [T, na, nb], sb / sa = (mean, tstat, nobs) of the two views."""
    la, lb = list(range(na)) + ["H-L", "avg"], list(range(nb)) + ["H-L", "avg"]
    srt = status == 1
    g = _dsort_grid(np.moveaxis(rec_b, 1, 0)[srt], np.moveaxis(rec_a, 1, 0)[srt], na, nb)
    index = pd.MultiIndex.from_product([np.asarray(months)[srt], la, lb], names=[date_col, "a_bin", "b_bin"])
    monthly = pd.DataFrame(g.reshape(-1, 4), index=index, columns=DOUBLE_SORT_COLUMNS)
    monthly["n"] = _dsort_counts(cnt[srt].astype(np.int64)).reshape(-1)
    stats = [_dsort_grid(b, a, na, nb) for b, a in zip(sb, sa)]   # mean, tstat, nobs: [na+2, nb+2, 4]
    summary = pd.DataFrame({(c, stat): v[..., j].reshape(-1) for j, c in enumerate(DOUBLE_SORT_COLUMNS)
                            for stat, v in zip(("mean", "tstat", "nobs"), stats)},
                           index=pd.MultiIndex.from_product([la, lb], names=["a_bin", "b_bin"]))
    return monthly, summary


def _signal(df, x, what):
    """A column name or one value per row -> float64 [rows]."""
    v = _api.as_f64(df[x]) if isinstance(x, str) else np.asarray(x, dtype=np.float64)
    if v.shape != (len(df),):
        raise ValueError(f"{what} must be a column name or hold one value per row of df")
    return v


def _double_sort_frame(df, a, bs, return_col, weight_col, universe, nyse_breakpoints, date_col, **kw):
    """The device work of the two functions below: the frame's panel (rows by (month, input order))
    and the ``DoubleSort`` of signal ``a`` against every signal of ``bs``, in one launch."""
    import torch
    if universe not in _UNIVERSE_LEVEL:
        raise ValueError(f"universe must be one of {list(_UNIVERSE_LEVEL)}")
    names = ["a"] + [f"b{j}" for j in range(len(bs))] + ["ret"] + (["weight"] if weight_col is not None else [])
    arrays = [a] + list(bs) + [_api.as_f64(df[return_col])] + ([_api.as_f64(df[weight_col])] if weight_col is not None else [])
    me = _api.as_f64(df["me"]) if universe is not None else None
    nyse = (df["primaryexch"] == "N").to_numpy().astype(np.uint8) if (nyse_breakpoints or universe is not None) else None
    panel = _E.panel_from_arrays(arrays, names, df[date_col].values, me=me, nyse=nyse)
    level = _E.universe(panel)[2] if universe is not None else None
    nb_ = len(bs)
    ds = _E.double_sort(panel.seg_off, panel.cols[0], panel.cols[1:1 + nb_], panel.cols[1 + nb_],
                        weight=panel.cols[2 + nb_] if weight_col is not None else None, level=level, nyse=panel.nyse,
                        min_level=_UNIVERSE_LEVEL[universe], nyse_breakpoints=nyse_breakpoints,
                        max_seg_len=panel.max_seg_len, **kw)
    torch.cuda.synchronize()
    return panel, ds


def double_sorted_portfolios(df: pd.DataFrame, a, b, return_col: str = "retx", weight_col: str = None, na: int = 5,
                             nb: int = 5, breakpoints_a=None, breakpoints_b=None, conditional: bool = False,
                             universe: str = None, nyse_breakpoints: bool = False, date_col: str = "mthcaldt",
                             nw_lags: int = 4):
    """A21: each month, sort the stocks two ways -- on ``a`` into ``na`` bins and on ``b`` into ``nb``
    (column names or one value per row), independently or, with ``conditional``, b within each a-bin
    -- at the np.quantile levels ``breakpoints_a`` / ``breakpoints_b`` (default k / na, k / nb; with
    ``nyse_breakpoints`` from the NYSE rows only), and average each cell's realised return and its two
    signals, equal- and ``weight_col``-weighted, on the device (fm_portfolio_double_sort).
    ``universe`` as in forecast_sorted_portfolios.
    Returns (monthly, summary): ``monthly`` is indexed by (month, a_bin, b_bin), the bins 0..n-1 plus
    the margins "H-L" (last bin minus first along that axis) and "avg" (the average across that
    axis' bins: ("avg", "H-L") is the a-neutral spread of b), with columns ew_ret, vw_ret, ew_a,
    ew_b and n (rows with a return), sorted months only; a margin carries the mean of the signal it
    is sorted on, NaN for the other, and the corners ("H-L", "H-L") and ("avg", "avg") are NaN.
    ``summary`` is indexed by (a_bin, b_bin) with columns (column, mean / tstat / nobs): the FM mean
    and its Newey-West(nw_lags) t-statistic."""
    panel, ds = _double_sort_frame(df, _signal(df, a, "a"), [_signal(df, b, "b")], return_col, weight_col, universe,
                                   nyse_breakpoints, date_col, na=na, nb=nb, qa=breakpoints_a, qb=breakpoints_b,
                                   conditional=conditional)
    sb, sa = _E.portfolio_summary(ds.by_b, nw_lags), _E.portfolio_summary(ds.by_a, nw_lags)
    host = lambda s: [t.cpu().numpy() for t in (s.mean, s.tstat, s.nobs)]
    return _dsort_frames(ds.status[0].cpu().numpy(), ds.rec_b[0].cpu().numpy(), ds.rec_a[0].cpu().numpy(),
                         ds.cnt[0].cpu().numpy(), host(sb), host(sa), panel.months, int(na), int(nb), date_col)


def characteristic_factors(df: pd.DataFrame, char_cols, size_col: str = "me", weight_col: str = "me",
                           breakpoints_size=(0.5,), breakpoints_char=(0.3, 0.7), nyse_breakpoints: bool = True,
                           universe: str = None, return_col: str = "retx", date_col: str = "mthcaldt") -> pd.DataFrame:
    """A21: factor returns built from the panel itself.  Each month the stocks are sorted
    independently on ``size_col`` (breakpoints ``breakpoints_size``, the median) and on every column of
    ``char_cols`` (``breakpoints_char``, 30 / 70 per cent), at NYSE breakpoints, all characteristics
    in one batched launch; the cells' returns are ``weight_col``-weighted (None: equal-weighted).
    Returns a DataFrame indexed by month with one column per characteristic -- the size-neutral
    high-minus-low return, i.e. the average over the size groups of (top minus bottom characteristic
    group) -- and "SMB": minus the mean over the characteristics of the characteristic-neutral
    size spread (small minus big).  NaN in months that could not be sorted.  ``build_table_alphas``
    takes the frame as ``factors``.
    What this is not: the Fama-French factors.  The sorts are rebalanced every month on the rows' own
    values of that month: there is no June formation, no six-month accounting lag, and nothing is
    held between rebalancing dates.  Lagging the weight (last month's market equity) is the caller's
    job, through ``weight_col``."""
    char_cols = list(char_cols)
    if not char_cols:
        raise ValueError("characteristic_factors: char_cols is empty")
    bs = [_signal(df, c, c) for c in char_cols]
    panel, ds = _double_sort_frame(df, _signal(df, size_col, "size_col"), bs, return_col, weight_col, universe,
                                   nyse_breakpoints, date_col, na=len(breakpoints_size) + 1,
                                   nb=len(breakpoints_char) + 1, qa=breakpoints_size, qb=breakpoints_char)
    weighted = weight_col is not None
    hml = _E.sort_factors(ds, "b", weighted).cpu().numpy()           # [T, nchar]
    smb = -_E.sort_factors(ds, "a", weighted).cpu().numpy().mean(axis=1)
    out = pd.DataFrame(hml, index=pd.Index(np.asarray(panel.months), name=date_col), columns=char_cols)
    out["SMB"] = smb
    return out


def build_table_double_sort(crsp_comp: pd.DataFrame, by: str = "log_size", variables_dict: dict = None, shape=(5, 5),
                            **cfg):
    """build_table_5's spread controlled for ``by`` (build-defined A21; no reference line), from ONE
    device pipeline run: for every Table-2 model and universe the stocks are sorted each month into
    ``shape`` = (na, nb) cells, na bins of the panel column ``by`` (size) by nb bins of the
    out-of-sample forecast (``conditional=True``: the forecast within each bin of ``by``).  ``cfg``:
    further PipelineConfig fields (portfolios: the single sort's nport, default 10;
    portfolio_nyse_breakpoints; window, min_periods, lag, nw_lags, ...).
    Returns {(model name, universe name): DataFrame} with the rows 0..na-1 (the bins of ``by``) and
    "avg" (the ``by``-neutral portfolios) and the columns (weighting, 0..nb-1): the mean realised
    return of the cell, (weighting, "H-L"): the row's high-minus-low forecast spread and (weighting,
    "t(H-L)"): its Newey-West t-statistic."""
    panel, model_cols = _pipeline_panel(crsp_comp, variables_dict, cfg.pop("group_col", None))
    na, nb = (int(v) for v in shape)
    conditional = bool(cfg.pop("conditional", False))
    cfg.setdefault("portfolios", 10)
    pcfg = _LW.PipelineConfig(**dict(cfg, double_sort=by, double_sort_shape=(na, nb), double_sort_conditional=conditional))
    out = _LW.run_pipeline(panel, pcfg, model_cols=model_cols)
    sb = out.double_sort_summary[0]
    mean, tstat = sb.mean.cpu().numpy(), sb.tstat.cpu().numpy()   # [nsort, na+1, nb+1, 4]
    rows = pd.Index(list(range(na)) + ["avg"], name=by)
    frames = {}
    for j, k in enumerate(out.portfolio_problems):
        prob = out.res.problems[k]
        data = {}
        for wn, c in (("ew", 0), ("vw", 2)):
            for jj in range(nb):
                data[(wn, jj)] = mean[j, :, jj, c]
            data[(wn, "H-L")] = mean[j, :, nb, c]
            data[(wn, "t(H-L)")] = tstat[j, :, nb, c]
        frames[(out.model_names[prob.model], _LW.SUBSET_NAMES[prob.level])] = pd.DataFrame(data, index=rows)
    return frames


def build_table_3(crsp_comp: pd.DataFrame, variables_dict: dict = None, q=(0.1, 0.9), **cfg):
    """Paper Table 3 from ONE device pipeline run (build-defined; no reference line): for every
    Table-2 model and universe, the univariate properties of the out-of-sample forecast from that
    problem's lagged rolling coefficients and the winsorized characteristics -- the time-series
    averages of each month's cross-sectional mean (``Avg``), standard deviation (``Std``) and
    ``q`` quantiles (``p10``, ``p90``) -- beside its predictive ability: the Fama-MacBeth slope of
    returns on the forecast, its Newey-West standard error and t-statistic and the average R2
    (``PipelineResult.pred_summary`` as it stands).  ``cfg``: further PipelineConfig fields
    (window, min_periods, lag, nw_lags, ...).  Returns a DataFrame indexed by (model, universe)."""
    panel, model_cols = _pipeline_panel(crsp_comp, variables_dict, cfg.pop("group_col", None))
    pcfg = _LW.PipelineConfig(**dict(cfg, forecast_dist=True, forecast_dist_q=tuple(q)))
    out = _LW.run_pipeline(panel, pcfg, model_cols=model_cols)
    dmean = out.forecast_dist_summary.mean.cpu().numpy()
    ps = out.pred_summary
    pmean, pse, pt = ps.mean.cpu().numpy(), ps.se.cpu().numpy(), ps.tstat.cpu().numpy()
    keys, rows = [], []
    for j, k in enumerate(out.forecast_dist_problems):
        prob = out.res.problems[k]
        keys.append((out.model_names[prob.model], _LW.SUBSET_NAMES[prob.level]))
        rows.append(list(dmean[j]) + [pmean[k, 0], pse[k, 0], pt[k, 0], pmean[k, 1]])
    return pd.DataFrame(rows, index=pd.MultiIndex.from_tuples(keys, names=["model", "universe"]),
                        columns=["Avg", "Std"] + _dist_columns(q) + ["Slope", "S.E.", "t-stat", "R2"])


def build_table_3_extrapolated(crsp_comp: pd.DataFrame, horizon: int, variables_dict: dict = None, decay: float = 0.9,
                               q=(0.1, 0.9), **cfg):
    """The lower panels of the paper's Tables 9a / 9b (horizon 6 / 12) from ONE device pipeline run
    (build-defined A17; no reference line): build_table_3's frame for the monthly forecasts
    extrapolated to ``horizon`` months, F_ik = k * mean + (1 + decay + ... + decay^(k-1)) (F_i1 - mean)
    with the mean taken over the universe each month -- the time-series averages of each month's
    cross-sectional mean (``Avg``), standard deviation (``Std``) and ``q`` quantiles of F_ik, and the
    Fama-MacBeth slope of the compounded ``horizon``-month return on F_ik with its Newey-West
    standard error, t-statistic and the average R2.  The regressions and forecasts stay monthly
    (``PipelineConfig(extrapolate=horizon)``).  ``cfg``: further PipelineConfig fields;
    ``extrapolate_nw_lags`` is the caller's choice (the paper uses 10 lags for 6 and 16 for 12 months;
    the default is ``nw_lags``).  Returns a DataFrame indexed by (model, universe)."""
    panel, model_cols = _pipeline_panel(crsp_comp, variables_dict, cfg.pop("group_col", None))
    pcfg = _LW.PipelineConfig(**dict(cfg, extrapolate=horizon, extrapolate_decay=decay, extrapolate_q=tuple(q)))
    out = _LW.run_pipeline(panel, pcfg, model_cols=model_cols)
    s = out.extrapolated_summary
    mean, se, t = s.mean.cpu().numpy(), s.se.cpu().numpy(), s.tstat.cpu().numpy()
    keys, rows = [], []
    for j, k in enumerate(out.extrapolated_problems):
        prob = out.res.problems[k]
        keys.append((out.model_names[prob.model], _LW.SUBSET_NAMES[prob.level]))
        rows.append([mean[j, 0], mean[j, 1]] + list(mean[j, _L.FM_FHOR_NREC:]) + [mean[j, 2], se[j, 2], t[j, 2], mean[j, 4]])
    return pd.DataFrame(rows, index=pd.MultiIndex.from_tuples(keys, names=["model", "universe"]),
                        columns=["Avg", "Std"] + _dist_columns(q) + ["Slope", "S.E.", "t-stat", "R2"])


def build_table_4(crsp_comp: pd.DataFrame, variables_dict: dict = None, **cfg):
    """Paper Table 4 (model comparison) from ONE device pipeline run (build-defined; no reference
    line): for every universe and every pair i < j of the Table-2 models, how much of model j's
    out-of-sample forecast model i's already holds -- the time-series averages of each month's
    cross-sectional ``Correlation``, ``Slope`` and residual standard deviation (``Res. std.``) of
    forecast j regressed on forecast i -- and whether the rest predicts returns: the Fama-MacBeth
    slope of returns on that residual (``Pred. slope``) with its Newey-West standard error and
    t-statistic.  ``cfg``: further PipelineConfig fields (window, min_periods, lag, nw_lags, ...).
    Returns a DataFrame indexed by (universe, "Model j on Model i")."""
    panel, model_cols = _pipeline_panel(crsp_comp, variables_dict, cfg.pop("group_col", None))
    out = _LW.run_pipeline(panel, _LW.PipelineConfig(**dict(cfg, forecast_compare=True)), model_cols=model_cols)
    s = out.forecast_compare_summary
    mean, se, t = s.mean.cpu().numpy(), s.se.cpu().numpy(), s.tstat.cpu().numpy()
    keys, rows = [], []
    for p, (ka, kb) in enumerate(out.forecast_compare_pairs):
        pa, pb = out.res.problems[ka], out.res.problems[kb]
        short = [out.model_names[q.model].split(":")[0] for q in (pb, pa)]
        keys.append((_LW.SUBSET_NAMES[pa.level], "%s on %s" % tuple(short)))
        rows.append([mean[p, 0], mean[p, 1], mean[p, 3], mean[p, 4], se[p, 4], t[p, 4]])
    return pd.DataFrame(rows, index=pd.MultiIndex.from_tuples(keys, names=["universe", "comparison"]),
                        columns=["Correlation", "Slope", "Res. std.", "Pred. slope", "S.E.", "t-stat"])


def build_table_2_horizon(crsp_comp: pd.DataFrame, horizon: int, variables_dict: dict = None, **cfg):
    """Paper Tables 8a / 8b (horizon 6 / 12) from ONE device pipeline run (build-defined A16; no
    reference line): Table 2 with the compounded ``horizon``-month return as the dependent variable --
    Fama-MacBeth slopes, Newey-West t-statistics, mean R^2 and mean N of Models 1-3 on each universe,
    in build_table_2's frame format.  ``cfg``: further PipelineConfig fields; ``nw_lags`` is the
    caller's choice (the paper uses 10 lags for 6-month and 16 for 12-month returns; the default is
    PipelineConfig's 4) and ``lag`` defaults to the horizon.  Returns are decimals, so the slopes are
    1/100 of the paper's, which regresses percent returns."""
    panel, model_cols = _pipeline_panel(crsp_comp, variables_dict, cfg.pop("group_col", None))
    pcfg = _LW.PipelineConfig(**dict({"lag": max(int(horizon), 1)}, **cfg, horizon=horizon))
    out = _LW.run_pipeline(panel, pcfg, model_cols=model_cols)
    res, s = out.res, out.summary
    status_h = res.status.cpu().numpy()
    order = sorted(range(len(res.problems)), key=lambda k: (res.problems[k].model, res.problems[k].level))
    for k in order:
        if out.model_names[res.problems[k].model] != "Figure 1":
            _api.raise_like_reference(status_h[:, k], res.problems[k].K)
    mean, se, t, nobs = (x.cpu().numpy() for x in (s.mean, s.se, s.tstat, s.nobs))
    stats = {}
    for k, p in enumerate(res.problems):
        name = out.model_names[p.model]
        if name == "Figure 1":
            continue
        xs = model_cols[name]
        ser = _api.summary_from_device(mean[k], se[k], t[k], nobs[k], xs, k_slope0=1, k_r2=res.pmax,
                                       k_n=res.pmax + 1)
        stats[(name, _LW.SUBSET_NAMES[p.level])] = {
            "coef": [ser[f"{x}_coef"] for x in xs], "tstat": [ser[f"{x}_tstat"] for x in xs],
            "mean_R2": ser["mean_R2"], "mean_N": ser["mean_N"]}
    return _format_table_2(stats, list(_LW.SUBSET_NAMES))
