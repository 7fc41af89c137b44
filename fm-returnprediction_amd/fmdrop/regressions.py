"""Drop-in replacement for the reference's src/regressions.py, on MI355X.

Same names, signatures, return types, column/key order and error behaviour as
BaileyMeche/FM-ReturnPrediction src/regressions.py:9-131; the per-month OLS, the
Newey-West errors and the time-series means run in libfm_hip kernels (fm_gram, fm_solve,
fm_ts_summary) through ctypes.  statsmodels is not needed.
"""

import numpy as np
import pandas as pd

from fmcore import api as _api
from fmcore import engine as _E

MissingDataError = _api.MissingDataError


def run_monthly_cs_regressions(df: pd.DataFrame, return_col: str, predictor_cols: list,
                               date_col: str = "mthcaldt", weight_col: str = None) -> pd.DataFrame:
    """Per-month cross-sectional OLS of ``return_col`` on an intercept and
    ``predictor_cols`` (reference src/regressions.py:9-76).

    Rows with NaN in any of [return_col, date_col] + predictor_cols are dropped; months
    with fewer than K+1 rows are skipped; returns one row per fitted month with columns
    [date_col, 'N', 'R2', 'slope_<col>'...] in ascending month order.

    ``weight_col`` (build-defined, A22; no reference line): the frame's column of row weights, e.g.
    "me": every month is then a weighted least-squares fit (statsmodels' WLS; fm_wls), R2 its
    weighted R2 and N the rows used -- rows whose weight is NaN, infinite, zero or negative drop out
    too.  The same frame and columns; months whose regressors are collinear or constant
    (FM_ST_RANK_DEF) are absent like skipped months, an inf regressor raises MissingDataError.
    """
    predictor_cols = list(predictor_cols)
    sub = df[[return_col, date_col] + predictor_cols]
    names = predictor_cols + [return_col]
    arrays = [_api.as_f64(sub[c]) for c in names]
    K = len(predictor_cols)
    if weight_col is not None:
        panel = _E.panel_from_arrays(arrays, names, sub[date_col].values, me=_api.as_f64(df[weight_col]))
        res = _E.fm_pass_wls(panel, [_E.Model("m", y=K, xs=list(range(K)))], weight="me")
    else:
        panel = _E.panel_from_arrays(arrays, names, sub[date_col].values)
        res = _E.fm_pass(panel, [_E.Model("m", y=K, xs=list(range(K)))])
    status = res.status[:, 0].cpu().numpy()
    rec = res.rec[:, 0, :].cpu().numpy()
    if weight_col is not None:
        _api.raise_like_reference_wls(status)
    else:
        _api.raise_like_reference(status, K)
    return _api.cs_frame(panel.months, rec, status, res.pmax, predictor_cols, date_col)


def newey_west_mean_se(slopes: np.ndarray, lags: int = 4) -> float:
    """Newey-West standard error of the mean with weights 1-k/T (reference
    src/regressions.py:78-100)."""
    x = np.asarray(slopes, dtype=float)
    T = x.size
    if T < 2:
        return np.nan
    if not np.all(np.isfinite(x)):
        return np.nan   # the reference's arithmetic turns any NaN/inf into NaN here
    _, se, _, _ = _api.records_summary(x.reshape(T, 1), nw_lags=int(lags))
    return float(se[0])


def fama_macbeth_summary(cs_results: pd.DataFrame, predictor_cols: list, date_col="mthcaldt",
                         nw_lags=4) -> pd.Series:
    """Time-series means of the monthly slopes with Newey-West t-stats, plus mean R2
    and mean N (reference src/regressions.py:102-131)."""
    predictor_cols = list(predictor_cols)
    cols = [cs_results[f"slope_{c}"] for c in predictor_cols]
    r2 = cs_results["R2"]
    n = cs_results["N"]
    T = len(cs_results)
    if T == 0:
        out = {}
        for c in predictor_cols:
            out[f"{c}_coef"] = np.nan
            out[f"{c}_tstat"] = np.nan
        out["mean_R2"] = np.nan
        out["mean_N"] = np.nan
        return pd.Series(out, dtype=np.float64)
    vals = np.column_stack([_api.as_f64(c) for c in cols] + [_api.as_f64(r2), _api.as_f64(n)])
    mean, se, t, nobs = _api.records_summary(vals, nw_lags=int(nw_lags))
    K = len(predictor_cols)
    return _api.summary_from_device(mean, se, t, nobs, predictor_cols, k_slope0=0, k_r2=K, k_n=K + 1)


POOLED_KINDS = ("classical", "white", "month", "firm", "twoway")


def run_pooled_regression(df: pd.DataFrame, return_col: str, predictor_cols: list, date_col: str = "mthcaldt",
                          id_col: str = "permno", month_fe: bool = False, small_sample: bool = True) -> pd.DataFrame:
    """Pooled panel OLS of ``return_col`` on an intercept and ``predictor_cols`` over all months at
    once (build-defined, A23; no reference line; fm_pool), with the standard errors of the robustness
    table beside Fama-MacBeth (Petersen 2009): classical, White, clustered by month, by firm
    (``id_col``) and by both (Cameron, Gelbach and Miller 2011).  ``month_fe``: month fixed effects
    (the within-month demeaned regression; no intercept, its row is NaN); ``small_sample``: White
    times N / (N - K - 1), a clustering over G clusters times G / (G - 1) (N - 1) / (N - K - 1).

    Rows with NaN in any of [return_col] + predictor_cols (or a missing date) are dropped.  Returns
    a frame indexed by ["const"] + predictor_cols with the columns ``coef``, ``se_<kind>`` and
    ``t_<kind>`` for kind in classical, white, month, firm, twoway; ``.attrs`` holds N, n_months,
    n_firms and r2 (the within R2 under ``month_fe``).  A two-way variance that is not positive gives
    NaN.  Too few rows, collinear or constant regressors: every entry NaN; an inf raises
    MissingDataError.  ``date_col`` must be datetime64 or integer months and ``id_col`` whole-number
    firm ids, one row per (month, firm): ValueError otherwise."""
    predictor_cols = list(predictor_cols)
    K = len(predictor_cols)
    ids = p = np.asarray(df[id_col])
    dates = df[date_col].to_numpy()
    if p.dtype.kind == "f" and len(p) and bool(np.all(np.isfinite(p))) and bool(np.all(p == np.floor(p))):
        ids = p.astype(np.int64)
    if ids.dtype.kind not in "iu" or dates.dtype.kind not in "Miu":
        raise ValueError(f"run_pooled_regression: {id_col!r} must hold whole-number firm ids and {date_col!r} "
                         "datetime64 or integer months")
    ids = ids.astype(np.int64)
    order = np.lexsort((ids, dates))
    names = predictor_cols + [return_col]
    panel = _E.panel_from_arrays([_api.as_f64(df[c])[order] for c in names], names, dates[order], ids=ids[order])
    res = _E.pooled_regressions(panel, [_E.Model("m", y=K, xs=list(range(K)))], month_fe=month_fe,
                                small_sample=small_sample)
    status = int(res.status[0].item())
    if status & (_E.L.FM_ST_INF_IN_X | _E.L.FM_ST_INF_IN_Y):
        raise MissingDataError("exog contains inf or nans" if status & _E.L.FM_ST_INF_IN_X
                               else "endog contains inf or nans")
    coef = res.coef[0, :K + 1].cpu().numpy()
    se = res.se[0, :, :K + 1].cpu().numpy()
    stat = res.stat[0].cpu().numpy()
    out = pd.DataFrame({"coef": coef}, index=pd.Index(["const"] + predictor_cols))
    for k, kind in enumerate(POOLED_KINDS):
        out[f"se_{kind}"] = se[k]
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, kind in enumerate(POOLED_KINDS):
            out[f"t_{kind}"] = coef / se[k]
    out.attrs.update(N=int(stat[0]), n_months=int(stat[1]), n_firms=0 if np.isnan(stat[2]) else int(stat[2]),
                     r2=float(stat[3]))
    return out
