"""The Lewellen (2015) Table-2 / Figure-1 pass as one device-resident pipeline.

winsorize (1/99, every column, reference src/calc_Lewellen_2014.py:505-529)
 -> NYSE 20th/50th me breakpoints and nested universe levels (:44-112)
 -> Models 1/2/3 x {All, All-but-tiny, Large} and the Figure-1 5-variable model x {All,
    Large} in ONE batched Gram pass (:714-770, :882-921)
 -> Fama-MacBeth means + Newey-West(4) t-stats (src/regressions.py:102-131)
 -> 120-month rolling coefficient means (:926)
 -> lagged-rolling forecasts and predictive-slope FM summaries (build-defined A7/A8)
 -> optionally (``PipelineConfig.portfolios``) the forecast-sorted portfolios of every Table-2
    problem (paper Table 5, build-defined A12) in one more launch that forecasts and sorts
 -> optionally (``PipelineConfig.forecast_dist``) each month's mean, standard deviation and
    quantiles of those forecasts (paper Table 3, build-defined A14), likewise in one launch
 -> optionally (``PipelineConfig.forecast_compare``) per universe and pair of Table-2 models the
    monthly regression of one model's forecast on the other's and of returns on its residual
    (paper Table 4, build-defined A15), likewise in one launch
With ``PipelineConfig.alpha_factors`` the portfolios' monthly returns are also regressed on factor
returns (CAPM and three-factor alphas, the second table of the paper's portfolio section;
build-defined A18), in one more launch.
With ``PipelineConfig.portfolio_hold`` = k those portfolios are held for k months as overlapping
cohorts (the calendar-time strategy; build-defined A19): its monthly record, summary, turnover and,
with the factors, its alphas, in one more launch.
With ``PipelineConfig.double_sort`` = a panel column those forecasts are also sorted two ways, against
that column (size, say), into na x nb cells: each row's spread and the column-neutral spread
(build-defined A21).
With ``PipelineConfig.wls_weights`` (e.g. "me") every monthly cross-section is a weighted
least-squares fit (engine.fm_pass_wls) and every later stage runs on the weighted slopes.
With ``PipelineConfig.extrapolate`` = k the monthly run also scales every month's forecasts to k
months and regresses the compounded k-month return on them (paper Section 4's second approach, the
lower panels of Tables 9a and 9b; build-defined A17), in one more launch.
With ``PipelineConfig.horizon`` = k > 1 the dependent variable of all of this is the compounded
k-month return (paper Section 4, Tables 8 and 9; build-defined A16), a column built once at ingest.
All stages are libfm_hip kernels; the panel is read from HBM twice (cuts, Gram).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import engine as E

# Model definitions: reference src/calc_Lewellen_2014.py:714-745 (labels) and the notebook's
# variables_dict (src/get_data.ipynb cell 24).
MODELS_PREDICTORS = {
    "Model 1: Three Predictors": [
        "Log Size (-1)", "Log B/M (-1)", "Return (-2, -12)"],
    "Model 2: Seven Predictors": [
        "Log Size (-1)", "Log B/M (-1)", "Return (-2, -12)", "Log Issues (-1,-36)",
        "Accruals (-1)", "ROA (-1)", "Log Assets Growth (-1)"],
    "Model 3: Fourteen Predictors": [
        "Log Size (-1)", "Log B/M (-1)", "Return (-2, -12)", "Log Issues (-1,-12)",
        "Accruals (-1)", "ROA (-1)", "Log Assets Growth (-1)", "Dividend Yield (-1,-12)",
        "Log Return (-13,-36)", "Log Issues (-1,-36)", "Beta (-1,-36)", "Std Dev (-1,-12)",
        "Debt/Price (-1)", "Sales/Price (-1)"],
}
VARIABLES_DICT = {
    "Return (%)": "retx", "Log Size (-1)": "log_size", "Log B/M (-1)": "log_bm",
    "Return (-2, -12)": "return_12_2", "Log Issues (-1,-12)": "log_issues_12",
    "Accruals (-1)": "accruals_final", "ROA (-1)": "roa",
    "Log Assets Growth (-1)": "log_assets_growth", "Dividend Yield (-1,-12)": "dy",
    "Log Return (-13,-36)": "log_return_13_36", "Log Issues (-1,-36)": "log_issues_36",
    "Beta (-1,-36)": "beta", "Std Dev (-1,-12)": "rolling_std_252", "Debt/Price (-1)": "debt_price",
    "Sales/Price (-1)": "sales_price",
}
FIG1_VARS = ["log_bm", "return_12_2", "log_issues_36", "accruals_final", "log_assets_growth"]
SUBSET_NAMES = ["All stocks", "All-but-tiny stocks", "Large stocks"]


def table2_models(variables_dict=None):
    vd = variables_dict or VARIABLES_DICT
    out = {}
    for name, labels in MODELS_PREDICTORS.items():
        cols = []
        for lbl in labels:
            if lbl not in vd:
                raise ValueError(f"'{lbl}' not found in variables_dict!")
            cols.append(vd[lbl])
        out[name] = cols
    return out


@dataclass
class PipelineConfig:
    lower_percentile: float = 1
    upper_percentile: float = 99
    winsorize: bool = True
    standardize: bool = False      # north-star extension; OFF on the parity path
    universes: bool = True
    nw_lags: int = 4
    window: int = 120
    min_periods: int = 60
    lag: int = 1
    forecasts: bool = True
    fig1: bool = True
    # A12 inside the pipeline (paper Table 5): the number of portfolios, None = off (the pipeline
    # then issues exactly the launches it issues without these fields).  Every problem of the
    # Table-2 models (not Figure 1) is sorted each month on F = a + b'clip(x) with that problem's
    # lagged rolling coefficients -- the row its predictive record reads -- over its own universe.
    # Needs forecasts=True (the rolling means and the lag come from that stage) and excludes
    # standardize=True (coefficients on z-scores need the moment tables): ValueError otherwise.
    # Keyword-only, so that the positional order of the fields above and of ``rank`` (pinned as
    # the trailing field by tests/test_rank_host.py) stays what it was.
    portfolios: Optional[int] = field(default=None, kw_only=True)
    portfolio_q: Optional[Sequence[float]] = field(default=None, kw_only=True)   # nport - 1 levels (None: k / nport)
    portfolio_nyse_breakpoints: bool = field(default=False, kw_only=True)        # breakpoints from the NYSE rows only
    # A21 (the Table-5 spread controlled for a second variable): ``double_sort`` = a panel column (by
    # name, e.g. "log_size") sorts every month's stocks into ``double_sort_shape`` = (na, nb) cells, na
    # bins of that column by nb bins of each Table-2 problem's forecast, independently or
    # (``double_sort_conditional``) the forecast within each bin of the column, over the problem's
    # universe and with ``portfolio_nyse_breakpoints`` (engine.double_sort): every row's H-L and the
    # column-neutral H-L.  The portfolio launch is asked for its forecasts, which the double sort
    # reads as vectors; one more launch per universe level.  Needs ``portfolios``; excludes horizon > 1,
    # ``extrapolate`` and ``portfolio_hold`` (not wired): ValueError otherwise.  None = no launch more.
    # Here, in front of every field whose place tests pin.
    double_sort: Optional[str] = field(default=None, kw_only=True)
    double_sort_shape: Sequence[int] = field(default=(5, 5), kw_only=True)
    double_sort_conditional: bool = field(default=False, kw_only=True)
    # A22 (the value-weighted regressions): ``wls_weights`` = "me" (the panel's market equity), a panel
    # column by name or a [rows] tensor makes every monthly cross-section a weighted least-squares fit
    # (engine.fm_pass_wls in place of fm_pass: rows of NaN, infinite, zero or negative weight drop
    # out); group adjustment, ranks, cuts and universes run in front of it as they are, the
    # time-series stage and every forecast stage behind it, on the weighted slopes.  Excludes
    # standardize and a planes-only panel: ValueError.  None = exactly the launches of before.  Here,
    # in front of every field whose place tests pin.
    wls_weights: Optional[object] = field(default=None, kw_only=True)
    # A23 (the robustness table beside the FM numbers): ``pooled`` runs every problem of the Table-2
    # pass -- the same panel (after group adjustment and ranks), cuts, universe levels, models and
    # dependent column -- once more as ONE pooled panel OLS over all months (engine.pooled_regressions)
    # and reports classical, White, month-clustered, firm-clustered and two-way clustered standard
    # errors, ``pooled_month_fe`` with month fixed effects, ``pooled_small_sample`` with the usual
    # finite-sample factors.  With ``horizon`` > 1 the dependent variable is the overlapping k-month
    # return: clustering by firm is the textbook treatment of the serial correlation that the overlap
    # builds into a firm's residuals (Petersen 2009), beside the Newey-West lags of the FM path.
    # Needs a panel with firm ids and FP64 columns; excludes ``wls_weights`` (weighted pooled fits are
    # not built) and ``standardize`` (the z-scores exist only inside the Gram): ValueError otherwise.
    # False = no launch more.  Here, in front of every field whose place tests pin.
    pooled: bool = field(default=False, kw_only=True)
    pooled_month_fe: bool = field(default=False, kw_only=True)
    pooled_small_sample: bool = field(default=True, kw_only=True)
    # A14 inside the pipeline (paper Table 3's univariate properties): each month's cross-sectional
    # mean, standard deviation and ``forecast_dist_q`` quantiles of the same forecasts, over the same
    # problems and universes, under the same two rules as ``portfolios``; off = no launch more.
    forecast_dist: bool = field(default=False, kw_only=True)
    forecast_dist_q: Sequence[float] = field(default=(0.1, 0.9), kw_only=True)
    # A18 (the portfolio section's second table, factor-model alphas): ``alpha_factors`` = the factor
    # returns, float64 [T, K] with K <= 6 and row t = the panel's month t (a device tensor, or anything
    # torch.as_tensor takes; a NaN row drops the month), regresses every portfolio's and the spread's
    # ew and vw monthly return over the sorted months on each of ``alpha_models`` (sequences of factor
    # columns; None: CAPM on column 0 and, when K > 1, all K factors), ``alpha_rf`` [T] subtracted
    # from the portfolios' returns (not from the spread), with classical and Newey-West
    # (``alpha_nw_lags``; None: ``nw_lags``) standard errors (engine.portfolio_alphas) -- one more
    # launch.  Needs ``portfolios`` and horizon == 1 (overlapping k-month portfolio returns on monthly
    # factors are not this table): ValueError otherwise, and for a first dimension other than the
    # panel's month count.  None = no launch more.  In front of ``extrapolate``: tests pin the seven
    # trailing fields.
    # A20 (in front of ``alpha_factors``, whose place tests pin): ``group_adjust`` = "demean", "mean"
    # or "zscore" replaces the predictor columns ``group_adjust_cols`` (names; None: every predictor
    # of every model, never the dependent column) by their adjustment within the panel's groups
    # (industries) of each month (engine.group_adjust: x minus the group mean, the group mean, the
    # within-group z-score; groups below ``group_min_count`` rows give NaN) before anything else:
    # the adjusted columns are winsorized like any others, ``rank`` ranks them, and every forecast
    # stage reads them.  Needs a panel with group codes and excludes standardize: ValueError
    # otherwise.  None = no launch more.
    group_adjust: Optional[str] = field(default=None, kw_only=True)
    group_adjust_cols: Optional[Sequence[str]] = field(default=None, kw_only=True)
    group_min_count: int = field(default=1, kw_only=True)
    alpha_factors: Optional[object] = field(default=None, kw_only=True)
    alpha_models: Optional[Sequence[Sequence[int]]] = field(default=None, kw_only=True)
    alpha_rf: Optional[object] = field(default=None, kw_only=True)
    alpha_nw_lags: Optional[int] = field(default=None, kw_only=True)
    # A19 (k-month holding of the Table-5 portfolios): ``portfolio_hold`` = k in 1..engine.MAX_HOLD
    # follows every month's portfolios for k months over the firm links and reports the strategy that
    # holds the k latest cohorts (engine.held_portfolios: its monthly record, FM summary, cohort sizes,
    # persistence and name turnover) -- one more launch; with ``alpha_factors`` the held record is
    # regressed on the factors too.  The held returns are monthly, so month t of the factor table is
    # month t of the record.  Needs ``portfolios``, a panel with firm ids and horizon == 1 (held
    # monthly returns are the alternative to k-month dependent returns): ValueError otherwise.  None =
    # no launch more.  In front of ``extrapolate``: tests pin the seven trailing fields.
    portfolio_hold: Optional[int] = field(default=None, kw_only=True)
    # A17 (paper Section 4, second approach): ``extrapolate`` = k in 2..engine.MAX_HORIZON keeps the
    # monthly regressions and forecasts and, in one more launch, scales every month's forecasts to k
    # months, G = k * mean + (1 + rho + ... + rho^(k-1)) (F - mean) with rho = ``extrapolate_decay`` in
    # (0, 1] (the paper rounds the forecasts' autocorrelation to 0.9; 1 = plain k-fold scaling) and the
    # mean taken over the problem's universe, then regresses the compounded k-month return on G
    # (engine.forecast_horizon), over the same problems and universes and under the same two rules as
    # ``portfolios``.  The alternative to ``horizon`` > 1, so the two exclude each other; the panel
    # needs firm ids.  ``extrapolate_nw_lags`` (None: ``nw_lags``) is the caller's choice, as for
    # ``horizon``: the paper uses 10 lags for 6 months and 16 for 12.  None = no launch more.
    extrapolate: Optional[int] = field(default=None, kw_only=True)
    extrapolate_decay: float = field(default=0.9, kw_only=True)
    extrapolate_q: Sequence[float] = field(default=(0.1, 0.9), kw_only=True)
    extrapolate_nw_lags: Optional[int] = field(default=None, kw_only=True)
    # A16 (paper Section 4, Tables 8 and 9): the dependent variable of every stage is the compounded
    # ``horizon``-month return y_t .. y_{t+horizon-1} (column f"{y}_{horizon}m", built once by
    # engine.horizon_panel when the panel lacks it; the panel then needs firm ids).  1 = monthly
    # returns and no launch more or less; 1..engine.MAX_HORIZON, ValueError otherwise.  Above 1 the
    # forecast lag must be at least the horizon (ValueError): the coefficients of month t - lag are
    # fitted on returns that end in month t - lag + horizon - 1, which must lie before t.  ``nw_lags``
    # stays the caller's choice: overlapping k-month returns are autocorrelated to k - 1 lags, and
    # the paper uses 10 lags for 6 months and 16 for 12.
    # Keyword-only and in front of ``forecast_compare``: the two trailing fields are pinned by tests.
    horizon: int = field(default=1, kw_only=True)
    # A15 inside the pipeline (paper Table 4, model comparison): for every universe and every pair
    # i < j of the Table-2 models (not Figure 1), each month's regression of forecast j on forecast i
    # and of the return on its residual, from the same forecasts under the same two rules as
    # ``portfolios``; off = no launch more.
    forecast_compare: bool = field(default=False, kw_only=True)
    rank: Optional[str] = None     # A13: predictors -> per-month ranks, a scale name ("raw", "pct", "uniform")


@dataclass
class PipelineResult:
    model_names: List[str]
    model_cols: Dict[str, List[str]]
    res: E.FMResult
    ix: E.TSIndex
    summary: E.Summary
    rolling: Optional[torch.Tensor] = None
    pred: Optional[torch.Tensor] = None
    pred_status: Optional[torch.Tensor] = None
    pred_summary: Optional[E.Summary] = None
    cuts: Optional[E.Cuts] = None
    level: Optional[torch.Tensor] = None
    breakpoints: Optional[tuple] = None
    portfolios: Optional[E.Portfolios] = None        # cfg.portfolios: tensors with a leading [nsort] dimension
    portfolio_summary: Optional[E.Summary] = None    # [nsort, nport+1, 4]
    portfolio_problems: Optional[List[int]] = None   # the problem index (res.problems) of each sort
    double_sort: Optional[E.DoubleSort] = None        # cfg.double_sort: tensors with a leading [nsort] dimension
    double_sort_summary: Optional[tuple] = None       # (Summary of by_b [nsort, na+1, nb+1, 4], of by_a [nsort, nb+1, na+1, 4])
    pooled: Optional[E.PooledResult] = None               # cfg.pooled: the problems of ``res``, in its order
    forecast_dist: Optional[E.ForecastDist] = None       # cfg.forecast_dist: [nsort, T, 2+nq] and [nsort, T]
    forecast_dist_summary: Optional[E.Summary] = None    # [nsort, 2+nq]
    forecast_dist_problems: Optional[List[int]] = None   # the problem index (res.problems) of each sort
    y_col: str = "retx"                                   # the dependent column (cfg.horizon > 1: f"{y}_{h}m")
    group_stats: Optional[E.GroupStats] = None            # cfg.group_adjust: [len(group_adjusted), T, ngroups]
    group_adjusted: Optional[List[str]] = None            # the adjusted columns' names, in panel order
    held: Optional[E.HeldPortfolios] = None               # cfg.portfolio_hold: tensors with a leading [nsort] dimension
    held_summary: Optional[E.Summary] = None              # [nsort, nport+1, 4]
    held_alphas: Optional[E.PortfolioAlphas] = None       # with cfg.alpha_factors: [nsort, nport+1, 2, M, ...]
    portfolio_alphas: Optional[E.PortfolioAlphas] = None  # cfg.alpha_factors: [nsort, nport+1, 2, M, ...]
    # cfg.extrapolate (in front of the comparison's fields, which tests pin as the trailing three)
    extrapolated: Optional[E.ForecastHorizon] = None      # [nsort, T, 6+nq], [nsort, T, 2], [nsort, T]
    extrapolated_summary: Optional[E.Summary] = None      # [nsort, 6+nq]
    extrapolated_problems: Optional[List[int]] = None     # the problem index (res.problems) of each sort
    forecast_compare: Optional[E.ForecastCompare] = None     # cfg.forecast_compare: [npair, T, 7], [npair, T, 2], [npair, T]
    forecast_compare_summary: Optional[E.Summary] = None     # [npair, 7]
    forecast_compare_pairs: Optional[List[tuple]] = None     # (problem_a, problem_b) of each pair: b regressed on a


def build_models(panel: E.DevicePanel, model_cols: Dict[str, List[str]], y="retx", fig1=True,
                 universes=True):
    levels = (0, 1, 2) if universes else (0,)
    models, names = [], []
    for name, cols in model_cols.items():
        models.append(E.Model(name, y=panel.col(y), xs=[panel.col(c) for c in cols], levels=levels))
        names.append(name)
    if fig1:
        # create_figure_1: has_constant='add' (no constant-column error), All & Large only
        models.append(E.Model("Figure 1", y=panel.col(y), xs=[panel.col(c) for c in FIG1_VARS],
                              levels=(0, 2) if universes else (0,), const_check=False))
        names.append("Figure 1")
    return models, names


def _standardize_params(panel: E.DevicePanel, cuts: E.Cuts, yi: int):
    """A9 (build-defined): the Gram sees z = (clip(x) - mean_t) / sd_t for every predictor
    column (shift = mean, inv_scale = 1/sd, nothing added back: the regressors ARE the
    z-scores), while the dependent column keeps its units (shift = its pivot, scale 1,
    added back to the intercept).  All [C, T] month tables, built on the device."""
    shift = cuts.mean.clone()
    inv_scale = 1.0 / cuts.sd
    add_back = torch.zeros_like(shift)
    shift[yi] = cuts.center[yi]
    inv_scale[yi] = 1.0
    add_back[yi] = cuts.center[yi]
    return shift, inv_scale, add_back


def local_stage(panel: E.DevicePanel, cfg: PipelineConfig, model_cols, y="retx"):
    """Panel-sized work for one shard of months: cuts, universes, batched Gram + solve."""
    return _local_stage(panel, cfg, model_cols, y)[:5]


def _local_stage(panel: E.DevicePanel, cfg: PipelineConfig, model_cols, y="retx"):
    """local_stage, plus the panel the Gram read (the group-adjusted one under cfg.group_adjust, the
    ranked one under cfg.rank), the models and, under cfg.group_adjust, (GroupStats, adjusted names)."""
    cuts = None
    shift = None
    inv_scale = None
    level, bp = None, None
    nlevels = 1
    check_wls(cfg, panel)
    models, names = build_models(panel, model_cols, y=y, fig1=cfg.fig1, universes=cfg.universes)
    gadj = None
    if cfg.group_adjust is not None:
        # A20 (build-defined): the raw predictor columns (never y) adjusted within the month's groups,
        # before the cuts: the adjusted columns are winsorized (and ranked) like any others
        check_group_adjust(cfg, panel, model_cols, y)
        adjusted = sorted({i for m in models for i in m.xs} - {panel.col(y)})
        if cfg.group_adjust_cols is not None:
            adjusted = sorted({panel.col(c) for c in cfg.group_adjust_cols})
        panel = E.group_adjust(panel, cols=adjusted, mode=cfg.group_adjust, min_count=cfg.group_min_count,
                               stats=True)
        gadj = (panel.group_stats, [panel.names[i] for i in adjusted])
    ranked = None
    if cfg.rank is not None:
        # A13 (build-defined): every predictor column (never y) becomes its average-tie rank
        # within the month's full cross-section; the ranked columns are not winsorized
        if cfg.standardize:
            raise ValueError("PipelineConfig: rank and standardize exclude each other")
        ranked = sorted({i for m in models for i in m.xs} - {panel.col(y)})
        panel = E.rank_transform(panel, cols=ranked, method="average", scale=cfg.rank)
    select = cfg.winsorize or cfg.standardize
    # get_subsets' NYSE breakpoints + level bytes come with the winsorize call
    # (fm_select_universe): on the bench's short months they share the select fix-up's launch
    # (the universe no longer needs a launch of its own), on C5's long months they ride the
    # long-month kernel's launch (one more grid column); other paths launch fm_universe first
    fused_universe = cfg.universes and select and not cfg.standardize
    if cfg.universes and not fused_universe:
        a, b, level = E.universe(panel)
        nlevels = 3
        bp = (a, b)
    add_back = None
    if select:
        mc = 5 if cfg.winsorize else 2 ** 31 - 1
        # standardize needs the exact clipped moments; otherwise the Gram pivot is the
        # select kernel's free center (midpoint of the cuts), and no moments pass runs
        cuts = E.select_cuts(panel, cfg.lower_percentile / 100, cfg.upper_percentile / 100, mc,
                             E.LERP_NUMPY, moments=cfg.standardize, center=True,
                             universe=(0.2, 0.5) if fused_universe else None)
        if fused_universe:
            cuts, (a, b, level) = cuts
            nlevels = 3
            bp = (a, b)
        if ranked:
            cuts.lo[ranked] = float("nan")
            cuts.hi[ranked] = float("nan")
        shift = cuts.center
        if cfg.standardize:
            shift, inv_scale, add_back = _standardize_params(panel, cuts, panel.col(y))
        if not cfg.winsorize:
            cuts = E.Cuts(torch.full_like(cuts.lo, float("nan")), torch.full_like(cuts.hi, float("nan")),
                          cuts.nvalid, cuts.mean, cuts.sd, cuts.center)
    if cfg.wls_weights is not None:
        # A22: the weighted cross-sections; the cuts' centre is only the pivot of its first pass
        res = E.fm_pass_wls(panel, models, weight=cfg.wls_weights, level=level, nlevels=nlevels, cuts=cuts,
                            shift=shift, moments=cfg.forecasts)
        return res, names, cuts, level, bp, panel, models, gadj
    res = E.fm_pass(panel, models, level=level, nlevels=nlevels, cuts=cuts, shift=shift,
                    inv_scale=inv_scale, add_back=add_back if cfg.standardize else shift,
                    moments=cfg.forecasts)
    if cfg.standardize:
        E.drop_degenerate_months(res, models, cuts.sd)
    return res, names, cuts, level, bp, panel, models, gadj


def time_series_stage(res: E.FMResult, cfg: PipelineConfig, moments=None, seg_lo=0, seg_hi=None,
                      sum_range=None, roll_own=False):
    """One launch (fm_ts_fused): compaction, FM summaries, rolling means, predictive slopes.
    Their FM summary follows in summarize_predictive.  Returns (ix, summ, roll, pred, pst).
    Month-sharded ranks pass their problem block (``sum_range``) and ``roll_own`` (rolling
    means only where their own months' predictive records read them); the summaries are then
    SUM-combined across ranks (fmcore.step.ShardedStep)."""
    return E.time_series_result(
        res, cfg.nw_lags, cfg.window, cfg.min_periods, cfg.lag, seg_lo=seg_lo, seg_hi=seg_hi,
        moments=moments, rolling=cfg.forecasts or cfg.fig1, predictive=cfg.forecasts,
        sum_range=sum_range, roll_own=roll_own)


def check_wls(cfg: PipelineConfig, panel=None, y="retx"):
    """The rules of ``PipelineConfig.wls_weights`` (no device work); ``panel``: the run's panel, when
    there is one; ``y``: the dependent column's name before ``horizon`` renames it."""
    if cfg.wls_weights is None:
        return
    if cfg.standardize:
        raise ValueError("PipelineConfig: wls_weights excludes standardize (weighted z-scores are not wired)")
    if panel is not None and panel.cols is None:
        raise ValueError("PipelineConfig: wls_weights needs a panel with FP64 columns, not a planes-only one")
    if panel is not None:
        # fm_wls takes a panel of at most 15 columns; horizon > 1 appends the k-month return to it
        extra = int(cfg.horizon > 1 and f"{y}_{cfg.horizon}m" not in panel.names)
        if panel.ncols + extra > E.L.FM_WLS_MAX_COLS:
            raise ValueError(f"PipelineConfig: wls_weights takes a panel of at most {E.L.FM_WLS_MAX_COLS} columns, this "
                             f"one has {panel.ncols}" + (f" and horizon={cfg.horizon} adds the k-month return" if extra
                                                         else ""))


def check_pooled(cfg: PipelineConfig, panel=None):
    """The rules of ``PipelineConfig.pooled`` (no device work); ``panel``: the run's panel, when there
    is one."""
    if not cfg.pooled:
        return
    if cfg.wls_weights is not None:
        raise ValueError("PipelineConfig: pooled excludes wls_weights (weighted pooled fits are not built)")
    if cfg.standardize:
        raise ValueError("PipelineConfig: pooled excludes standardize (the z-scores exist only inside the Gram)")
    if panel is not None and panel.ids is None:
        raise ValueError("PipelineConfig: pooled needs a panel with firm ids (build it with ids=...)")
    if panel is not None and panel.cols is None:
        raise ValueError("PipelineConfig: pooled needs a panel with FP64 columns, not a planes-only one")


def check_horizon(cfg: PipelineConfig):
    """The rules of ``PipelineConfig.horizon`` (no device work)."""
    h = cfg.horizon
    if not isinstance(h, (int, np.integer)) or isinstance(h, bool) or h < 1 or h > E.MAX_HORIZON:
        raise ValueError(f"PipelineConfig: horizon must be an integer in 1..{E.MAX_HORIZON}, got {h!r}")
    if h > 1 and cfg.lag < h:
        raise ValueError(f"PipelineConfig: horizon={h} needs lag >= horizon, got lag={cfg.lag} (the coefficients "
                         "of month t - lag would be fitted on returns that end after month t)")


def check_extrapolate(cfg: PipelineConfig):
    """The rules of ``PipelineConfig.extrapolate`` that need no panel (no device work)."""
    k, rho = cfg.extrapolate, cfg.extrapolate_decay
    if k is None:
        return
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 2 or k > E.MAX_HORIZON:
        raise ValueError(f"PipelineConfig: extrapolate must be an integer in 2..{E.MAX_HORIZON}, got {k!r}")
    if isinstance(rho, bool) or not isinstance(rho, (int, float, np.integer, np.floating)) or not 0.0 < rho <= 1.0:
        raise ValueError(f"PipelineConfig: extrapolate_decay must lie in (0, 1], got {rho!r}")
    if cfg.horizon != 1:
        raise ValueError(f"PipelineConfig: extrapolate={k} excludes horizon={cfg.horizon} (monthly forecasts scaled "
                         "to k months and regressions refitted on k-month returns are alternatives)")


def check_alphas(cfg: PipelineConfig, nseg=None):
    """The rules of ``PipelineConfig.alpha_factors`` (no device work); ``nseg``: the panel's month
    count, when there is a panel."""
    f = cfg.alpha_factors
    if f is None:
        for name in ("alpha_models", "alpha_rf", "alpha_nw_lags"):
            if getattr(cfg, name) is not None:
                raise ValueError(f"PipelineConfig: {name} needs alpha_factors")
        return
    if cfg.portfolios is None:
        raise ValueError("PipelineConfig: alpha_factors needs portfolios (the returns it regresses)")
    if cfg.horizon != 1:
        raise ValueError(f"PipelineConfig: alpha_factors excludes horizon={cfg.horizon} (overlapping k-month "
                         "portfolio returns on monthly factors are not this table; portfolio_hold=k regresses "
                         "the monthly returns of the portfolios held for k months)")
    shape = tuple(getattr(f, "shape", np.shape(f)))
    if len(shape) != 2 or not 1 <= shape[1] <= E.L.FM_MAX_FACTORS:
        raise ValueError(f"PipelineConfig: alpha_factors must be [T, K] with K in 1..{E.L.FM_MAX_FACTORS}, "
                         f"got shape {shape}")
    E.alpha_model_masks(cfg.alpha_models, shape[1])
    for what, t, want in (("alpha_factors", shape, None),
                          ("alpha_rf", None if cfg.alpha_rf is None else
                           tuple(getattr(cfg.alpha_rf, "shape", np.shape(cfg.alpha_rf))), 1)):
        if t is None:
            continue
        if want is not None and len(t) != want:
            raise ValueError(f"PipelineConfig: {what} must be a [T] vector, got shape {t}")
        if nseg is not None and t[0] != nseg:
            raise ValueError(f"PipelineConfig: {what} has {t[0]} rows, the panel has {nseg} months")
        if t[0] != shape[0]:
            raise ValueError(f"PipelineConfig: {what} has {t[0]} rows, alpha_factors {shape[0]}")


def check_hold(cfg: PipelineConfig, panel=None):
    """The rules of ``PipelineConfig.portfolio_hold`` (no device work); ``panel``: the run's panel,
    when there is one."""
    k = cfg.portfolio_hold
    if k is None:
        return
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 1 or k > E.MAX_HOLD:
        raise ValueError(f"PipelineConfig: portfolio_hold must be an integer in 1..{E.MAX_HOLD}, got {k!r}")
    if cfg.portfolios is None:
        raise ValueError("PipelineConfig: portfolio_hold needs portfolios (the sorts it holds)")
    if cfg.horizon != 1:
        raise ValueError(f"PipelineConfig: portfolio_hold={k} excludes horizon={cfg.horizon} (held monthly returns "
                         "and k-month dependent returns are alternatives)")
    if panel is not None and (panel.ids is None or panel.month_index is None):
        raise ValueError("PipelineConfig: portfolio_hold needs a panel with firm ids (build it with ids=...)")


def check_double_sort(cfg: PipelineConfig, panel=None):
    """The rules of ``PipelineConfig.double_sort`` (no device work); ``panel``: the run's panel, when
    there is one."""
    col = cfg.double_sort
    if col is None:
        return
    if not isinstance(col, str):
        raise ValueError(f"PipelineConfig: double_sort must name a panel column, got {col!r}")
    shape = cfg.double_sort_shape
    ok = not isinstance(shape, str) and len(tuple(shape)) == 2 and all(
        isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 2 <= v <= E.MAX_DSORT for v in shape)
    if not ok:
        raise ValueError(f"PipelineConfig: double_sort_shape must be (na, nb) with both in 2..{E.MAX_DSORT}, "
                         f"got {shape!r}")
    if cfg.portfolios is None:
        raise ValueError("PipelineConfig: double_sort needs portfolios (the launch that makes the forecasts)")
    for on, what in ((cfg.horizon != 1, f"horizon={cfg.horizon}"), (cfg.extrapolate is not None, "extrapolate"),
                     (cfg.portfolio_hold is not None, "portfolio_hold")):
        if on:
            raise ValueError(f"PipelineConfig: double_sort excludes {what} (the combination is not wired)")
    if panel is not None and col not in panel.names:
        raise ValueError(f"PipelineConfig: double_sort names column {col!r}, which the panel lacks")


def double_sort_forecasts(panel: E.DevicePanel, cfg: PipelineConfig, forecast, levels, level, y="retx"):
    """A21 of the pipeline: the panel column ``cfg.double_sort`` against every forecast vector
    (``forecast`` [nsort, rows], sort j over the universe ``levels[j]``), one ``engine.double_sort``
    launch per distinct level, gathered back in sort order."""
    na, nb = (int(v) for v in cfg.double_sort_shape)
    a = E.column_vector(panel, cfg.double_sort)
    ret = E.column_vector(panel, y)
    parts, order = [], []
    for lv in sorted(set(levels)):
        js = [j for j, l in enumerate(levels) if l == lv]
        order += js
        parts.append(E.double_sort(panel.seg_off, a, forecast[js], ret, weight=panel.me, level=level, nyse=panel.nyse,
                                   na=na, nb=nb, conditional=cfg.double_sort_conditional, min_level=lv,
                                   nyse_breakpoints=cfg.portfolio_nyse_breakpoints, max_seg_len=panel.max_seg_len))
    if len(parts) == 1:
        return parts[0]
    inv = torch.as_tensor(np.argsort(np.asarray(order)), device=forecast.device)
    cat = {k: torch.cat([getattr(p, k) for p in parts])[inv]
           for k in ("rec_b", "rec_a", "cnt", "cell", "bpa", "bpb", "status")}
    return E.DoubleSort(na=na, nb=nb, conditional=bool(cfg.double_sort_conditional), **cat)


def check_group_adjust(cfg: PipelineConfig, panel=None, model_cols=None, y="retx"):
    """The rules of ``PipelineConfig.group_adjust`` (no device work); ``panel``: the run's panel, when
    there is one (touched only when group_adjust is set)."""
    mode = cfg.group_adjust
    if mode is None:
        if cfg.group_adjust_cols is not None:
            raise ValueError("PipelineConfig: group_adjust_cols needs group_adjust")
        return
    if mode not in E.GADJ_MODES:
        raise ValueError(f"PipelineConfig: group_adjust must be one of {sorted(E.GADJ_MODES)}, got {mode!r}")
    k = cfg.group_min_count
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
        raise ValueError(f"PipelineConfig: group_min_count must be an integer >= 0, got {k!r}")
    if cfg.standardize:
        raise ValueError("PipelineConfig: group_adjust excludes standardize (z-scores of the month on top of "
                         "an adjustment within its groups; use group_adjust='zscore')")
    if cfg.group_adjust_cols is not None:
        model_cols = model_cols or table2_models()
        predictors = {c for cols in model_cols.values() for c in cols} | (set(FIG1_VARS) if cfg.fig1 else set())
        predictors.discard(y)
        unknown = [c for c in cfg.group_adjust_cols if c not in predictors]
        if isinstance(cfg.group_adjust_cols, str) or unknown:
            raise ValueError(f"PipelineConfig: group_adjust_cols must name predictors of the models, not {unknown}")
    if panel is not None and panel.group is None:
        raise ValueError("PipelineConfig: group_adjust needs a panel with group codes (build it with group=...)")


def horizon_column(panel: E.DevicePanel, cfg: PipelineConfig, y="retx"):
    """The panel and dependent column of a run: (panel, y) at horizon 1; else the column
    f"{y}_{h}m", appended by engine.horizon_panel when the panel lacks it."""
    if cfg.horizon == 1:
        return panel, y
    y_col = f"{y}_{cfg.horizon}m"
    if y_col not in panel.names:
        panel = E.horizon_panel(panel, cfg.horizon, ret=y, name=y_col)
    return panel, y_col


def run_pipeline(panel: E.DevicePanel, cfg: PipelineConfig = None, model_cols=None, y="retx"):
    """The whole pass on one device.  ``cfg.horizon`` = h > 1 (A16): every stage -- the Gram, the
    fix-ups, the predictive records and the returns of the portfolio and comparison stages -- takes
    the compounded h-month return f"{y}_{h}m" as the dependent variable (``PipelineResult.y_col``).
    ``cfg.pooled`` (A23) adds the pooled panel OLS of the same problems on the same panel, cuts,
    levels and dependent column (``PipelineResult.pooled``); with h > 1 its firm-clustered errors are
    the textbook treatment of the overlapping returns' serial correlation within a firm."""
    cfg = cfg or PipelineConfig()
    model_cols = model_cols or table2_models()
    check_horizon(cfg)
    check_extrapolate(cfg)
    check_alphas(cfg, None if panel is None else panel.nseg)
    check_hold(cfg, panel)
    check_double_sort(cfg, panel)
    check_group_adjust(cfg, panel, model_cols, y)
    check_wls(cfg, panel, y)
    check_pooled(cfg, panel)
    for on, what in ((cfg.portfolios is not None, "portfolios"), (cfg.forecast_dist, "forecast_dist"),
                     (cfg.forecast_compare, "forecast_compare"), (cfg.extrapolate is not None, "extrapolate")):
        if on and cfg.standardize:
            raise ValueError(f"PipelineConfig: {what} excludes standardize (coefficients on z-scores "
                             "need the moment tables)")
        if on and not cfg.forecasts:
            raise ValueError(f"PipelineConfig: {what} needs forecasts=True (the lagged rolling coefficients)")
    if cfg.extrapolate is not None and (panel.ids is None or panel.month_index is None):
        raise ValueError("PipelineConfig: extrapolate needs a panel with firm ids (build it with ids=...)")
    panel, y = horizon_column(panel, cfg, y)
    res, names, cuts, level, bp, gpanel, models, gadj = _local_stage(panel, cfg, model_cols, y)
    ix, summ, roll, pred, pst = time_series_stage(res, cfg)
    psumm = None
    if cfg.forecasts:
        psumm, _ = E.summarize_predictive(pred, pst, cfg.nw_lags)
    pooled = None
    if cfg.pooled:
        # A23: the Table-2 pass's problems as one pooled panel OLS each, on the panel the Gram read
        pooled = E.pooled_regressions(gpanel, models, level=level, nlevels=3 if level is not None else 1, cuts=cuts,
                                      month_fe=cfg.pooled_month_fe, small_sample=cfg.pooled_small_sample)
    ports = port_summ = port_probs = None
    dist = dist_summ = dist_probs = None
    comp = comp_summ = comp_pairs = None
    extr = extr_summ = extr_probs = None
    if cfg.portfolios is not None or cfg.forecast_dist or cfg.forecast_compare or cfg.extrapolate is not None:
        # Tables 5, 3 and 4: every Table-2 problem's forecast, sorted, summarized or compared in one launch each
        # on the panel the Gram read, with the pipeline's cuts and the coefficient rows the
        # predictive stage read
        probs = [k for k, p in enumerate(res.problems) if names[p.model] != "Figure 1"]
        coef = E.lagged_coefficients(roll, ix, probs, cfg.lag)
        sel = [(models[res.problems[k].model].xs, res.problems[k].level) for k in probs]
    if cfg.forecast_dist:
        dist_probs = probs
        dist = E.forecast_dist(gpanel, coef, sel, cuts=cuts, level=level, q=cfg.forecast_dist_q)
        dist_summ = E.forecast_dist_summary(dist, cfg.nw_lags)
    if cfg.forecast_compare:
        # universe by universe, model j's forecast on model i's for i < j (both fitted on that universe)
        at = {(res.problems[k].level, res.problems[k].model): j for j, k in enumerate(probs)}
        pairs = [(at[u, mi], at[u, mj], u) for u in sorted({u for u, _ in at})
                 for mi in range(len(names)) for mj in range(mi + 1, len(names)) if (u, mi) in at and (u, mj) in at]
        comp_pairs = [(probs[a], probs[b]) for a, b, _ in pairs]
        comp = E.forecast_compare(gpanel, coef, sel, pairs, cuts=cuts, ret=gpanel.col(y), level=level)
        comp_summ = E.forecast_compare_summary(comp, cfg.nw_lags)
    if cfg.extrapolate is not None:
        # the monthly forecasts scaled to k months, against the k-month return compounded over the firm links
        k = int(cfg.extrapolate)
        extr_probs = probs
        ret_k = E.horizon_return(panel.seg_off, E.column_vector(panel, y), E.month_links(panel, 1), k)
        extr = E.forecast_horizon(gpanel, coef, sel, ret_k, level_mult=k,
                                  gain=E.extrapolation_gain(k, cfg.extrapolate_decay), cuts=cuts, level=level,
                                  q=cfg.extrapolate_q)
        extr_summ = E.forecast_horizon_summary(
            extr, cfg.nw_lags if cfg.extrapolate_nw_lags is None else cfg.extrapolate_nw_lags)
    if cfg.portfolios is not None:
        port_probs = probs
        ports = E.forecast_portfolio_sort(gpanel, coef, sel, cuts=cuts, ret=gpanel.col(y), weight=gpanel.me,
                                          level=level, nyse=gpanel.nyse, nport=cfg.portfolios, q=cfg.portfolio_q,
                                          nyse_breakpoints=cfg.portfolio_nyse_breakpoints,
                                          forecast_out=cfg.double_sort is not None)
        port_summ = E.portfolio_summary(ports, cfg.nw_lags)
    dsort = dsort_summ = None
    if cfg.double_sort is not None:
        # the sort's own forecasts, as vectors (the fused sorts never write them), against the column
        dsort = double_sort_forecasts(gpanel, cfg, ports.forecast, [lv for _, lv in sel], level, y)
        S, na, nb = len(sel), dsort.na, dsort.nb
        sb, sa = E.portfolio_summary(dsort.by_b, cfg.nw_lags), E.portfolio_summary(dsort.by_a, cfg.nw_lags)
        dsort_summ = (E.Summary(*(t.view(S, na + 1, nb + 1, 4) for t in (sb.mean, sb.se, sb.tstat, sb.nobs))),
                      E.Summary(*(t.view(S, nb + 1, na + 1, 4) for t in (sa.mean, sa.se, sa.tstat, sa.nobs))))
    held = held_summ = None
    if cfg.portfolio_hold is not None:
        # the sorts' port bytes followed for k months over the firm links of the panel the sort read
        held = E.held_portfolios(gpanel, ports, int(cfg.portfolio_hold), ret=gpanel.col(y), weight=gpanel.me)
        held_summ = E.portfolio_summary(held, cfg.nw_lags)
    alphas = held_alphas = None
    if cfg.alpha_factors is not None:
        dev = ports.rec.device
        akw = dict(models=cfg.alpha_models,
                   rf=None if cfg.alpha_rf is None else torch.as_tensor(cfg.alpha_rf, dtype=torch.float64).to(dev),
                   nw_lags=cfg.nw_lags if cfg.alpha_nw_lags is None else cfg.alpha_nw_lags)
        factors = torch.as_tensor(cfg.alpha_factors, dtype=torch.float64).to(dev)
        alphas = E.portfolio_alphas(ports, factors, **akw)
        if held is not None:
            held_alphas = E.portfolio_alphas(held, factors, **akw)
    return PipelineResult(model_names=names, model_cols=dict(model_cols, **({"Figure 1": FIG1_VARS} if cfg.fig1 else {})),
                          res=res, ix=ix, summary=summ, rolling=roll, pred=pred, pred_status=pst,
                          pred_summary=psumm, cuts=cuts, level=level, breakpoints=bp, portfolios=ports,
                          portfolio_summary=port_summ, portfolio_problems=port_probs, double_sort=dsort,
                          double_sort_summary=dsort_summ, forecast_dist=dist,
                          forecast_dist_summary=dist_summ, forecast_dist_problems=dist_probs,
                          forecast_compare=comp, forecast_compare_summary=comp_summ, forecast_compare_pairs=comp_pairs,
                          y_col=y, group_stats=None if gadj is None else gadj[0],
                          group_adjusted=None if gadj is None else gadj[1], held=held, held_summary=held_summ, held_alphas=held_alphas, portfolio_alphas=alphas,
                          pooled=pooled, extrapolated=extr, extrapolated_summary=extr_summ, extrapolated_problems=extr_probs)


def problem_index(res: E.FMResult, names, model_name, level):
    mi = names.index(model_name)
    for k, p in enumerate(res.problems):
        if p.model == mi and p.level == level:
            return k
    raise KeyError((model_name, level))
