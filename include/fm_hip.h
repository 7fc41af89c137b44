/*
 * fm_hip.h — C ABI of libfm_hip.so, the MI355X (gfx950) Fama-MacBeth engine.
 *
 * Drop-in boundary.  The reference (BaileyMeche/FM-ReturnPrediction) has no FFI layer: its
 * hot path is a set of pandas-in/pandas-out Python functions.  The Python mirror in
 * fm-returnprediction_amd/fmdrop/{regressions,calc_Lewellen_2014,transform_compustat}.py
 * keeps those names and signatures and calls the entry points below through ctypes.  Each entry point names
 * the reference computation it replaces:
 *
 *   fm_select_cuts  <- np.percentile(vals, 1/99) per month per var
 *                      (src/calc_Lewellen_2014.py:519-523) and pandas
 *                      groupby("mthcaldt")["me"].quantile([.2,.5]) over NYSE rows (:74-82)
 *   fm_select       <- the same, struct-argument form: wave-per-(month, column) tail
 *                      selection with an exact workgroup fallback, plus the Gram pivot
 *                      `center` (the Table-2 fast path; fm_select_cuts calls it); months
 *                      of 6,145 .. 20,480 rows (C5) one register-resident 512-thread
 *                      workgroup per (month, column), longer ones streamed; optionally the
 *                      universe level bytes from the cuts (get_subsets :95-105)
 *   fm_clip         <- subdf[var].clip(lower, upper) (src/calc_Lewellen_2014.py:524)
 *   fm_standardize  <- per-month z-score (north-star extension; no reference line)
 *   fm_universe_level <- me >= me_20 / me >= me_50 masks (src/calc_Lewellen_2014.py:95-96)
 *   fm_universe     <- get_subsets in one launch: the NYSE groupby.quantile([.2,.5]) of me
 *                      (src/calc_Lewellen_2014.py:74-82) and the nested masks (:95-105)
 *   fm_pilot_shift  <- (numerics only) per-month pivot used to center the Gram
 *   fm_gram         <- dropna (src/regressions.py:39) + X'X, X'y, y'y inside sm.OLS
 *                      (src/regressions.py:57; src/calc_Lewellen_2014.py:917-919), batched
 *                      over models x universes in one read of the panel
 *   fm_solve        <- sm.OLS(Y, X).fit() params / rsquared / N and the N<K+1 skip
 *                      (src/regressions.py:52-72; src/calc_Lewellen_2014.py:914-921)
 *   fm_solve_fixup  <- statsmodels' pinv semantics where fm_solve's normal equations do not
 *                      reach them (src/regressions.py:57-64): pinv(X) @ y with an infinite
 *                      return (+-inf/NaN params, NaN R2), and ill-conditioned / rank-
 *                      deficient months re-solved from their rows (Householder QR + SVD),
 *                      and add_constant(has_constant='skip') nonzero-constant detection
 *                      (src/regressions.py:50, which leads to IndexError at :71)
 *   fm_ts_compact, fm_ts_summary <- fama_macbeth_summary + newey_west_mean_se
 *                      (src/regressions.py:78-131)
 *   fm_rolling_mean <- slopes_df.rolling(window=120, min_periods=60).mean()
 *                      (src/calc_Lewellen_2014.py:926)
 *   fm_predictive   <- build-defined extension: lagged-rolling-coefficient forecasts and
 *                      predictive-slope regressions (paper Table 3; no reference line)
 *   fm_ts_fused     <- fm_ts_compact + fm_ts_summary + fm_rolling_mean + fm_predictive in
 *                      one launch (src/regressions.py:78-131; src/calc_Lewellen_2014.py:926)
 *   fm_forecast     <- build-defined extension A7: per-row F = a_{t-1} + b_{t-1}'x_t
 *   fm_portfolio_sort <- build-defined extension: forecast-sorted portfolios, paper Table 5;
 *                      no reference line
 *   fm_forecast_portfolio_sort, fm_lagged_coef <- build-defined extension: the same sorts with
 *                      the clipped lagged-rolling forecast computed in the sort kernel's load
 *                      phase (Table 5 inside the device pipeline); no reference line
 *   fm_forecast_dist <- build-defined extension A14: per-month mean, standard deviation and
 *                      quantiles of the forecasts (paper Table 3's univariate properties); no
 *                      reference line
 *   fm_forecast_compare <- build-defined extension A15: per month and pair of forecasts, the
 *                      cross-sectional regression of one forecast on the other and of returns
 *                      on its residual (paper Table 4, "model comparison"); no reference line
 *   fm_rank_transform <- build-defined extension A13: per-month cross-sectional ranks of the
 *                      characteristics (pandas groupby(month)[x].rank); no reference line
 *   fm_month_links, fm_horizon_return <- build-defined extension A16: each row's position in the
 *                      same firm's row of the neighbouring calendar month, and from those links
 *                      the compounded k-month return (1 + r_t) ... (1 + r_{t+k-1}) - 1 (the
 *                      dependent variable of the paper's Tables 8 and 9, "longer-horizon
 *                      expected returns"); no reference line
 *   fm_forecast_horizon <- build-defined extension A17: per month, the monthly forecasts scaled
 *                      to k months (geometric decay toward the cross-sectional mean) and the
 *                      k-month return regressed on them (the paper's second long-horizon
 *                      approach, lower panels of Tables 9a and 9b); no reference line
 *   fm_portfolio_alpha <- build-defined extension A18: the time-series regressions of every
 *                      forecast-sorted portfolio's return on factor returns (CAPM and three-factor
 *                      alphas with classical and Newey-West t-statistics, the second table of the
 *                      paper's portfolio section); no reference line
 *   fm_portfolio_hold <- build-defined extension A19; no reference line: the forecast-sorted
 *                      portfolios held for k months as overlapping cohorts (the calendar-time
 *                      strategy of Jegadeesh and Titman), its monthly return record, the cohorts'
 *                      sizes and persistence, and the monthly name turnover
 *   fm_group_adjust <- build-defined extension A20; no reference line: each characteristic
 *                      adjusted within a group of firms (an industry) per month -- the value minus
 *                      its group's mean, the group mean, or the within-group z-score (pandas
 *                      groupby([month, industry]).transform; Asness, Porter and Stevens 2000)
 *   fm_wls          <- build-defined extension A22; no reference line: the weighted (value-weighted)
 *                      monthly cross-sections, statsmodels' WLS per month, written as fm_solve
 *                      writes the OLS ones
 *   fm_pool         <- build-defined extension A23; no reference line: the pooled panel OLS of the
 *                      same regressions with classical, White, month-clustered, firm-clustered and
 *                      two-way clustered standard errors, with or without month fixed effects
 *                      (Petersen 2009; Thompson 2011; Cameron, Gelbach and Miller 2011)
 *   fm_segment_moments, fm_distinct_count <- build_table_1's monthly mean / std(ddof=1)
 *                      and permno nunique (src/calc_Lewellen_2014.py:623-646)
 *   fm_firm_chars   <- get_factors' twelve monthly characteristics: groupby("permno")
 *                      .shift(k) lags, rolling(11).apply(np.prod), rolling(12).sum(),
 *                      rolling(24).sum() and the log / ratio arithmetic of calc_log_size ..
 *                      calc_sales_price (src/calc_Lewellen_2014.py:137-341, called at :537-548)
 *   fm_rolling_std  <- calc_std_12's groupby("permno")["retx"].rolling(252,
 *                      min_periods=100).std() * sqrt(252) (src/calc_Lewellen_2014.py:448-456)
 *   fm_rolling_beta <- calculate_rolling_beta's polars 156-week group_by_dynamic beta
 *                      (src/calc_Lewellen_2014.py:344-434)
 *   fm_ffill_expand <- expand_compustat_annual_to_monthly's per-gvkey monthly reindex +
 *                      forward fill (src/transform_compustat.py:101-172)
 *   fm_sorted_join  <- merge_CRSP_and_Compustat's gvkey and (permno, jdate) equality merges
 *                      (src/transform_compustat.py:218-225)
 *   fm_gen_panel    <- (bench/test data) counter-based synthetic panel, bit-identical to
 *                      fmcore/synth.py
 *
 * Conventions: every pointer is device memory allocated by the caller (PyTorch); the
 * library never allocates device memory and keeps no pointer after return.  `stream` is a
 * hipStream_t passed as void*; all work is enqueued on it asynchronously.  Return 0 on
 * success, < 0 on error (fm_last_error() has the message, per thread).  Panels are
 * column-major SoA: column c of a panel is cols[c*col_stride + row], rows sorted by
 * (month, permno); seg_off[nseg+1] are the month (segment) row offsets.
 */
#ifndef FM_HIP_H
#define FM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_OK 0
#define FM_EINVAL (-1)
#define FM_EHIP (-2)
#define FM_ETOOBIG (-3)

/* per (segment, problem) status bits */
#define FM_ST_FITTED 0x1u
#define FM_ST_SKIPPED 0x2u        /* N < K+1: month absent from the output            */
#define FM_ST_INF_IN_X 0x4u       /* statsmodels MissingDataError('exog contains inf') */
#define FM_ST_INF_IN_Y 0x8u
#define FM_ST_CONST_SUSPECT 0x10u /* near-zero centered variance; exact check pending  */
#define FM_ST_CONST_COL 0x20u     /* nonzero constant regressor -> IndexError          */
#define FM_ST_RANK_DEF 0x40u      /* pinv min-norm solution (a null direction was cut)  */
#define FM_ST_REFIT 0x80u         /* ill-conditioned Sxx (pivot < 1e-6 of its diagonal):
                                     fm_solve_fixup re-solves from the rows (QR + SVD)   */
#define FM_ST_NEG_VAR 0x100u      /* fm_pool: a two-way clustered variance is not above 0 */

#define FM_MAX_COLS 31            /* z = [1, cols] fits two 16-wide MFMA tiles          */
#define FM_MAX_MODELS 6
#define FM_MAX_LEVELS 3

typedef struct fm_gram_args {
    const double* cols;       /* [ncols][col_stride] */
    int64_t col_stride;
    int32_t ncols;            /* <= FM_MAX_COLS */
    int32_t nseg;
    const int64_t* seg_off;   /* [nseg+1] */
    const int32_t* chunk_seg; /* [nchunks] segment of each chunk */
    const int64_t* chunk_row; /* [2*nchunks]: (row0, row1) of each chunk, inside one segment */
    int32_t nchunks;
    const double* lo;         /* [ncols][nseg] clip bounds or NULL (NaN bound = none) */
    const double* hi;
    const double* shift;      /* [ncols][nseg] pivot subtracted before accumulation, or NULL */
    const double* inv_scale;  /* [ncols][nseg] multiplier after the shift (standardize), or NULL */
    const uint8_t* level;     /* [rows] universe level 0..nlevels-1, or NULL */
    int32_t nlevels;
    const uint32_t* model_mask;   /* [nmodels] bit c: column c must be non-NaN */
    const uint32_t* model_ymask;  /* [nmodels] bit of the dependent column */
    int32_t nmodels;
    const uint8_t* pattern_id;    /* [1<<nmodels] validity pattern -> id, 255 = drop row */
    int32_t npatterns;            /* buckets = npatterns * nlevels */
    double* partial;              /* [nchunks][nbuckets][zw*(zw+1)/2] packed upper triangle, zw = 16 or 32 */
    uint32_t* flags;              /* [nseg][nmodels] reserved (not written: fm_solve detects inf in
                                     X / y per problem from the Gram diagonal); zeroed by caller */
    const int32_t* chunk_order;   /* [nchunks] chunk processed by workgroup b, or NULL: chunks in
                                     reverse index order (the months fm_select streamed last, still
                                     in the Infinity Cache, first).  Only the launch order: each
                                     chunk's partial is the same either way */
    /* optional: cols as 32-bit planes (fm_split_planes / fm_gen_panel_planes, [ncols][plane_stride]
     * each): rows are read from the planes instead of cols (the same bytes; the high plane
     * fm_select just streamed is still in the Infinity Cache), and cols may be NULL.  NULL: cols */
    const uint32_t* hi_plane;
    const uint32_t* lo_plane;
    int64_t plane_stride;
    /* optional balanced plan: workgroup b accumulates chunks [wg_chunk_off[b], wg_chunk_off[b+1])
     * one after another (a chunk still lies inside one segment; a workgroup's chunks are
     * consecutive, so a workgroup can take the tail of one month and the head of the next and
     * every workgroup gets the same number of rows).  NULL: one chunk per workgroup */
    const int32_t* wg_chunk_off;
    int32_t nwg;
} fm_gram_args;
/* The argument structs (fm_gram_args, fm_solve_args, fm_select_args, ...) grow at the end:
 * zero-initialize them before filling fields, so fields a caller does not know are NULL / 0. */

typedef struct fm_solve_args {
    const double* partial;        /* from fm_gram */
    const int32_t* seg_chunk_off; /* [nseg+1] chunk range of each segment */
    int32_t nseg;
    int32_t zw;                   /* 16 or 32 */
    int32_t nlevels;
    int32_t npatterns;
    const uint32_t* pattern_models; /* [npatterns] bitmask of models valid in that pattern */
    int32_t nprob;
    const int32_t* prob_model;    /* [nprob] */
    const int32_t* prob_level;    /* [nprob] universe level u: buckets with level >= u */
    const int32_t* prob_z;        /* [nprob][32] z indices: 0 (intercept), x..., y */
    const int32_t* prob_nz;       /* [nprob] number of z indices P+1 (<= 32) */
    const int32_t* prob_flags;    /* [nprob] bit0: check nonzero-constant columns */
    const double* add_back;       /* [ncols][nseg] shift to add back for raw intercept, or NULL */
    const uint32_t* gram_flags;   /* [nseg][nmodels] extra FM_ST_INF_* bits OR-ed in, or NULL */
    int32_t nmodels;
    int32_t pmax;                 /* >= max P (= K+1) over problems, <= 32 */
    double* rec;                  /* [nseg][nprob][pmax+2]: intercept, slopes..., NaN pad,
                                     R2 at [pmax], N at [pmax+1] */
    uint32_t* status;             /* [nseg][nprob] FM_ST_* bits */
    double* moments;              /* [nseg][nprob][mom_stride] or NULL: n, means(K+1), centered (K+1)^2 */
    int32_t mom_stride;
    int32_t ab_ncols;             /* rows of add_back ([ab_ncols][nseg]; the panel's ncols) */
    /* What the statsmodels fix-ups read besides the problem tables, add_back, moments, pmax, rec
     * and status above: the panel columns the Gram read ([ncols][fix_stride], months
     * fix_seg_off[nseg+1]), its cuts, the standardizing shift / scale and the universe levels;
     * moments must be set.  The fix-ups take the same row set as fm_gram (clip to fix_lo /
     * fix_hi, NaN drop, level >= the problem's); with fix_inv_scale the design value is
     * (x - fix_shift) * fix_inv_scale (+ add_back), without it the raw clipped x (add_back
     * must then restore the shift, as fm_solve assumes); fix_check_const != 0 adds the exact
     * nonzero-constant test of the CONST_SUSPECT pairs.
     *   fm_solve with these set (zw 16 and pmax <= 15 only): each month's own workgroup does the
     *     fix-ups right after its solve, inside that launch;
     *   fm_solve with all of them NULL / 0 (the zero-initialised default): none; set them on the
     *     same struct afterwards and call fm_solve_fixup. */
    const double* fix_cols;
    int64_t fix_stride;
    const int64_t* fix_seg_off;
    const double* fix_lo;
    const double* fix_hi;
    const double* fix_shift;
    const double* fix_inv_scale;
    const uint8_t* fix_level;
    int32_t fix_check_const;
    int32_t fix_pad;
    /* the fix-ups' rows from the split panel's planes instead (fix_cols NULL; plane stride =
     * fix_stride): a panel that holds no FP64 columns */
    const uint32_t* fix_hi_plane;
    const uint32_t* fix_lo_plane;
} fm_solve_args;

const char* fm_version(void);
const char* fm_last_error(void);
/* Every argument struct of this header, once: X(name) per struct.  A new struct is one more
 * entry here (and its class in the bindings). */
#define FM_ARG_STRUCTS(X)                                                                     \
    X(fm_gram_args) X(fm_solve_args) X(fm_select_args) X(fm_universe_args) X(fm_ts_args)      \
    X(fm_chars_args) X(fm_port_args) X(fm_rank_args) X(fm_forecast_src) X(fm_fport_args)      \
    X(fm_fdist_args) X(fm_fcmp_args) X(fm_links_args) X(fm_horizon_args) X(fm_fhor_args)      \
    X(fm_alpha_args) X(fm_hold_args) X(fm_gadj_args) X(fm_dsort_args) X(fm_wls_args) \
    X(fm_pool_args)
/* sizeof the named struct of FM_ARG_STRUCTS ("fm_gram_args", ...); -1 for an unknown name.
 * Bindings check their struct layouts against it before the first call. */
int64_t fm_struct_size(const char* name);
int fm_device_arch(char* buf, int32_t len);

int fm_select_cuts(const double* cols, int64_t col_stride, int32_t ncols,
                   const int64_t* seg_off, int32_t nseg, int32_t max_seg_len,
                   const uint8_t* row_mask, double q_lo, double q_hi, int32_t min_count,
                   int32_t lerp_mode, double* lo, double* hi, int32_t* nvalid,
                   double* mean, double* sd, void* ws, void* stream);

/* Bytes of fm_select_args.ws for a call over nseg x ncols units of <= max_seg_len rows (the
 * fix-up worklist; past 6,144 rows also the zero-sign replay slots).  The caller zeroes the
 * buffer ONCE; every fm_select / fm_select_cuts / fm_select_universe call leaves it zeroed,
 * so one buffer serves any number of calls on one stream.  < 0: bad sizes. */
int64_t fm_select_ws_bytes(int32_t nseg, int32_t ncols, int32_t max_seg_len);

/* fm_select: fm_select_cuts with an argument struct and one more optional output.
 * Outputs are [ncols][nseg]; every output pointer except lo / hi may be NULL.
 *   mean, sd: moments of the clipped values (ddof = 1), for the per-month standardization;
 *   center:   a pivot inside the data for the Gram (midpoint of the cuts, else of the
 *             segment's finite range, else 0); costs nothing beyond the cuts;
 *   level:    the universe level byte of every row from the two cuts (see the field).
 * ws is required (nvalid enables the wave fast paths).  Every path ends with a fix-up launch that redoes, exactly, the
 * units the fast kernels could not finish and the units whose numpy cut is exactly +-0: for
 * those, when the unit holds both -0.0 and +0.0, numpy 1.26.4's partition order is replayed
 * (np.percentile takes the sign of a zero cut from it; reference :519-524), so the cuts are
 * bit-exact including that sign.  The struct must be zero-initialized before filling it (new
 * trailing fields are then NULL / 0). */
typedef struct fm_select_args {
    const double* cols;
    int64_t col_stride;
    int32_t ncols;
    const int64_t* seg_off;
    int32_t nseg;
    int32_t max_seg_len;
    const uint8_t* row_mask;     /* [rows] nonzero = row takes part, or NULL */
    double q_lo, q_hi;           /* quantiles in [0, 1] */
    int32_t min_count;           /* fewer valid values: cuts are NaN (no clipping) */
    int32_t lerp_mode;           /* 0 numpy 'linear', 1 pandas groupby.quantile */
    double* lo;
    double* hi;
    int32_t* nvalid;
    double* mean;
    double* sd;
    double* center;
    uint8_t* level;              /* [rows] or NULL; ncols == 1 only: every row's universe level
                                    (x >= lo) + (x >= hi) of the UNMASKED column (NaN compares
                                    False), i.e. get_subsets' nested masks from the NYSE cuts
                                    (src/calc_Lewellen_2014.py:95-105), by a streaming
                                    launch after the cuts (same stream) */
    void* ws;                    /* fm_select_ws_bytes(nseg, ncols, max_seg_len) bytes, zeroed
                                    once by the caller, left zeroed by every call */
    const uint32_t* hi_plane;    /* optional: the high 32-bit words of cols ([ncols][plane_stride],
                                    fm_split_planes).  The two-wave (<= 6,144-row months) and
                                    long-month kernels then order values by these words (half the
                                    bytes) and gather full values from cols only at the target ranks */
    int64_t plane_stride;
    const uint32_t* lo_plane;    /* optional, with hi_plane: the low words.  With both planes cols may
                                    be NULL (a split panel without FP64 columns): the gathers and the
                                    fix-up paths then read values from the planes.  Paths that need
                                    FP64 columns (moments, row masks, > 20,480-row months) return
                                    FM_EINVAL for such a panel. */
} fm_select_args;

int fm_select(const fm_select_args* args, void* stream);

/* fm_select_universe: fm_select's cuts of `args` AND fm_universe's NYSE breakpoints + level
 * bytes (get_subsets, reference src/calc_Lewellen_2014.py:69-105) over the same month
 * segments (args->seg_off / nseg / max_seg_len), written to cut_a / cut_b [nseg] and level
 * [rows]: the winsorize cuts of calc_Lewellen_2014.py:516-527 and the universes of :74-96 in
 * one call.  Months of <= 5,120 rows (the register select paths) run the universe months in
 * the select fix-up's launch; months of 6,145 .. 20,480 rows (fm_select's long-month path,
 * no row mask, no moments) put them into the long-month launch (one more grid column);
 * otherwise the universe runs first, on its own (fm_universe, or the row-masked select +
 * level bytes past 16,384 rows).  Outputs are identical to fm_select + fm_universe. */
typedef struct fm_universe_args {
    const double* me;            /* [rows] */
    const uint8_t* nyse;         /* [rows] nonzero = NYSE row */
    double q_a, q_b;             /* pandas groupby.quantile levels (0.2, 0.5) */
    double* cut_a;               /* [nseg] */
    double* cut_b;               /* [nseg] */
    uint8_t* level;              /* [rows] (me >= cut_a) + (me >= cut_b) */
} fm_universe_args;

int fm_select_universe(const fm_select_args* args, const fm_universe_args* u, void* stream);

int fm_clip(const double* src, double* dst, int64_t col_stride, int32_t ncols,
            const int64_t* seg_off, int32_t nseg, int64_t nrows,
            const double* lo, const double* hi, void* stream);

int fm_standardize(const double* src, double* dst, int64_t col_stride, int32_t ncols,
                   const int64_t* seg_off, int32_t nseg, int64_t nrows,
                   const double* mean, const double* sd, void* stream);

int fm_universe_level(const double* me, const int64_t* seg_off, int32_t nseg, int64_t nrows,
                      const double* cut_a, const double* cut_b, uint8_t* level, void* stream);

/* fm_universe: per month the pandas-lerp q_a / q_b quantiles of `me` over rows with
 * nyse != 0 (NaN me skipped; no such row -> NaN cuts) into cut_a / cut_b [nseg], and every
 * row's level (me >= cut_a) + (me >= cut_b) (NaN compares False).  Months of at most
 * 64 * 256 rows; longer ones return FM_ETOOBIG (fm_select_cuts with a row mask +
 * fm_universe_level do any length). */
int fm_universe(const double* me, const uint8_t* nyse, const int64_t* seg_off, int32_t nseg,
                int32_t max_seg_len, double q_a, double q_b, double* cut_a, double* cut_b,
                uint8_t* level, void* stream);

int fm_pilot_shift(const double* cols, int64_t col_stride, int32_t ncols,
                   const int64_t* seg_off, int32_t nseg, double* shift, void* stream);

int fm_gram(const fm_gram_args* args, void* stream);

int fm_solve(const fm_solve_args* args, void* stream);

/* fm_solve_fixup: the statsmodels fix-ups as a launch of their own, for solves that did not
 * run them inline (zw 32, or pmax > 15).  `args` is the struct of the preceding fm_solve call
 * with its fix_* fields now set (see fm_solve_args): the launch reads those, the problem
 * tables (prob_level, prob_z, prob_nz), add_back, moments, mom_stride, pmax, nseg and nprob,
 * scans every (month, problem) status word on the device and fixes the pairs whose bits ask
 * for it (CONST_SUSPECT with fix_check_const; FITTED|INF_IN_Y or FITTED|REFIT) in rec /
 * status, so callers need no host round trip.  FP64 columns only: fix_cols is required and a
 * plane set is FM_EINVAL. */
int fm_solve_fixup(const fm_solve_args* args, void* stream);

int fm_ts_compact(const uint32_t* status, int64_t s_seg, int64_t s_prob, int32_t nseg,
                  int32_t nprob, int32_t* idx, int32_t* count, void* stream);

/* fm_ts_summary: work holds nprob * kmax * (nseg + ceil(nseg / 2048) * 28) doubles (series of
 * >= 4096 months take the chunked one-pass kernels, whose partials follow the series). */
int fm_ts_summary(const double* rec, int64_t r_seg, int64_t r_prob, const int32_t* idx,
                  const int32_t* count, int32_t nseg, int32_t nprob, int32_t kmax,
                  int32_t nw_lags, double* mean, double* se, double* tstat, int32_t* nobs,
                  double* work, void* stream);

int fm_rolling_mean(const double* rec, int64_t r_seg, int64_t r_prob, const int32_t* idx,
                    const int32_t* count, int32_t nseg, int32_t nprob, int32_t kmax,
                    int32_t window, int32_t min_periods, double* out, void* stream);

/* fm_rolling_mean for a month-sharded rank: only the output rows a predictive stage of months
 * [seg_lo, seg_hi) reads (the fitted rows of those months and the `lag` rows before the
 * first), computed exactly as fm_rolling_mean computes them (same bits); other rows of `out`
 * are left unwritten (the per-thread row blocks that hold no such row are skipped). */
int fm_rolling_mean_own(const double* rec, int64_t r_seg, int64_t r_prob, const int32_t* idx,
                        const int32_t* count, int32_t nseg, int32_t nprob, int32_t kmax,
                        int32_t window, int32_t min_periods, int32_t seg_lo, int32_t seg_hi,
                        int32_t lag, double* out, void* stream);

int fm_predictive(const double* moments, int32_t mom_stride, int32_t nseg, int32_t nprob,
                  const int32_t* prob_k, const int32_t* idx, const int32_t* count,
                  const double* rolling, int32_t pmax, int32_t lag, int32_t seg_lo,
                  int32_t seg_hi, double* pred, uint32_t* pred_status, void* stream);

/* fm_ts_fused: fm_ts_compact + fm_ts_summary + fm_rolling_mean + fm_predictive in one
 * launch (per problem: a workgroup per coefficient summary and per 64 fitted-month rows of
 * rolling means + predictive slopes, each staging its records in LDS).  roll == NULL skips
 * the rolling and predictive phases, pred == NULL the predictive phase; called on the
 * predictive records (rec = pred, status = pred_status) it gives their FM summary.  Outputs
 * as in the separate entry points; work is unused (may be NULL). */
typedef struct fm_ts_args {
    const double* rec;            /* records, element (month s, problem p, k) at s*r_seg + p*r_prob + k */
    int64_t r_seg, r_prob;
    const uint32_t* status;       /* status of (s, p) at s*s_seg + p*s_prob */
    int64_t s_seg, s_prob;
    int32_t nseg, nprob, kmax, nw_lags;
    int32_t* idx;                 /* [nprob][nseg] fitted months, ascending */
    int32_t* count;               /* [nprob] */
    double* mean;                 /* [nprob][kmax] */
    double* se;
    double* tstat;
    int32_t* nobs;
    double* work;                 /* unused (ABI slot), may be NULL */
    int32_t window, min_periods, pmax;
    double* roll;                 /* [nprob][nseg][pmax] or NULL */
    const double* moments;        /* [seg_hi - seg_lo][nprob][mom_stride] */
    int32_t mom_stride;
    const int32_t* prob_k;        /* [nprob] */
    int32_t lag, seg_lo, seg_hi;
    double* pred;                 /* [nprob][nseg][4] or NULL */
    uint32_t* pred_status;        /* [nprob][nseg] */
    /* Month-sharded runs (zero-initialised = off; every rank runs the stage on the gathered
     * series, each doing only its share):
     *   sum_p_hi > 0: the FM summaries (mean, se, tstat, nobs) of problems [sum_p_lo,
     *     sum_p_hi) only; the other problems' summaries are written as -0.0 / 0, so a SUM
     *     all-reduce over the ranks returns every problem's summary bit for bit;
     *   roll_own != 0: rolling means only in the rolling workgroups whose rows hold a fitted
     *     month in [seg_lo, seg_hi) or one of the `lag` rows before the first such row (the
     *     rows this rank's predictive records read); the other workgroups write no rolling
     *     means (those roll rows are left unwritten) but still their predictive records
     *     (-0.0 / status 0 for other ranks' months).  Computed rows are bit-identical to a
     *     full run's. */
    int32_t sum_p_lo, sum_p_hi;
    int32_t roll_own;
    int32_t pad_ts;
} fm_ts_args;

/* LDS bytes the fused launch stages per workgroup; it must not exceed FM_TS_FUSED_MAX_LDS
 * (otherwise use fm_ts_compact / fm_ts_summary / fm_rolling_mean / fm_predictive). */
#define FM_TS_FUSED_MAX_LDS (128 * 1024)
size_t fm_ts_fused_lds_bytes(int32_t nseg, int32_t pmax, int32_t window, int32_t lag,
                             int32_t rolling, int32_t predictive);
int fm_ts_fused(const fm_ts_args* args, void* stream);

int fm_forecast(const double* cols, int64_t col_stride, int32_t K, const int64_t* seg_off,
                int32_t nseg, int64_t nrows, const double* coef, int32_t coef_stride,
                double* out, void* stream);

/* fm_portfolio_sort: per month, sort the stocks into nport portfolios by forecast and average
 * each portfolio's realised return and forecast (build-defined extension A12; no reference
 * line).  Rows sorted by (month, permno), months seg_off[nseg+1] of at most 16,384 rows
 * (longer: FM_ETOOBIG before any launch).  Per month t:
 *   eligible rows:   isfinite(forecast) and level >= min_level (level NULL: every row);
 *   breakpoint rows: the eligible rows; with nyse_breakpoints those with nyse != 0;
 *   fewer than min_count breakpoint rows: status[t] = 0, bp NaN, every port byte 255, rec NaN,
 *     cnt 0; otherwise status[t] = 1 and
 *   bp[t][j]   = numpy 'linear' quantile q[j] of the breakpoint rows' forecasts (exact order
 *                statistics; the sign of an exactly-zero breakpoint is not specified);
 *   port[row]  = #{ j : forecast > bp[t][j] } (right-closed bins) for eligible rows, else 255;
 *   cnt[t][k]  = rows of portfolio k with a finite return; over those rows
 *   rec[t][k]  = { mean return, mean forecast, sum(w ret) / sum(w), sum(w forecast) / sum(w) },
 *                the last two over the rows that also have a finite weight > 0 (weight NULL:
 *                NaN); an empty set gives NaN;
 *   rec[t][nport] = rec[t][nport-1] - rec[t][0] (high minus low; NaN if either end is).
 * Every output of a month depends on that month's rows alone, summed in a fixed order: two
 * calls, or a month-sharded call, give the same bits.  Zero-initialize the struct (it grows
 * at the end). */
#define FM_MAX_PORTS 20
typedef struct fm_port_args {
    const double* forecast;      /* [rows] */
    const double* ret;           /* [rows] */
    const double* weight;        /* [rows] or NULL */
    const uint8_t* level;        /* [rows] universe level or NULL */
    const uint8_t* nyse;         /* [rows] nonzero = NYSE row, or NULL */
    const int64_t* seg_off;      /* [nseg+1] */
    int32_t nseg;
    int32_t max_seg_len;         /* >= every month's rows, <= 16,384 */
    int32_t nport;               /* 2 .. FM_MAX_PORTS */
    int32_t min_level;
    int32_t nyse_breakpoints;    /* nonzero: breakpoints from the NYSE rows only */
    int32_t min_count;           /* >= 1 */
    double q[FM_MAX_PORTS - 1];  /* [nport-1] levels, strictly ascending in (0, 1) */
    double* bp;                  /* [nseg][nport-1] or NULL */
    uint8_t* port;               /* [rows] or NULL */
    double* rec;                 /* [nseg][nport+1][4] */
    int32_t* cnt;                /* [nseg][nport] */
    uint32_t* status;            /* [nseg] */
} fm_port_args;

int fm_portfolio_sort(const fm_port_args* args, void* stream);

/* fm_forecast_src: the fused forecast -- nsel forecasts of one panel, each row's value computed
 * in the consuming kernel's load phase from the panel's own layout instead of read from a vector.
 * It is embedded as the field `src` of fm_fport_args, fm_fdist_args, fm_fcmp_args and fm_fhor_args; nseg, seg_off and
 * max_seg_len are the embedding struct's.  Exactly one predictor source: FP64 columns (cols,
 * col_stride) or the split planes (hi_plane, lo_plane, plane_stride); both or neither: FM_EINVAL.
 * For sort j (K = sel_k[j] in 1..FM_MAX_SORT_K predictors, panel columns sel_cols[j][0..K) in
 * coefficient order), month t with the coefficient row c = coef[(j * nseg + t) * coef_stride +
 * 0..K] (coef_stride >= K + 1) and row i:
 *   x'_k = clip(x_k) exactly as fm_clip clips with lo / hi [ncols][nseg] (x < lo -> lo, x > hi
 *          -> hi; a NaN bound is ignored, a NaN x stays NaN; lo == hi == NULL: no clipping);
 *   F    = c[0], then for k = 1..K in order F = F + c[k] * x'_k, every product and every sum
 *          rounded on its own (fm_forecast's bits on the fm_clip-ped columns).
 * So a NaN in the coefficient row makes every F of the month NaN, and a NaN or +-inf predictor
 * makes the row's F not finite.  A row is eligible for sort j when F is finite and level >=
 * sel_level[j]; forecast_out (optional) receives every row's F. */
#define FM_MAX_SORTS 16
#define FM_MAX_SORT_K 30
typedef struct fm_forecast_src {
    const double* cols;          /* [ncols][col_stride] or NULL (planes) */
    int64_t col_stride;
    const uint32_t* hi_plane;    /* [ncols][plane_stride] high / low words, or NULL (cols) */
    const uint32_t* lo_plane;
    int64_t plane_stride;
    const double* lo;            /* [ncols][nseg] clip bounds, or both NULL */
    const double* hi;
    const double* coef;          /* [nsel][nseg][coef_stride] */
    double* forecast_out;        /* [nsel][nrows] or NULL */
    int64_t nrows;               /* seg_off[nseg]: the row stride of the per-row vectors */
    int32_t ncols;
    int32_t coef_stride;
    int32_t nsel;                /* 0 .. FM_MAX_SORTS */
    int32_t pad_src;
    int32_t sel_k[FM_MAX_SORTS];
    int32_t sel_level[FM_MAX_SORTS];
    int32_t sel_cols[FM_MAX_SORTS][FM_MAX_SORT_K];
} fm_forecast_src;

/* fm_forecast_portfolio_sort: src.nsel forecast sorts of one panel in one launch (grid (month,
 * sort)): fm_portfolio_sort's definition with forecast = the F of `src` (fm_forecast_src above),
 * ret = panel column ret_col (read raw, never clipped, from the same layout) and min_level =
 * src.sel_level[j] (paper Table 5 inside the device pipeline; no reference line).  A month whose
 * coefficient row holds a NaN is unsorted.  Outputs are fm_port_args' with a leading [nsel]
 * dimension.  Months of more than 16,384 rows: FM_ETOOBIG before any launch, outputs untouched.
 * nsel == 0 or nseg == 0 is a valid empty call.  Zero-initialize the struct (it grows at the
 * end). */
typedef struct fm_fport_args {
    fm_forecast_src src;
    int32_t ret_col;             /* panel column of the realised return */
    int32_t nseg;
    int32_t max_seg_len;         /* >= every month's rows, <= 16,384 */
    int32_t nport;               /* 2 .. FM_MAX_PORTS */
    int32_t nyse_breakpoints;
    int32_t min_count;           /* >= 1 */
    const double* weight;        /* [rows] or NULL */
    const uint8_t* level;        /* [rows] universe level or NULL */
    const uint8_t* nyse;         /* [rows] nonzero = NYSE row, or NULL */
    const int64_t* seg_off;      /* [nseg+1] */
    double q[FM_MAX_PORTS - 1];
    double* bp;                  /* [nsel][nseg][nport-1] or NULL */
    uint8_t* port;               /* [nsel][nrows] or NULL */
    double* rec;                 /* [nsel][nseg][nport+1][4] */
    int32_t* cnt;                /* [nsel][nseg][nport] */
    uint32_t* status;            /* [nsel][nseg] */
} fm_fport_args;

int fm_forecast_portfolio_sort(const fm_fport_args* args, void* stream);

/* fm_lagged_coef: the coefficient tables fm_forecast_portfolio_sort reads, from the time-series
 * stage's outputs without a host sync on the fitted-month counts.  For j < nsel with
 * p = problems[j] (device int32 [nsel], each in 0..nprob-1): every row out[j][t][0..pmax) is NaN
 * except, for the fitted-month rows i in [lag, count[p]),
 *   out[j][idx[p][i]][k] = roll[p][i - lag][k]
 * -- the row fm_predictive reads for the same month (roll [nprob][nseg][pmax], idx
 * [nprob][nseg] ascending, count [nprob]; lag >= 0). */
int fm_lagged_coef(const double* roll, const int32_t* idx, const int32_t* count, int32_t nseg,
                   int32_t nprob, int32_t pmax, const int32_t* problems, int32_t nsel, int32_t lag,
                   double* out, void* stream);

/* fm_forecast_dist: per month, the cross-sectional mean, standard deviation and quantiles of
 * nsel expected-return forecasts in one launch, grid (month, sort) (build-defined extension A14;
 * no reference line; paper Table 3, "univariate properties").  Rows sorted by (month, permno),
 * months seg_off[nseg+1] of at most 16,384 rows (it shares fm_portfolio_sort's selection; longer:
 * FM_ETOOBIG before any launch, outputs untouched).  Exactly one forecast source, anything else
 * FM_EINVAL:
 *   forecast [nsel][nrows]: the caller's vectors (of `src` only nsel, nrows and sel_level are
 *   then read; its cols, planes and forecast_out must be NULL), or
 *   the panel of `src` (fm_forecast_src above): sort j's forecast is its F, which is
 *   fm_forecast_portfolio_sort's, bit for bit.
 * Per (sort j, month t), all outputs with a leading [nsel] dimension:
 *   eligible rows: isfinite(F) and level >= sel_level[j] (level NULL: every row);
 *   cnt    = the number of eligible rows;
 *   cnt < min_count: status = 0 and rec[0..2+nq) NaN; otherwise status = 1 and
 *   rec[0] = the mean of F over the eligible rows: sum / cnt;
 *   rec[1] = the ddof-1 standard deviation, two passes: sqrt(sum((F - rec[0])^2) / (cnt - 1)),
 *            NaN when cnt == 1;
 *   rec[2+i] = numpy 'linear' quantile q[i] of the eligible forecasts (exact order statistics;
 *            the sign of an exactly-zero quantile is not specified).
 * Both sums run in one fixed order: the month's rows in row order are cut into tiles of 64 (rows
 * that are not eligible, and rows past the month's end, count as +0.0); a tile is summed by the
 * wave butterfly (lane l adds the value of lane l ^ 32, then ^ 16, 8, 4, 2, 1); lane l then adds
 * the tile sums l, l + 64, l + 128, ... in that order, starting from +0.0, and the 64 lane sums go
 * through the same butterfly.  So a month's bits depend on that month's rows alone: not on the
 * source, the panel's layout, the grid, the other months or max_seg_len (which picks the
 * workgroup's shape); two calls, or a month-sharded call, give the same bits.  nsel == 0 or
 * nseg == 0 is a valid empty call.  Zero-initialize the struct (it grows at the end). */
#define FM_MAX_DIST_Q 8
typedef struct fm_fdist_args {
    fm_forecast_src src;
    const double* forecast;      /* [nsel][nrows] forecast vectors, or NULL (the panel of src) */
    const uint8_t* level;        /* [rows] universe level or NULL */
    const int64_t* seg_off;      /* [nseg+1] */
    int32_t nseg;
    int32_t max_seg_len;         /* >= every month's rows, <= 16,384 */
    int32_t min_count;           /* >= 1 */
    int32_t nq;                  /* 0 .. FM_MAX_DIST_Q */
    double q[FM_MAX_DIST_Q];     /* [nq] levels, strictly ascending in (0, 1) */
    double* rec;                 /* [nsel][nseg][2+nq] */
    int32_t* cnt;                /* [nsel][nseg] */
    uint32_t* status;            /* [nsel][nseg] */
} fm_fdist_args;

int fm_forecast_dist(const fm_fdist_args* args, void* stream);

/* fm_forecast_compare: per month and per pair (a, b) of expected-return forecasts, how much of
 * forecast b forecast a already holds, and whether the rest predicts returns: the cross-sectional
 * regression of F_b on F_a and of the realised return on its residual, npair pairs in one launch,
 * grid (month, pair) (build-defined extension A15; no reference line; paper Table 4, "model
 * comparison").  Rows sorted by (month, permno), months seg_off[nseg+1] of at most 16,384 rows
 * (its siblings' limit and their three workgroup shapes; longer: FM_ETOOBIG before any launch,
 * outputs untouched).  Exactly one forecast source, anything else FM_EINVAL:
 *   forecast [nsel][nrows]: the caller's vectors, with the returns in ret [rows] (of `src` only
 *   nsel and nrows are then read; its cols, planes and forecast_out must be NULL), or
 *   the panel of `src` (fm_forecast_src above): forecast j is its F -- fm_forecast_dist's and
 *   fm_forecast_portfolio_sort's, bit for bit -- and the return is panel column ret_col, read raw
 *   (never clipped) through the same layout; ret must be NULL.  src.forecast_out, if set, receives
 *   every row's F of the forecasts some pair names (each workgroup that computes a forecast
 *   writes the same bytes).
 * Pair p regresses forecast pair_b[p] on forecast pair_a[p] (indices into the nsel forecasts) over
 * the universe pair_level[p] (0..255); src.sel_level is not read.  Per (pair p, month t), all
 * outputs with a leading [npair] dimension:
 *   set E: the rows with F_a and F_b finite and level >= pair_level[p] (level NULL: every row);
 *   set R: the rows of E with a finite return;
 *   cnt[0] = nE, cnt[1] = nR;
 *   nE < max(min_count, 2): status = 0 and rec[0..7) NaN; otherwise status = 1 and, over E,
 *   ma = sum(F_a) / nE, mb = sum(F_b) / nE; with da = F_a - ma and db = F_b - mb:
 *   Saa = sum(da * da), Sbb = sum(db * db), Sab = sum(da * db);
 *   rec[1] = the slope beta = Sab / Saa;
 *   rec[0] = the correlation Sab / sqrt(Saa * Sbb);
 *   rec[2] = the intercept mb - beta * ma;
 *   the row's residual e = db - beta * da;
 *   rec[3] = sqrt(sum(e * e) / (nE - 1)): the residual's ddof-1 standard deviation
 *            (fm_forecast_dist's convention), from a pass of its own over e -- two identical
 *            forecasts give beta == 1.0 and rec[3] == 0.0 exactly;
 *   over R with the same e (nR < 2: rec[4..7) NaN): me = sum(e) / nR, mr = sum(r) / nR,
 *   See = sum((e - me)^2), Ser = sum((e - me) * (r - mr)), Srr = sum((r - mr)^2);
 *   rec[4] = the predictive slope Ser / See;
 *   rec[5] = its intercept mr - rec[4] * me;
 *   rec[6] = its R2 (Ser * Ser) / (See * Srr).
 * Degenerate months have no special cases, IEEE arithmetic decides them: a constant F_a gives
 * 0 / 0 = NaN for the slope, the correlation and all that follows, a zero residual a NaN
 * predictive slope.  Every product, sum and quotient above is rounded on its own, in the order
 * written, and each of the eleven sums runs in fm_forecast_dist's fixed order (tiles of 64 rows in
 * row order, rows outside the set or past the month's end as +0.0, the wave butterfly, lane l
 * adding the tile sums l, l + 64, ... from +0.0, the butterfly again).  So a month's bits depend
 * on that month's rows alone: not on the source, the panel's layout, the grid, the other months,
 * the other pairs or max_seg_len; two calls, or a month-sharded call, give the same bits.
 * npair == 0 or nseg == 0 is a valid empty call.  Zero-initialize the struct (it grows at the
 * end). */
#define FM_MAX_PAIRS 16
#define FM_FCMP_NREC 7
typedef struct fm_fcmp_args {
    fm_forecast_src src;
    const double* forecast;      /* [nsel][nrows] forecast vectors, or NULL (the panel of src) */
    const double* ret;           /* [rows] returns of the vector source, else NULL */
    const uint8_t* level;        /* [rows] universe level or NULL */
    const int64_t* seg_off;      /* [nseg+1] */
    int32_t ret_col;             /* panel column of the realised return (panel source) */
    int32_t nseg;
    int32_t max_seg_len;         /* >= every month's rows, <= 16,384 */
    int32_t min_count;           /* >= 1 */
    int32_t npair;               /* 0 .. FM_MAX_PAIRS */
    int32_t pad_fcmp;
    int32_t pair_a[FM_MAX_PAIRS];     /* the regressor forecast, in [0, nsel) */
    int32_t pair_b[FM_MAX_PAIRS];     /* the regressed forecast, in [0, nsel) */
    int32_t pair_level[FM_MAX_PAIRS]; /* the pair's universe, 0..255 */
    double* rec;                 /* [npair][nseg][FM_FCMP_NREC] */
    int32_t* cnt;                /* [npair][nseg][2] */
    uint32_t* status;            /* [npair][nseg] */
} fm_fcmp_args;

int fm_forecast_compare(const fm_fcmp_args* args, void* stream);

/* fm_forecast_horizon: per month, nsel monthly expected-return forecasts scaled to a longer
 * horizon and held against the return realised over it, in one launch, grid (month, sort)
 * (build-defined extension A17; no reference line; the paper's Section 4, second approach, the
 * lower panels of Tables 9a and 9b: F_ik = k * mean + (1 + .9 + ... + .9^(k-1)) (F_i1 - mean), the
 * monthly forecast extrapolated to k months under a geometric decay toward the cross-sectional mean,
 * then the k-month return regressed on it).  Rows sorted by (month, permno), months
 * seg_off[nseg+1] of at most 16,384 rows (its siblings' limit and their three workgroup shapes;
 * longer: FM_ETOOBIG before any launch, outputs untouched).  Exactly one forecast source, anything
 * else FM_EINVAL:
 *   forecast [nsel][nrows]: the caller's vectors (of `src` only nsel, nrows and sel_level are
 *   then read; its cols, planes and forecast_out must be NULL), or
 *   the panel of `src` (fm_forecast_src above): sort j's forecast is its F, fm_forecast_dist's bit
 *   for bit; src.forecast_out, if set, receives every row's F.
 * The realised return is always the vector ret [rows] (fm_horizon_return's output), whatever the
 * forecast's source.  With a = level_mult (finite) and g = gain (finite, > 0), per (sort j, month
 * t), all outputs with a leading [nsel] dimension:
 *   set E: the rows with F finite and level >= sel_level[j] (level NULL: every row);
 *   set R: the rows of E with a finite ret;
 *   cnt[0] = nE, cnt[1] = nR;
 *   nE < min_count: status = 0, rec[0..6+nq) NaN and the month's rows of scaled_out NaN;
 *   otherwise status = 1 and
 *   m = sum(F over E) / nE: fm_forecast_dist's rec[0] on the same input, bit for bit;
 *   the scaled forecast of a row of E is G = a * m + g * (F - m), three operations rounded one by
 *   one: base = a * m; d = F - m; G = base + g * d.  Rows outside E have G = NaN.  scaled_out, if
 *   set, receives every row's G;
 *   rec[0] = sum(G over E) / nE;
 *   rec[1] = the ddof-1 standard deviation of G over E, two passes:
 *            sqrt(sum((G - rec[0])^2) / (nE - 1)), NaN when nE == 1;
 *   rec[5] = m;
 *   rec[6+i] = numpy 'linear' quantile q[i] of G over E: G is non-decreasing in F, so the two
 *            neighbouring order statistics of F (exact, fm_forecast_dist's) are mapped through the
 *            three operations above and interpolated as there;
 *   over R (nR < 2: rec[2..5) NaN): mg = sum(G) / nR, mr = sum(ret) / nR,
 *   Sgg = sum((G - mg)^2), Sgr = sum((G - mg) * (ret - mr)), Srr = sum((ret - mr)^2);
 *   rec[2] = the predictive slope Sgr / Sgg;
 *   rec[3] = its intercept mr - rec[2] * mg;
 *   rec[4] = its R2 (Sgr * Sgr) / (Sgg * Srr).
 * Degenerate months have no special cases, IEEE arithmetic decides them, as in
 * fm_forecast_compare: a constant forecast gives a NaN slope.  Every product, sum and quotient
 * above is rounded on its own, in the order written, and each of the eight sums runs in
 * fm_forecast_dist's fixed order (tiles of 64 rows in row order, rows outside the set or past the
 * month's end as +0.0, the wave butterfly, lane l adding the tile sums l, l + 64, ... from +0.0,
 * the butterfly again).  So a month's bits depend on that month's rows alone: not on the source,
 * the panel's layout, the grid, the other months, the other sorts or max_seg_len; two calls, or a
 * month-sharded call, give the same bits.  nsel == 0 or nseg == 0 is a valid empty call.
 * Zero-initialize the struct (it grows at the end). */
#define FM_FHOR_NREC 6
typedef struct fm_fhor_args {
    fm_forecast_src src;
    const double* forecast;      /* [nsel][nrows] forecast vectors, or NULL (the panel of src) */
    const double* ret;           /* [rows] the realised k-month return */
    const uint8_t* level;        /* [rows] universe level or NULL */
    const int64_t* seg_off;      /* [nseg+1] */
    int32_t nseg;
    int32_t max_seg_len;         /* >= every month's rows, <= 16,384 */
    int32_t min_count;           /* >= 1 */
    int32_t nq;                  /* 0 .. FM_MAX_DIST_Q */
    double q[FM_MAX_DIST_Q];     /* [nq] levels, strictly ascending in (0, 1) */
    double level_mult;           /* a: the multiple of the month's mean forecast; finite */
    double gain;                 /* g: the factor on the deviation from it; finite, > 0 */
    double* scaled_out;          /* [nsel][nrows] or NULL */
    double* rec;                 /* [nsel][nseg][FM_FHOR_NREC + nq] */
    int32_t* cnt;                /* [nsel][nseg][2] */
    uint32_t* status;            /* [nsel][nseg] */
} fm_fhor_args;

int fm_forecast_horizon(const fm_fhor_args* args, void* stream);

/* fm_rank_transform: every chosen column's cross-sectional rank within its month (build-defined
 * extension A13; no reference line).  It is pandas' groupby(month)[x].rank(method, pct) and is
 * pinned to it bit for bit.  Rows sorted by (month, permno), months seg_off[nseg+1] of at most
 * FM_RANK_MAX_ROWS = 65,536 rows (longer: FM_ETOOBIG before any launch, outputs untouched).  Per
 * column and month:
 *   eligible rows: the value is not NaN and, with level given, level >= min_level;
 *   order:         +-inf are ordinary values; -0.0 and +0.0 are equal;
 *   counts:        n = the month's eligible rows; for an eligible row, less = the eligible rows
 *                  with a smaller value, eq = those with an equal value, itself included;
 *   rank r:        FM_RANK_AVERAGE less + (eq + 1) / 2, FM_RANK_MIN less + 1, FM_RANK_MAX less + eq;
 *   output:        FM_RANK_RAW r, FM_RANK_PCT r / n, FM_RANK_UNIFORM r / (n + 1) - 0.5 (two IEEE
 *                  operations, not contracted); ineligible rows get NaN;
 *   nvalid[c][t] = n.
 * Every r is a multiple of 0.5 and exact in FP64, so every output is specified to the bit.  A
 * month's outputs depend on that month's rows alone: two calls, or a month-sharded call, give
 * the same bits.  dst == src is refused (FM_EINVAL).  pandas' methods "first" and "dense" are
 * out of scope: the three methods above need only the two counts of a row's key, which a sort
 * of the keys alone gives; "first" needs a stable (key, row) sort and "dense" a distinct count.
 * Cost and the limit: with max_seg_len <= 16,384 one workgroup sorts a month's keys in LDS.  A
 * longer max_seg_len takes another kernel for every month of the call: less, less + eq and n
 * are sums over any partition of the month's eligible rows, so the month is visited in parts
 * of 16,384 rows and one workgroup per part sorts every part in turn and sums the counts of its
 * own rows' keys over them (one launch, no workspace, no atomics; same bits).  That is parts^2
 * part-sorts per (column, month): quadratic in the length, which is why the limit is 4 parts
 * and not any length -- past that a global segmented sort is the right tool.  Keep months of up
 * to 16,384 rows in calls of their own where that is possible.
 * Zero-initialize the struct (it grows at the end). */
#define FM_RANK_MAX_ROWS 65536
#define FM_RANK_AVERAGE 0
#define FM_RANK_MIN 1
#define FM_RANK_MAX 2
#define FM_RANK_RAW 0
#define FM_RANK_PCT 1
#define FM_RANK_UNIFORM 2
typedef struct fm_rank_args {
    const double* src;           /* [ncols][src_stride], rows sorted by (month, permno) */
    int64_t src_stride;
    double* dst;                 /* [ncols][dst_stride] */
    int64_t dst_stride;
    int32_t ncols;
    int32_t nseg;
    const int64_t* seg_off;      /* [nseg+1] */
    int32_t max_seg_len;         /* >= every month's rows, <= FM_RANK_MAX_ROWS; chooses the kernel */
    int32_t min_level;
    const uint8_t* level;        /* [rows] universe level or NULL (every row) */
    int32_t method;              /* FM_RANK_AVERAGE / MIN / MAX */
    int32_t scale;               /* FM_RANK_RAW / PCT / UNIFORM */
    int32_t* nvalid;             /* [ncols][nseg] the month's count of ranked rows, or NULL */
} fm_rank_args;

int fm_rank_transform(const fm_rank_args* args, void* stream);

/* fm_month_links: for every row of a month-sorted panel, where the same firm's row lies in the
 * neighbouring calendar month (build-defined extension A16; no reference line).  Rows sorted by
 * (month, firm id), months seg_off[nseg+1] of any length below 2^31 rows, nrows = seg_off[nseg];
 * ids are full int64 and strictly ascending inside a month; month_index[s] is the calendar month
 * number of segment s (year * 12 + month - 1, or any integer count of months), strictly ascending.
 * For row i of segment s, with t = s + step:
 *   link[i] = the position inside segment t (0-based) of the row of t with ids == ids[i], when
 *             0 <= t < nseg, month_index[t] == month_index[s] + step and such a row exists;
 *   link[i] = -1 otherwise (no neighbouring segment, a gap in the calendar, the firm is absent).
 * bad[0] (zeroed by the caller) receives the number of rows whose id is not greater than their
 * predecessor's in the month.  The links of a call with bad != 0 are unspecified (the searches
 * assume the order), but every access stays inside ids[0, nrows).  Arguments are refused with
 * FM_EINVAL before any launch: step other than +1 / -1, nseg or nrows below zero, a NULL pointer
 * (the message names the field).  nseg == 0 or nrows == 0 is a valid empty call.  Zero-initialize
 * the struct (it grows at the end). */
typedef struct fm_links_args {
    const int64_t* ids;          /* [nrows] firm id of each row */
    const int64_t* seg_off;      /* [nseg+1] */
    const int32_t* month_index;  /* [nseg] calendar month number, strictly ascending */
    int64_t nrows;               /* seg_off[nseg] */
    int32_t nseg;
    int32_t step;                /* +1: the following month, -1: the preceding one */
    int32_t* link;               /* [nrows] */
    int32_t* bad;                /* [1], zeroed by the caller */
} fm_links_args;

int fm_month_links(const fm_links_args* args, void* stream);

/* fm_horizon_return: the compounded `horizon`-month return of every row from the step +1 links
 * of fm_month_links (build-defined extension A16; no reference line; the dependent variable of
 * the paper's Tables 8a/8b and 9a/9b).  Returns are decimals.  For row i of segment s:
 *   row_0 = i; for j = 1 .. horizon-1: row_j = seg_off[s+j] + link[row_{j-1}];
 *   a hop is missing when s + j >= nseg, when the link is negative or not below the length of
 *   segment s + j (a stale or foreign link array gives NaN, never a read outside [0, nrows));
 *   a missing hop: out[i] = NaN; otherwise p = 1 + ret[row_0], then p = p * (1 + ret[row_j]) for
 *   j = 1 .. horizon-1 in that order, and out[i] = p - 1.
 * Every operation is rounded on its own, so the output is specified to the bit: a NaN or infinite
 * return propagates by the IEEE rules, and horizon 1 gives (1 + r) - 1, not r.  A month's output
 * depends on that month's rows and the following horizon-1 months' rows alone.  Refused with
 * FM_EINVAL before any launch: horizon outside 1..FM_MAX_HORIZON, nseg or nrows below zero, a NULL
 * pointer, out overlapping ret or link.  nseg == 0 or nrows == 0 is a valid empty call.
 * Zero-initialize the struct (it grows at the end). */
#define FM_MAX_HORIZON 60
typedef struct fm_horizon_args {
    const double* ret;           /* [nrows] one-month returns */
    const int32_t* link;         /* [nrows] fm_month_links with step +1 */
    const int64_t* seg_off;      /* [nseg+1] */
    int64_t nrows;               /* seg_off[nseg] */
    int32_t nseg;
    int32_t horizon;             /* 1 .. FM_MAX_HORIZON */
    double* out;                 /* [nrows] */
} fm_horizon_args;

int fm_horizon_return(const fm_horizon_args* args, void* stream);

/* fm_portfolio_alpha: the factor-model alphas of the forecast-sorted portfolios -- every
 * portfolio's (and the high-minus-low spread's) equal- and value-weighted monthly return regressed
 * on M sets of factor returns, with classical and Newey-West (HAC) coefficient standard errors, in
 * one launch with one workgroup per (series, model) (build-defined extension A18; no reference
 * line; the 2014 working paper's "Alphas for expected-return sorted portfolios", the second table
 * of the paper's portfolio section).  Inputs are fm_portfolio_sort's rec / status, read in place
 * through their strides, and factors [T][K] (row t = month t, contiguous) with an optional rf [T].
 * A series is (sort j < nsel, row p < nrow, weighting w in {0: ew, 1: vw}).  Its dependent value in
 * month t is
 *   d_t = rec[j * rec_sort + t * rec_month + p * rec_row + 2 * w * rec_col] - rf[t]
 * with rf NULL or p == spread_row (a difference of two returns): the raw rec value.
 * Model m is the set of factor columns in model_mask[m] (bit f = column f), k = its size.  It uses
 * month t of a series only if status[j * st_sort + t * st_month] == 1, d_t is finite and every
 * factor of m is finite at t.  The used months in month order are treated as consecutive
 * (fm_ts_summary's dropna convention); n is their count.  Per (series, model), x = [1, f_m]:
 *   means d- = sum(d) / n and f-_a = sum(f_a) / n first, then the centred cross-products
 *   A = sum (f - f-)(f - f-)', c = sum (f - f-)(d - d-), Syy = sum (d - d-)^2;
 *   Cholesky of A in ascending factor order, beta = A^-1 c, alpha = d- - beta'f-;
 *   e_t = (d_t - d-) - beta'(f_t - f-), s^2 = e'e / (n - k - 1);
 *   coef  [K+1]: slot 0 alpha, slot 1 + f factor column f; factors outside the model NaN;
 *   se    [K+1]: classical, sqrt diag of s^2 (X'X)^-1;
 *   se_hac[K+1]: sqrt diag of (X'X)^-1 S (X'X)^-1 with S = sum_t e_t^2 x_t x_t' + sum_{l = 1 ..
 *                min(nw_lags, n - 1)} (1 - l / (nw_lags + 1)) sum_t e_t e_{t-l} (x_t x_{t-l}' +
 *                x_{t-l} x_t'), no small-sample correction (evaluated in the centred basis
 *                [1, f - f-], which is the same quadratic form); a variance that rounds below 0 is
 *                written as se 0;
 *   stat  [4]:   R^2 = 1 - e'e / Syy (NaN when Syy == 0), s, d-, and the ddof-1 standard deviation
 *                of d, sqrt(Syy / (n - 1));
 *   nobs:        n.
 * Refusals per (series, model) write NaN, they are no error: n < k + 2 leaves everything NaN except
 * nobs; a diagonal entry A_aa == 0 or a Cholesky pivot (A_aa minus the squares of its row of the
 * factor so far) <= 1e-10 * A_aa -- collinear or constant factors -- leaves coef, se, se_hac, R^2
 * and s NaN, with d-, the standard deviation and nobs still written.
 * Every sum runs in one fixed order (thread i of 256 adds the used months i, i + 256, ... from +0.0,
 * the wave butterfly, then the four wave sums in order), so the bits of a (series, model) depend on
 * its own months alone: not on the other series or models of the launch, nor on the run.  The
 * launch needs no workspace and no host sync.  Outputs have the leading dimensions
 * [nsel][nrow][2][M].  Refused with FM_EINVAL before any launch (the message names the field): a
 * NULL required pointer, K outside 1..FM_MAX_FACTORS, M outside 1..FM_MAX_ALPHA_MODELS, nw_lags
 * outside 0..FM_ALPHA_MAX_LAGS, an empty mask, a mask bit >= K, a negative dimension.  T >
 * FM_ALPHA_MAX_MONTHS: FM_ETOOBIG before any launch (the used months' index and the residuals stay
 * in LDS).  T == 0, nsel == 0 or nrow == 0 is a valid empty call.  Zero-initialize the struct (it
 * grows at the end). */
#define FM_MAX_FACTORS 6
#define FM_MAX_ALPHA_MODELS 4
#define FM_ALPHA_MAX_LAGS 64
#define FM_ALPHA_MAX_MONTHS 4096
#define FM_ALPHA_NSTAT 4
typedef struct fm_alpha_args {
    const double* rec;           /* portfolio records; column 0 ew return, column 2 vw return */
    int64_t rec_month, rec_sort, rec_row, rec_col;   /* strides in doubles */
    const uint32_t* status;      /* 1 = sorted month */
    int64_t st_month, st_sort;   /* strides in words */
    int32_t nsel, nrow, T, K, M;
    int32_t nw_lags;             /* 0 .. FM_ALPHA_MAX_LAGS */
    const double* factors;       /* [T][K] */
    const double* rf;            /* [T] or NULL */
    uint32_t model_mask[FM_MAX_ALPHA_MODELS];   /* [M] bit f: factor column f is in the model */
    int32_t spread_row;          /* the row that is a difference of returns (no rf), or -1 */
    int32_t pad_alpha;
    double* coef;                /* [nsel][nrow][2][M][K+1] */
    double* se;                  /* [nsel][nrow][2][M][K+1] */
    double* se_hac;              /* [nsel][nrow][2][M][K+1] */
    double* stat;                /* [nsel][nrow][2][M][FM_ALPHA_NSTAT] */
    int32_t* nobs;               /* [nsel][nrow][2][M] */
} fm_alpha_args;

int fm_portfolio_alpha(const fm_alpha_args* args, void* stream);

/* fm_portfolio_hold: the forecast-sorted portfolios held for `hold` = k months as overlapping
 * cohorts (build-defined extension A19; no reference line; the calendar-time strategy of Jegadeesh
 * and Titman 1993 applied to the paper's Table 5 sorts).  In month t the strategy holds, per sort
 * and portfolio, the k cohorts formed in months t, t-1, .., t-k+1; its return is a monthly series
 * with fm_portfolio_sort's record layout, so fm_ts_summary and fm_portfolio_alpha read it as they
 * read the sort's own.  Inputs: the month-sorted panel's seg_off [nseg+1], month_index [nseg] and
 * nrows = seg_off[nseg]; link_prev [nrows], fm_month_links with step -1; port [nsel][nrows], the
 * sorts' portfolio bytes (a value >= nport: the row is in no portfolio); status [nsel][nseg] (1 = a
 * sorted month); ret [nrows]; weight [nrows] or NULL; sort_rec [nsel][nseg][nport+1][4] or NULL, the
 * sorts' own records, read for the predicted columns 1 and 3 only.
 * Ancestors.  For row i of segment t: anc_0 = i, and for a = 1..k
 *   anc_a = seg_off[t-a] + link_prev[anc_{a-1}];
 *   a hop is missing when t - a < 0, or when the link is negative or not below the length of
 *   segment t - a (a stale or foreign link array never causes a read outside [0, nrows)); all later
 *   hops are then missing too.
 * Membership.  Row i is a member of cohort (j, t, a, q) when anc_a exists and port[j][anc_a] == q <
 * nport.  status is not consulted: fm_portfolio_sort writes 255 in unsorted months.
 * Outputs per sort j and month t:
 *   members [j][t][a][q], a = 0..k: the number of members;
 *   stay    [j][t][a][q], a = 0..k: the members whose own port[j][i] == q (age 0: all of them);
 *   cohort_n[j][t][a][q][2], a = 0..k-1: slot 0 the members with a finite ret[i], slot 1 those that
 *            also have a finite weight[i] > 0 (weight NULL: 0);
 *   cohort  [j][t][a][q][2], a = 0..k-1: slot 0 sum(ret) / n over the first set, slot 1
 *            sum(w * ret) / sum(w) over the second, with the return and weight of the row in month
 *            t -- the month-t return of the stocks chosen a months earlier, equal-weighted among
 *            the cohort's survivors or weighted by their current weight; an empty set gives NaN;
 *   status_out[j][t]: 1 when the month is complete, else 0.  Complete: t - k + 1 >= 0 and for every
 *            a < k, status[j][t-a] == 1 and month_index[t-a] == month_index[t] - a;
 *   rec     [j][t][nport+1][4]: for a complete month and q < nport, column 0 = (c_0 + c_1 + .. +
 *            c_{k-1}) / k over the equal-weighted cohort values, added in age order from c_0, every
 *            operation rounded on its own; column 2 the same over the value-weighted cohort values;
 *            columns 1 and 3 the same average of sort_rec[j][t-a][q][1] and [3], the formation
 *            months' predicted returns (NaN when sort_rec is NULL).  A NaN term makes the entry NaN.
 *            Row nport = row nport-1 minus row 0, one rounding per column.  A month that is not
 *            complete is all NaN;
 *   turnover[j][t][q]: the share of names the strategy replaces in month t (the cohort formed in
 *            t - k leaves, the new one enters): (1.0 - (double)stay[..][k][q] / (double)
 *            members[..][0][q]) / k, every operation rounded on its own, when the month is
 *            complete, t - k >= 0, status[j][t-k] == 1, month_index[t-k] == month_index[t] - k and
 *            members[..][0][q] > 0; NaN otherwise.  k = 1: each portfolio's month-to-month name
 *            turnover.
 * Months may have any length (a wave takes 64 rows wherever they lie; none of the sorts' 16,384-row
 * limit applies).  Every output of (j, t) depends on the rows of months t-k..t alone.  Every sum of
 * (j, t, a, q) runs in one fixed order: wave w of four starts from +0.0 and adds the terms of the
 * month's rows 64 (w + 4 i) .. 64 (w + 4 i) + 63, i = 0, 1, .., in ascending row order, then the
 * four wave sums are added in wave order.  Two calls give the same bits, and so does a call with
 * other sorts beside sort j.  No floating-point atomics, no workspace, no host sync; the launch is
 * capture-safe.  Refused with FM_EINVAL before any launch (the message names the field): a NULL
 * required pointer, nport outside 2..FM_MAX_PORTS, hold outside 1..FM_MAX_HOLD, nsel outside
 * 0..FM_MAX_SORTS, a negative dimension, an output overlapping an input.  nseg == 0, nrows == 0 or
 * nsel == 0 is a valid empty call: nothing is launched and nothing is written.  Zero-initialize the
 * struct (it grows at the end). */
#define FM_MAX_HOLD 36
typedef struct fm_hold_args {
    const int64_t* seg_off;      /* [nseg+1] */
    const int32_t* month_index;  /* [nseg] calendar month number, strictly ascending */
    const int32_t* link_prev;    /* [nrows] fm_month_links with step -1 */
    const uint8_t* port;         /* [nsel][nrows] */
    const uint32_t* status;      /* [nsel][nseg] 1 = sorted month */
    const double* ret;           /* [nrows] */
    const double* weight;        /* [nrows] or NULL */
    const double* sort_rec;      /* [nsel][nseg][nport+1][4] or NULL */
    int64_t nrows;               /* seg_off[nseg] */
    int32_t nseg;
    int32_t nsel;                /* 0 .. FM_MAX_SORTS */
    int32_t nport;               /* 2 .. FM_MAX_PORTS */
    int32_t hold;                /* 1 .. FM_MAX_HOLD */
    int32_t* members;            /* [nsel][nseg][hold+1][nport] */
    int32_t* stay;               /* [nsel][nseg][hold+1][nport] */
    int32_t* cohort_n;           /* [nsel][nseg][hold][nport][2] */
    double* cohort;              /* [nsel][nseg][hold][nport][2] */
    uint32_t* status_out;        /* [nsel][nseg] */
    double* rec;                 /* [nsel][nseg][nport+1][4] */
    double* turnover;            /* [nsel][nseg][nport] */
} fm_hold_args;

int fm_portfolio_hold(const fm_hold_args* args, void* stream);

/* fm_group_adjust: every chosen column adjusted within a group of firms, per month (build-defined
 * extension A20; no reference line).  It is pandas' groupby([month, group])[x].transform: the
 * industry-relative characteristic x - mean, the industry mean, or the within-industry z-score
 * (Asness, Porter and Stevens 2000).  Rows sorted by (month, permno), months seg_off[nseg+1] of any
 * length, nrows = seg_off[nseg]; group[nrows] is an int32 code per row.  For every column c and
 * month t taken separately:
 *   eligible rows: the value is not NaN, 0 <= group < ngroups and, with level given, level >=
 *                  min_level.  Any other code (-1, ngroups, INT32_MIN, ...) means "no group".  +-inf
 *                  are ordinary values and propagate by the IEEE rules: a group with a +inf gives
 *                  -inf to its finite rows and NaN to the +inf row, a group with both infinities is
 *                  all NaN;
 *   statistics of group g: n = its eligible rows, S = their sum, m = S / (double)n (one division),
 *                  ss = the sum of (x - m)^2 over the same rows, sd = sqrt(ss / (double)(n - 1));
 *   output:        FM_GADJ_DEMEAN x - m, FM_GADJ_MEAN m, FM_GADJ_ZSCORE (x - m) / sd; every operation
 *                  is rounded on its own (none is contracted into an FMA);
 *   NaN output:    ineligible rows; the rows of a group with n < max(1, min_count); under
 *                  FM_GADJ_ZSCORE also the groups with n < 2 and those whose sd is not finite and
 *                  positive (a constant group, a group with an infinity);
 *   optional tables, each [ncols][nseg][ngroups]: gcount = n, always; gmean = m, NaN where n <
 *                  max(1, min_count); gsd = sd, NaN where n < 2, with FM_GADJ_ZSCORE only (FM_EINVAL
 *                  otherwise).  Every element of a given table is written, those of groups without
 *                  rows and of empty months too.
 * Order of summation.  S and ss are each added in one fixed order: wave w of four starts from +0.0
 * and adds the group's eligible values among the month's rows 64 (w + 4 i) .. 64 (w + 4 i) + 63,
 * i = 0, 1, .., in ascending row order, then the four wave sums are added in wave order.  The order
 * depends on the month's own rows and codes alone: not on the run, the other months or columns of
 * the call, how the launch batches the columns, nor on ngroups beyond the codes that occur.  So a
 * repeat call gives the same bits, and so does a call on a sub-range of the months or on a subset
 * of the columns.  No floating-point atomics, no workspace, no host sync; the launch is
 * capture-safe.
 * Limits: ngroups <= FM_MAX_GROUPS = 256 (SIC-2, the 48 / 49 Fama-French and the GICS industries);
 * none on the month length or on ncols (the launch batches the columns: fm_group_adjust_batch
 * (ngroups) columns share a workgroup's LDS bins: 8 while those fit, 4 at 256 groups).  Refused with
 * FM_EINVAL before any launch, outputs untouched (the message names the field): ngroups outside
 * 1..FM_MAX_GROUPS, an unknown mode, min_count < 0, a negative dimension, gsd without
 * FM_GADJ_ZSCORE, a stride below nrows, a NULL src, dst, seg_off or group, dst or a table
 * overlapping src, seg_off, group or level.  nseg == 0, nrows == 0 or ncols == 0 is a valid empty
 * call: nothing is launched and nothing is written.  A foreign seg_off reads nothing outside
 * [0, nrows).  Zero-initialize the struct (it grows at the end). */
#define FM_MAX_GROUPS 256
#define FM_GADJ_DEMEAN 0
#define FM_GADJ_MEAN 1
#define FM_GADJ_ZSCORE 2
typedef struct fm_gadj_args {
    const double* src;           /* [ncols][src_stride], rows sorted by (month, permno) */
    int64_t src_stride;
    double* dst;                 /* [ncols][dst_stride] */
    int64_t dst_stride;
    const int64_t* seg_off;      /* [nseg+1] */
    const int32_t* group;        /* [nrows] group code of each row */
    const uint8_t* level;        /* [nrows] universe level or NULL (every row) */
    int64_t nrows;               /* seg_off[nseg] */
    int32_t ncols;
    int32_t nseg;
    int32_t ngroups;             /* 1 .. FM_MAX_GROUPS */
    int32_t mode;                /* FM_GADJ_DEMEAN / MEAN / ZSCORE */
    int32_t min_count;           /* >= 0 */
    int32_t min_level;
    int32_t* gcount;             /* [ncols][nseg][ngroups] or NULL */
    double* gmean;               /* [ncols][nseg][ngroups] or NULL */
    double* gsd;                 /* [ncols][nseg][ngroups] or NULL; FM_GADJ_ZSCORE only */
} fm_gadj_args;

int fm_group_adjust(const fm_gadj_args* args, void* stream);
/* the columns that share a workgroup at `ngroups` groups (0 for ngroups outside 1..FM_MAX_GROUPS) */
int fm_group_adjust_batch(int32_t ngroups);

/* fm_portfolio_double_sort: per month, sort the stocks two ways, on signals a and b, into na x nb
 * cells, and average each cell's realised return and signals (build-defined extension A21; no
 * reference line): the 5 x 5 control of one sort for a second variable, and the 2 x 3 sorts that
 * size, value and characteristic factors are built from.  Rows sorted by (month, permno), months
 * seg_off[nseg+1] of at most 16,384 rows (longer: FM_ETOOBIG before any launch, outputs
 * untouched), nrows = seg_off[nseg].  nsel sorts share one launch (grid (month, sort)): sort s
 * reads a + s * a_sort_stride and b + s * b_sort_stride (elements; a stride of 0 shares that
 * signal across the sorts), and writes row vectors at [s][row] and month records at [s][t].
 * Per month t of sort s:
 *   eligible rows:   isfinite(a) and isfinite(b) and level >= min_level (level NULL: every row);
 *   breakpoint rows: the eligible rows; with nyse_breakpoints those with nyse != 0;
 *   fewer than min_count breakpoint rows: status = 0, bpa and bpb NaN, every cell byte 255, every
 *     record NaN, every count 0; otherwise status = 1 and
 *   bpa[i]     = numpy 'linear' quantile qa[i] of the breakpoint rows' a (exact order statistics;
 *                the sign of an exactly-zero breakpoint is not specified);
 *   pa         = #{ i : a > bpa[i] } (right-closed bins);
 *   bpb[i'][j] = conditional == 0: the quantile qb[j] of all breakpoint rows' b, the same row
 *                written for every i' < na; conditional != 0: the quantile over the breakpoint
 *                rows with pa == i'.  An a-bin with fewer than min_count_bin such rows has NaN
 *                bpb, its rows get cell byte 255, its cells count 0 and NaN records;
 *   pb         = #{ j : b > bpb[pa][j] };
 *   cell[row]  = pa * nb + pb for the eligible rows of a sorted a-bin, else 255;
 *   cnt[pa][pb] = the cell's rows with a finite return.  Over those rows the cell has six sums:
 *                ret, a, b, and w ret, w a, w b over the rows that also have a finite weight > 0
 *                (weight NULL: none); the means are sum / count and sum / sum(w), an empty set
 *                gives NaN.
 * Records, in two views that each have fm_portfolio_sort's record layout:
 *   rec_b[s][i][t][j] (i < na, j < nb) = { ew ret, ew mean b, vw ret, vw mean b } of cell (i, j);
 *   rec_b[s][i][t][nb] = row nb-1 minus row 0 (NaN if either end is);
 *   rec_b[s][na][t][j][c] = (x_0 + x_1 + ... + x_{na-1}) / na over the na slabs' entries
 *                (j, c), added in that order (NaN if any term is): the a-neutral b portfolios;
 *                the slab's row nb is its own row nb-1 minus its row 0;
 *   rec_a[s][j][t][i] = { ew ret, ew mean a, vw ret, vw mean a } of cell (i, j), with the roles
 *                swapped throughout: row na = row na-1 minus row 0, slab nb the b-neutral a
 *                portfolios (x_0 + ... + x_{nb-1}) / nb and their spread.
 * Every output of a month depends on that month's rows alone and every sum runs in one fixed
 * order (the cell's rows in row order, lane l of a wave taking the list's entries l, l + 64, ...,
 * then the wave butterfly): a repeat call, a sub-range of the months, a sort alone or in a batch
 * and any workgroup form give the same bits.  No floating-point atomics, no workspace, no host
 * sync: three launches on the stream (a's breakpoints, b's breakpoints with the a-bins of a
 * conditional sort side by side, then cells and sums), the breakpoints waiting in the month's own
 * records in between.
 * Refused with FM_EINVAL before any launch: na or nb outside 2..FM_MAX_DSORT, qa / qb not strictly
 * ascending in (0, 1), min_count or min_count_bin < 1, min_level outside 0..255, nyse_breakpoints
 * without nyse, nsel outside 0..65,535, a negative size or stride, a NULL required pointer.
 * nsel == 0 or nseg == 0 is a valid empty call.  Zero-initialize the struct (it grows at the
 * end). */
#define FM_MAX_DSORT 10
typedef struct fm_dsort_args {
    const double* a;             /* [nsel or 1][nrows] first signal */
    const double* b;             /* [nsel or 1][nrows] second signal */
    int64_t a_sort_stride;       /* elements between the sorts' a vectors; 0: shared */
    int64_t b_sort_stride;       /* elements between the sorts' b vectors; 0: shared */
    const double* ret;           /* [nrows] */
    const double* weight;        /* [nrows] or NULL */
    const uint8_t* level;        /* [nrows] universe level or NULL */
    const uint8_t* nyse;         /* [nrows] nonzero = NYSE row, or NULL */
    const int64_t* seg_off;      /* [nseg+1] */
    int64_t nrows;               /* seg_off[nseg] */
    int32_t nseg;
    int32_t nsel;                /* 0 .. 65,535 (the grid's second dimension) */
    int32_t max_seg_len;         /* >= every month's rows, <= 16,384 */
    int32_t na;                  /* 2 .. FM_MAX_DSORT */
    int32_t nb;                  /* 2 .. FM_MAX_DSORT */
    int32_t conditional;         /* 0: independent; nonzero: b within the a-bins */
    int32_t min_level;
    int32_t nyse_breakpoints;    /* nonzero: breakpoints from the NYSE rows only */
    int32_t min_count;           /* >= 1 */
    int32_t min_count_bin;       /* >= 1; read in conditional mode only */
    double qa[FM_MAX_DSORT - 1]; /* [na-1] levels, strictly ascending in (0, 1) */
    double qb[FM_MAX_DSORT - 1]; /* [nb-1] */
    double* rec_b;               /* [nsel][na+1][nseg][nb+1][4] */
    double* rec_a;               /* [nsel][nb+1][nseg][na+1][4] */
    int32_t* cnt;                /* [nsel][nseg][na][nb] */
    uint8_t* cell;               /* [nsel][nrows] or NULL */
    double* bpa;                 /* [nsel][nseg][na-1] or NULL */
    double* bpb;                 /* [nsel][nseg][na][nb-1] or NULL */
    uint32_t* status;            /* [nsel][nseg] */
} fm_dsort_args;

int fm_portfolio_double_sort(const fm_dsort_args* args, void* stream);

/* fm_wls: the weighted (value-weighted) monthly cross-sections: for every month and every problem
 * (model x universe level) the weighted least-squares fit of y on [1, x], in one launch, grid
 * (month, problem) (build-defined extension A22; the reference has no WLS, so no reference line:
 * the definition is statsmodels' WLS(y, add_constant(x), weights=w) on the rows used).  It writes
 * what fm_solve writes for OLS -- rec, status and the optional moments in the same layouts -- so the
 * time-series and forecast stages run on it unchanged.  FP64 columns, at most FM_WLS_MAX_COLS of
 * them (z = [1, x.., y] is at most 16 wide); rows sorted by (month, permno), months
 * seg_off[nseg+1] of any length.  Problem p reads the z list prob_z[p][0..prob_nz[p]) = 0 (the
 * intercept), 1 + the panel columns of x_1 .. x_K, 1 + the panel column of y (fm_solve_args'
 * tables; K = prob_nz[p] - 2 <= pmax - 1): the model's columns are exactly that list, so there is no
 * mask table.  Per (month t, problem p):
 *   a row is used when every column of the list (y included) is non-NaN, level >= prob_level[p]
 *     (level NULL: every row) and its weight is finite and > 0: fm_gram's rule plus the weight's.
 *     Rows of NaN, +-inf, zero or negative weight are dropped and do not count;
 *   values are clipped first, as fm_gram clips: max with lo, then min with hi, both [ncols][nseg];
 *     a NaN bound is ignored; lo == hi == NULL: no clipping;
 *   N = the number of rows used.  N < K + 1: status FM_ST_SKIPPED alone, rec NaN but rec[pmax+1] = N;
 *   a used row with +-inf after clipping in x / in y: status FM_ST_INF_IN_X / FM_ST_INF_IN_Y (or
 *     both) alone -- not FITTED -- and rec as for a skipped month;
 *   with W = sum(w), the weighted means m = sum(w z) / W and w~ = w N / W (the weights scaled to
 *     sum to N), the centred moments S = sum(w~ (z - m)(z - m)') over (x_1 .. x_K, y);
 *   a predictor whose S_kk is not above 1e-20 (S_kk + N m_k^2) -- rounding beside its raw second
 *     moment: a constant, or all-zero, column -- or a Cholesky pivot of Sxx that is not above 1e-6
 *     (fm_solve's REFIT_REL) of its diagonal entry S_kk: status FM_ST_RANK_DEF alone, rec as for a
 *     skipped month.  There is no CONST_COL / CONST_SUSPECT logic and no pinv re-solve;
 *   otherwise status FM_ST_FITTED and b = Sxx^-1 Sxy (the minimiser of sum(w (y - a - b'x)^2)),
 *     rec[0] = a = m_y - b'm_x, rec[1..K] = b, rec[K+1..pmax) NaN,
 *     rec[pmax] = R2 = 1 - (Syy - b'Sxy) / Syy = 1 - SSR_w / sum(w (y - m_y)^2) (statsmodels'
 *     WLS.rsquared), rec[pmax+1] = N.  N == K + 1 is fitted.  A constant y is no special case, as in
 *     fm_solve: Syy = 0 gives slopes of 0 and R2 = 0 / 0 = NaN under FM_ST_FITTED (statsmodels
 *     divides by the same zero); the time-series summaries skip a NaN R2 as they skip any NaN;
 *   moments (optional; written where N >= K + 1 and no value is +-inf): [0] = N, [1 + i] = m_i in
 *     raw units, [1 + K1 + i K1 + j] = S_ij with K1 = K + 1 and i, j over (x_1 .. x_K, y): fm_solve's
 *     index layout and its centred block, so fm_predictive / fm_ts_fused give the weighted
 *     predictive slope and R2 from it (fm_solve's means are about its pivot; these are raw).
 * Numerics: two passes over the month (L2-resident), the first about `shift` ([ncols][nseg], NULL:
 * 0) for the means, the second about the means for S; the first moments the second pass still
 * finds are subtracted.  Every sum runs in one fixed order that depends on the month's USED rows
 * alone: they are numbered in row order, cut into tiles of 64, tile c goes to wave c % 4 of the
 * workgroup, which adds its tiles in order, four rows per v_mfma_f64_16x16x4_f64 (A = w z, B = z);
 * the four waves' sums are then added in wave order.  No floating-point atomics.  So a repeat, a
 * sub-range of the months, a subset of the problems, the panel with dropped rows taken out, and
 * weights multiplied by a power of two (short of overflow and underflow) all give the same bits.
 * Refused with FM_EINVAL before the launch: ncols outside 1..FM_WLS_MAX_COLS, pmax outside
 * 1..FM_WLS_MAX_COLS, more than 65,535 problems, a negative size, col_stride < nrows, lo without hi,
 * a mom_stride that does not hold 1 + (pmax+1) + (pmax+1)^2, a NULL required pointer.  Column
 * indices outside the panel are clamped into it.  nseg == 0 or nprob == 0 is a valid empty call.
 * Zero-initialize the struct (it grows at the end). */
#define FM_WLS_MAX_COLS 15
typedef struct fm_wls_args {
    const double* cols;          /* [ncols][col_stride] */
    int64_t col_stride;
    int64_t nrows;               /* seg_off[nseg] */
    int32_t ncols;               /* 1 .. FM_WLS_MAX_COLS */
    int32_t nseg;
    const int64_t* seg_off;      /* [nseg+1] */
    const double* lo;            /* [ncols][nseg] clip bounds, or both NULL */
    const double* hi;
    const double* shift;         /* [ncols][nseg] pivot of the first pass, or NULL */
    const uint8_t* level;        /* [rows] universe level, or NULL */
    const double* weight;        /* [rows] */
    int32_t nprob;
    int32_t pmax;                /* >= max K + 1 over the problems, <= FM_WLS_MAX_COLS */
    const int32_t* prob_level;   /* [nprob] */
    const int32_t* prob_z;       /* [nprob][32] z indices: 0, 1 + x columns..., 1 + y column */
    const int32_t* prob_nz;      /* [nprob] K + 2 */
    double* rec;                 /* [nseg][nprob][pmax+2] */
    uint32_t* status;            /* [nseg][nprob] FM_ST_* bits */
    double* moments;             /* [nseg][nprob][mom_stride] or NULL */
    int32_t mom_stride;
    int32_t pad_wls;
} fm_wls_args;

int fm_wls(const fm_wls_args* args, void* stream);

/* fm_pool: the pooled panel OLS of y on [1, x] over all months of a range at once, for every problem
 * (model x universe level), with five covariance estimates of its coefficients (build-defined
 * extension A23; the reference has no pooled fit, so no reference line: the definition is the
 * textbook sandwich of Petersen 2009 / Cameron, Gelbach and Miller 2011).  FP64 columns (cols ==
 * NULL, a planes-only panel, is refused); rows sorted by (month, firm), months seg_off[nseg+1] of
 * any length; only the months [seg_lo, seg_hi) take part.  The problem tables are fm_wls's (prob_z[p]
 * = 0, 1 + the panel columns of x_1 .. x_K, 1 + the panel column of y; K = prob_nz[p] - 2 <=
 * FM_POOL_MAX_K, so z = [1, x, y] is one 16-wide tile): the limit is on the model's width, the panel
 * may have any number of columns.  firm[rows] is a dense firm code in 0 .. nfirms-1, strictly
 * ascending inside each month; bad[0] (zeroed by the caller) receives the number of rows of the range
 * whose code is outside 0 .. nfirms-1 or not above their predecessor's in the month.  The results of
 * a call with bad != 0 are unspecified, but every access stays in bounds.  Per problem:
 *   a row is used when every column of the list (y included) is non-NaN and level >= prob_level[p]
 *     (level NULL: every row); values are clipped first, as fm_gram / fm_wls clip (max with lo, then
 *     min with hi, both [ncols][nseg]; a NaN bound is ignored; both NULL: no clipping);
 *   N = rows used, G_t = months with a used row, G_f = firms with a used row, p0 = K + 1;
 *   month_fe == 0: the pooled means m and the moments S centred about them give b = Sxx^-1 Sxy,
 *     a = m_y - b'm_x, R2 = 1 - SSR / Syy, classical dof = N - K - 1; the covariances are formed for
 *     the regressors x~ = [1, x - m_x] and mapped back to the raw intercept (exactly: x~ is a
 *     reparametrisation);
 *   month_fe != 0: x and y are demeaned within each month over that month's used rows; no intercept
 *     (coef[0] and every se[.][0] are NaN, the covariances' row and column 0 too),
 *     b = (sum_t S_t,xx)^-1 sum_t S_t,xy, R2 is the within R2, classical dof = N - K - G_t;
 *   residuals e come from the centred data, scores u_i = x~_i e_i; with A the inverse of x~'x~:
 *     FM_POOL_SE_CLASSICAL s2 A with s2 = SSR / dof;  FM_POOL_SE_WHITE A (sum u u') A;
 *     FM_POOL_SE_MONTH A sum_t (sum_{i in t} u)(..)' A;  FM_POOL_SE_FIRM A sum_f (sum_t u_ft)(..)' A;
 *     FM_POOL_SE_TWOWAY V_firm + V_month - V_white;
 *   small_sample != 0: White is multiplied by N / (N - p0), a clustered kind with G clusters by
 *     G / (G - 1) (N - 1) / (N - p0), two-way combines the corrected terms.  A clustered kind with
 *     G < 2 is NaN, and so is two-way.  A diagonal entry of V_twoway that is not above 0 gives a NaN
 *     se and sets FM_ST_NEG_VAR beside FM_ST_FITTED;
 *   status: N < p0 + 1 or dof < 1: FM_ST_SKIPPED alone; else a used row with +-inf after clipping:
 *     FM_ST_INF_IN_X / FM_ST_INF_IN_Y alone; else a predictor whose centred second moment is not
 *     above 1e-20 of its raw one, or a Cholesky pivot not above 1e-6 (fm_solve's REFIT_REL) of its
 *     diagonal entry: FM_ST_RANK_DEF alone (no pinv re-solve, as in fm_wls).  In these cases coef, se
 *     and cov are NaN and stat[0] = N.
 * Outputs: coef[nprob][pmax] (a, b_1 .. b_K, NaN pad), se[nprob][5][pmax], cov[nprob][5][pmax][pmax]
 * (optional), stat[nprob][8] = N, G_t, G_f, R2, SSR, s2, classical dof, 0; status[nprob];
 * resid[nprob][nrows] (optional): e on the used rows of the range's months and NaN on their other
 * rows (rows of months outside the range are not written).
 * Eight launches, all on `stream`: (1) the code check; (2) per (month, problem) the sums about
 * `shift` ([ncols][nseg], NULL: 0); (3) per problem the means, N, G_t and the skipped / inf verdict;
 * (4) the pass of (2) about the means for the centred moments; (5) per problem the fit; (6) per
 * (month, problem) the residuals, sum u and sum u u'; (7) per (block of FM_POOL_FIRM_BLOCK firm
 * codes, problem) the firms' score sums, kept in LDS while the workgroup walks the months in order
 * (its rows of a month are one run, found by binary search in `firm`), then sum_f s_f s_f' over
 * its firms in code order; (8) per problem the sandwiches.  The month passes put 64 rows into an
 * LDS tile and add them with sixteen v_mfma_f64_16x16x4_f64 (A = B = the tile's rows, unused rows
 * as zeros); tile c of a month is wave c % 4's, the waves are added in
 * wave order, months and firm blocks in index order.  No floating-point atomics.  So a repeat, a
 * problem alone or in a batch, firm codes that are the same, and [seg_lo, seg_hi) of a panel against
 * a panel of those months alone give the same bits.
 * Refused with FM_EINVAL before any launch (the message names the field): a negative size, ncols
 * < 1, more than 65,535 problems, pmax outside 2 .. FM_POOL_MAX_K + 1, col_stride < nrows, lo
 * without hi, a stage outside 0 .. 8, seg_lo > seg_hi or outside [0, nseg], nfirms < 0, a NULL
 * required pointer, ws_bytes below fm_pool_ws_bytes(nseg, nprob, pmax, nfirms) (-1 for sizes below
 * zero).  Column indices outside the panel are clamped into it, a prob_nz outside 2 .. pmax + 1
 * into that range.  nseg == 0, nprob == 0 or seg_lo == seg_hi is a valid empty call.
 * Zero-initialize the struct (it grows at the end). */
#define FM_POOL_MAX_K 14
#define FM_POOL_FIRM_BLOCK 256
#define FM_POOL_SE_CLASSICAL 0
#define FM_POOL_SE_WHITE 1
#define FM_POOL_SE_MONTH 2
#define FM_POOL_SE_FIRM 3
#define FM_POOL_SE_TWOWAY 4
typedef struct fm_pool_args {
    const double* cols;          /* [ncols][col_stride] */
    int64_t col_stride;
    int64_t nrows;               /* seg_off[nseg] */
    int32_t ncols;               /* >= 1, any width */
    int32_t nseg;
    const int64_t* seg_off;      /* [nseg+1] */
    const double* lo;            /* [ncols][nseg] clip bounds, or both NULL */
    const double* hi;
    const double* shift;         /* [ncols][nseg] pivot of the first pass, or NULL */
    const uint8_t* level;        /* [rows] universe level, or NULL */
    const int32_t* firm;         /* [rows] dense firm code, strictly ascending inside a month */
    int32_t nfirms;
    int32_t seg_lo, seg_hi;      /* the months that take part */
    int32_t month_fe;
    int32_t small_sample;
    int32_t nprob;
    int32_t pmax;                /* >= max K + 1 over the problems, 2 .. FM_POOL_MAX_K + 1 */
    int32_t stage;               /* 0: every launch; 1..8 (timing tools): that launch alone, on the
                                    workspace and outputs a full call with the same arguments left */
    const int32_t* prob_level;   /* [nprob] */
    const int32_t* prob_z;       /* [nprob][32] z indices: 0, 1 + x columns..., 1 + y column */
    const int32_t* prob_nz;      /* [nprob] K + 2 */
    double* coef;                /* [nprob][pmax] */
    double* se;                  /* [nprob][5][pmax] */
    double* cov;                 /* [nprob][5][pmax][pmax] or NULL */
    double* stat;                /* [nprob][8] */
    uint32_t* status;            /* [nprob] FM_ST_* bits */
    double* resid;               /* [nprob][nrows] or NULL */
    int32_t* bad;                /* [1], zeroed by the caller */
    void* ws;                    /* fm_pool_ws_bytes(nseg, nprob, pmax, nfirms) bytes */
    int64_t ws_bytes;
} fm_pool_args;

int64_t fm_pool_ws_bytes(int32_t nseg, int32_t nprob, int32_t pmax, int32_t nfirms);
int fm_pool(const fm_pool_args* args, void* stream);

/* Table 1.  A row counts for column c when level == NULL or level[r] >= min_level, its value
 * is not NaN and, with finite_only != 0, not +-inf.  fm_segment_moments: per (column, segment)
 * count[c * nseg + s], mean (NaN for count 0) and ddof=1 standard deviation (NaN for count
 * < 2), two passes; with finite_only == 0 an inf among the rows gives IEEE results (mean
 * +-inf or NaN, sd NaN).  fm_distinct_count: out[c] = the number of distinct ids among column
 * c's rows; every id lies in [id_lo, id_lo + id_range), 1 <= id_range <= 2^34; bitmap is a
 * workspace of ncols * ceil(id_range / 32) words.  Sizes below zero, ncols < 1 and an id
 * range out of bounds return FM_EINVAL before any HIP call. */
int fm_segment_moments(const double* cols, int64_t col_stride, int32_t ncols,
                       const int64_t* seg_off, int32_t nseg, const uint8_t* level,
                       int32_t min_level, int32_t finite_only, int32_t* count, double* mean,
                       double* sd, void* stream);

int fm_distinct_count(const int64_t* ids, int64_t nrows, const double* cols, int64_t col_stride,
                      int32_t ncols, const uint8_t* level, int32_t min_level, int32_t finite_only,
                      int64_t id_lo, int64_t id_range, uint32_t* bitmap, int32_t* out,
                      void* stream);

/* Firm-axis characteristic construction.  Rows are FIRM-major:
 * grouped by firm id (each firm's rows contiguous, in the reference frame's order inside the
 * group — get_factors sorts by (permno, mthcaldt), src/calc_Lewellen_2014.py:533).  Row i's
 * lag-k value exists iff ids[i-k] == ids[i].  field[f] / out[c] are device columns of n
 * doubles indexed by FM_FIELD_* / FM_CHAR_*; out[c] == NULL skips characteristic c, and a
 * requested characteristic needs its fields non-NULL (else FM_EINVAL).  Rolling windows turn
 * +-inf into NaN first (pandas _prep_values). */
#define FM_NFIELDS 12
#define FM_FIELD_ME 0
#define FM_FIELD_BE 1
#define FM_FIELD_RETX 2
#define FM_FIELD_ACCRUALS 3
#define FM_FIELD_DEPRECIATION 4
#define FM_FIELD_EARNINGS 5
#define FM_FIELD_ASSETS 6
#define FM_FIELD_DVC 7
#define FM_FIELD_PRC 8
#define FM_FIELD_SHROUT 9
#define FM_FIELD_TOTAL_DEBT 10
#define FM_FIELD_SALES 11

#define FM_NCHARS 12
#define FM_CHAR_LOG_SIZE 0          /* log(me[t-1])                       :137-147 */
#define FM_CHAR_LOG_BM 1            /* log(be[t-1]) - log(me[t-1])        :150-163 */
#define FM_CHAR_RETURN_12_2 2       /* prod(1 + retx[t-12..t-2]) - 1      :166-192 */
#define FM_CHAR_ACCRUALS_FINAL 3    /* accruals - depreciation            :195-204 */
#define FM_CHAR_ROA 4               /* earnings / assets                  :241-249 */
#define FM_CHAR_LOG_ASSETS_GROWTH 5 /* log(assets / assets[t-12])         :252-262 */
#define FM_CHAR_DY 6                /* sum(dvc[t-11..t], minp 1) / prc[t-1] :265-287 */
#define FM_CHAR_LOG_RETURN_13_36 7  /* sum(log(1 + retx[t-36..t-13]))     :290-313 */
#define FM_CHAR_LOG_ISSUES_12 8     /* log(shrout[t-1]) - log(shrout[t-12]) :224-238 */
#define FM_CHAR_LOG_ISSUES_36 9     /* log(shrout[t-1]) - log(shrout[t-36]) :207-221 */
#define FM_CHAR_DEBT_PRICE 10       /* total_debt / me[t-1]               :316-327 */
#define FM_CHAR_SALES_PRICE 11      /* sales / me[t-1]                    :330-341 */

typedef struct fm_chars_args {
    const int64_t* ids;                 /* [n] firm id per row (grouped)                 */
    int64_t n;
    const double* field[FM_NFIELDS];    /* FM_FIELD_* columns, NULL if absent           */
    double* out[FM_NCHARS];             /* FM_CHAR_* outputs, NULL = not computed       */
} fm_chars_args;

int fm_firm_chars(const fm_chars_args* args, void* stream);

/* Per-row rolling std (ddof=1) over the last `window` rows of each firm group (rows grouped
 * as for fm_firm_chars), NaN below `min_periods` observations, exactly 0 when all
 * observations are equal, times `scale`.  1 <= window <= 4096, 1 <= min_periods <= window
 * (a std needs at least 2 observations, so min_periods 1 behaves as 2).  ids, x and out must be
 * 16-byte aligned (row pairs move as 16-byte accesses); FM_EINVAL otherwise. */
int fm_rolling_std(const int64_t* ids, const double* x, int64_t n, int32_t window,
                   int32_t min_periods, double scale, double* out, void* stream);

/* calculate_rolling_beta's 156-week rolling market beta (src/calc_Lewellen_2014.py:344-434,
 * polars group_by_dynamic(every="1w", period="156w", by="permno"), closed left, label left,
 * windows from the Monday of each firm's first date while the start <= its last date,
 * empty windows not emitted).  Rows: the inner join of daily stock and market returns,
 * firm-major (seg_off[nseg+1] firm row ranges), days ascending within a firm (`day` =
 * days since 1970-01-01); ri / rm the raw daily returns (log(1 + r) is taken here).  Query
 * q = (firm segment q_seg, calendar month [q_day0, q_day1]): the beta of the LAST emitted
 * window starting in that month, NaN if none (the reference's drop_duplicates(keep="last")
 * + left merge, :426-431).  ws: [5][n] workspace.  Parity unpinned (no polars here). */
int fm_rolling_beta(const int32_t* day, const double* ri, const double* rm, int64_t n,
                    const int64_t* seg_off, int32_t nseg, int32_t period_days,
                    const int32_t* q_seg, const int32_t* q_day0, const int32_t* q_day1,
                    int32_t nq, double* ws, double* beta, void* stream);

int fm_gen_panel(uint64_t seed, int64_t month0, int32_t nmonths, int32_t nfirms,
                 double nan_rate, double nyse_rate, double* cols, int64_t col_stride,
                 double* me, uint8_t* nyse, void* stream);

/* fm_gen_panel writing the split layout directly: the values' high / low 32-bit words into
 * hi / lo ([ncols][plane_stride]), the FP64 columns into cols too when cols != NULL (else
 * not at all).  The same values as fm_gen_panel bit for bit; no separate layout pass. */
int fm_gen_panel_planes(uint64_t seed, int64_t month0, int32_t nmonths, int32_t nfirms,
                        double nan_rate, double nyse_rate, double* cols, int64_t col_stride,
                        uint32_t* hi, uint32_t* lo, int64_t plane_stride, double* me, uint8_t* nyse,
                        void* stream);

/* The inverse of fm_split_planes: FP64 columns from the two planes (for consumers of a split
 * panel that read FP64 columns: clip, forecasts, Table 1, moments). */
int fm_merge_planes(const uint32_t* hi, const uint32_t* lo, int64_t plane_stride, int32_t ncols, int64_t nrows,
                    double* cols, int64_t col_stride, void* stream);

/* The FP64 columns as two 32-bit planes: hi[c][r] / lo[c][r] = the high / low words of
 * cols[c][r] (plane_stride >= nrows).  The split panel's hi plane feeds fm_select_args.hi_plane
 * and, with the lo plane, fm_gram_args.hi_plane / lo_plane. */
int fm_split_planes(const double* cols, int64_t col_stride, int32_t ncols, int64_t nrows, uint32_t* hi,
                    uint32_t* lo, int64_t plane_stride, void* stream);
int fm_stream_probe(const double* src, int64_t n, double* out, void* stream);
/* Copy n doubles src -> dst as the probe's 16-byte stream (measures the HBM copy rate;
 * bench.py's measured_copy_peak).  src / dst 16-byte aligned, not overlapping. */
int fm_stream_copy_probe(const double* src, double* dst, int64_t n, void* stream);

/* fm_ffill_expand: records sorted by (group, month code) with CSR rec_off[ngroups+1];
 * out_off[ngroups+1] is the prefix of each group's output month count (planned by the
 * caller: from its first record month to its last output month).  Output row i of group g
 * is month rec_month[rec_off[g]] + (i - out_off[g]); it takes the group's last record with
 * rec_month <= that month: out_src[i] = that record, out_month[i] = the month, and the
 * ncols FP64 columns vals[c * v_stride + record] are gathered to out_vals[c * o_stride + i]. */
int fm_ffill_expand(const int64_t* rec_off, const int32_t* rec_month, const int64_t* out_off,
                    int32_t ngroups, int64_t nout, const double* vals, int64_t v_stride,
                    int32_t ncols, double* out_vals, int64_t o_stride, int32_t* out_month,
                    int64_t* out_src, void* stream);

/* fm_sorted_join: for each left key (lk1[i], lk2[i]) the range [lo[i], hi[i]) of equal keys
 * in the right keys (rk1, rk2), sorted lexicographically (stably: equal keys in the right
 * frame's order).  lk2 / rk2 may both be NULL (one-part key). */
int fm_sorted_join(const int64_t* lk1, const int64_t* lk2, int64_t nl, const int64_t* rk1,
                   const int64_t* rk2, int64_t nr, int64_t* lo, int64_t* hi, void* stream);

#ifdef __cplusplus
}
#endif
#endif
