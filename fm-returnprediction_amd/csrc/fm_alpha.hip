// fm_portfolio_alpha: factor-model alphas of the forecast-sorted portfolios (build-defined
// extension A18; the definition is in fm_hip.h).
//
// One workgroup per (series, model), a series being (sort, portfolio row, weighting).  The work of
// a workgroup is a time-series OLS of a few hundred months on at most six factors:
//   1. compact: the used months (status 1, finite dependent value, finite factors of the model) in
//      month order -> their month index and dependent value in LDS (block scan, as fm_ts_summary);
//   2. the means of d and of the model's factors;
//   3. the centred cross-products A, c, Syy (28 sums in one sweep);
//   4. every thread solves the k x k system in registers (Cholesky, its inverse), then the
//      residuals replace the dependent values in LDS and e'e is summed;
//   5. the HAC meat in the centred basis x~ = [1, f - f-]: with u_t = e_t x~_t and
//      z_t = sum_l w_l u_{t-l}, S = sum_t u_t u_t' + u_t z_t' + z_t u_t' -- the Bartlett sum of the
//      definition with the lag loop inside the month loop, so the 28 accumulators are touched once
//      per month and not once per (month, lag);
//   6. thread 0 writes the (series, model)'s outputs.
// The factor table is read from global memory in every sweep (a 4096 x 6 table beside the index
// and the residuals does not fit the LDS a workgroup may take; the table is a few tens of KB that
// all workgroups share, so these are cache hits).  Out-of-model factors stay in their slots as
// zeros under a wave-uniform mask test, so every small array below is indexed by unrolled loop
// counters and lives in registers.
#include <math.h>

#include "fm_common.h"

namespace fm {
namespace {

constexpr int AT = 256;
constexpr int ANW = AT / WAVE;
constexpr int AK = FM_MAX_FACTORS;
constexpr int AX = AK + 1;                 // [f_0 .. f_5, d] for the moments, [1, f~_0 .. f~_5] for the HAC sums
constexpr int ATRI = AX * (AX + 1) / 2;    // packed lower triangle
constexpr double PIVOT_TOL = 1e-10;

__host__ __device__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // i >= j

struct AlphaShared {
    int32_t idx[FM_ALPHA_MAX_MONTHS];   // the used months, ascending
    double val[FM_ALPHA_MAX_MONTHS];    // their dependent values, later the residuals
    double red[ANW * ATRI];
    double tot[ATRI];
    int scan[ANW];
};

// v[0..NV) summed over the block in a fixed order (the wave butterfly, then the waves in order);
// every thread gets the totals back in v
template <int NV>
__device__ __forceinline__ void block_sum_vec(double (&v)[NV], AlphaShared& sh) {
    const int w = threadIdx.x / WAVE;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane_id() == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) sh.red[w * NV + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = sh.red[threadIdx.x];
#pragma unroll
        for (int i = 1; i < ANW; ++i) s += sh.red[i * NV + threadIdx.x];
        sh.tot[threadIdx.x] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = sh.tot[i];
}

// h' S h for the packed symmetric S
__device__ __forceinline__ double quad_form(const double (&S)[ATRI], const double (&h)[AX]) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < AX; ++i) {
        double r = 0.0;
#pragma unroll
        for (int j = 0; j < AX; ++j) r += S[i >= j ? tri(i, j) : tri(j, i)] * h[j];
        q += h[i] * r;
    }
    return q;
}

__global__ __launch_bounds__(AT) void portfolio_alpha_kernel(fm_alpha_args a) {
    __shared__ AlphaShared sh;
    const int tid = threadIdx.x;
    const int m = blockIdx.x % a.M;
    const int ser = blockIdx.x / a.M;
    const int w = ser & 1;
    const int p = (ser >> 1) % a.nrow;
    const int j = (ser >> 1) / a.nrow;
    const uint32_t mask = a.model_mask[m];
    const int K = a.K, T = a.T;
    const int k = __builtin_popcount(mask);
    bool in[AK];
#pragma unroll
    for (int f = 0; f < AK; ++f) in[f] = (mask >> f) & 1u;

    const double* rec = a.rec + (int64_t)j * a.rec_sort + (int64_t)p * a.rec_row + (int64_t)(2 * w) * a.rec_col;
    const uint32_t* st = a.status + (int64_t)j * a.st_sort;
    const bool use_rf = a.rf != nullptr && p != a.spread_row;

    // 1. the used months, in month order
    int n = 0;
    for (int t0 = 0; t0 < T; t0 += AT) {
        const int t = t0 + tid;
        double d = NAN;
        bool ok = false;
        if (t < T && st[(int64_t)t * a.st_month] == 1u) {
            d = rec[(int64_t)t * a.rec_month];
            if (use_rf) d = d - a.rf[t];
            ok = isfinite(d);
#pragma unroll
            for (int f = 0; f < AK; ++f)
                if (in[f]) ok = ok && isfinite(a.factors[(int64_t)t * K + f]);
        }
        int tot = 0;
        const int off = block_excl_scan<ANW>(ok ? 1 : 0, sh.scan, &tot);
        if (ok) {
            sh.idx[n + off] = t;
            sh.val[n + off] = d;
        }
        n += tot;
    }
    __syncthreads();

    const int64_t o = (int64_t)ser * a.M + m;
    double* coef = a.coef + o * (K + 1);
    double* se = a.se + o * (K + 1);
    double* hac = a.se_hac + o * (K + 1);
    double* stat = a.stat + o * FM_ALPHA_NSTAT;
    if (n < k + 2) {
        if (tid == 0) a.nobs[o] = n;
        if (tid <= K) coef[tid] = se[tid] = hac[tid] = NAN;
        if (tid < FM_ALPHA_NSTAT) stat[tid] = NAN;
        return;
    }
    const double dn = (double)n;

    // 2. means
    double mean[AX];
    {
        double s[AX];
#pragma unroll
        for (int i = 0; i < AX; ++i) s[i] = 0.0;
        for (int i = tid; i < n; i += AT) {
            const double* fr = a.factors + (int64_t)sh.idx[i] * K;
#pragma unroll
            for (int f = 0; f < AK; ++f)
                if (in[f]) s[f] += fr[f];
            s[AK] += sh.val[i];
        }
        block_sum_vec(s, sh);
#pragma unroll
        for (int i = 0; i < AX; ++i) mean[i] = s[i] / dn;
    }

    // 3. centred cross-products of y = [f_0 .. f_5, d]: A = rows / columns < AK, c = row AK, Syy = (AK, AK)
    double G[ATRI];
#pragma unroll
    for (int i = 0; i < ATRI; ++i) G[i] = 0.0;
    for (int i = tid; i < n; i += AT) {
        const double* fr = a.factors + (int64_t)sh.idx[i] * K;
        double y[AX];
#pragma unroll
        for (int f = 0; f < AK; ++f) y[f] = in[f] ? fr[f] - mean[f] : 0.0;
        y[AK] = sh.val[i] - mean[AK];
#pragma unroll
        for (int r = 0; r < AX; ++r) {
            if (r < AK && !in[r]) continue;
#pragma unroll
            for (int c = 0; c <= r; ++c) G[tri(r, c)] += y[r] * y[c];
        }
    }
    block_sum_vec(G, sh);
    const double syy = G[tri(AK, AK)];

    // 4. Cholesky of A in ascending factor order (every thread, in registers), beta, A^-1
    double Lc[AK][AK], Li[AK][AK], Ai[AK][AK], beta[AK];
    bool full = true;
#pragma unroll
    for (int r = 0; r < AK; ++r) {
#pragma unroll
        for (int c = 0; c < AK; ++c) Lc[r][c] = Li[r][c] = Ai[r][c] = 0.0;
        beta[r] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < AK; ++c) {
        if (!in[c]) continue;
        const double acc = G[tri(c, c)];
        double piv = acc;
#pragma unroll
        for (int b = 0; b < c; ++b) piv -= Lc[c][b] * Lc[c][b];
        if (acc == 0.0 || !(piv > PIVOT_TOL * acc)) full = false;
        const double lcc = sqrt(piv);
        Lc[c][c] = lcc;
#pragma unroll
        for (int r = c + 1; r < AK; ++r) {
            if (!in[r]) continue;
            double v = G[tri(r, c)];
#pragma unroll
            for (int b = 0; b < c; ++b) v -= Lc[r][b] * Lc[c][b];
            Lc[r][c] = v / lcc;
        }
    }
    double ee = NAN;
    if (full) {
        // Li = Lc^-1 (lower), Ai = Li' Li, beta = Ai c
#pragma unroll
        for (int c = 0; c < AK; ++c) {
            if (!in[c]) continue;
            Li[c][c] = 1.0 / Lc[c][c];
#pragma unroll
            for (int r = c + 1; r < AK; ++r) {
                if (!in[r]) continue;
                double v = 0.0;
#pragma unroll
                for (int b = c; b < r; ++b) v -= Lc[r][b] * Li[b][c];
                Li[r][c] = v / Lc[r][r];
            }
        }
#pragma unroll
        for (int r = 0; r < AK; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                double v = 0.0;
#pragma unroll
                for (int b = r; b < AK; ++b) v += Li[b][r] * Li[b][c];
                Ai[r][c] = Ai[c][r] = v;
            }
        // beta by the two triangular solves (forward with Lc, back with Lc')
        double yv[AK];
#pragma unroll
        for (int r = 0; r < AK; ++r) {
            double v = in[r] ? G[tri(AK, r)] : 0.0;
#pragma unroll
            for (int b = 0; b < r; ++b) v -= Lc[r][b] * yv[b];
            yv[r] = in[r] ? v / Lc[r][r] : 0.0;
        }
#pragma unroll
        for (int r = AK - 1; r >= 0; --r) {
            double v = yv[r];
#pragma unroll
            for (int b = r + 1; b < AK; ++b) v -= Lc[b][r] * beta[b];
            beta[r] = in[r] ? v / Lc[r][r] : 0.0;
        }

        // residuals into LDS (each thread rewrites the slots it read), e'e
        double s1[1] = {0.0};
        for (int i = tid; i < n; i += AT) {
            const double* fr = a.factors + (int64_t)sh.idx[i] * K;
            double e = sh.val[i] - mean[AK];
#pragma unroll
            for (int f = 0; f < AK; ++f)
                if (in[f]) e -= beta[f] * (fr[f] - mean[f]);
            sh.val[i] = e;
            s1[0] += e * e;
        }
        block_sum_vec(s1, sh);   // its barriers also publish the residuals
        ee = s1[0];
    }

    // 5. the HAC meat in the centred basis
    double S[ATRI];
#pragma unroll
    for (int i = 0; i < ATRI; ++i) S[i] = 0.0;
    if (full) {
        const int nl = a.nw_lags;
        const double bw = (double)(nl + 1);
        for (int i = tid; i < n; i += AT) {
            const double* fr = a.factors + (int64_t)sh.idx[i] * K;
            const double e = sh.val[i];
            double u[AX], z[AX];
            u[0] = e;
#pragma unroll
            for (int f = 0; f < AK; ++f) u[1 + f] = in[f] ? e * (fr[f] - mean[f]) : 0.0;
#pragma unroll
            for (int r = 0; r < AX; ++r) z[r] = 0.0;
            const int lmax = nl < i ? nl : i;
            for (int l = 1; l <= lmax; ++l) {
                const double* fl = a.factors + (int64_t)sh.idx[i - l] * K;
                const double we = (1.0 - (double)l / bw) * sh.val[i - l];
                z[0] += we;
#pragma unroll
                for (int f = 0; f < AK; ++f)
                    if (in[f]) z[1 + f] += we * (fl[f] - mean[f]);
            }
#pragma unroll
            for (int r = 0; r < AX; ++r) {
                if (r > 0 && !in[r - 1]) continue;
#pragma unroll
                for (int c = 0; c <= r; ++c) S[tri(r, c)] += u[r] * u[c] + (u[r] * z[c] + z[r] * u[c]);
            }
        }
        block_sum_vec(S, sh);
    }

    // 6. outputs
    if (tid != 0) return;
    a.nobs[o] = n;
    stat[2] = mean[AK];
    stat[3] = sqrt(syy / (dn - 1.0));
    if (!full) {
        for (int i = 0; i <= K; ++i) coef[i] = se[i] = hac[i] = NAN;
        stat[0] = stat[1] = NAN;
        return;
    }
    const double s2 = ee / (double)(n - k - 1);
    stat[0] = syy == 0.0 ? NAN : 1.0 - ee / syy;
    stat[1] = sqrt(s2);
    // alpha = d- - beta'f-: its weights on the centred coefficients are g = [1, -f-], and with
    // B = diag(1 / n, A^-1) its variances are s2 g'Bg and (Bg)' S (Bg)
    double h[AX], alpha = mean[AK], va = 1.0 / dn;
    h[0] = 1.0 / dn;
#pragma unroll
    for (int r = 0; r < AK; ++r) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < AK; ++c) v += Ai[r][c] * mean[c];
        h[1 + r] = in[r] ? -v : 0.0;
        if (in[r]) {
            alpha -= beta[r] * mean[r];
            va += mean[r] * v;
        }
    }
    const double qa = quad_form(S, h);
    coef[0] = alpha;
    se[0] = sqrt(s2 * va);
    hac[0] = qa > 0.0 ? sqrt(qa) : 0.0;
#pragma unroll
    for (int f = 0; f < AK; ++f) {
        if (f >= K) continue;
        if (!in[f]) {
            coef[1 + f] = se[1 + f] = hac[1 + f] = NAN;
            continue;
        }
        double hf[AX];
        hf[0] = 0.0;
#pragma unroll
        for (int c = 0; c < AK; ++c) hf[1 + c] = Ai[c][f];
        const double q = quad_form(S, hf);
        coef[1 + f] = beta[f];
        se[1 + f] = sqrt(s2 * Ai[f][f]);
        hac[1 + f] = q > 0.0 ? sqrt(q) : 0.0;
    }
}

}  // namespace
}  // namespace fm

extern "C" int fm_portfolio_alpha(const fm_alpha_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_portfolio_alpha: null args");
    const fm_alpha_args& a = *args;
    FM_REQUIRE(a.nsel >= 0, "fm_portfolio_alpha: nsel must not be negative");
    FM_REQUIRE(a.nrow >= 0, "fm_portfolio_alpha: nrow must not be negative");
    FM_REQUIRE(a.T >= 0, "fm_portfolio_alpha: T must not be negative");
    FM_REQUIRE(a.K >= 1 && a.K <= FM_MAX_FACTORS, "fm_portfolio_alpha: K must be 1..%d, got %d", FM_MAX_FACTORS, a.K);
    FM_REQUIRE(a.M >= 1 && a.M <= FM_MAX_ALPHA_MODELS, "fm_portfolio_alpha: M must be 1..%d, got %d",
               FM_MAX_ALPHA_MODELS, a.M);
    FM_REQUIRE(a.nw_lags >= 0 && a.nw_lags <= FM_ALPHA_MAX_LAGS, "fm_portfolio_alpha: nw_lags must be 0..%d, got %d",
               FM_ALPHA_MAX_LAGS, a.nw_lags);
    for (int m = 0; m < a.M; ++m) {
        FM_REQUIRE(a.model_mask[m] != 0, "fm_portfolio_alpha: model_mask[%d] is empty", m);
        FM_REQUIRE((a.model_mask[m] >> a.K) == 0, "fm_portfolio_alpha: model_mask[%d] = 0x%x names a factor >= K = %d",
                   m, a.model_mask[m], a.K);
    }
    FM_REQUIRE(a.spread_row >= -1, "fm_portfolio_alpha: spread_row must be a row or -1, got %d", a.spread_row);
    if (a.T > FM_ALPHA_MAX_MONTHS) {
        set_error("fm_portfolio_alpha: T = %d exceeds the %d months a series may have", a.T, FM_ALPHA_MAX_MONTHS);
        return FM_ETOOBIG;
    }
    const int64_t nwg = (int64_t)a.nsel * a.nrow * 2 * a.M;
    FM_REQUIRE(nwg <= INT32_MAX, "fm_portfolio_alpha: nsel * nrow is too large");
    if (a.T == 0 || nwg == 0) return FM_OK;
    FM_REQUIRE(a.rec != nullptr, "fm_portfolio_alpha: rec is NULL");
    FM_REQUIRE(a.status != nullptr, "fm_portfolio_alpha: status is NULL");
    FM_REQUIRE(a.factors != nullptr, "fm_portfolio_alpha: factors is NULL");
    FM_REQUIRE(a.coef != nullptr, "fm_portfolio_alpha: coef is NULL");
    FM_REQUIRE(a.se != nullptr, "fm_portfolio_alpha: se is NULL");
    FM_REQUIRE(a.se_hac != nullptr, "fm_portfolio_alpha: se_hac is NULL");
    FM_REQUIRE(a.stat != nullptr, "fm_portfolio_alpha: stat is NULL");
    FM_REQUIRE(a.nobs != nullptr, "fm_portfolio_alpha: nobs is NULL");
    hipLaunchKernelGGL(portfolio_alpha_kernel, dim3((unsigned)nwg), dim3(AT), 0, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_portfolio_alpha");
    return FM_OK;
}
