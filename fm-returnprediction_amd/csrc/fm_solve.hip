// fm_solve: per (month, model, universe) OLS from the bucketed shifted Grams.
//
// Replaces sm.OLS(Y, X).fit() -> params / rsquared / N and the N < K+1 month skip of
// run_monthly_cs_regressions (reference src/regressions.py:52-72) and the create_figure_1
// OLS (src/calc_Lewellen_2014.py:913-921).  statsmodels solves with an SVD pseudo-inverse
// of X; here the slopes come from the centered normal equations
//     Sxx b = Sxy,  Sxx = sum (x-xbar)(x-xbar)', Sxy = sum (x-xbar)(y-ybar)
// by a Cholesky factorization (one wavefront per problem, lanes over matrix entries).
// When a pivot collapses (1 - R^2 of a regressor on the previous ones <= 1e-9, e.g. an
// all-zero column or an exactly collinear pair) the wave falls back to a Jacobi
// eigen-decomposition of Sxx and the minimum-norm (pseudo-inverse) solution of the
// uncentered design [1, X] (what statsmodels' pinv returns, see jacobi_pinv).
// R^2 = 1 - (Syy - b'Sxy)/Syy (centered TSS: the model has a constant).
//
// One workgroup (4 waves) per month: the month's bucket Grams are first summed over its
// chunks into LDS, then the waves take the month's problems round-robin.
#include <math.h>

#include <type_traits>

#include "fm_reg16_dev.h"

FM_PROBE_BUFFER(solve)

namespace fm {
namespace {

constexpr int VT = 256;
constexpr int VNW = VT / WAVE;
constexpr int MAXB_LDS = 8192;   // doubles of bucket sums held in LDS (64 KB max)
constexpr int64_t SCAN_GRID = 1024;   // workgroups of the status-scanning fix-up launches
constexpr double CHOL_REL = 1e-9;
constexpr double EIG_REL = 1e-12;

template <int MD>
struct WaveScratch {
    double A[MD * MD];   // G, then L (Cholesky) or the Jacobi matrix
    double V[MD * MD];   // centered S, then Jacobi eigenvectors
    double sxy[MD], sdiag[MD], mu[MD], b[MD];
};

// Cyclic Jacobi + pseudo-inverse solve by lane 0 (rare fallback path).  A = Sxx (centered),
// mur[0..K-1] = the regressors' raw means and mur[K] = y's.  The range part is the centered
// minimum-norm slope vector b_c; statsmodels' pinv minimizes over the UNCENTERED design
// [1, X] instead, whose null space also holds every affine dependence (a regressor constant
// within the month, x2 = a x1 + c): with N = the null eigenvectors of Sxx, w = N' mur and
// beta0_c = ybar - b_c' mur, the min-norm LS solution is
//     b = b_c + N w beta0_c / (1 + |w|^2),  beta0 = beta0_c / (1 + |w|^2)
// (minimize beta0^2 + |b|^2 over b = b_c + N t, beta0 = beta0_c - w' t).  The intercept is
// then ybar - b' mur as on the regular path, which equals the beta0 above.
template <int MD>
__device__ void jacobi_pinv(double* A, double* V, int K, const double* sxy, const double* mur, double* b) {
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) V[i * MD + j] = i == j ? 1.0 : 0.0;
    double frob = 0.0;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) frob += A[i * MD + j] * A[i * MD + j];
    for (int sweep = 0; sweep < 80; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < K; ++p)
            for (int q = p + 1; q < K; ++q) off += A[p * MD + q] * A[p * MD + q];
        if (off <= 1e-34 * frob) break;
        for (int p = 0; p < K; ++p) {
            for (int q = p + 1; q < K; ++q) {
                const double apq = A[p * MD + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * MD + q] - A[p * MD + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < K; ++k) {
                    const double akp = A[k * MD + p], akq = A[k * MD + q];
                    A[k * MD + p] = c * akp - s * akq;
                    A[k * MD + q] = s * akp + c * akq;
                }
                for (int k = 0; k < K; ++k) {
                    const double apk = A[p * MD + k], aqk = A[q * MD + k];
                    A[p * MD + k] = c * apk - s * aqk;
                    A[q * MD + k] = s * apk + c * aqk;
                }
                A[p * MD + q] = 0.0;
                A[q * MD + p] = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double vkp = V[k * MD + p], vkq = V[k * MD + q];
                    V[k * MD + p] = c * vkp - s * vkq;
                    V[k * MD + q] = s * vkp + c * vkq;
                }
            }
        }
    }
    double lmax = 0.0;
    for (int i = 0; i < K; ++i) lmax = fmax(lmax, fabs(A[i * MD + i]));
    for (int j = 0; j < K; ++j) b[j] = 0.0;
    for (int i = 0; i < K; ++i) {
        const double l = A[i * MD + i];
        if (!(l > EIG_REL * lmax)) continue;
        double proj = 0.0;
        for (int k = 0; k < K; ++k) proj += V[k * MD + i] * sxy[k];
        proj /= l;
        for (int j = 0; j < K; ++j) b[j] += proj * V[j * MD + i];
    }
    double b0 = mur[K], den = 1.0;
    for (int j = 0; j < K; ++j) b0 -= b[j] * mur[j];
    for (int i = 0; i < K; ++i) {
        if (A[i * MD + i] > EIG_REL * lmax) continue;
        double wi = 0.0;
        for (int k = 0; k < K; ++k) wi += V[k * MD + i] * mur[k];
        den += wi * wi;
    }
    if (!(den > 1.0) || !isfinite(b0)) return;   // the null space misses the intercept
    for (int i = 0; i < K; ++i) {
        if (A[i * MD + i] > EIG_REL * lmax) continue;
        double wi = 0.0;
        for (int k = 0; k < K; ++k) wi += V[k * MD + i] * mur[k];
        const double t = b0 * wi / den;
        for (int j = 0; j < K; ++j) b[j] += t * V[j * MD + i];
    }
}

// Sum the month's chunk partials into LDS: BCH loads per thread in flight per chunk (a
// one-load-per-iteration loop waits out one HBM round trip per element).
template <int NT>
__device__ __forceinline__ void sum_partials(const double* partial, int c0, int c1, int n, double* bs) {
    constexpr int BCH = 8;
    const int tid = threadIdx.x;
    for (int e0 = tid; e0 < n; e0 += NT * BCH) {
        double acc[BCH];
#pragma unroll
        for (int k = 0; k < BCH; ++k) acc[k] = 0.0;
        for (int c = c0; c < c1; ++c) {
            const double* pc = partial + (int64_t)c * n;
#pragma unroll
            for (int k = 0; k < BCH; ++k) {
                const int e = e0 + k * NT;
                acc[k] += pc[e < n ? e : n - 1];   // clamped: unconditional loads
            }
        }
#pragma unroll
        for (int k = 0; k < BCH; ++k) {
            const int e = e0 + k * NT;
            if (e < n) bs[e] = acc[k];
        }
    }
}

// Per month: bucket sums -> level-cumulative sums (bucket (pattern, u) becomes the sum over
// levels >= u, so a problem adds one bucket per pattern that contains its model) -> one
// wave per problem.  The wave keeps the centered moment matrix S over (x_1..x_K, y) in
// registers, lane i = row i (MD doubles), and factors it by a right-looking Cholesky whose
// pivot-row broadcasts are readlanes (no LDS round trip per column).  Factoring the
// augmented matrix [Sxx Sxy; Sxy' Syy] leaves l = L^-1 Sxy in the y row, so the forward
// substitution comes free; the back substitution L' b = l runs on the transposed factor
// (one LDS transpose), lane i owning b_i.
template <int MD>
__global__ __launch_bounds__(VT) void solve_kernel(fm_solve_args a) {
    extern __shared__ double bs[];   // [nb][zw(zw+1)/2] packed bucket sums of this month
    __shared__ WaveScratch<MD> ws_all[VNW];
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int zw = a.zw, zz = zw * (zw + 1) / 2;   // packed upper triangle per bucket
    const int nl = a.nlevels, npat = a.npatterns, nb = npat * nl;
    const int c0 = a.seg_chunk_off[s], c1 = a.seg_chunk_off[s + 1];
    sum_partials<VT>(a.partial, c0, c1, nb * zz, bs);
    __syncthreads();
    for (int e = tid; e < npat * zz; e += VT) {
        const int pid = e / zz, f = e - pid * zz;
        double* b0 = bs + (int64_t)pid * nl * zz + f;
        double run = b0[(nl - 1) * zz];
        for (int l = nl - 2; l >= 0; --l) {
            run += b0[l * zz];
            b0[l * zz] = run;
        }
    }
    __syncthreads();
    WaveScratch<MD>& ws = ws_all[w];
    const int rs = a.pmax + 2;
    constexpr int PKW = MD * (MD + 1) / 2;   // packed entries of one problem Gram
    constexpr int EPL = (PKW + WAVE - 1) / WAVE;
    for (int p = w; p < a.nprob; p += VNW) {
        const int m = a.prob_model[p], u = a.prob_level[p], nz = a.prob_nz[p];
        const int* zi = a.prob_z + p * 32;
        const int K = nz - 2, K1 = K + 1;
        // ---- the problem's Gram G[i][j] (i, j < nz over its z indices) into the wave's V:
        // lanes over packed (i <= j) entries, patterns in the outer loop, so each pattern
        // costs one batch of independent LDS reads; G is written in both triangles
        int off[EPL], dst[EPL], dsw[EPL];
        double acc[EPL];
#pragma unroll
        for (int t = 0; t < EPL; ++t) {
            const int e = lane + WAVE * t;
            int i = 0, rem = e;   // packed index e -> (i, j), rows of length nz - i
            while (i < nz && rem >= nz - i) {
                rem -= nz - i;
                ++i;
            }
            const bool in = i < nz;
            const int j = in ? i + rem : 0;
            const int zr = in ? zi[i] : 0, zc = in ? zi[j] : 0;
            const int r = zr < zc ? zr : zc, c = zr < zc ? zc : zr;
            off[t] = in ? r * zw - (r * (r - 1)) / 2 + (c - r) : 0;
            dst[t] = in ? i * MD + j : -1;
            dsw[t] = in ? j * MD + i : -1;
            acc[t] = 0.0;
        }
        for (int q = 0; q < npat; ++q) {
            if (!((a.pattern_models[q] >> m) & 1u)) continue;   // wave-uniform
            const double* bq = bs + (q * nl + u) * zz;
#pragma unroll
            for (int t = 0; t < EPL; ++t) acc[t] += bq[off[t]];
        }
#pragma unroll
        for (int t = 0; t < EPL; ++t)
            if (dst[t] >= 0) {
                ws.V[dst[t]] = acc[t];
                ws.V[dsw[t]] = acc[t];
            }
        wave_sync();
        const double* Gp = ws.V;   // G[i][j], row stride MD; z index 0 is the intercept
        const int zl = lane < K1 ? zi[1 + lane] : 0;   // panel z index of this lane's row
        const int li = lane < K1 ? 1 + lane : 0;       // this lane's row in Gp
        const double n = Gp[0];
        const double g0 = lane < K1 ? Gp[li] : 0.0;    // first moment of this lane's variable
        const double gdiag = lane < K1 ? Gp[li * MD + li] : 0.0;
        const int64_t ro = ((int64_t)s * a.nprob + p) * rs;
        uint32_t st = 0;
        // inf in the problem's rows: a regressor or y value of +-inf makes its Gram diagonal
        // sum(z^2) = +inf (columns the problem does not use are never read)
        if (__ballot(lane < K && isinf(gdiag)) != 0) st |= FM_ST_INF_IN_X;
        if (__ballot(lane == K && isinf(gdiag)) != 0) st |= FM_ST_INF_IN_Y;
        if (a.gram_flags) st |= a.gram_flags[(int64_t)s * a.nmodels + m] & (FM_ST_INF_IN_X | FM_ST_INF_IN_Y);
        if (!(n >= (double)(K + 1))) {
            write_failed_rec(a.rec, ro, rs, a.pmax, n, lane, WAVE);
            if (lane == 0) a.status[(int64_t)s * a.nprob + p] = FM_ST_SKIPPED;
            continue;
        }
        // ---- centered moments: row i of S, S[i][j] = G(z_i, z_j) - G(0, z_i) G(0, z_j) / n
        double row[MD];
        double sii = 0.0, sxy = 0.0;   // S[i][i], S[i][K] of this lane
#pragma unroll
        for (int j = 0; j < MD; ++j) {
            row[j] = 0.0;
            if (j < K1) {
                const double v = lane < K1 ? Gp[li * MD + 1 + j] - g0 * Gp[1 + j] / n : 0.0;
                row[j] = v;
                if (j == lane) sii = v;
                if (j == K) sxy = v;
            }
        }
        const double mu = g0 / n;
        if (a.moments) {
            double* mo = a.moments + ((int64_t)s * a.nprob + p) * a.mom_stride;
            if (lane == 0) mo[0] = n;
            if (lane < K1) {
                mo[1 + lane] = mu;
#pragma unroll
                for (int j = 0; j < MD; ++j)
                    if (j < K1) mo[1 + K1 + lane * K1 + j] = row[j];
            }
        }
        if ((a.prob_flags[p] & 1) != 0) {
            if (__ballot(lane < K && !(sii > 1e-10 * gdiag)) != 0) st |= FM_ST_CONST_SUSPECT;
        }
        const double syy = readlane_f64(sii, K);
        // ---- augmented Cholesky, lane i = row i; rows >= K1 are zero
        bool ok = true;
#pragma unroll
        for (int k = 0; k < MD - 1; ++k) {
            if (ok && k < K) {   // wave-uniform
                const double orig = readlane_f64(sii, k);
                const double piv = readlane_f64(row[k], k);
                if (!(piv > REFIT_REL * orig)) st |= FM_ST_REFIT;
                if (!(orig > 0.0) || !(piv > CHOL_REL * orig)) {
                    ok = false;
                } else {
                    const double lkk = sqrt(piv);
                    const double rinv = 1.0 / lkk;
                    const double lik = row[k] * rinv;
#pragma unroll
                    for (int j = k + 1; j < MD; ++j) {
                        if (j <= K) {
                            const double sj = readlane_f64(row[j], k) * rinv;   // L[j][k]
                            row[j] -= lik * sj;
                        }
                    }
                    row[k] = lane == k ? lkk : lik;
                }
            }
        }
        double bi = 0.0;
        if (ok) {
            // transpose through LDS: lane i then holds column i of L (and l_i)
            double* T = ws.A;
#pragma unroll
            for (int j = 0; j < MD; ++j)
                if (lane < K1) T[lane * MD + j] = row[j];
            wave_sync();
            double col[MD];
#pragma unroll
            for (int r = 0; r < MD; ++r) col[r] = lane < MD ? T[r * MD + (lane & (MD - 1))] : 0.0;
            double t = lane < K ? T[K * MD + lane] : 0.0;   // l_i
#pragma unroll
            for (int j = MD - 2; j >= 0; --j) {
                if (j < K) {
                    const double bj = readlane_f64(t, j) / readlane_f64(col[j], j);
                    if (lane == j) t = bj;
                    else if (lane < j) t -= col[j] * bj;
                }
            }
            bi = lane < K ? t : 0.0;
            wave_sync();
        } else {
            st |= FM_ST_RANK_DEF | FM_ST_REFIT;
            // rebuild Sxx (rows were overwritten) for the pseudo-inverse fallback
#pragma unroll
            for (int j = 0; j < MD; ++j)
                if (j < K && lane < K) ws.A[lane * MD + j] = Gp[li * MD + 1 + j] - g0 * Gp[1 + j] / n;
            if (lane < K) ws.sxy[lane] = sxy;
            if (lane < K1) ws.mu[lane] = mu + (a.add_back ? a.add_back[(int64_t)(zl - 1) * a.nseg + s] : 0.0);
            wave_sync();
            if (lane == 0) jacobi_pinv<MD>(ws.A, ws.V, K, ws.sxy, ws.mu, ws.b);
            wave_sync();
            bi = lane < K ? ws.b[lane] : 0.0;
            wave_sync();
        }
        // R^2 = 1 - SSR/SST (centered), raw-coordinate intercept
        double t_sxy = lane < K ? bi * sxy : 0.0;
        double t_mu = lane < K ? bi * mu : 0.0;
        double t_ab = 0.0;
        if (a.add_back && lane < K) t_ab = bi * a.add_back[(int64_t)(zl - 1) * a.nseg + s];
        t_sxy = wave_sum(t_sxy);
        t_mu = wave_sum(t_mu);
        t_ab = wave_sum(t_ab);
        const double r2 = 1.0 - (syy - t_sxy) / syy;
        double icpt = readlane_f64(mu, K) - t_mu;
        if (a.add_back) icpt += a.add_back[(int64_t)(zi[K + 1] - 1) * a.nseg + s] - t_ab;
        // b_{k-1} to lane k (all lanes active: a bpermute reads nothing from inactive lanes);
        // rs <= 34 < 64, so lane k writes record entry k
        const double bsh = __shfl(bi, lane > 0 ? lane - 1 : 0, WAVE);
        write_fitted_rec(a.rec, ro, rs, a.pmax, K, icpt, bsh, r2, n, lane, WAVE);
        if (lane == 0) a.status[(int64_t)s * a.nprob + p] = st | FM_ST_FITTED;
    }
}

// ---------------------------------------------------------------------------------------
// The statsmodels fix-ups of flagged (month, problem) pairs.  They run inside solve16_kernel
// (zw == 16) or as the separate fm_solve_fixup launch, and all read the
// same things, held in one context: the panel rows (CA: FP64 columns or the two planes), the
// per-(column, month) transforms, the problem tables and the solve's outputs.
template <class CA>
struct FixCtx {
    CA cols; int64_t stride; const int64_t* seg_off; int nseg;   // rows of month s: seg_off[s..s+1]
    const double *lo, *hi;                       // [ncols][nseg] clip bounds (both or neither)
    const double *shift, *inv_scale, *add_back;  // [ncols][nseg] x -> (x - shift) * inv_scale (+ add_back)
    const uint8_t* level;                        // per-row universe level, or null
    int nprob; const int32_t *prob_level, *prob_z, *prob_nz;
    const double* moments; int mom_stride;       // the solve's n, means and centered moments
    int pmax; double* rec; uint32_t* status;
    int check_const;
};

// The context of the fix-ups of solve `a`, its rows read through `cols` (both launches build it here)
template <class CA>
__host__ __device__ __forceinline__ FixCtx<CA> fix_ctx(const fm_solve_args& a, CA cols) {
    FixCtx<CA> fx{};
    fx.check_const = a.fix_check_const;
    fx.cols = cols, fx.stride = a.fix_stride, fx.seg_off = a.fix_seg_off, fx.nseg = a.nseg;
    fx.lo = a.fix_lo, fx.hi = a.fix_hi;
    fx.shift = a.fix_shift, fx.inv_scale = a.fix_inv_scale, fx.add_back = a.add_back;
    fx.level = a.fix_level;
    fx.nprob = a.nprob, fx.prob_level = a.prob_level, fx.prob_z = a.prob_z, fx.prob_nz = a.prob_nz;
    fx.moments = a.moments, fx.mom_stride = a.mom_stride;
    fx.pmax = a.pmax, fx.rec = a.rec, fx.status = a.status;
    return fx;
}

// Exact nonzero-constant test for problems flagged CONST_SUSPECT (statsmodels
// add_constant(has_constant='skip'): np.ptp(x)==0 & all(x != 0), src/regressions.py:50).
template <int NT = VT, class CA = F64Cols>
__device__ __forceinline__ void const_pair(int s, int p, uint64_t* red, const FixCtx<CA>& fx) {
    const int nz = fx.prob_nz[p], K = nz - 2, u = fx.prob_level[p];
    const int* zi = fx.prob_z + p * 32;
    const int64_t r0 = fx.seg_off[s], r1 = fx.seg_off[s + 1];
    bool any_const = false;
    for (int j = 0; j < K; ++j) {
        const int cx = zi[1 + j] - 1;
        uint64_t kmin = SENT, kmax = 0;
        bool allnz = true;
        for (int64_t r = r0 + threadIdx.x; r < r1; r += NT) {
            if (fx.level && (int)fx.level[r] < u) continue;
            bool ok = true;
            double xv = 0.0;
            for (int q = 1; q < nz; ++q) {
                const int c = zi[q] - 1;
                double x = fx.cols[(int64_t)c * fx.stride + r];
                if (fx.lo) {
                    const double l = fx.lo[(int64_t)c * fx.nseg + s], h = fx.hi[(int64_t)c * fx.nseg + s];
                    if (x < l) x = l;
                    if (x > h) x = h;
                }
                if (isnan(x)) ok = false;
                if (c == cx) xv = x;
            }
            if (!ok) continue;
            const uint64_t k = dkey(xv == 0.0 ? 0.0 : xv);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
            if (xv == 0.0) allnz = false;
        }
        kmin = block_min_u64<NT / WAVE>(kmin, red);
        kmax = block_max_u64<NT / WAVE>(kmax, red);
        const int nzr = block_sum<NT / WAVE>(allnz ? 0 : 1, (int*)red);
        if (kmin != SENT && kmin == kmax && nzr == 0) any_const = true;
    }
    if (threadIdx.x == 0 && any_const) fx.status[(int64_t)s * fx.nprob + p] |= FM_ST_CONST_COL;
}

// inf in y (statsmodels keeps the month): params = pinv(X) @ y, so each coefficient is the
// IEEE sum of pinv[j,i] * y_i; with y_i = +-inf the finite rows do not matter and the
// result is +inf, -inf or NaN (mixed signs, or 0*inf).  pinv[:,i] for the slopes is
// Sxx^{-1}(x_i - xbar) and for the intercept 1/n - xbar'Sxx^{-1}(x_i - xbar).  One
// workgroup per flagged (month, problem); R^2 becomes NaN as in statsmodels.
struct InfySmem {
    double Lm[32 * 32];
    double mu[32], xb[32];
    unsigned bits[32];
    int okf;
};

template <int NT = VT, int NC = 32, class CA = F64Cols>
__device__ __forceinline__ void infy_pair(int s, int p, InfySmem& sm, const FixCtx<CA>& fx) {
    double* Lm = sm.Lm;
    double* mu = sm.mu;
    double* xb = sm.xb;
    unsigned* bits = sm.bits;
    int& okf = sm.okf;
    const int nz = fx.prob_nz[p], K = nz - 2, K1 = K + 1, u = fx.prob_level[p];
    const int* zi = fx.prob_z + p * 32;
    const double* mo = fx.moments + ((int64_t)s * fx.nprob + p) * fx.mom_stride;
    const double n = mo[0];
    for (int e = threadIdx.x; e < K * K; e += NT) Lm[(e / K) * 32 + e % K] = mo[1 + K1 + (e / K) * K1 + e % K];
    if (threadIdx.x < K1) mu[threadIdx.x] = mo[1 + threadIdx.x];
    if (threadIdx.x < 32) bits[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x < K) {
        const int c = zi[1 + threadIdx.x] - 1;
        xb[threadIdx.x] = mu[threadIdx.x] + (fx.add_back ? fx.add_back[(int64_t)c * fx.nseg + s] : 0.0);
    }
    if (threadIdx.x == 0) {
        int ok = 1;
        for (int k = 0; k < K && ok; ++k) {
            double d = Lm[k * 32 + k];
            for (int j = 0; j < k; ++j) d -= Lm[k * 32 + j] * Lm[k * 32 + j];
            if (!(d > 0.0)) { ok = 0; break; }
            d = sqrt(d);
            Lm[k * 32 + k] = d;
            for (int i = k + 1; i < K; ++i) {
                double t = Lm[i * 32 + k];
                for (int j = 0; j < k; ++j) t -= Lm[i * 32 + j] * Lm[k * 32 + j];
                Lm[i * 32 + k] = t / d;
            }
        }
        okf = ok;
    }
    __syncthreads();
    if (!okf) return;   // rank-deficient with an inf y: left as computed (NaN)
    const int64_t r0 = fx.seg_off[s], r1 = fx.seg_off[s + 1];
    if constexpr (NC <= 16) {
        // register arrays (fully unrolled, statically indexed: no scratch, which would throttle
        // the waves of the solve kernel these fix-ups ride); the opaque zero keeps the factor's
        // LDS reads inside the row loop instead of hoisted into ~120 live registers
        for (int64_t r = r0 + threadIdx.x; r < r1; r += NT) {
            if (fx.level && (int)fx.level[r] < u) continue;
            int zo = 0;
            asm volatile("" : "+v"(zo));
            double d[NC];
            double y = 0.0;
            bool valid = true;
#pragma unroll
            for (int q = 1; q <= NC; ++q) {
                if (q < nz) {
                    const int c = zi[q] - 1;
                    double x = fx.cols[(int64_t)c * fx.stride + r];
                    if (fx.lo) {
                        const double l = fx.lo[(int64_t)c * fx.nseg + s], h = fx.hi[(int64_t)c * fx.nseg + s];
                        if (x < l) x = l;
                        if (x > h) x = h;
                    }
                    if (isnan(x)) valid = false;
                    if (q == nz - 1) {
                        y = x;
                    } else {
                        if (fx.shift) x -= fx.shift[(int64_t)c * fx.nseg + s];
                        if (fx.inv_scale) x *= fx.inv_scale[(int64_t)c * fx.nseg + s];
                        d[q - 1] = x - mu[q - 1 + zo];
                    }
                }
            }
            if (!valid || !isinf(y)) continue;
#pragma unroll
            for (int i = 0; i < NC; ++i) {          // L w = d
                if (i < K) {
                    double t = d[i];
#pragma unroll
                    for (int j = 0; j < i; ++j) t -= Lm[i * 32 + j + zo] * d[j];
                    d[i] = t / Lm[i * 32 + i + zo];
                }
            }
#pragma unroll
            for (int i = NC - 1; i >= 0; --i) {     // L' c = w
                if (i < K) {
                    double t = d[i];
#pragma unroll
                    for (int j = i + 1; j < NC; ++j)
                        if (j < K) t -= Lm[j * 32 + i + zo] * d[j];
                    d[i] = t / Lm[i * 32 + i + zo];
                }
            }
            double c0 = 1.0 / n;
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j < K) c0 -= xb[j + zo] * d[j];
#pragma unroll
            for (int j = 0; j <= NC; ++j) {
                if (j <= K) {
                    const double term = (j == 0 ? c0 : d[j == 0 ? 0 : j - 1]) * y;
                    const unsigned b = isnan(term) ? 4u : (term > 0.0 ? 1u : 2u);
                    atomicOr(&bits[j], b);
                }
            }
        }
    } else
    for (int64_t r = r0 + threadIdx.x; r < r1; r += NT) {
        if (fx.level && (int)fx.level[r] < u) continue;
        double v[32];
        bool valid = true;
        for (int q = 1; q < nz; ++q) {
            const int c = zi[q] - 1;
            double x = fx.cols[(int64_t)c * fx.stride + r];
            if (fx.lo) {
                const double l = fx.lo[(int64_t)c * fx.nseg + s], h = fx.hi[(int64_t)c * fx.nseg + s];
                if (x < l) x = l;
                if (x > h) x = h;
            }
            if (isnan(x)) valid = false;
            v[q - 1] = x;
        }
        if (!valid || !isinf(v[K])) continue;
        const double y = v[K];
        double d[32];
        for (int j = 0; j < K; ++j) {
            const int c = zi[1 + j] - 1;
            double x = v[j];
            if (fx.shift) x -= fx.shift[(int64_t)c * fx.nseg + s];
            if (fx.inv_scale) x *= fx.inv_scale[(int64_t)c * fx.nseg + s];
            d[j] = x - mu[j];
        }
        for (int i = 0; i < K; ++i) {          // L w = d
            double t = d[i];
            for (int j = 0; j < i; ++j) t -= Lm[i * 32 + j] * d[j];
            d[i] = t / Lm[i * 32 + i];
        }
        for (int i = K - 1; i >= 0; --i) {     // L' c = w
            double t = d[i];
            for (int j = i + 1; j < K; ++j) t -= Lm[j * 32 + i] * d[j];
            d[i] = t / Lm[i * 32 + i];
        }
        double c0 = 1.0 / n;
        for (int j = 0; j < K; ++j) c0 -= xb[j] * d[j];
        for (int j = 0; j <= K; ++j) {
            const double term = (j == 0 ? c0 : d[j - 1]) * y;
            const unsigned b = isnan(term) ? 4u : (term > 0.0 ? 1u : 2u);
            atomicOr(&bits[j], b);
        }
    }
    __syncthreads();
    const int64_t ro = ((int64_t)s * fx.nprob + p) * (fx.pmax + 2);
    if (threadIdx.x <= K) {
        const unsigned b = bits[threadIdx.x];
        if (b != 0u) {
            double val = NAN;
            if (!(b & 4u) && b != 3u) val = (b & 1u) ? INFINITY : -INFINITY;
            fx.rec[ro + threadIdx.x] = val;
        }
    }
    if (threadIdx.x == 0) fx.rec[ro + fx.pmax] = NAN;
}

// ---------------------------------------------------------------------------------------
// Row-level refit of FM_ST_REFIT problems (ill-conditioned or rank-deficient Sxx), so that
// statsmodels' pinv semantics hold where the normal equations cannot: pinv_extended takes
// the SVD of the UNCENTERED design X = [1, x_1..x_K] (rcond 1e-15) and returns
// params = V S^+ U' y (min-norm over [1, X]), rsquared = 1 - SSR / centered TSS.
//   1. Householder TSQR of [X | y] over the problem's rows (the Gram's row set: universe
//      level >= u, every model column non-NaN after the clip), each wave absorbing 64-row
//      tiles into its own triangular factor, the four factors then merged by wave 0.
//      Backward stable: the factor's error is ~eps * |X|, not eps * |X|^2.
//   2. One-sided (Hestenes) Jacobi SVD of R_xx, cut at SVD_REL * sigma_max, and
//      beta = V S^+ U' r_y with r_y = Q'y.  SSR = |r_y - R_xx beta|^2 + rho^2 (rho = y's
//      diagonal of R), centered TSS = sum_{i >= 1} r_y[i]^2 + rho^2 (column 0 is the
//      constant, so Q's first column is 1/sqrt(n)).
// SVD_REL is 1e-13, not statsmodels' 1e-15: an exact dependence (a zero column, x2 = 2 x1,
// a regressor constant within the month) leaves a singular value at the QR's rounding
// floor (~N eps sigma_max), which must be cut; genuine near-dependences down to 1e-13 are
// kept.
constexpr double SVD_REL = 1e-13;
// A centered sum of squares below this was summed from squares near or under the subnormal
// range (absolute error ~2^-1075 each): the normal equations cannot be trusted, whatever the
// pivot ratios say, and the problem is refitted from its rows with the column scaled.
constexpr double TINY_SS = 0x1p-1000;

__device__ __forceinline__ double wave_sum_dpp(double v) {
    v += xor_lanes_f64(v, 1);
    v += xor_lanes_f64(v, 2);
    v += xor_lanes_f64(v, 4);
    v += xor_lanes_f64(v, 8);
    v += xor_lanes_f64(v, 16);
    v += xor_lanes_f64(v, 32);
    return v;
}

template <int NC, int NW = VNW>
struct RefitSmem {
    double R[NW][NC][NC + 1];    // per-wave triangular factors of [1, x, y]
    double Ac[NC][NC + 1];       // Jacobi: rotated columns of R_xx, Ac[j][i] = (R_xx V)[i][j]
    double Vc[NC][NC + 1];       // Jacobi: V[i][j] at Vc[j][i]
    double bv[NC];
};

// Absorb one 64-row tile (lane = row, a[] = its NC values, zero rows allowed) into the
// wave's triangular factor R: Householder reflections over [R row k; tile column k].
template <int NC>
__device__ __forceinline__ void hh_absorb(double (&a)[NC], double (*R)[NC + 1], int nzc) {
    const int lane = lane_id();
    static_for<0, NC>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if (k < nzc) {
            const double ss = wave_sum_dpp(a[k] * a[k]);
            if (ss != 0.0) {   // wave-uniform: a zero tile column leaves R as it is
                const double alpha = R[k][k];
                const double nrm = sqrt(alpha * alpha + ss);
                const double beta = alpha > 0.0 ? -nrm : nrm;
                const double v0 = alpha - beta;
                const double tau = -v0 / beta;
                const double vl = a[k] / v0;   // v = (1, a[:,k] / v0)
                double w[NC];
                static_for<k + 1, NC>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    w[j] = vl * a[j];
                });
                static_for<k + 1, NC>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    w[j] = wave_sum_dpp(w[j]) + R[k][j];
                });
                static_for<k + 1, NC>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    a[j] -= (tau * w[j]) * vl;
                });
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (lane == 0) {
                    R[k][k] = beta;
                    static_for<k + 1, NC>([&](auto jc) {
                        constexpr int j = decltype(jc)::value;
                        R[k][j] -= tau * w[j];
                    });
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                a[k] = 0.0;
            }
        }
    });
}

template <int NC, int NT = VT, class CA = F64Cols>
__device__ void refit_pair(int s, int p, RefitSmem<NC, NT / WAVE>& sm, const FixCtx<CA>& fx) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int nz = fx.prob_nz[p], P = nz - 1, u = fx.prob_level[p];
    const int* zi = fx.prob_z + p * 32;
    constexpr int NW = NT / WAVE;
    for (int e = tid; e < NW * NC * (NC + 1); e += NT) (&sm.R[0][0][0])[e] = 0.0;
    // A regressor whose centered sum of squares is below TINY_SS (its squares were subnormal in
    // the Gram) is scaled by a power of two that brings the sum near 1, and its slope scaled
    // back at the end: both exact.  Every other column's factor is 1.0 (x * 1.0 keeps its bits).
    // The factors sit in sm.bv until the slopes replace them.
    if (tid < NC) {
        double f = 1.0;
        if (tid >= 1 && tid <= P - 1) {
            const int K1 = P;
            const double sd = fx.moments[((int64_t)s * fx.nprob + p) * fx.mom_stride + 1 + K1 + (tid - 1) * K1 + (tid - 1)];
            if (sd > 0.0 && sd < TINY_SS) f = __builtin_ldexp(1.0, -ilogb(sd) / 2);
        }
        sm.bv[tid] = f;
    }
    __syncthreads();
    int zc[NC];   // panel column of z index q (q >= 1)
    static_for<0, NC>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        zc[q] = (q >= 1 && q < nz) ? zi[q] - 1 : 0;
    });
    const int64_t r0 = fx.seg_off[s], r1 = fx.seg_off[s + 1];
    for (int64_t base = r0 + (int64_t)w * WAVE; base < r1; base += NT) {
        const int64_t r = base + lane;
        bool valid = r < r1 && !(fx.level && (int)fx.level[r] < u);
        double a[NC];
        static_for<0, NC>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            double v = 0.0;
            if constexpr (q == 0) {
                v = 1.0;
            } else {
                if (valid && q < nz) {
                    const int c = zc[q];
                    double x = fx.cols[(int64_t)c * fx.stride + r];
                    if (fx.lo) {
                        const double l = fx.lo[(int64_t)c * fx.nseg + s], h = fx.hi[(int64_t)c * fx.nseg + s];
                        if (x < l) x = l;
                        if (x > h) x = h;
                    }
                    if (fx.inv_scale) {
                        x = (x - fx.shift[(int64_t)c * fx.nseg + s]) * fx.inv_scale[(int64_t)c * fx.nseg + s];
                        if (fx.add_back) x += fx.add_back[(int64_t)c * fx.nseg + s];
                    }
                    if (isnan(x)) valid = false;
                    v = x * sm.bv[q];
                }
            }
            a[q] = v;
        });
        static_for<0, NC>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            if (!valid) a[q] = 0.0;
        });
        hh_absorb<NC>(a, sm.R[w], nz);
    }
    __syncthreads();
    if (w == 0) {   // merge the other waves' factors into wave 0's
        for (int o = 1; o < NW; ++o) {
            double a[NC];
            static_for<0, NC>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                a[j] = (lane < NC && j >= lane) ? sm.R[o][lane < NC ? lane : 0][j] : 0.0;
            });
            hh_absorb<NC>(a, sm.R[0], nz);
        }
        // ---- one-sided Jacobi SVD of R_xx (P x P upper triangular), lane i = row i
        double (*R)[NC + 1] = sm.R[0];
        const bool li = lane < P;
        const int lr = li ? lane : 0;
        if (li)
            for (int j = 0; j < P; ++j) {
                sm.Ac[j][lane] = j >= lane ? R[lane][j] : 0.0;
                sm.Vc[j][lane] = j == lane ? 1.0 : 0.0;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int sweep = 0; sweep < 60; ++sweep) {
            bool rotated = false;
            for (int pc = 0; pc < P - 1; ++pc) {
                for (int qc = pc + 1; qc < P; ++qc) {
                    const double ap = li ? sm.Ac[pc][lr] : 0.0, aq = li ? sm.Ac[qc][lr] : 0.0;
                    const double al = wave_sum_dpp(ap * ap);
                    const double be = wave_sum_dpp(aq * aq);
                    const double ga = wave_sum_dpp(ap * aq);
                    if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;   // wave-uniform
                    rotated = true;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = fabs(zeta) > 1e150
                                         ? 0.5 / zeta
                                         : (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                    const double vp = li ? sm.Vc[pc][lr] : 0.0, vq = li ? sm.Vc[qc][lr] : 0.0;
                    if (li) {
                        sm.Ac[pc][lane] = c * ap - sn * aq;
                        sm.Ac[qc][lane] = sn * ap + c * aq;
                        sm.Vc[pc][lane] = c * vp - sn * vq;
                        sm.Vc[qc][lane] = sn * vp + c * vq;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
            }
            if (!rotated) break;
        }
        // ---- beta = V S^+ (R_xx V)' r_y; singular values below SVD_REL * sigma_max cut
        const double ry = li ? R[lane][P] : 0.0;   // Q'y
        const double rho = R[P][P];
        double smax = 0.0;
        for (int j = 0; j < P; ++j) smax = fmax(smax, wave_sum_dpp(li ? sm.Ac[j][lr] * sm.Ac[j][lr] : 0.0));
        smax = sqrt(smax);
        double bi = 0.0;
        bool cut = false;
        for (int j = 0; j < P; ++j) {
            const double aj = li ? sm.Ac[j][lr] : 0.0;
            const double s2 = wave_sum_dpp(aj * aj);
            if (!(sqrt(s2) > SVD_REL * smax)) {
                cut = true;
                continue;
            }
            const double cj = wave_sum_dpp(aj * ry) / s2;
            if (li) bi += sm.Vc[j][lane] * cj;
        }
        const double cs = li ? sm.bv[lane] : 1.0;   // this lane's column factor (read before the slopes go there)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (li) sm.bv[lane] = bi;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double fit = 0.0;
        if (li)
            for (int j = lane; j < P; ++j) fit += R[lane][j] * sm.bv[j];
        const double e = li ? ry - fit : 0.0;
        const double ssr = wave_sum_dpp(e * e) + rho * rho;
        const double tss = wave_sum_dpp((li && lane >= 1) ? ry * ry : 0.0) + rho * rho;
        const int64_t ro = ((int64_t)s * fx.nprob + p) * (fx.pmax + 2);
        if (li) fx.rec[ro + lane] = bi * cs;
        if (lane == 0) {
            fx.rec[ro + fx.pmax] = 1.0 - ssr / tss;
            const uint32_t st = fx.status[(int64_t)s * fx.nprob + p];
            fx.status[(int64_t)s * fx.nprob + p] = (st & ~FM_ST_RANK_DEF) | (cut ? FM_ST_RANK_DEF : 0u);
        }
    }
}

// statsmodels fix-ups after fm_solve, one workgroup per flagged (month, problem):
// CONST_SUSPECT (with check_const) -> const_pair; FITTED|INF_IN_Y -> infy_pair;
// FITTED|REFIT (no inf) -> refit_pair.
template <int NC, int NT>
union FixSmem {
    InfySmem infy;
    RefitSmem<NC, NT / WAVE> refit;
    uint64_t red[NT / WAVE];
};
inline __device__ bool fix_wanted(uint32_t st, int check_const) {
    return (check_const && (st & FM_ST_CONST_SUSPECT)) ||
           ((st & FM_ST_FITTED) && (st & (FM_ST_INF_IN_Y | FM_ST_REFIT)));
}
// The fix-ups of one flagged (month, problem) whose solve status is `st`, by the whole
// NT-thread workgroup (block-uniform; ends with the workgroup synchronized)
template <int NC, int NT, class CA>
__device__ __forceinline__ void fix_one(int s, int p, uint32_t st, FixSmem<NC, NT>& sm, const FixCtx<CA>& fx) {
    if (fx.check_const && (st & FM_ST_CONST_SUSPECT)) {
        const_pair<NT>(s, p, sm.red, fx);
        __syncthreads();
    }
    if (!(st & FM_ST_FITTED)) return;
    if (st & FM_ST_INF_IN_Y) {
        infy_pair<NT, NC>(s, p, sm.infy, fx);
    } else if ((st & FM_ST_REFIT) && !(st & FM_ST_INF_IN_X) && fx.prob_nz[p] <= NC) {
        refit_pair<NC, NT>(s, p, sm.refit, fx);
    } else {
        return;
    }
    __syncthreads();   // sm is reused by the next pair
}

// ---------------------------------------------------------------------------------------
// zw == 16 (<= 15 panel columns): four problems per wave.  A problem owns one 16-lane row of
// the wave and lane i holds row i of its Gram (row 0 = the intercept, rows 1..K+1 = the
// centered moments S of x_1..x_K, y), so the pivot-row broadcasts of the Cholesky are DPP
// row_newbcast moves (VALU modifiers: no LDS round trip, no readlane hazards) and four
// factorizations run in the time of one.  Rank-deficient problems (rare) take the Jacobi
// pseudo-inverse path one at a time.

// 1 / sqrt(x) for a positive x: v_rsq_f64 refined by two Newton steps.  As the compiler's own
// sqrt lowering does, an x below 2^-767 is scaled by 2^768 first and the result by 2^384 (both
// exact), so the estimate and the steps' 0.5 * x never work on a subnormal.  v_ldexp_f64 by 0
// changes nothing, so every x >= 2^-767 keeps its bits.
__device__ __forceinline__ double rsq_nr(double x) {
    const int e = x < 0x1p-767 ? 768 : 0;
    const double xs = __builtin_ldexp(x, e);
    double y = __builtin_amdgcn_rsq(xs);
    const double h = 0.5 * xs;
    y = y * fma(-h * y, y, 1.5);
    y = y * fma(-h * y, y, 1.5);
    return __builtin_ldexp(y, e >> 1);
}

template <int L>
__device__ __forceinline__ int rowbc_i(int v) {   // lane L of this lane's 16-lane row
    // every lane has a source (row_newbcast): mov_dpp needs no zero-initialised destination
    return __builtin_amdgcn_mov_dpp(v, 0x150 + L, 0xF, 0xF, true);
}
template <int L>
__device__ __forceinline__ double rowbc(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)rowbc_i<L>((int)(uint32_t)b), hi = (uint32_t)rowbc_i<L>((int)(uint32_t)(b >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double rowsum(double v) { return row16_sum(v); }

constexpr int G16 = 16;   // lanes per problem
constexpr int Z16 = G16 * (G16 + 1) / 2;   // packed z-space Gram of the 16-wide solve
constexpr int TT = G16 * (G16 + 1);        // one transpose tile (row stride 17)

// Packed z-space offsets of row i of a problem's Gram: entry (z_i, z_j), j = 0..NJ-1, of the
// 16 lanes of the problem's row (they depend on the problem's z map only)
template <int NJ>
__device__ __forceinline__ void gram_offsets(int zi, int (&off)[NJ]) {
    static_for<0, NJ>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const int zj = rowbc_i<j>(zi);
        const int r = zi < zj ? zi : zj, c = zi < zj ? zj : zi;
        off[j] = r * G16 - (r * (r - 1)) / 2 + (c - r);
    });
}

// The month's level-cumulative bucket sums and the patterns' model sets (LDS)
struct Buckets16 {
    const double* bs;
    const uint32_t* pat;
    int npat, nl;
};

// Row i (its first NJ columns) of the Gram of problem (model m, level u): one level-cumulative
// bucket per pattern with m, from 0.0 in ascending pattern order.  A pattern's NJ LDS reads are
// issued together and waited for once (left to the compiler, each read was followed by its own
// wait: NJ round trips per pattern on the wave's chain).
template <int NJ>
__device__ __forceinline__ void gram_row(const Buckets16& B, int m, int u, int zi, double (&G)[NJ]) {
    int off[NJ];
    gram_offsets<NJ>(zi, off);
#pragma unroll
    for (int j = 0; j < NJ; ++j) G[j] = 0.0;
    for (int q = 0; q < B.npat; ++q) {
        if (!((B.pat[q] >> m) & 1u)) continue;   // per problem
        const double* bq = B.bs + (q * B.nl + u) * Z16;
        double v[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[j] = bq[off[j]];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) G[j] += v[j];   // columns past the problem's: unused
    }
}

// One wave slot's problem (a 16-lane row of the wave) and what its factorization leaves
struct Slot16 {
    int s, pp, m, u, K, zi;   // month, problem, its model and level, regressors, z index of this lane's row
    bool live;
    int flags;
};
struct Fact16 {
    double n, mu, sii, sxy, t;   // t: lane i's slope of x_{i-1} where ok
    bool act0, ok, illc;
    uint32_t st;
};

// Gram rows -> centered moments -> augmented Cholesky -> back substitution of a wave's four
// problems, for waves whose largest K is at most KW: every loop runs to the constant, so the
// body is straight-line code.  Columns and pivots past a problem's own K are computed and
// never read (as for a K = 7 problem beside three K = 14 ones), so a wave may take any bound
// >= its largest K.
template <int KW>
__device__ __forceinline__ Fact16 factor16(const fm_solve_args& a, const Slot16& q, const Buckets16& B, double* T,
                                           uint32_t* t_st) {
    static_assert(KW >= 1 && KW <= G16 - 2, "factor16: 1..14 regressors");
    const int lane = lane_id(), g = lane >> 4, i = lane & 15;
    const int K = q.K, K1 = K + 1;
    double G[KW + 2];   // row i of the problem Gram
    gram_row<KW + 2>(B, q.m, q.u, q.zi, G);
    const double n = rowbc<0>(G[0]);
    const double ninv = 1.0 / n;   // one division per lane (centering below multiplies)
    // centered moments: lane i (1 <= i <= K1) holds S row r = i - 1, S[r][c] in row[c]
    const bool srow = i >= 1 && i <= K1;
    double row[KW + 1];
    double sii = 0.0, sxy = 0.0, gdiag = 0.0;
    static_for<0, KW + 2>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        gdiag = i == j ? G[j] : gdiag;   // selects, not conditional stores (see below)
    });
    static_for<0, KW + 1>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const double g0j = rowbc<0>(G[j + 1]);   // G[0][j+1]
        const double c = G[j + 1] - G[0] * g0j * ninv;
        const double v = (srow & (j < K1)) ? c : 0.0;
        row[j] = v;
        // conditional assignments to these per-lane scalars were merged by the
        // compiler into a store through a selected address, which kept them in
        // scratch memory; plain selects keep them in registers
        sii = i == j + 1 ? v : sii;
        sxy = j == K ? v : sxy;
    });
    FM_PROBE_AT(solve, 4);
    const double mu = G[0] * ninv;   // lane i: mean of its variable
    const uint64_t gm = 0xFFFFull << (16 * g);
    uint32_t st = 0;
    if ((__ballot(i >= 1 && i <= K && isinf(gdiag)) & gm) != 0) st |= FM_ST_INF_IN_X;
    if ((__ballot(i == K1 && isinf(gdiag)) & gm) != 0) st |= FM_ST_INF_IN_Y;
    const int rs = a.pmax + 2;
    const int64_t ro = ((int64_t)q.s * a.nprob + q.pp) * rs;
    const bool skip = !(n >= (double)(K + 1));
    if (q.live && skip) {
        write_failed_rec(a.rec, ro, rs, a.pmax, n, i, G16);
        if (i == 0) a.status[(int64_t)q.s * a.nprob + q.pp] = t_st[q.pp] = FM_ST_SKIPPED;
    }
    const bool act0 = q.live && !skip;
    if (act0 && a.moments) {
        double* mo = a.moments + ((int64_t)q.s * a.nprob + q.pp) * a.mom_stride;
        if (i == 0) mo[0] = n;
        if (srow) {
            mo[i] = mu;   // mo[1 + r]
            // S is exactly symmetric (S[r][c] and S[c][r] are the same products of the
            // same packed sums), so lane r stores column r of S: S[c][r] for every c, and
            // each store instruction writes K1 consecutive doubles (a row-per-lane store
            // strides K1 doubles between lanes)
#pragma unroll
            for (int c = 0; c < KW + 1; ++c)
                if (c < K1) mo[1 + K1 + c * K1 + (i - 1)] = row[c];
        }
    }
    if (act0 && (q.flags & 1) != 0) {
        if ((__ballot(i >= 1 && i <= K && !(sii > 1e-10 * gdiag)) & gm) != 0) st |= FM_ST_CONST_SUSPECT;
    }
    FM_PROBE_AT(solve, 5);
    // ---- augmented Cholesky of S (pivot r = k sits in lane k + 1)
    bool ok = act0;
    // a regressor whose sum of squares lost its bits to the subnormal range: refit from the rows
    int illc = (act0 && (__ballot(i >= 1 && i <= K && sii > 0.0 && sii < TINY_SS) & gm) != 0) ? 1 : 0;
    const int tr = i >= 1 ? i - 1 : G16 - 1;   // this lane's tile row (lane 0: the spare last row)
    double dinv = 0.0;   // lane k + 1: 1 / L[k][k] (the back substitution multiplies by it)
    static_for<0, KW>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const bool act = ok & (k < K);
        const double orig = rowbc<k + 1>(sii);
        const double piv = rowbc<k + 1>(row[k]);
        illc |= (act & !(piv > REFIT_REL * orig)) ? 1 : 0;
        // pinned here: left to the end of the factorization (its only use), the test would
        // keep every step's pivot and diagonal live
        asm volatile("" : "+v"(illc));
        const bool bad = act & (!(orig > 0.0) | !(piv > CHOL_REL * orig));
        ok = ok & !bad;
        const bool go = act & !bad;
        // 1 / sqrt(piv) by the hardware estimate and two Newton steps (error ~1 ulp), sqrt
        // as piv times it: no IEEE sqrt and division sequences on the pivot chain
        const double rinv = rsq_nr(piv);
        const double lkk = piv * rinv;
        const double lik = row[k] * rinv;
        // unguarded: the entries a guard would keep are never read again -- columns past
        // the problem's K (and, once k >= K, everything this step touches) are not used by
        // the back substitution, and a problem whose pivot failed is refactored from G by
        // the Jacobi path -- so the two selects per entry are not needed
        static_for<k + 1, KW + 1>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const double sj = rowbc<k + 1>(row[j]) * rinv;   // L[j][k] = S(k)[k][j] / lkk
            row[j] = row[j] - lik * sj;
        });
        row[k] = go ? (i == k + 1 ? lkk : lik) : row[k];
        dinv = i == k + 1 ? rinv : dinv;
        // column k of the factor is final: to its transpose tile now (frees its registers);
        // unguarded, lanes outside the problem's rows write tile rows that are never read
        T[tr * (G16 + 1) + k] = row[k];
    });
    FM_PROBE_AT(solve, 6);
    // ---- back substitution L' b = l on the transposed factor: lane i then holds
    // column r = i - 1 of L (col[c] = L[c][r]) and t = l_r
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double col[KW];
    const int rr = i >= 1 ? i - 1 : 0;
#pragma unroll
    for (int c = 0; c < KW; ++c) col[c] = T[c * (G16 + 1) + rr];
    double t = (i >= 1 && i <= K) ? T[K * (G16 + 1) + rr] : 0.0;
    static_for<0, KW>([&](auto jc) {
        constexpr int j = KW - 1 - decltype(jc)::value;   // descending
        const double bj = rowbc<j + 1>(t) * rowbc<j + 1>(dinv);   // t_j / L[j][j]
        const double tm = t - col[j] * bj;
        const double tn = i == j + 1 ? bj : (((i >= 1) & (i - 1 < j)) ? tm : t);
        t = (ok & (j < K)) ? tn : t;
    });
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    FM_PROBE_AT(solve, 7);
    return Fact16{n, mu, sii, sxy, t, act0, ok, illc != 0, st};
}

// 192 threads (three waves, twelve problems at a time: a Table-2 month's 11 problems in ONE
// round, so no wave factors twice) at two waves per SIMD: 256 VGPRs (the factorization's
// register rows and columns fit without spills); every month of a 600-month panel is
// resident at once.
constexpr int S16T = 192;
constexpr int S16W = S16T / WAVE;
constexpr int S16_MAXP = 32;   // problems per group held in LDS tables
__global__ __launch_bounds__(S16T, 3) void solve16_kernel(fm_solve_args a) {
    extern __shared__ double bs[];   // [nb][136] packed bucket sums of this month
    // per wave: four transpose tiles, or (afterwards, one problem at a time) the Jacobi
    // fallback's scratch (a union)
    static_assert(sizeof(WaveScratch<16>) <= 4 * TT * sizeof(double), "scratch union");
    __shared__ double wsc[S16W][4 * TT];
    static_assert(sizeof(FixSmem<G16, S16T>) <= sizeof(wsc), "solve16's inline fix-ups reuse its per-wave scratch");
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    constexpr int zz = Z16;
    const int nl = a.nlevels, npat = a.npatterns, nb = npat * nl;
    // The small per-problem tables and this month's add-back values go to LDS first, all
    // loads issued together with the partials' (read in place, each would be a dependent
    // memory round trip inside the problem loop)
    __shared__ int t_model[S16_MAXP], t_level[S16_MAXP], t_nz[S16_MAXP], t_flags[S16_MAXP];
    __shared__ int t_slot[S16_MAXP];   // wave slot -> problem, by descending K
    __shared__ uint32_t t_st[S16_MAXP];   // the month's solve status (inline fix-ups)
    __shared__ uint8_t t_z[S16_MAXP][32];
    __shared__ uint32_t t_pat[64];
    __shared__ double t_ab[32];
    for (int e = tid; e < a.nprob * 32; e += S16T) t_z[e >> 5][e & 31] = (uint8_t)a.prob_z[e];
    if (tid < a.nprob) {
        t_model[tid] = a.prob_model[tid];
        t_level[tid] = a.prob_level[tid];
        const int nzp = a.prob_nz[tid];
        t_nz[tid] = nzp;
        t_flags[tid] = a.prob_flags[tid];
        // Problems go to wave slots by descending K (ties: index order): the factorization
        // loops run to a bound on the largest K of the wave's four problems, so grouping
        // similar K cuts the issued work (Table 2: 3 x K 14, 3 x 7, 2 x 5, 3 x 3 per month)
        int rank = 0;
        for (int q = 0; q < a.nprob; ++q) {
            const int nzq = a.prob_nz[q];
            rank += (nzq > nzp || (nzq == nzp && q < tid)) ? 1 : 0;
        }
        t_slot[rank] = tid;
    }
    if (tid < npat) t_pat[tid] = a.pattern_models[tid];
    if (a.add_back && tid >= 64 && tid < 96) {
        const int c = tid - 64;   // panel columns past ncols are never indexed
        t_ab[c] = c < a.ab_ncols ? a.add_back[(int64_t)c * a.nseg + s] : 0.0;
    }
    FM_PROBE_AT(solve, 0);
    const int c0 = a.seg_chunk_off[s], c1 = a.seg_chunk_off[s + 1];
    sum_partials<S16T>(a.partial, c0, c1, nb * zz, bs);
    __syncthreads();
    FM_PROBE_AT(solve, 1);
    for (int e = tid; e < npat * zz; e += S16T) {   // level-cumulative buckets
        const int pid = e / zz, f = e - pid * zz;
        double* b0 = bs + (int64_t)pid * nl * zz + f;
        double run = b0[(nl - 1) * zz];
        for (int l = nl - 2; l >= 0; --l) {
            run += b0[l * zz];
            b0[l * zz] = run;
        }
    }
    __syncthreads();
    const Buckets16 B{bs, t_pat, npat, nl};
    const int g = lane >> 4, i = lane & 15;
    const int rs = a.pmax + 2;
    double* T = wsc[w] + g * TT;
    FM_PROBE_AT(solve, 2);
    for (int p0 = w * 4; p0 < a.nprob; p0 += S16W * 4) {
        const int p = p0 + g;
        const bool live = p < a.nprob;
        const int pp = t_slot[live ? p : p0];
        const int m = t_model[pp], u = t_level[pp], nz = t_nz[pp];
        const int K = nz - 2;
        const int zi = i < nz ? t_z[pp][i] : 0;   // z index of this lane's row
        const Slot16 sl{s, pp, m, u, K, zi, live, t_flags[pp]};
        // One instantiation per column bound, chosen once per wave on the largest K of its
        // problems (slots by descending K: the first live slot's): the Table-2 values
        const int kw = __builtin_amdgcn_readfirstlane(K);
        Fact16 F;
        if (kw <= 3) F = factor16<3>(a, sl, B, T, t_st);
        else if (kw <= 5) F = factor16<5>(a, sl, B, T, t_st);
        else if (kw <= 7) F = factor16<7>(a, sl, B, T, t_st);
        else F = factor16<14>(a, sl, B, T, t_st);
        const double n = F.n, mu = F.mu, sii = F.sii, sxy = F.sxy;
        const bool act0 = F.act0, ok = F.ok;
        uint32_t st = F.st;
        const int K1 = K + 1;
        const int64_t ro = ((int64_t)s * a.nprob + pp) * rs;
        // lanes of a live, unskipped problem with a collapsed pivot: rank deficient
        const bool rank_def = act0 && !ok;
        double bi = (ok && i >= 1 && i <= K) ? F.t : 0.0;   // slope of x_{i-1}
        // ---- rank-deficient problems of this wave: Jacobi pseudo-inverse, one at a time.
        // G is read again from the buckets instead of kept (and its offsets) live through the
        // factorization
        const uint64_t rd = __ballot(rank_def && i == 0);
        double G2[G16];
        if (rd) gram_row<G16>(B, m, u, zi, G2);   // wave-uniform
        for (uint64_t q = rd; q; q &= q - 1) {
            const int gq = __builtin_ctzll(q) >> 4;   // wave-uniform
            WaveScratch<16>& J = *reinterpret_cast<WaveScratch<16>*>(wsc[w]);
            const int Kq = __shfl(K, gq * 16, WAVE);
            const double (&G)[G16] = G2;
            // rebuild Sxx (rows were overwritten) from G, the shuffles with every lane active
            {
                double g0c[G16 - 1];
#pragma unroll
                for (int c = 0; c < G16 - 1; ++c) g0c[c] = __shfl(G[c + 1], gq * 16, WAVE);
                const double nq = __shfl(n, gq * 16, WAVE);
                if (g == gq && i >= 1 && i <= Kq) {
#pragma unroll
                    for (int c = 0; c < G16 - 1; ++c)
                        if (c < Kq) J.A[(i - 1) * 16 + c] = G[c + 1] - G[0] * g0c[c] / nq;
                    J.sxy[i - 1] = sxy;
                }
                if (g == gq && i >= 1 && i <= Kq + 1)   // raw means of x_0..x_{K-1}, y
                    J.mu[i - 1] = mu + (a.add_back ? t_ab[zi - 1] : 0.0);
            }
            wave_sync();
            if (lane == 0) jacobi_pinv<16>(J.A, J.V, Kq, J.sxy, J.mu, J.b);
            wave_sync();
            if (g == gq && i >= 1 && i <= Kq) bi = J.b[i - 1];
            wave_sync();
        }
        if (rank_def) st |= FM_ST_RANK_DEF;
        if (F.illc) st |= FM_ST_REFIT;
        // ---- R^2 = 1 - SSR/SST (centered), raw-coordinate intercept
        const bool xl = i >= 1 && i <= K;
        double t_sxy = xl ? bi * sxy : 0.0;
        double t_mu = xl ? bi * mu : 0.0;
        double t_abx = 0.0;
        if (a.add_back && xl && act0) t_abx = bi * t_ab[zi - 1];
        t_sxy = rowsum(t_sxy);
        t_mu = rowsum(t_mu);
        t_abx = rowsum(t_abx);
        const double syy = __shfl(sii, g * 16 + (K1 < 16 ? K1 : 15), WAVE);   // S[K][K]
        const double muy = __shfl(mu, g * 16 + (K1 < 16 ? K1 : 15), WAVE);
        const double r2 = 1.0 - (syy - t_sxy) / syy;
        double icpt = muy - t_mu;
        if (a.add_back && act0) {
            const int zy = t_z[pp][K + 1];
            icpt += t_ab[zy - 1] - t_abx;
        }
        if (act0) {
            // write_fitted_rec's layout, in this kernel's own text: through the helper (one select
            // fewer per entry) the kernel spills four more registers
            for (int k = i; k < rs; k += G16) {
                double v = NAN;   // pad between the slopes and R^2
                if (k == 0) v = icpt;
                else if (k <= K) v = k == i ? bi : NAN;   // k == i on the first pass
                else if (k == a.pmax) v = r2;
                else if (k == a.pmax + 1) v = n;
                a.rec[ro + k] = v;
            }
            if (i == 0) a.status[(int64_t)s * a.nprob + pp] = t_st[pp] = st | FM_ST_FITTED;
        }
    }
    FM_PROBE_AT(solve, 3);
    // the statsmodels fix-ups of this month's flagged problems (fm_solve_fixup's work, rare),
    // by this workgroup: its own rec / moments / status writes are visible after the barrier
    // the rows come from the FP64 columns, else (a planes-only panel) from the two planes: one
    // instantiation per layout (a per-access branch raised the kernel to 231 VGPRs)
    auto fix_all = [&](auto cols) {
        __syncthreads();
        const FixCtx<decltype(cols)> fx = fix_ctx(a, cols);
        for (int q = 0; q < a.nprob; ++q) {
            const uint32_t st = t_st[q];
            if (!fix_wanted(st, fx.check_const)) continue;   // block-uniform
            fix_one<G16, S16T>(s, q, st, *reinterpret_cast<FixSmem<G16, S16T>*>(&wsc[0][0]), fx);
        }
    };
    if (a.fix_cols != nullptr) fix_all(F64Cols{a.fix_cols});   // block-uniform
    else if (a.fix_hi_plane != nullptr) fix_all(PlaneCols{a.fix_hi_plane, (int64_t)(a.fix_lo_plane - a.fix_hi_plane)});
}

template <int NC>
__global__ __launch_bounds__(VT) void fixup_kernel(FixCtx<F64Cols> fx) {
    __shared__ FixSmem<NC, VT> sm;
    // Every (month, problem) is scanned for the flags (no host round trip).  Each workgroup
    // reads VT status words at once and lists the flagged pairs in LDS (a pair-by-pair scan
    // would wait out one memory round trip per pair), then fixes them.
    __shared__ int flagged[VT];
    __shared__ int nflag;
    const int total = fx.nseg * fx.nprob;
    const int tid = threadIdx.x;
    FM_PROBE_AT(solve, 4);
    for (int base = blockIdx.x * VT; base < total; base += gridDim.x * VT) {
        if (tid == 0) nflag = 0;
        __syncthreads();
        {
            const int e = base + tid;
            if (e < total && fix_wanted(fx.status[e], fx.check_const)) flagged[atomicAdd(&nflag, 1)] = e;
        }
        __syncthreads();
        const int nf = nflag;
        for (int f = 0; f < nf; ++f) {
            const int sp = flagged[f];
            const int s = sp / fx.nprob, p = sp - s * fx.nprob;
            fix_one<NC, VT>(s, p, fx.status[sp], sm, fx);
        }
        __syncthreads();   // the list is rebuilt for the next range
    }
    FM_PROBE_AT(solve, 5);
}

// What the inline fix-ups of fm_solve and fm_solve_fixup both ask of the fix_* arguments
int check_fix_args(const fm_solve_args& a, const char* who) {
    FM_REQUIRE(a.fix_seg_off != nullptr, "%s: fix_seg_off is NULL", who);
    FM_REQUIRE(a.moments != nullptr, "%s: the fix-ups need moments", who);
    FM_REQUIRE((a.fix_lo == nullptr) == (a.fix_hi == nullptr), "%s: fix_lo and fix_hi go together", who);
    FM_REQUIRE(a.fix_inv_scale == nullptr || a.fix_shift != nullptr, "%s: fix_inv_scale needs fix_shift", who);
    FM_REQUIRE(a.pmax >= 2 && a.pmax <= 32, "%s: pmax must be 2..32", who);
    return FM_OK;
}

}  // namespace
}  // namespace fm

extern "C" int fm_solve(const fm_solve_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_solve: null args");
    const fm_solve_args& a = *args;
    FM_REQUIRE(a.partial && a.seg_chunk_off && a.pattern_models && a.prob_model && a.prob_level &&
                   a.prob_z && a.prob_nz && a.prob_flags && a.rec && a.status,
               "fm_solve: null pointer");
    FM_REQUIRE(a.zw == 16 || a.zw == 32, "fm_solve: zw must be 16 or 32");
    FM_REQUIRE(a.npatterns * a.nlevels * (a.zw * (a.zw + 1) / 2) <= MAXB_LDS,
               "fm_solve: %d buckets of a %d-wide Gram exceed the LDS budget", a.npatterns * a.nlevels, a.zw);
    FM_REQUIRE(a.pmax >= 2 && a.pmax <= 32, "fm_solve: pmax must be 2..32");
    FM_REQUIRE(a.moments == nullptr || a.mom_stride > 0, "fm_solve: bad mom_stride");
    FM_REQUIRE(a.add_back == nullptr || (a.ab_ncols >= 1 && a.ab_ncols <= FM_MAX_COLS),
               "fm_solve: add_back needs ab_ncols in 1..%d", FM_MAX_COLS);
    FM_REQUIRE(a.zw == 32 || a.nprob <= S16_MAXP, "fm_solve: at most %d problems per group", S16_MAXP);
    FM_REQUIRE((a.fix_hi_plane == nullptr) == (a.fix_lo_plane == nullptr),
               "fm_solve: fix_hi_plane and fix_lo_plane go together");
    if (a.fix_cols != nullptr || a.fix_hi_plane != nullptr) {
        FM_REQUIRE(a.zw == 16 && a.pmax + 1 <= 16, "fm_solve: inline fix-ups need zw 16 and pmax <= 15");
        if (const int rc = check_fix_args(a, "fm_solve")) return rc;
    }
    if (a.nseg == 0 || a.nprob == 0) return FM_OK;
    const size_t dyn = (size_t)a.npatterns * a.nlevels * (a.zw * (a.zw + 1) / 2) * sizeof(double);
    const int rc = a.zw == 16 ? raise_dynamic_lds<solve16_kernel>(MAXB_LDS * sizeof(double), "fm_solve")
                              : raise_dynamic_lds<solve_kernel<32>>(MAXB_LDS * sizeof(double), "fm_solve");
    if (rc != FM_OK) return rc;
    if (a.zw == 16)
        hipLaunchKernelGGL(solve16_kernel, dim3(a.nseg), dim3(S16T), dyn, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(solve_kernel<32>, dim3(a.nseg), dim3(VT), dyn, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_solve");
    return FM_OK;
}

extern "C" int fm_solve_fixup(const fm_solve_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_solve_fixup: null args");
    const fm_solve_args& a = *args;
    FM_REQUIRE(a.fix_hi_plane == nullptr && a.fix_lo_plane == nullptr, "fm_solve_fixup: FP64 columns only (a plane is set)");
    FM_REQUIRE(a.fix_cols && a.prob_level && a.prob_z && a.prob_nz && a.rec && a.status, "fm_solve_fixup: null pointer");
    if (const int rc = check_fix_args(a, "fm_solve_fixup")) return rc;
    const int64_t work = (int64_t)a.nseg * a.nprob;
    if (work == 0) return FM_OK;
    const int64_t ranges = (work + VT - 1) / VT;   // VT pairs per workgroup pass
    const int grid = (int)(ranges < SCAN_GRID ? ranges : SCAN_GRID);
    const FixCtx<F64Cols> fx = fix_ctx(a, F64Cols{a.fix_cols});
    if (a.pmax + 1 <= 16)
        hipLaunchKernelGGL(fixup_kernel<16>, dim3(grid), dim3(VT), 0, (hipStream_t)stream, fx);
    else
        hipLaunchKernelGGL(fixup_kernel<32>, dim3(grid), dim3(VT), 0, (hipStream_t)stream, fx);
    FM_CHECK_LAUNCH("fm_solve_fixup");
    return FM_OK;
}
