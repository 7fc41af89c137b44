// fm_pool: pooled panel OLS with classical, White, month-, firm- and two-way clustered covariances
// (build-defined extension A23; the definition is in fm_hip.h).
//
// Eight launches on the caller's stream, each a fixed-order reduction:
//   check   the firm codes of the range's months (in range, ascending) into bad[0];
//   pass<0> grid (month, problem): sum z and sum z z' of z = [1, clip(x) - shift, clip(y) - shift];
//   means   per problem: N, G_t, the +-inf bits, the pooled (or, under month FE, the months') means:
//           the pivots of the next passes; a problem that is skipped or holds an inf ends here;
//   pass<1> the same sums about the pivots: the centred moments;
//   fit     per problem: the months' moments added in month order, Cholesky of Sxx, b, Sxx^-1, coef;
//   pass<2> per row e and u = [e, (x - piv) e]; per month sum u u' and sum u; the optional resid;
//   firm    grid (block of FM_POOL_FIRM_BLOCK codes, problem): the workgroup keeps its firms' score
//           sums in LDS and walks the months in order; codes ascend inside a month, so its rows of a
//           month are one run of at most 256 rows (two binary searches, made for 256 months at a
//           time, a month per thread), one row per thread, and no two rows of a month meet in one
//           slot.  Then sum_f s_f s_f' over its firms in code order, one partial per workgroup;
//   cov     per problem: months and firm blocks added in index order, the sandwiches, se, stat, status.
// The three passes are one piece of code: a wave's lanes hold one row each, compute the row's z (or
// u) and put it into the wave's LDS tile, unused rows marked; the tile is then added to the wave's
// 16 x 16 accumulator with sixteen v_mfma_f64_16x16x4_f64 (lane (k, q) holds column q of row k of a
// 4-row group; A = B = z).  Tile c of a month is wave c % 4's, the four waves are added in wave
// order.  What fm_wls.hip does the same way is in fm_reg16_dev.h: a problem's width and columns, a
// month's column parameters (ColPar), the accumulator epilogue.  pass<2> and firm compute a row's scores with the same function, so a firm that
// occurs once has the bits of its White term.
#include <math.h>

#include "fm_reg16_dev.h"

namespace fm {
namespace {

constexpr int PT = 256;                    // threads of a workgroup
constexpr int PNW = PT / WAVE;             // waves
constexpr int FB = FM_POOL_FIRM_BLOCK;

// workspace, in doubles
constexpr int REC = 288;                   // per (month, problem): [0, 256) the 16 x 16 sums, [256, 272) sum u, 272 the inf bits
constexpr int REC_VEC = 256, REC_FLAGS = 272;
constexpr int FIT = 320;                   // per problem
constexpr int FIT_B = 0;                   // [16] b by z index (1 .. K)
constexpr int FIT_A = 16;                  // [16][16] inverse of x~'x~ by z index (0: the intercept)
constexpr int FIT_M = 272;                 // [16] the pooled means by z index: the pivots
constexpr int FIT_MR = 296;                // [16] the same with what the pivots left of the first moments
constexpr int FIT_OK = 288, FIT_N = 289, FIT_GT = 290, FIT_SYY = 291, FIT_DOF = 292;
constexpr int FPART = 257;                 // per (problem, firm block): 16 x 16 partial meat, then the block's G_f

struct Ws {
    double* rec;    // [nseg][nprob][REC]
    double* piv;    // [nseg][nprob][16]
    double* fit;    // [nprob][FIT]
    double* fpart;  // [nprob][nblk][FPART]
    int nblk;
};
__host__ __device__ inline int pool_blocks(int nfirms) { return (nfirms + FB - 1) / FB; }
__host__ __device__ inline int64_t ws_doubles(int nseg, int nprob, int nfirms) {
    return (int64_t)nseg * nprob * (REC + 16) + (int64_t)nprob * FIT + (int64_t)nprob * pool_blocks(nfirms) * FPART;
}
__host__ __device__ inline Ws ws_of(const fm_pool_args& a) {
    Ws w;
    w.nblk = pool_blocks(a.nfirms);
    w.rec = (double*)a.ws;
    w.piv = w.rec + (int64_t)a.nseg * a.nprob * REC;
    w.fit = w.piv + (int64_t)a.nseg * a.nprob * 16;
    w.fpart = w.fit + (int64_t)a.nprob * FIT;
    return w;
}

// Row r of a month (a tile row holds z and, in slot ZW, whether the row is used): z[0] = 1, z[j] = clip(column j) - piv[j] for j < nz, 0 past the list.  Returns
// whether the row is used; *inf gets the FM_ST_INF_* bits of its clipped values.
__device__ __forceinline__ bool pool_row(const fm_pool_args& a, const int64_t* coff, const ColPar& cp, int nz, int u,
                                         int64_t r, double (&z)[ZW], uint32_t* inf) {
    bool use = a.level ? (int)a.level[r] >= u : true;
    uint32_t bits = 0;
    z[0] = 1.0;
#pragma unroll
    for (int j = 1; j < ZW; ++j) {
        double v = 0.0;
        if (j < nz) {
            const double x = a.cols[coff[j] + r];
            use = use && x == x;
            const double c = hw_min(hw_max(x, cp.lo[j]), cp.hi[j]);
            if (isinf(c)) bits |= j == nz - 1 ? FM_ST_INF_IN_Y : FM_ST_INF_IN_X;
            v = c - cp.piv[j];
        }
        z[j] = v;
    }
    *inf = bits;
    return use;
}
// z -> the scores u = [e, z_1 e .. z_K e, 0 ..] with e = z_y - sum_k b_k z_k (k ascending); returns e
__device__ __forceinline__ double pool_scores(const double* b, int nz, double (&z)[ZW]) {
    double acc = 0.0, zy = 0.0;
#pragma unroll
    for (int j = 1; j < ZW; ++j) {
        if (j < nz - 1) acc += b[j] * z[j];
        zy = j == nz - 1 ? z[j] : zy;
    }
    const double e = zy - acc;
    z[0] = e;
#pragma unroll
    for (int j = 1; j < ZW; ++j) z[j] = j < nz - 1 ? z[j] * e : 0.0;
    return e;
}

__global__ __launch_bounds__(PT) void pool_check_kernel(fm_pool_args a) {
    const int s = a.seg_lo + blockIdx.x;
    int64_t b0, b1;
    month_rows(a.seg_off, s, a.nrows, &b0, &b1);
    int n = 0;
    for (int64_t r = b0 + threadIdx.x; r < b1; r += PT) {
        const int f = a.firm[r];
        bool bad = f < 0 || f >= a.nfirms;
        if (r > b0) bad = bad || f <= a.firm[r - 1];
        n += bad ? 1 : 0;
    }
    n = wave_sum(n);
    if (lane_id() == 0 && n != 0) atomicAdd(a.bad, n);
}

struct PassLds {
    double tile[PNW * WAVE * RS];   // the waves' tiles; at the end their accumulator images
    ColPar cp;
    double b[ZW];
    int64_t coff[ZW];
    unsigned flags;
};
static_assert(2 * PNW * ZW * ZW <= PNW * WAVE * RS, "the accumulator images must fit the tiles");

// MODE 0: about `shift`; 1: about the pivots; 2: the scores
template <int MODE>
__global__ __launch_bounds__(PT) void pool_pass_kernel(fm_pool_args a) {
    __shared__ PassLds L;
    const Ws W = ws_of(a);
    const int s = a.seg_lo + blockIdx.x, p = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int q = lane & 15, kr = lane >> 4;
    const int nz = prob_width(a, p);
    const int u = a.prob_level[p];
    const int32_t* zi = a.prob_z + (int64_t)p * 32;
    int64_t b0, b1;
    month_rows(a.seg_off, s, a.nrows, &b0, &b1);
    const int64_t so = (int64_t)s * a.nprob + p;
    double* rec = W.rec + so * REC;
    const double* fit = W.fit + (int64_t)p * FIT;
    if (MODE != 0 && fit[FIT_OK] == 0.0) {   // block-uniform: not fitted
        if (MODE == 2 && a.resid)
            for (int64_t r = b0 + tid; r < b1; r += PT) a.resid[(int64_t)p * a.nrows + r] = NAN;
        return;
    }
    if (tid < ZW) {
        const int j = tid;
        L.coff[j] = col_offset(a, zi, j, nz) * a.col_stride;
        stage_col_par(a, zi, j, nz, s, MODE == 0 ? nullptr : W.piv + so * 16, L.cp);
        L.b[j] = MODE == 2 && j >= 1 && j < nz - 1 ? fit[FIT_B + j] : 0.0;
    }
    if (tid == 0) L.flags = 0;
    __syncthreads();

    d4 acc = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    double* tb = L.tile + w * (WAVE * RS);
    uint32_t inf = 0;
    for (int64_t r0 = b0 + (int64_t)w * WAVE; r0 < b1; r0 += PT) {   // tile c = (r0 - b0) / 64 is wave c % 4's
        const int64_t row = r0 + lane;
        const int64_t rc = row < b1 ? row : b1 - 1;
        double z[ZW];
        uint32_t bits;
        const bool use = pool_row(a, L.coff, L.cp, nz, u, rc, z, &bits) && row < b1;
        inf |= use ? bits : 0u;
        if (MODE == 2) {
            const double e = pool_scores(L.b, nz, z);
            if (a.resid && row < b1) a.resid[(int64_t)p * a.nrows + row] = use ? e : NAN;
        }
#pragma unroll
        for (int j = 0; j < ZW; ++j) tb[lane * RS + j] = z[j];
        tb[lane * RS + ZW] = use ? 1.0 : 0.0;
        wave_sync();
#pragma unroll 4
        for (int g = 0; g < WAVE / 4; ++g) {
            const int r = 4 * g + kr;
            const bool ok = tb[r * RS + ZW] != 0.0;
            const double v = ok ? tb[r * RS + q] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 0);
            if (MODE == 2) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ok && q == 0 ? 1.0 : 0.0, v, acc1, 0, 0, 0);
        }
        wave_sync();
    }
    if (MODE == 0) {
        inf = wave_or_u32(inf);
        if (lane == 0 && inf != 0) atomicOr(&L.flags, inf);
    }
    __syncthreads();   // every wave is done with its tile
    gram16_store_image(acc, L.tile, w, kr, q);
    if (MODE == 2 && kr == 0) L.tile[PNW * ZW * ZW + w * ZW + q] = acc1[0];   // D[0][q] = sum u_q
    __syncthreads();
    rec[tid] = gram16_sum_images<PNW>(L.tile, tid);
    if (MODE == 2 && tid < ZW) {
        double v = L.tile[PNW * ZW * ZW + tid];
#pragma unroll
        for (int x = 1; x < PNW; ++x) v += L.tile[PNW * ZW * ZW + x * ZW + tid];
        rec[REC_VEC + tid] = v;
    }
    if (MODE == 0 && tid == 0) rec[REC_FLAGS] = (double)L.flags;
}

// coef, se, cov of a problem that is not fitted; stat[0] = N, stat[1] = G_t
__device__ void pool_write_failed(const fm_pool_args& a, int p, double N, double Gt, uint32_t st) {
    const int tid = threadIdx.x, pm = a.pmax;
    for (int k = tid; k < pm; k += PT) a.coef[(int64_t)p * pm + k] = NAN;
    for (int k = tid; k < 5 * pm; k += PT) a.se[(int64_t)p * 5 * pm + k] = NAN;
    if (a.cov)
        for (int k = tid; k < 5 * pm * pm; k += PT) a.cov[(int64_t)p * 5 * pm * pm + k] = NAN;
    if (tid < 8) a.stat[(int64_t)p * 8 + tid] = tid == 0 ? N : (tid == 1 ? Gt : (tid == 7 ? 0.0 : NAN));
    if (tid == 0) a.status[p] = st;
}

__global__ __launch_bounds__(PT) void pool_means_kernel(fm_pool_args a) {
    __shared__ double m[ZW];
    __shared__ double sc[4];
    const Ws W = ws_of(a);
    const int p = blockIdx.x, tid = threadIdx.x;
    const int nz = prob_width(a, p), K = nz - 2;
    const int32_t* zi = a.prob_z + (int64_t)p * 32;
    double* fit = W.fit + (int64_t)p * FIT;
    if (tid < ZW) {   // thread j: column j's sum over the months, in month order
        const int j = tid;
        // (the shift by hand, not through col_par: inside this serial loop over the months the helper's
        // column lookup is not hoisted and the launch takes 156 us instead of 91)
        const int64_t c = col_offset(a, zi, j, nz);
        const bool col = j >= 1 && j < nz;
        double sum = 0.0, N = 0.0, Gt = 0.0;
        uint32_t fl = 0;
        for (int s = a.seg_lo; s < a.seg_hi; ++s) {
            const double* rec = W.rec + ((int64_t)s * a.nprob + p) * REC;
            const double nt = rec[0];
            const double sh = col && a.shift ? a.shift[c * a.nseg + s] : 0.0;
            N += nt;
            Gt += nt > 0.0 ? 1.0 : 0.0;
            sum += rec[j] + nt * sh;
            fl |= (uint32_t)rec[REC_FLAGS];
        }
        m[j] = col && N > 0.0 ? sum / N : 0.0;
        if (j == 0) {
            sc[0] = N;
            sc[1] = Gt;
            sc[2] = (double)fl;
        }
    }
    __syncthreads();
    const double N = sc[0], Gt = sc[1];
    const uint32_t fl = (uint32_t)sc[2];
    const double dof = a.month_fe ? N - K - Gt : N - K - 1;
    uint32_t st = 0;
    if (N < (double)(K + 2) || dof < 1.0) st = FM_ST_SKIPPED;
    else if (fl != 0) st = fl;
    if (tid < ZW) fit[FIT_M + tid] = m[tid];
    if (tid == 0) {
        fit[FIT_OK] = st == 0 ? 1.0 : 0.0;
        fit[FIT_N] = N;
        fit[FIT_GT] = Gt;
        fit[FIT_DOF] = dof;
    }
    if (st != 0) {
        pool_write_failed(a, p, N, Gt, st);
        return;
    }
    // the pivots of the next passes: the pooled means, or under month FE the month's own
    const int nm = a.seg_hi - a.seg_lo;
    for (int e = tid; e < nm * ZW; e += PT) {
        const int s = a.seg_lo + e / ZW, j = e % ZW;
        const int64_t so = (int64_t)s * a.nprob + p;
        double pv = m[j];
        if (a.month_fe) {
            const double* rec = W.rec + so * REC;
            const double nt = rec[0];
            const bool col = j >= 1 && j < nz;
            const double sh = col && a.shift ? a.shift[col_offset(a, zi, j, nz) * a.nseg + s] : 0.0;
            pv = col && nt > 0.0 ? sh + rec[j] / nt : 0.0;
        }
        W.piv[so * 16 + j] = pv;
    }
}

__global__ __launch_bounds__(PT) void pool_fit_kernel(fm_pool_args a) {
    __shared__ double S[ZW * ZW];    // centred moments by z index; Sxx is factorised in place
    __shared__ double Li[ZW * ZW];   // the factor's inverse
    __shared__ double b[ZW];
    __shared__ int fail;
    const Ws W = ws_of(a);
    const int p = blockIdx.x, tid = threadIdx.x;
    const int i = tid / ZW, j = tid % ZW;
    const int nz = prob_width(a, p), K = nz - 2, Y = nz - 1;
    double* fit = W.fit + (int64_t)p * FIT;
    if (fit[FIT_OK] == 0.0) return;
    const double N = fit[FIT_N];
    // entry (i, j) over the months in month order; what the pivots left of the first moments goes
    double sij = 0.0, g0i = 0.0, g0j = 0.0;
    for (int s = a.seg_lo; s < a.seg_hi; ++s) {
        const double* rec = W.rec + ((int64_t)s * a.nprob + p) * REC;
        const double nt = rec[0];
        if (a.month_fe) {
            if (nt > 0.0) sij += rec[tid] - rec[i] * rec[j] / nt;
        } else {
            sij += rec[tid];
            g0i += rec[i];
            g0j += rec[j];
        }
    }
    if (!a.month_fe) sij -= g0i * g0j / N;
    S[tid] = sij;
    if (tid == 0) fail = 0;
    __syncthreads();
    const bool inx = i >= 1 && i <= K && j >= 1 && j <= K;
    const double orig = S[i * ZW + i];   // before the factorisation
    const double syy = S[Y * ZW + Y];
    if (j == 0 && i >= 1 && i <= K) {
        const double mi = fit[FIT_M + i];
        if (!(orig > CONST_REL * (orig + N * mi * mi))) fail = 1;   // a constant column
    }
    __syncthreads();
    for (int k = 1; k <= K; ++k) {   // right-looking Cholesky of S[1..K][1..K], the lower triangle
        const double pk = S[k * ZW + k];
        __syncthreads();   // every thread holds the pivot
        const double lkk = sqrt(pk);
        if (i == k && j == k) {
            if (!(orig > 0.0 && pk > REFIT_REL * orig)) fail = 1;
            S[k * ZW + k] = lkk;
        }
        if (j == k && i > k && i <= K) S[i * ZW + k] = S[i * ZW + k] / lkk;
        __syncthreads();
        if (inx && i > k && j > k && j <= i) S[i * ZW + j] -= S[i * ZW + k] * S[j * ZW + k];
        __syncthreads();
    }
    if (fail) {
        __syncthreads();
        if (tid == 0) fit[FIT_OK] = 0.0;
        pool_write_failed(a, p, N, fit[FIT_GT], FM_ST_RANK_DEF);
        return;
    }
    // column c of the factor's inverse: thread c, forward substitution
    Li[tid] = 0.0;
    __syncthreads();
    if (tid >= 1 && tid <= K) {
        const int c = tid;
        for (int r = c; r <= K; ++r) {
            double v = r == c ? 1.0 : 0.0;
            for (int k = c; k < r; ++k) v -= S[r * ZW + k] * Li[k * ZW + c];
            Li[r * ZW + c] = v / S[r * ZW + r];
        }
    }
    __syncthreads();
    // A = Li' Li on the x block, 1 / N for the intercept of x~ (nothing under month FE)
    double aij = 0.0;
    if (inx)
        for (int k = (i > j ? i : j); k <= K; ++k) aij += Li[k * ZW + i] * Li[k * ZW + j];
    if (tid == 0 && !a.month_fe) aij = 1.0 / N;
    fit[FIT_A + tid] = aij;
    __syncthreads();
    if (tid < ZW) {   // b = A Sxy (column Y of S is untouched by the factorisation)
        double v = 0.0;
        if (tid >= 1 && tid <= K)
            for (int c = 1; c <= K; ++c) v += fit[FIT_A + tid * ZW + c] * S[c * ZW + Y];
        b[tid] = v;
        fit[FIT_B + tid] = v;
        // the means with what the pivots left of the first moments (thread j of row 0 summed it)
        fit[FIT_MR + tid] = !a.month_fe && tid >= 1 && tid <= Y ? fit[FIT_M + tid] + g0j / N : 0.0;
    }
    if (tid == 0) fit[FIT_SYY] = syy;
    __syncthreads();
    if (tid == 0) {
        double icpt = NAN;
        if (!a.month_fe) {
            double t = 0.0;
            for (int k = 1; k <= K; ++k) t += b[k] * fit[FIT_MR + k];
            icpt = fit[FIT_MR + Y] - t;
        }
        a.coef[(int64_t)p * a.pmax] = icpt;
    }
    if (tid >= 1 && tid < a.pmax) a.coef[(int64_t)p * a.pmax + tid] = tid <= K ? b[tid] : NAN;
}

struct FirmLds {
    double s[FB * RS];       // firm f0 + i's score sums
    int used[FB];
    ColPar cp[2];            // this month's and the next one's
    double b[ZW];
    int64_t coff[ZW];
    int run_lo[PT], run_n[PT];   // of a chunk of 256 months: the block's first row (from the month's first) and row count
};

__global__ __launch_bounds__(PT) void pool_firm_kernel(fm_pool_args a) {
    __shared__ FirmLds L;
    const Ws W = ws_of(a);
    const int blk = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const double* fit = W.fit + (int64_t)p * FIT;
    if (fit[FIT_OK] == 0.0) return;
    const int nz = prob_width(a, p), K1 = nz - 1;   // scores: K + 1 wide
    const int u = a.prob_level[p];
    const int32_t* zi = a.prob_z + (int64_t)p * 32;
    const int f0 = blk * FB;
    for (int e = tid; e < FB * RS; e += PT) L.s[e] = 0.0;
    L.used[tid] = 0;
    if (tid < ZW) {
        L.coff[tid] = col_offset(a, zi, tid, nz) * a.col_stride;
        L.b[tid] = tid >= 1 && tid < nz - 1 ? fit[FIT_B + tid] : 0.0;
    }
    auto stage = [&](int j, int s) {   // sixteen threads: month s's parameters into its slot
        stage_col_par(a, zi, j, nz, s, W.piv + ((int64_t)s * a.nprob + p) * 16, L.cp[(s - a.seg_lo) & 1]);
    };
    if (tid < ZW) stage(tid, a.seg_lo);
    for (int c0 = a.seg_lo; c0 < a.seg_hi; c0 += PT) {
        __syncthreads();   // the previous chunk's runs are consumed
        {
            const int s = c0 + tid;
            int lo = 0, n = 0;
            if (s < a.seg_hi) {
                int64_t b0, b1;
                month_rows(a.seg_off, s, a.nrows, &b0, &b1);
                const int64_t x0 = lower_bound(a.firm, b0, b1, f0);
                const int64_t x1 = lower_bound(a.firm, x0, b1, f0 + FB);
                const int64_t len = x1 - x0;
                lo = (int)(x0 - b0);
                n = (int)(len > FB ? FB : len);   // more than FB only where the codes do not ascend
            }
            L.run_lo[tid] = lo;
            L.run_n[tid] = n;
        }
        __syncthreads();
        const int cend = a.seg_hi - c0 < PT ? a.seg_hi - c0 : PT;
        for (int m = 0; m < cend; ++m) {
            const int s = c0 + m, slot = (s - a.seg_lo) & 1;
            if (tid >= PT - ZW && s + 1 < a.seg_hi) stage(tid - (PT - ZW), s + 1);   // the last sixteen threads: the next month
            if (tid < L.run_n[m]) {
                int64_t b0, b1;
                month_rows(a.seg_off, s, a.nrows, &b0, &b1);
                const int64_t r = b0 + L.run_lo[m] + tid;   // inside [b0, b1): the searches stay there
                const int f = a.firm[r] - f0;
                double z[ZW];
                uint32_t bits;
                const bool use = pool_row(a, L.coff, L.cp[slot], nz, u, r, z, &bits);
                if (use && (unsigned)f < (unsigned)FB) {
                    pool_scores(L.b, nz, z);
                    double* d = L.s + f * RS;
#pragma unroll
                    for (int j = 0; j < ZW; ++j)
                        if (j < K1) d[j] += z[j];
                    L.used[f] = 1;
                }
            }
            __syncthreads();   // a firm's slot may be another thread's next month
        }
    }
    __syncthreads();
    // sum_f s_f s_f' in code order: entry (i, j) per thread
    const int i = tid / ZW, j = tid % ZW;
    double acc = 0.0;
    int nf = 0;
    for (int f = 0; f < FB; ++f) {
        acc += L.s[f * RS + i] * L.s[f * RS + j];
        nf += L.used[f];
    }
    double* out = W.fpart + ((int64_t)p * W.nblk + blk) * FPART;
    out[tid] = acc;
    if (tid == 0) out[ZW * ZW] = (double)nf;
}

__global__ __launch_bounds__(PT) void pool_cov_kernel(fm_pool_args a) {
    __shared__ double M[4][ZW * ZW];   // the meats, then the covariances
    __shared__ double A[ZW * ZW], P1[ZW * ZW], mean[ZW];
    __shared__ unsigned neg;
    __shared__ double ssr_s;
    const Ws W = ws_of(a);
    const int p = blockIdx.x, tid = threadIdx.x;
    const int i = tid / ZW, j = tid % ZW;
    const double* fit = W.fit + (int64_t)p * FIT;
    if (fit[FIT_OK] == 0.0) return;
    const int nz = prob_width(a, p), K = nz - 2, pm = a.pmax;
    const double N = fit[FIT_N], Gt = fit[FIT_GT], dof = fit[FIT_DOF], syy = fit[FIT_SYY];
    const int lo = a.month_fe ? 1 : 0;   // the first coefficient that exists
    double mw = 0.0, mm = 0.0, mf = 0.0, gf = 0.0;
    for (int s = a.seg_lo; s < a.seg_hi; ++s) {
        const double* rec = W.rec + ((int64_t)s * a.nprob + p) * REC;
        mw += rec[tid];
        mm += rec[REC_VEC + i] * rec[REC_VEC + j];
    }
    for (int b = 0; b < W.nblk; ++b) {
        const double* fp = W.fpart + ((int64_t)p * W.nblk + b) * FPART;
        mf += fp[tid];
        gf += fp[ZW * ZW];
    }
    const double Gf = gf;
    A[tid] = fit[FIT_A + tid];
    if (tid < ZW) mean[tid] = tid >= 1 && tid <= K ? fit[FIT_MR + tid] : 0.0;
    if (tid == 0) {
        neg = 0;
        ssr_s = mw;
    }
    __syncthreads();
    const double SSR = ssr_s;   // sum e^2: entry (0, 0) of sum u u'
    const double s2 = SSR / dof;
    const bool in = i >= lo && i <= K && j >= lo && j <= K;
    M[0][tid] = 0.0;   // classical: s2 A, no sandwich
    M[1][tid] = in ? mw : 0.0;
    M[2][tid] = in ? mm : 0.0;
    M[3][tid] = in ? mf : 0.0;
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
        double v;
        if (k == 0) {
            v = s2 * A[tid];
        } else {
            double t = 0.0;
            for (int c = 0; c <= K; ++c) t += A[i * ZW + c] * M[k][c * ZW + j];
            P1[tid] = t;
            __syncthreads();
            v = 0.0;
            for (int c = 0; c <= K; ++c) v += P1[i * ZW + c] * A[c * ZW + j];
        }
        __syncthreads();
        M[k][tid] = v;
        __syncthreads();
        if (!a.month_fe) {   // back to the raw intercept: V = T V~ T', T = I but T[0][c] = -m_c
            double qv = M[k][tid];
            if (i == 0)
                for (int c = 1; c <= K; ++c) qv -= mean[c] * M[k][c * ZW + j];
            P1[tid] = qv;
            __syncthreads();
            double vv = P1[tid];
            if (j == 0)
                for (int c = 1; c <= K; ++c) vv -= P1[i * ZW + c] * mean[c];
            __syncthreads();
            M[k][tid] = vv;
            __syncthreads();
        }
    }
    const double p0 = K + 1;
    const double cw = a.small_sample ? N / (N - p0) : 1.0;
    const double cn = a.small_sample ? (N - 1.0) / (N - p0) : 1.0;
    const double cmn = Gt >= 2.0 ? (a.small_sample ? Gt / (Gt - 1.0) * cn : 1.0) : NAN;
    const double cfm = Gf >= 2.0 ? (a.small_sample ? Gf / (Gf - 1.0) * cn : 1.0) : NAN;
    double v[5];
    v[0] = M[0][tid];
    v[1] = M[1][tid] * cw;
    v[2] = M[2][tid] * cmn;
    v[3] = M[3][tid] * cfm;
    v[4] = v[3] + v[2] - v[1];
    for (int k = 0; k < 5; ++k) {
        const double x = in ? v[k] : NAN;
        if (a.cov && i < pm && j < pm) a.cov[(((int64_t)p * 5 + k) * pm + i) * pm + j] = x;
        if (i == j && i < pm) {
            double se = NAN;
            if (in) {
                if (k == 4) {
                    if (x > 0.0) se = sqrt(x);
                    else if (x == x) atomicOr(&neg, 1u);
                } else {
                    se = sqrt(x);
                }
            }
            a.se[((int64_t)p * 5 + k) * pm + i] = se;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double* st = a.stat + (int64_t)p * 8;
        st[0] = N;
        st[1] = Gt;
        st[2] = Gf;
        st[3] = 1.0 - SSR / syy;
        st[4] = SSR;
        st[5] = s2;
        st[6] = dof;
        st[7] = 0.0;
        a.status[p] = FM_ST_FITTED | (neg ? FM_ST_NEG_VAR : 0u);
    }
}

}  // namespace
}  // namespace fm

extern "C" int64_t fm_pool_ws_bytes(int32_t nseg, int32_t nprob, int32_t pmax, int32_t nfirms) {
    if (nseg < 0 || nprob < 0 || pmax < 0 || nfirms < 0) return -1;
    return fm::ws_doubles(nseg, nprob, nfirms) * (int64_t)sizeof(double);
}

extern "C" int fm_pool(const fm_pool_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_pool: null args");
    const fm_pool_args& a = *args;
    FM_REQUIRE(a.nseg >= 0 && a.nprob >= 0 && a.nrows >= 0, "fm_pool: negative size (nseg, nprob, nrows)");
    FM_REQUIRE(a.nfirms >= 0, "fm_pool: nfirms must not be negative, got %d", a.nfirms);
    FM_REQUIRE(a.ncols >= 1, "fm_pool: ncols must be at least 1, got %d", a.ncols);
    FM_REQUIRE(a.nprob <= 65535, "fm_pool: at most 65,535 problems per call");
    FM_REQUIRE(a.pmax >= 2 && a.pmax <= FM_POOL_MAX_K + 1, "fm_pool: pmax must be 2..%d (K <= %d), got %d",
               FM_POOL_MAX_K + 1, FM_POOL_MAX_K, a.pmax);
    FM_REQUIRE(a.seg_lo >= 0 && a.seg_lo <= a.seg_hi && a.seg_hi <= a.nseg,
               "fm_pool: seg_lo <= seg_hi inside [0, nseg] wanted, got [%d, %d) of %d", a.seg_lo, a.seg_hi, a.nseg);
    if (a.nseg == 0 || a.nprob == 0 || a.seg_lo == a.seg_hi) return FM_OK;
    FM_REQUIRE(a.cols != nullptr, "fm_pool: cols is NULL (FP64 columns are required; a planes-only panel is not supported)");
    FM_REQUIRE(a.seg_off && a.firm && a.bad, "fm_pool: null pointer (seg_off, firm and bad are required)");
    FM_REQUIRE(a.prob_level && a.prob_z && a.prob_nz, "fm_pool: null pointer (prob_level, prob_z and prob_nz are required)");
    FM_REQUIRE(a.coef && a.se && a.stat && a.status, "fm_pool: null pointer (coef, se, stat and status are required)");
    FM_REQUIRE(a.col_stride >= a.nrows, "fm_pool: col_stride must be at least nrows");
    FM_REQUIRE((a.lo == nullptr) == (a.hi == nullptr), "fm_pool: lo and hi come together");
    FM_REQUIRE(a.stage >= 0 && a.stage <= 8, "fm_pool: stage must be 0 (every launch) or 1..8, got %d", a.stage);
    const int64_t need = fm_pool_ws_bytes(a.nseg, a.nprob, a.pmax, a.nfirms);
    FM_REQUIRE(a.ws != nullptr && a.ws_bytes >= need, "fm_pool: ws must hold fm_pool_ws_bytes = %lld bytes, got %lld",
               (long long)need, (long long)(a.ws ? a.ws_bytes : 0));
    hipStream_t st = (hipStream_t)stream;
    const unsigned nm = (unsigned)(a.seg_hi - a.seg_lo), np = (unsigned)a.nprob;
    const int nblk = pool_blocks(a.nfirms);
    auto on = [&](int k) { return a.stage == 0 || a.stage == k; };
    if (on(1)) hipLaunchKernelGGL(pool_check_kernel, dim3(nm), dim3(PT), 0, st, a);
    if (on(2)) hipLaunchKernelGGL(pool_pass_kernel<0>, dim3(nm, np), dim3(PT), 0, st, a);
    if (on(3)) hipLaunchKernelGGL(pool_means_kernel, dim3(np), dim3(PT), 0, st, a);
    if (on(4)) hipLaunchKernelGGL(pool_pass_kernel<1>, dim3(nm, np), dim3(PT), 0, st, a);
    if (on(5)) hipLaunchKernelGGL(pool_fit_kernel, dim3(np), dim3(PT), 0, st, a);
    if (on(6)) hipLaunchKernelGGL(pool_pass_kernel<2>, dim3(nm, np), dim3(PT), 0, st, a);
    if (on(7) && nblk > 0) hipLaunchKernelGGL(pool_firm_kernel, dim3((unsigned)nblk, np), dim3(PT), 0, st, a);
    if (on(8)) hipLaunchKernelGGL(pool_cov_kernel, dim3(np), dim3(PT), 0, st, a);
    FM_CHECK_LAUNCH("fm_pool");
    return FM_OK;
}
