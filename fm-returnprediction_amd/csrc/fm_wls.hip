// fm_wls: weighted (WLS) monthly cross-sections (build-defined extension A22; the definition is in
// fm_hip.h).
//
// One workgroup of four waves per (month, problem).  The month is walked in blocks of 256 rows, a
// wave's lanes holding one row each.  A row that takes part (no NaN among the problem's columns,
// level, a finite weight > 0) is written to an LDS ring at its COMPACT index, its position among
// the month's used rows (ballot ranks + the four waves' counts), so the ring holds the used rows
// densely, in row order, as [w, x_1 .. x_K, y].  Compact rows are cut into tiles of 64; tile c is
// always wave c % 4's, which adds it to its 16 x 16 accumulator with sixteen v_mfma_f64_16x16x4_f64
// (A = w z of four rows, B = z of the same rows, z = [1, clip(x) - pivot]; lane (k, q) holds
// column q of row k, as in fm_gram_dev.h, and clips its own column at the operand).  The next
// block's loads are issued before the tiles are consumed.  At the end the four accumulators are
// added in wave order (fm_reg16_dev.h, which also holds how a problem's width, columns and column
// parameters are read and how a record is laid out: fm_pool.hip reads them the same way).  So every sum depends on the sequence of used rows alone: dropped rows leave
// no trace, and weights times a power of two scale every term exactly.
//
// Two such passes: the first, about `shift` (or 0), gives the weighted means; the second, about
// those means, the centred moments (the remaining first moments, rounding-sized, are still
// subtracted).  Both passes are one piece of code, the pivot apart.  Wave 0 then centres, factorises
// and back-substitutes as fm_solve's wide kernel does (lane i holds row i of the augmented matrix;
// pivot rows are broadcast by readlane), on the zero-padded 16 x 16 matrix with no test of the size.
#include <math.h>

#include "fm_reg16_dev.h"

namespace fm {
namespace {

constexpr int WLT = 256;                   // threads of a workgroup
constexpr int WNW = WLT / WAVE;            // waves
constexpr int RING_TILES = 5;              // < 64 compact rows left over + <= 256 new ones
constexpr int RING = RING_TILES * WAVE;

struct WlsLds {
    double ring[RING * RS];   // the used rows; after a pass the four waves' accumulator images
    double G[ZW * ZW];        // the pass's weighted Gram, waves added in order
    double piv[ZW];           // pivot of local column q: the shift, then the weighted mean
    double T[ZW * ZW];        // the factor's transpose (back substitution)
    int64_t coff[ZW];         // element offset of local column j's panel column
    int wcnt[WNW];
    unsigned flags;
};
static_assert(WNW * ZW * ZW <= RING * RS, "the accumulator images must fit the ring");

__global__ __launch_bounds__(WLT, 3) void wls_kernel(fm_wls_args a) {
    __shared__ WlsLds L;
    const int s = blockIdx.x, p = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int q = lane & 15, kr = lane >> 4;   // MFMA operand: column q of row kr of a 4-row group
    const int nz = prob_width(a, p);
    const int K = nz - 2, K1 = K + 1;
    const int u = a.prob_level[p];
    const int32_t* zi = a.prob_z + (int64_t)p * 32;
    int64_t b0, b1;
    month_rows(a.seg_off, s, a.nrows, &b0, &b1);
    // this lane's operand column: its cuts and the first pass's pivot, in registers
    const bool colq = q >= 1 && q < nz;
    const ColVal pq = col_par(a, zi, q, nz, s);
    const double plo = pq.lo, phi = pq.hi, psh = pq.shift;
    if (tid == 0) L.flags = 0;
    if (tid >= 1 && tid < ZW) L.coff[tid] = col_offset(a, zi, tid, nz) * a.col_stride;
    __syncthreads();
    const int rs = a.pmax + 2;
    const int64_t ro = ((int64_t)s * a.nprob + p) * rs;
    const int64_t so = (int64_t)s * a.nprob + p;

    // One pass over the month about the lanes' pivots: leaves the weighted Gram of z = [1, clip(x) -
    // piv] in L.G and returns the number of used rows.  INF: note +-inf among the used rows' values.
    auto run_pass = [&](const double piv, const bool INF) -> uint32_t {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        uint32_t total = 0, done = 0;   // compact rows staged, compact tiles consumed
        bool infl = false;
        double xv[ZW - 1], wv = 0.0;
        int lv = 0;
        auto load = [&](int64_t r0) {   // rows past the month's end re-read its last row (masked later)
            const int64_t row = r0 + w * WAVE + lane;
            const int64_t rc = row < b1 ? row : b1 - 1;
#pragma unroll
            for (int j = 1; j < ZW; ++j)
                xv[j - 1] = a.cols[L.coff[j] + rc];
            wv = a.weight[rc];
            lv = a.level ? (int)a.level[rc] : 255;
        };
        // tile c of the compact rows: sixteen 4-row groups; rows at or past `total` add zeros
        auto consume = [&](uint32_t c) {
            const double* tb = L.ring + (c % RING_TILES) * (WAVE * RS);
            const uint32_t left = total - c * WAVE;
#pragma unroll 4
            for (int g = 0; g < WAVE / 4; ++g) {
                const int r = 4 * g + kr;
                const double v = tb[r * RS + q], wg = tb[r * RS];
                const bool ok = (uint32_t)r < left;
                double z = q == 0 ? 1.0 : hw_min(hw_max(v, plo), phi) - piv;
                z = ok && q < nz ? z : 0.0;
                const double A = ok ? wg * z : 0.0;
                if (INF) infl = infl || isinf(z);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A, z, acc, 0, 0, 0);
            }
        };
        if (b1 > b0) load(b0);
        for (int64_t r0 = b0; r0 < b1; r0 += WLT) {
            const int64_t row = r0 + w * WAVE + lane;
            bool use = row < b1 && wv > 0.0 && wv < INFINITY && lv >= u;
#pragma unroll
            for (int j = 1; j < ZW; ++j)
                use = use && xv[j - 1] == xv[j - 1];
            const uint64_t m = __builtin_amdgcn_ballot_w64(use);
            if (lane == 0) L.wcnt[w] = __builtin_popcountll(m);
            __syncthreads();   // the counts; and every wave is done with the tiles it consumed
            int before = 0, all = 0;
#pragma unroll
            for (int i = 0; i < WNW; ++i) {
                const int c = L.wcnt[i];
                all += c;
                before += i < w ? c : 0;
            }
            if (use) {
                double* d = L.ring + ((total + (uint32_t)before + (uint32_t)mask_rank(m)) % RING) * RS;
                d[0] = wv;
#pragma unroll
                for (int j = 1; j < ZW; ++j)
                    d[j] = xv[j - 1];
            }
            total += (uint32_t)all;
            if (r0 + WLT < b1) load(r0 + WLT);   // in flight during the MFMAs
            __syncthreads();
            const uint32_t full = total / WAVE;
            for (uint32_t c = done + (((uint32_t)w - done) & (WNW - 1)); c < full; c += WNW) consume(c);
            done = full;
        }
        if (total % WAVE != 0 && (done & (WNW - 1)) == (uint32_t)w) consume(done);   // the partial last tile
        if (INF) {
            uint32_t bits = !infl ? 0u : (q <= K ? FM_ST_INF_IN_X : FM_ST_INF_IN_Y);   // q == 0 holds 1.0
            bits = wave_or_u32(bits);
            if (lane == 0 && bits != 0) atomicOr(&L.flags, bits);
        }
        __syncthreads();   // every wave is done with the ring
        gram16_store_image(acc, L.ring, w, kr, q);
        __syncthreads();
        L.G[tid] = gram16_sum_images<WNW>(L.ring, tid);
        __syncthreads();
        return total;
    };

    uint32_t N = 0;
    double piv = psh;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        N = run_pass(piv, pass == 0);
        if (pass == 0) {
            if (N < (uint32_t)K1 || L.flags != 0) {   // block-uniform
                const uint32_t st = N < (uint32_t)K1 ? FM_ST_SKIPPED : L.flags;
                write_failed_rec(a.rec, ro, rs, a.pmax, (double)N, tid, WLT);
                if (tid == 0) a.status[so] = st;
                return;
            }
            if (tid < ZW) L.piv[tid] = colq ? psh + L.G[tid] / L.G[0] : 0.0;   // wave 0: q == tid
            __syncthreads();
            piv = L.piv[q];
        }
    }
    if (w != 0) return;

    // ---- wave 0: lane i = variable i of (x_1 .. x_K, y), local column 1 + i.  The Gram is exactly zero
    // in the rows and columns past the problem's width (z = 0 there), so the sixteen steps below run
    // on the zero-padded matrix without a test of the size; a test per step would keep sixteen scalar
    // masks alive.
    const double sw = L.G[0];
    const double f = (double)N / sw;   // w~ = w N / sum(w)
    const int li = lane < ZW - 1 ? 1 + lane : 0;
    const double g0 = lane < ZW - 1 ? L.G[li] : 0.0;   // what the first pass's mean left of the first moment
    const double gr = g0 / sw;
    double row[ZW];
    double sii = 0.0;
#pragma unroll
    for (int j = 0; j < ZW; ++j) {
        const int lj = j + 1 < ZW ? j + 1 : ZW - 1;
        const int r = li < lj ? li : lj, c = li < lj ? lj : li;   // the upper triangle, mirrored
        const double v = lane < ZW - 1 && j < ZW - 1 ? (L.G[r * ZW + c] - gr * L.G[lj]) * f : 0.0;
        row[j] = v;
        sii = j == lane ? v : sii;
    }
    const double sxy = lane < K ? (L.G[li * ZW + K1] - gr * L.G[K1]) * f : 0.0;   // row[K] of this lane
    const double mu = lane < K1 ? L.piv[li] + gr : 0.0;
    double* stage = L.ring;   // free after the passes
#pragma unroll
    for (int j = 0; j < ZW; ++j)
        if (lane < ZW) stage[lane * ZW + j] = row[j];
    wave_sync();
    if (a.moments) {
        double* mo = a.moments + so * a.mom_stride;
        if (lane == 0) mo[0] = (double)N;
        if (lane < K1) mo[1 + lane] = mu;
        for (int e = lane; e < K1 * K1; e += WAVE) mo[1 + K1 + e] = stage[(e / K1) * ZW + e % K1];
    }
    // a constant predictor: its centred second moment is rounding beside the raw one
    const bool plain = __ballot(lane < K && !(sii > CONST_REL * (sii + (double)N * mu * mu))) == 0;
    const double syy = readlane_f64(sii, K);
    const double sx = lane < K && plain ? sii : 0.0;   // the pivots' diagonal entries: zero past K, so no step there
    int ngood = 0;
#pragma unroll
    for (int k = 0; k < ZW - 1; ++k) {
        const double orig = readlane_f64(sx, k);
        const double piv = readlane_f64(row[k], k);
        const bool good = orig > 0.0 && piv > REFIT_REL * orig;   // wave-uniform
        ngood += good ? 1 : 0;
        const double lkk = sqrt(piv);
        const double rinv = 1.0 / lkk;
        const double lik = row[k] * rinv;
#pragma unroll
        for (int j = k + 1; j < ZW; ++j) {
            const double sj = readlane_f64(row[j], k) * rinv;   // L[j][k]
            row[j] = good ? row[j] - lik * sj : row[j];
        }
        row[k] = good ? (lane == k ? lkk : lik) : row[k];
    }
    if (ngood != K) {   // a refused pivot (what later steps did with it is dropped here)
        write_failed_rec(a.rec, ro, rs, a.pmax, (double)N, lane, WAVE);
        if (lane == 0) a.status[so] = FM_ST_RANK_DEF;
        return;
    }
    // transpose through LDS: lane i then holds column i of L (and l_i = (L^-1 Sxy)_i, the y row's
    // entries); the rows past K are the identity's, so the steps past K change nothing
    wave_sync();
#pragma unroll
    for (int j = 0; j < ZW; ++j)
        if (lane < ZW) L.T[lane * ZW + j] = lane < K ? row[j] : (j == lane ? 1.0 : 0.0);
    if (lane == K) {
#pragma unroll
        for (int j = 0; j < ZW; ++j) stage[j] = row[j];
    }
    wave_sync();
    double col[ZW];
#pragma unroll
    for (int r = 0; r < ZW; ++r) col[r] = L.T[r * ZW + q];
    double t = lane < K ? stage[lane] : 0.0;
#pragma unroll
    for (int j = ZW - 2; j >= 0; --j) {
        const double bj = readlane_f64(t, j) / readlane_f64(col[j], j);
        t = lane == j ? bj : (lane < j ? t - col[j] * bj : t);
    }
    const double bi = lane < K ? t : 0.0;
    const double t_sxy = wave_sum(lane < K ? bi * sxy : 0.0);
    const double t_mu = wave_sum(lane < K ? bi * mu : 0.0);
    const double r2 = 1.0 - (syy - t_sxy) / syy;
    const double icpt = readlane_f64(mu, K) - t_mu;
    const double bsh = __shfl(bi, lane > 0 ? lane - 1 : 0, WAVE);   // b_{k-1} to lane k
    write_fitted_rec(a.rec, ro, rs, a.pmax, K, icpt, bsh, r2, (double)N, lane, WAVE);
    if (lane == 0) a.status[so] = FM_ST_FITTED;
}

}  // namespace
}  // namespace fm

extern "C" int fm_wls(const fm_wls_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_wls: null args");
    const fm_wls_args& a = *args;
    FM_REQUIRE(a.ncols >= 1 && a.ncols <= FM_WLS_MAX_COLS, "fm_wls: ncols must be 1..%d, got %d", FM_WLS_MAX_COLS,
               a.ncols);
    FM_REQUIRE(a.nseg >= 0 && a.nprob >= 0 && a.nrows >= 0, "fm_wls: negative size");
    FM_REQUIRE(a.nprob <= 65535, "fm_wls: at most 65,535 problems per call");
    FM_REQUIRE(a.pmax >= 1 && a.pmax <= FM_WLS_MAX_COLS, "fm_wls: pmax must be 1..%d, got %d", FM_WLS_MAX_COLS, a.pmax);
    if (a.nseg == 0 || a.nprob == 0) return FM_OK;
    FM_REQUIRE(a.cols && a.seg_off && a.weight && a.prob_level && a.prob_z && a.prob_nz && a.rec && a.status,
               "fm_wls: null pointer (FP64 columns, seg_off, weight, the problem tables, rec and status are required)");
    FM_REQUIRE(a.col_stride >= a.nrows, "fm_wls: col_stride must be at least nrows");
    FM_REQUIRE((a.lo == nullptr) == (a.hi == nullptr), "fm_wls: lo and hi come together");
    FM_REQUIRE(a.moments == nullptr || a.mom_stride >= 1 + (a.pmax + 1) + (a.pmax + 1) * (a.pmax + 1),
               "fm_wls: mom_stride must hold n, pmax + 1 means and (pmax + 1)^2 moments");
    hipLaunchKernelGGL(wls_kernel, dim3((unsigned)a.nseg, (unsigned)a.nprob), dim3(WLT), 0, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_wls");
    return FM_OK;
}
