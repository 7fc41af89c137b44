// fm_portfolio_hold: k-month holding of the forecast-sorted portfolios by overlapping cohorts
// (build-defined extension A19; the definition is in fm_hip.h).
//
// One workgroup per (month t, batch of sorts).  Each of its four waves takes every fourth 64-row
// tile of the month and walks the tile's rows back through the step -1 links, one hop per age: k
// dependent rounds of one link load, with the earlier months' bounds as wave-uniform scalar loads
// (the month is the workgroup's, so no tile crosses a month boundary and months may have any
// length).  At every hop a lane reads one port byte per sort of the batch at its ancestor row.
//
// Bins [sort][age][portfolio] live in LDS.  The tile's three FP64 terms per row (ret, w * ret, w;
// +0.0 where the row does not count) are staged once per tile in the wave's own 1.5 KB, and the rows'
// own port bytes (for `stay`) in 64 B a sort.  The wave bins up to 64 / nport (at most 8) sorts at
// once: lane (g, p) stands for portfolio p of the group's sort g.  The group's port bytes are loaded
// first (independent loads, while the next hop's link is in flight too), then one ballot per
// (sort, portfolio) gives lane (g, p) the tile's members of its portfolio, so the four counts are
// popcounts (added to the workgroup's bins with integer LDS atomics, whose order does not matter),
// and every lane adds the staged terms of its portfolio's rows to the wave's own FP64 bin in
// ascending row order -- all sorts of the group in one loop, as long as the largest portfolio.
// At the end the four waves' bins are added in wave order.
// Every FP64 sum of (sort, month, age, portfolio) therefore runs in one fixed order that depends
// on the month's rows alone: not on the run, nor on the other sorts of the launch or the batch
// size.  The records (cohort means, the k-cohort average, turnover, status) are written by the
// same launch from the combined bins, with ordinary vector stores.
#include <math.h>

#include "fm_common.h"

namespace fm {
namespace {

constexpr int HDT = 256;
constexpr int HDW = HDT / WAVE;
constexpr size_t HOLD_LDS_BUDGET = 60 * 1024;    // bins of a batch of sorts (a batch is at least one sort)
constexpr size_t HOLD_LDS_MAX = 128 * 1024;      // one sort at hold 36 x 20 portfolios needs 81 KB
constexpr int HOLD_MAX_GROUP = 8;                // sorts a wave bins at once: lane = sort * nport + portfolio

__host__ __device__ inline size_t hold_sum_doubles(int B, int k, int P) { return (size_t)B * k * P * 3; }
__host__ __device__ inline size_t hold_cnt_ints(int B, int k, int P) { return (size_t)B * (k + 1) * P * 4; }
inline size_t hold_lds_bytes(int B, int k, int P) {
    return 8 * (HDW * hold_sum_doubles(B, k, P) + HDW * 3 * WAVE) + 4 * hold_cnt_ints(B, k, P) + (size_t)HDW * B * WAVE;
}

__global__ __launch_bounds__(HDT) void portfolio_hold_kernel(fm_hold_args a, int B) {
    extern __shared__ double hold_lds[];
    const int tid = threadIdx.x, lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int t = blockIdx.x;
    const int j0 = blockIdx.y * B;
    const int nb = a.nsel - j0 < B ? a.nsel - j0 : B;
    const int k = a.hold, P = a.nport;
    const int64_t nrows = a.nrows;
    const int nsum = (int)hold_sum_doubles(B, k, P), ncnt = (int)hold_cnt_ints(B, k, P);
    double* sums = hold_lds;                              // [HDW][B][k][P][3]
    double* term = sums + (size_t)HDW * nsum;             // [HDW][3][WAVE]
    int32_t* cnt = (int32_t*)(term + HDW * 3 * WAVE);     // [B][k+1][P][4]: members, stay, n ret, n weight
    uint8_t* own_port = (uint8_t*)(cnt + ncnt);           // [HDW][B][WAVE]: the tile's own port bytes
    const int G = WAVE / P < HOLD_MAX_GROUP ? WAVE / P : HOLD_MAX_GROUP;
    const int myg = lane / P, myp = lane - myg * P;       // lanes with myg >= G idle in the binning

    for (int i = tid; i < HDW * nsum; i += HDT) sums[i] = 0.0;
    for (int i = tid; i < ncnt; i += HDT) cnt[i] = 0;
    __syncthreads();

    // (month_rows' clamp in the looser form the loop below needs: the strict one cost 1 % at hold 1 and 6)
    int64_t b0 = a.seg_off[t], b1 = a.seg_off[t + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = b1 > nrows ? nrows : b1;
    double* ws = sums + (size_t)w * nsum;
    double* wt = term + w * 3 * WAVE;
    uint8_t* wo = own_port + (size_t)w * B * WAVE;

    for (int64_t r0 = b0 + (int64_t)w * WAVE; r0 < b1; r0 += HDT) {
        const int64_t i = r0 + lane;
        const bool live = i < b1;
        const double r = live ? a.ret[i] : NAN;
        const double wgt = live && a.weight != nullptr ? a.weight[i] : NAN;
        const bool f0 = live && isfinite(r);
        const bool f1 = f0 && isfinite(wgt) && wgt > 0.0;
        wave_sync();   // the previous tile's reads of the staged terms are done
        wt[lane] = f0 ? r : 0.0;
        wt[WAVE + lane] = f1 ? wgt * r : 0.0;
        wt[2 * WAVE + lane] = f1 ? wgt : 0.0;
        wave_sync();
        const uint64_t F0 = __builtin_amdgcn_ballot_w64(f0), F1 = __builtin_amdgcn_ballot_w64(f1);

        int64_t row = i, lnk = -1;
        bool alive = live;
        for (int age = 0; age <= k; ++age) {
            if (age > 0) {
                const int s = t - age;
                if (s < 0) break;
                const int64_t s0 = a.seg_off[s], len = a.seg_off[s + 1] - s0;
                alive = alive && lnk >= 0 && lnk < len && s0 >= 0 && s0 + lnk < nrows;
                row = s0 + lnk;
                if (__builtin_amdgcn_ballot_w64(alive) == 0) break;   // later hops are missing too
            }
            // the next hop's link, in flight while this age's sorts are binned
            if (age < k) lnk = alive ? (int64_t)a.link_prev[row] : -1;
            for (int jg = 0; jg < nb; jg += G) {
                // the group's port bytes first (independent loads), then their ballots
                int q[HOLD_MAX_GROUP];
#pragma unroll
                for (int g = 0; g < HOLD_MAX_GROUP; ++g)
                    q[g] = g < G && jg + g < nb && alive ? (int)a.port[(int64_t)(j0 + jg + g) * nrows + row] : 255;
                // lane (g, p) keeps the tile's members and stayers of portfolio p of the group's sort g
                uint64_t mm = 0, st = 0;
#pragma unroll
                for (int g = 0; g < HOLD_MAX_GROUP; ++g) {
                    if (g < G && jg + g < nb) {   // wave-uniform
                        int own = q[g];
                        if (age == 0) wo[(jg + g) * WAVE + lane] = (uint8_t)own;
                        else own = wo[(jg + g) * WAVE + lane];
                        const uint64_t bo = __builtin_amdgcn_ballot_w64(q[g] == own);
                        if (myg == g) st = bo;
                        for (int p = 0; p < P; ++p) {
                            const uint64_t bm = __builtin_amdgcn_ballot_w64(q[g] == p);
                            if (lane == g * P + p) mm = bm;
                        }
                    }
                }
                if (mm != 0) {   // not the idle lanes, nor portfolios without a member here
                    const int jj = jg + myg;
                    const uint64_t ms = mm & st;
                    int32_t* c = cnt + ((jj * (k + 1) + age) * P + myp) * 4;
                    atomicAdd(&c[0], __builtin_popcountll(mm));
                    if (ms != 0) atomicAdd(&c[1], __builtin_popcountll(ms));
                    uint64_t m = age < k ? mm & F0 : 0;
                    if (m != 0) {
                        atomicAdd(&c[2], __builtin_popcountll(m));
                        if ((mm & F1) != 0) atomicAdd(&c[3], __builtin_popcountll(mm & F1));
                        double* s = ws + ((jj * k + age) * P + myp) * 3;
                        double s0 = s[0], s1 = s[1], s2 = s[2];
                        while (m != 0) {   // ascending rows
                            const int l = __builtin_ctzll(m);
                            m &= m - 1;
                            s0 += wt[l];
                            s1 += wt[WAVE + l];
                            s2 += wt[2 * WAVE + l];
                        }
                        s[0] = s0;
                        s[1] = s1;
                        s[2] = s2;
                    }
                }
            }
        }
    }
    __syncthreads();

    // counts, cohort means: the waves' sums in wave order; the means stay in wave 0's bins
    for (int b = tid; b < nb * (k + 1) * P; b += HDT) {
        const int q = b % P, age = (b / P) % (k + 1), jj = b / (P * (k + 1));
        const int32_t* c = cnt + (size_t)b * 4;
        const int64_t o = (int64_t)(j0 + jj) * a.nseg + t;
        a.members[(o * (k + 1) + age) * P + q] = c[0];
        a.stay[(o * (k + 1) + age) * P + q] = c[1];
        if (age == k) continue;
        const int sb = ((jj * k + age) * P + q) * 3;
        double s[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            s[v] = sums[sb + v];
#pragma unroll
            for (int x = 1; x < HDW; ++x) s[v] += sums[(size_t)x * nsum + sb + v];
        }
        const double ew = c[2] > 0 ? s[0] / (double)c[2] : NAN;
        const double vw = c[3] > 0 ? s[1] / s[2] : NAN;
        const int64_t oc = ((o * k + age) * P + q) * 2;
        a.cohort_n[oc] = c[2];
        a.cohort_n[oc + 1] = c[3];
        a.cohort[oc] = ew;
        a.cohort[oc + 1] = vw;
        sums[sb] = ew;
        sums[sb + 1] = vw;
    }
    __syncthreads();

    // whether sort j's month t (t - d .. t for d = depth) is a run of sorted consecutive months
    auto run_ok = [&](int j, int d) {
        if (t - d < 0) return false;
        for (int x = 0; x <= d; ++x)
            if (a.status[(int64_t)j * a.nseg + t - x] != 1u || a.month_index[t - x] != a.month_index[t] - x) return false;
        return true;
    };
    // the k-cohort average of column `col` of portfolio q (a complete month)
    auto average = [&](int jj, int q, int col) {
        double x = 0.0;
        for (int age = 0; age < k; ++age) {
            double v;
            if ((col & 1) == 0) v = sums[((jj * k + age) * P + q) * 3 + (col >> 1)];
            else if (a.sort_rec == nullptr) v = NAN;
            else v = a.sort_rec[((((int64_t)(j0 + jj) * a.nseg + t - age) * (P + 1)) + q) * 4 + col];
            x = age == 0 ? v : x + v;
        }
        return x / (double)k;
    };
    for (int e = tid; e < nb * P * 4; e += HDT) {
        const int col = e & 3, q = (e >> 2) % P, jj = (e >> 2) / P;
        const int64_t o = ((int64_t)(j0 + jj) * a.nseg + t) * (P + 1);
        const bool complete = run_ok(j0 + jj, k - 1);
        const double v = complete ? average(jj, q, col) : NAN;
        a.rec[(o + q) * 4 + col] = v;
        if (q == P - 1) a.rec[(o + P) * 4 + col] = complete ? v - average(jj, 0, col) : NAN;
    }
    for (int e = tid; e < nb * P; e += HDT) {
        const int q = e % P, jj = e / P;
        const int32_t m0 = cnt[((jj * (k + 1) + 0) * P + q) * 4], sk = cnt[((jj * (k + 1) + k) * P + q) * 4 + 1];
        double v = NAN;
        if (m0 > 0 && run_ok(j0 + jj, k)) v = (1.0 - (double)sk / (double)m0) / (double)k;
        a.turnover[((int64_t)(j0 + jj) * a.nseg + t) * P + q] = v;
    }
    if (tid < nb) a.status_out[(int64_t)(j0 + tid) * a.nseg + t] = run_ok(j0 + tid, k - 1) ? 1u : 0u;
}

}  // namespace
}  // namespace fm

extern "C" int fm_portfolio_hold(const fm_hold_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_portfolio_hold: null args");
    const fm_hold_args& a = *args;
    FM_REQUIRE(a.nport >= 2 && a.nport <= FM_MAX_PORTS, "fm_portfolio_hold: nport must be 2..%d, got %d", FM_MAX_PORTS,
               a.nport);
    FM_REQUIRE(a.hold >= 1 && a.hold <= FM_MAX_HOLD, "fm_portfolio_hold: hold must be 1..%d, got %d", FM_MAX_HOLD,
               a.hold);
    FM_REQUIRE(a.nsel >= 0 && a.nsel <= FM_MAX_SORTS, "fm_portfolio_hold: nsel must be 0..%d, got %d", FM_MAX_SORTS,
               a.nsel);
    FM_REQUIRE(a.nseg >= 0, "fm_portfolio_hold: nseg must not be negative");
    FM_REQUIRE(a.nrows >= 0, "fm_portfolio_hold: nrows must not be negative");
    if (a.nseg == 0 || a.nrows == 0 || a.nsel == 0) return FM_OK;
    const int64_t S = a.nsel, T = a.nseg, P = a.nport, k = a.hold, n = a.nrows;
    const Span in[] = {{"seg_off", a.seg_off, 8 * (T + 1)}, {"month_index", a.month_index, 4 * T},
                       {"link_prev", a.link_prev, 4 * n},   {"port", a.port, S * n},
                       {"status", a.status, 4 * S * T},     {"ret", a.ret, 8 * n},
                       {"weight", a.weight, 8 * n, true},   {"sort_rec", a.sort_rec, 8 * S * T * (P + 1) * 4, true}};
    const Span out[] = {{"members", a.members, 4 * S * T * (k + 1) * P}, {"stay", a.stay, 4 * S * T * (k + 1) * P},
                        {"cohort_n", a.cohort_n, 4 * S * T * k * P * 2}, {"cohort", a.cohort, 8 * S * T * k * P * 2},
                        {"status_out", a.status_out, 4 * S * T},         {"rec", a.rec, 8 * S * T * (P + 1) * 4},
                        {"turnover", a.turnover, 8 * S * T * P}};
    if (const int rc = check_spans("fm_portfolio_hold", in, out)) return rc;   // every output is required
    // as few batches of sorts as the LDS budget allows, of equal size (every batch repeats the walk)
    const size_t per_sort = hold_lds_bytes(1, a.hold, a.nport) - 8 * HDW * 3 * WAVE;
    int B = (int)((HOLD_LDS_BUDGET - 8 * HDW * 3 * WAVE) / per_sort);
    B = B < 1 ? 1 : (B > a.nsel ? a.nsel : B);
    const int nbatch = (a.nsel + B - 1) / B;
    B = (a.nsel + nbatch - 1) / nbatch;
    const size_t lds = hold_lds_bytes(B, a.hold, a.nport);
    const int rc = raise_dynamic_lds<portfolio_hold_kernel>(HOLD_LDS_MAX, "fm_portfolio_hold");
    if (rc != FM_OK) return rc;
    hipLaunchKernelGGL(portfolio_hold_kernel, dim3((unsigned)a.nseg, (unsigned)((a.nsel + B - 1) / B)), dim3(HDT), lds,
                       (hipStream_t)stream, a, B);
    FM_CHECK_LAUNCH("fm_portfolio_hold");
    return FM_OK;
}
