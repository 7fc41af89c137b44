// fm_group_adjust: within-group (industry) adjustment of the characteristics, per month
// (build-defined extension A20; the definition is in fm_hip.h).
//
// One workgroup per (month t, batch of columns).  Each of its four waves takes every fourth 64-row
// tile of the month, as fm_hold.hip does (the month is the workgroup's, so no tile crosses a month
// boundary and months may have any length).
//
// The partition of a tile's rows by group code is the same for every column, so it is found once
// per tile: the wave loops over the distinct codes present (readlane of the first remaining row's
// code, one ballot each: at most 64 rounds, as many as the tile has distinct codes) and lane j keeps
// the row mask and the code of the tile's j-th distinct code.  The batch's values of the tile (their
// loads are issued before that loop, which hides them) are then staged in the wave's own LDS, the lane's mask is ANDed with the column's
// not-NaN ballot, and the lane adds its members in ascending row order to the wave's own
// [column][group] bin.  Distinct lanes own distinct codes, so no two lanes of a wave touch one bin
// and no floating-point atomic is needed; the counts are popcounts, added to the workgroup's bins
// with integer LDS atomics (whose order does not matter).  The four waves' bins are added in wave
// order.  Every sum of (column, month, group) therefore runs in one fixed order that depends on the
// month's rows and codes alone.  FM_GADJ_ZSCORE runs the same pass a second time over (x - m)^2.
// The last pass re-reads the month's rows (L2-resident) and writes dst with ordinary vector stores,
// reading n, m and sd from LDS.
#include <math.h>

#include "fm_common.h"

namespace fm {
namespace {

constexpr int GDT = 256;
constexpr int GDW = GDT / WAVE;
constexpr int GADJ_MAX_BATCH = 8;                // columns of a workgroup, staged together, when the bins allow it
constexpr size_t GADJ_LDS_BUDGET = 64 * 1024;    // below the 64 KB a launch gets without opting in

// per column and group: the four waves' FP64 bins, the mean and the count
constexpr size_t GADJ_BIN_BYTES = 8 * GDW + 8 + 4;
constexpr size_t GADJ_STAGE_BYTES = 8 * (size_t)GDW * GADJ_MAX_BATCH * WAVE;
inline size_t gadj_lds_bytes(int B, int G) { return (size_t)B * G * GADJ_BIN_BYTES + GADJ_STAGE_BYTES; }

// row i's group code, -1 for a row without a group (a foreign code, or outside the universe)
__device__ __forceinline__ int row_code(const fm_gadj_args& a, int64_t i) {
    const int c = a.group[i];
    const bool in = c >= 0 && c < a.ngroups && (a.level == nullptr || (int)a.level[i] >= a.min_level);
    return in ? c : -1;
}

// One pass over the month's tiles: SQ false adds x and counts, SQ true adds (x - mean)^2 (over the
// same rows, in the same order).  ws: this wave's bins [B][G]; wt: its staging area.
template <bool SQ>
__device__ __forceinline__ void bin_pass(const fm_gadj_args& a, int j0, int nb, int64_t b0, int64_t b1, double* ws,
                                         double* wt, const double* mean, int32_t* cnt, int w, int lane) {
    const int G = a.ngroups;
    for (int64_t r0 = b0 + (int64_t)w * WAVE; r0 < b1; r0 += GDT) {
        const int64_t i = r0 + lane;
        const int c = i < b1 ? row_code(a, i) : -1;
        // the batch's values of the row first: in flight while the tile's codes are sorted out
        double x[GADJ_MAX_BATCH];
#pragma unroll
        for (int s = 0; s < GADJ_MAX_BATCH; ++s)
            x[s] = s < nb && c >= 0 ? a.src[(int64_t)(j0 + s) * a.src_stride + i] : NAN;
        // lane j: the rows and the code of the tile's j-th distinct code
        uint64_t mine = 0;
        int code = 0;
        uint64_t rem = __builtin_amdgcn_ballot_w64(c >= 0);
        for (int j = 0; rem != 0; ++j) {
            const int cc = __builtin_amdgcn_readlane(c, __builtin_ctzll(rem));
            const uint64_t m = __builtin_amdgcn_ballot_w64(c == cc);
            if (lane == j) {
                mine = m;
                code = cc;
            }
            rem &= ~m;
        }
        wave_sync();   // the previous tile's reads of the staged terms are done
#pragma unroll
        for (int s = 0; s < GADJ_MAX_BATCH; ++s) {
            double v = x[s];
            if (SQ && s < nb && c >= 0) {
                const double d = v - mean[s * G + c];
                v = d * d;
            }
            wt[s * WAVE + lane] = v;
        }
        wave_sync();
#pragma unroll
        for (int s = 0; s < GADJ_MAX_BATCH; ++s) {
            if (s >= nb) break;   // wave-uniform
            uint64_t m = mine & __builtin_amdgcn_ballot_w64(x[s] == x[s]);
            if (m != 0) {
                const int bin = s * G + code;
                if (!SQ) atomicAdd(&cnt[bin], __builtin_popcountll(m));
                double acc = ws[bin];
                while (m != 0) {   // ascending rows
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    acc += wt[s * WAVE + l];
                }
                ws[bin] = acc;
            }
        }
    }
}

__global__ __launch_bounds__(GDT) void group_adjust_kernel(fm_gadj_args a, int B, int col0) {
    extern __shared__ double gadj_lds[];
    const int tid = threadIdx.x, lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int t = blockIdx.x;
    const int j0 = col0 + blockIdx.y * B;
    const int nb = a.ncols - j0 < B ? a.ncols - j0 : B;
    if (nb <= 0) return;   // (the host launches no such batch)
    const int G = a.ngroups, nbin = B * G;
    const int need = a.min_count > 1 ? a.min_count : 1;
    double* sums = gadj_lds;                            // [GDW][B][G]; wave 0's hold sd after the ZSCORE pass
    double* mean = sums + (size_t)GDW * nbin;           // [B][G]
    double* term = mean + nbin;                         // [GDW][GADJ_MAX_BATCH][WAVE]
    int32_t* cnt = (int32_t*)(term + GDW * GADJ_MAX_BATCH * WAVE);   // [B][G]

    for (int e = tid; e < GDW * nbin; e += GDT) sums[e] = 0.0;
    for (int e = tid; e < nbin; e += GDT) cnt[e] = 0;
    __syncthreads();

    int64_t b0 = a.seg_off[t], b1 = a.seg_off[t + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = b1 > a.nrows ? a.nrows : b1;   // a foreign seg_off reads nothing outside [0, nrows)
    double* ws = sums + (size_t)w * nbin;
    double* wt = term + w * GADJ_MAX_BATCH * WAVE;

    bin_pass<false>(a, j0, nb, b0, b1, ws, wt, mean, cnt, w, lane);
    __syncthreads();

    // n, m = S / n with the waves' sums added in wave order; the tables' elements of this (column, month)
    for (int e = tid; e < nb * G; e += GDT) {
        const int n = cnt[e];
        double S = sums[e];
#pragma unroll
        for (int x = 1; x < GDW; ++x) S += sums[(size_t)x * nbin + e];
        const double m = S / (double)n;
        mean[e] = m;
        const int b = e / G, g = e - b * G;
        const int64_t o = ((int64_t)(j0 + b) * a.nseg + t) * G + g;
        if (a.gcount != nullptr) a.gcount[o] = n;
        if (a.gmean != nullptr) a.gmean[o] = n >= need ? m : NAN;
    }
    __syncthreads();

    if (a.mode == FM_GADJ_ZSCORE) {
        for (int e = tid; e < GDW * nbin; e += GDT) sums[e] = 0.0;
        __syncthreads();
        bin_pass<true>(a, j0, nb, b0, b1, ws, wt, mean, cnt, w, lane);
        __syncthreads();
        for (int e = tid; e < nb * G; e += GDT) {
            const int n = cnt[e];
            double ss = sums[e];
#pragma unroll
            for (int x = 1; x < GDW; ++x) ss += sums[(size_t)x * nbin + e];
            const double sd = n >= 2 ? sqrt(ss / (double)(n - 1)) : NAN;
            sums[e] = sd;   // this thread alone reads and writes element e of the waves' bins
            const int b = e / G, g = e - b * G;
            if (a.gsd != nullptr) a.gsd[((int64_t)(j0 + b) * a.nseg + t) * G + g] = sd;
        }
        __syncthreads();
    }

    for (int64_t i = b0 + tid; i < b1; i += GDT) {
        const int c = row_code(a, i);
        double x[GADJ_MAX_BATCH];
#pragma unroll
        for (int s = 0; s < GADJ_MAX_BATCH; ++s)
            x[s] = s < nb && c >= 0 ? a.src[(int64_t)(j0 + s) * a.src_stride + i] : NAN;
#pragma unroll
        for (int s = 0; s < GADJ_MAX_BATCH; ++s) {
            if (s >= nb) break;
            double out = NAN;
            if (x[s] == x[s]) {   // c >= 0 too: the other rows were not loaded
                const int bin = s * G + c;
                const int n = cnt[bin];
                const double m = mean[bin];
                if (n >= need) {
                    if (a.mode == FM_GADJ_MEAN) {
                        out = m;
                    } else if (a.mode == FM_GADJ_DEMEAN) {
                        out = x[s] - m;
                    } else {
                        const double sd = sums[bin];
                        if (n >= 2 && sd > 0.0 && sd < INFINITY) out = (x[s] - m) / sd;
                    }
                }
            }
            a.dst[(int64_t)(j0 + s) * a.dst_stride + i] = out;
        }
    }
}

}  // namespace
}  // namespace fm

extern "C" int fm_group_adjust_batch(int32_t ngroups) {
    using namespace fm;
    if (ngroups < 1 || ngroups > FM_MAX_GROUPS) return 0;
    const int B = (int)((GADJ_LDS_BUDGET - GADJ_STAGE_BYTES) / ((size_t)ngroups * GADJ_BIN_BYTES));
    return B > GADJ_MAX_BATCH ? GADJ_MAX_BATCH : B;
}

extern "C" int fm_group_adjust(const fm_gadj_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_group_adjust: null args");
    const fm_gadj_args& a = *args;
    FM_REQUIRE(a.ngroups >= 1 && a.ngroups <= FM_MAX_GROUPS, "fm_group_adjust: ngroups must be 1..%d, got %d",
               FM_MAX_GROUPS, a.ngroups);
    FM_REQUIRE(a.mode == FM_GADJ_DEMEAN || a.mode == FM_GADJ_MEAN || a.mode == FM_GADJ_ZSCORE,
               "fm_group_adjust: unknown mode %d", a.mode);
    FM_REQUIRE(a.min_count >= 0, "fm_group_adjust: min_count must not be negative");
    FM_REQUIRE(a.gsd == nullptr || a.mode == FM_GADJ_ZSCORE, "fm_group_adjust: gsd needs FM_GADJ_ZSCORE");
    FM_REQUIRE(a.nseg >= 0, "fm_group_adjust: nseg must not be negative");
    FM_REQUIRE(a.nrows >= 0, "fm_group_adjust: nrows must not be negative");
    FM_REQUIRE(a.ncols >= 0, "fm_group_adjust: ncols must not be negative");
    if (a.nseg == 0 || a.nrows == 0 || a.ncols == 0) return FM_OK;
    FM_REQUIRE(a.src_stride >= a.nrows && a.dst_stride >= a.nrows,
               "fm_group_adjust: src_stride and dst_stride must be at least nrows");
    const int64_t C = a.ncols, T = a.nseg, G = a.ngroups, n = a.nrows;
    const Span in[] = {{"src", a.src, 8 * ((C - 1) * a.src_stride + n)}, {"seg_off", a.seg_off, 8 * (T + 1)},
                       {"group", a.group, 4 * n},                       {"level", a.level, n, true}};
    const Span out[] = {{"dst", a.dst, 8 * ((C - 1) * a.dst_stride + n)}, {"gcount", a.gcount, 4 * C * T * G, true},
                        {"gmean", a.gmean, 8 * C * T * G, true},          {"gsd", a.gsd, 8 * C * T * G, true}};
    if (const int rc = check_spans("fm_group_adjust", in, out)) return rc;   // the group tables are optional
    // as few batches of columns as the bins allow, of equal size (every batch finds the tiles' codes again)
    int B = fm_group_adjust_batch(a.ngroups);
    B = B > a.ncols ? a.ncols : B;
    const int nbatch = (a.ncols + B - 1) / B;
    B = (a.ncols + nbatch - 1) / nbatch;
    const size_t lds = gadj_lds_bytes(B, a.ngroups);
    constexpr int MAX_GRID_Y = 65535;
    for (int k = 0; k < nbatch; k += MAX_GRID_Y) {
        const int ny = nbatch - k < MAX_GRID_Y ? nbatch - k : MAX_GRID_Y;
        hipLaunchKernelGGL(group_adjust_kernel, dim3((unsigned)a.nseg, (unsigned)ny), dim3(GDT), lds,
                           (hipStream_t)stream, a, B, k * B);
        FM_CHECK_LAUNCH("fm_group_adjust");
    }
    return FM_OK;
}
