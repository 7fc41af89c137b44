// What the 16-wide regression kernels share (fm_wls.hip, fm_pool.hip; fm_solve.hip takes the record
// writers): how a problem's width, columns and per-month column parameters are read from the args
// struct, the epilogue that adds the waves' 16 x 16 MFMA accumulators in wave order, and the layout
// of a (month, problem) record.  The args structs (fm_wls_args, fm_pool_args) name these fields
// alike: prob_nz, pmax, ncols, nseg, lo, hi, shift.
#pragma once

#include <math.h>

#include "fm_common.h"

namespace fm {
namespace {

constexpr int ZW = 16;                     // z = [1, x_1 .. x_K, y], K + 2 <= 16
constexpr int RS = ZW + 1;                 // LDS row stride (doubles): odd, so a column read spreads over the banks
constexpr double CONST_REL = 1e-20;        // centred / raw second moment at or below this: a constant column

typedef double d4 __attribute__((ext_vector_type(4)));

// nz = K + 2 of problem p, inside the tile and what the outputs hold (K + 1 <= pmax)
template <typename Args>
__device__ __forceinline__ int prob_width(const Args& a, int p) {
    int nz = a.prob_nz[p];
    nz = nz > a.pmax + 1 ? a.pmax + 1 : nz;
    return nz < 2 ? 2 : (nz > ZW ? ZW : nz);
}
// Local column j of the z list zi -> panel column, inside the panel; the slots past the list repeat
// y's column, so a loop over all ZW slots needs no per-column condition.
template <typename Args>
__device__ __forceinline__ int64_t col_offset(const Args& a, const int32_t* zi, int j, int nz) {
    int c = zi[j < nz ? j : nz - 1] - 1;
    c = c < 0 ? 0 : (c >= a.ncols ? a.ncols - 1 : c);
    return (int64_t)c;
}
// Month s's parameters of local column j: the clip bounds (NaN: none) and the first pass's pivot;
// nothing for the intercept and the slots past the list.
struct ColVal {
    double lo = NAN, hi = NAN, shift = 0.0;
};
template <typename Args>
__device__ __forceinline__ ColVal col_par(const Args& a, const int32_t* zi, int j, int nz, int s) {
    ColVal v;
    if (j >= 1 && j < nz) {
        const int64_t o = col_offset(a, zi, j, nz) * a.nseg + s;
        if (a.lo) v.lo = a.lo[o];
        if (a.hi) v.hi = a.hi[o];
        if (a.shift) v.shift = a.shift[o];
    }
    return v;
}

// The month's parameters of the problem's local columns, staged in LDS: clip bounds and pivot.
struct ColPar {
    double lo[ZW], hi[ZW], piv[ZW];
};
// Thread j's part of it for month s.  piv: the (month, problem)'s sixteen pivots, or NULL for the
// first pass's shift.
template <typename Args>
__device__ __forceinline__ void stage_col_par(const Args& a, const int32_t* zi, int j, int nz, int s,
                                              const double* piv, ColPar& cp) {
    const ColVal v = col_par(a, zi, j, nz, s);
    cp.lo[j] = v.lo;
    cp.hi[j] = v.hi;
    cp.piv[j] = piv == nullptr ? v.shift : (j >= 1 && j < nz ? piv[j] : 0.0);
}

// The waves' accumulators as 16 x 16 images in LDS (wave w's at imgs + 256 w), then entry tid of
// their sum in wave order; a barrier goes between the two.
// v_mfma_f64_16x16x4_f64: register r of lane (kr, q) is D[kr + 4 r][q]
__device__ __forceinline__ void gram16_store_image(const d4& acc, double* imgs, int w, int kr, int q) {
    double* img = imgs + w * (ZW * ZW);
#pragma unroll
    for (int r = 0; r < 4; ++r) img[(kr + 4 * r) * ZW + q] = acc[r];
}
template <int NW>
__device__ __forceinline__ double gram16_sum_images(const double* imgs, int tid) {
    double g = imgs[tid];
#pragma unroll
    for (int x = 1; x < NW; ++x) g += imgs[x * (ZW * ZW) + tid];
    return g;
}

// The record of a (month, problem), rs = pmax + 2 doubles at rec + ro, written by the threads first,
// first + step, ..: a month without a fit holds NaN and N;
__device__ __forceinline__ void write_failed_rec(double* rec, int64_t ro, int rs, int pmax, double n, int first,
                                                 int step) {
    for (int k = first; k < rs; k += step) rec[ro + k] = k == pmax + 1 ? n : NAN;
}
// a fitted one the intercept at 0, b_{k-1} at k <= K (`slope`: thread k's own b_{k-1}; K < step, so
// a slope is always a thread's first entry), NaN between the slopes and R^2, R^2 at pmax, N at
// pmax + 1.
__device__ __forceinline__ void write_fitted_rec(double* rec, int64_t ro, int rs, int pmax, int K, double icpt,
                                                 double slope, double r2, double n, int first, int step) {
    for (int k = first; k < rs; k += step) {
        double v = NAN;
        if (k == 0) v = icpt;
        else if (k <= K) v = slope;
        else if (k == pmax) v = r2;
        else if (k == pmax + 1) v = n;
        rec[ro + k] = v;
    }
}

}  // namespace
}  // namespace fm
