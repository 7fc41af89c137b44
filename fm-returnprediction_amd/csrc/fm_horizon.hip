// fm_month_links, fm_horizon_return: multi-month return horizons on the month-sorted panel
// (build-defined extension A16; the dependent variable of the paper's Tables 8 and 9).
//
// The panel's rows are sorted by (month, firm id), so the same firm's row in the neighbouring
// month is found by a search of that month's id run.  Both kernels give one 64-row tile of the
// global row space to a wave (a grid-stride loop over tiles).  A tile usually lies inside one
// month; its month, the neighbouring month's bounds and the calendar test are then wave-uniform
// (scalar loads), and because both id runs ascend, the tile's matches lie in one narrow window of
// the neighbouring month: two wave-uniform searches (the tile's first and last id) bound it, and
// each lane searches only inside it -- log2(window) steps on lines the whole wave shares.  The
// wave-uniform searches (the tile's month, the window's two ends) are 64-ary: every lane probes
// one position per round (wave_partition_point).  On the 600 x 5,000 panel the launch took 75 us
// with binary searches there and takes 50 us with these.  A tile
// that crosses a month boundary takes the same code with per-lane months and the whole
// neighbouring month as the window.
//
// fm_horizon_return walks the +1 links: hop j of a row reads link[] and ret[] at the row reached
// by hop j-1, so a row costs `horizon` dependent rounds of two independent loads.  Link positions
// rise with the row index, so a wave's gathers of one hop fall on a few consecutive lines.
#include <math.h>

#include "fm_common.h"

namespace fm {
namespace {

constexpr int HT = 256;          // threads per workgroup: four 64-row tiles
constexpr int H_MAX_GRID = 4096; // 256 CUs x 8 workgroups x 2 rounds; longer panels stride

// the segment of row r: the s with seg_off[s] <= r < seg_off[s+1], searched in [s_lo, s_hi]
// (r lies in one of them); empty segments are skipped by the strict upper bound
__device__ __forceinline__ int seg_of_row(const int64_t* __restrict__ seg_off, int s_lo, int s_hi, int64_t r) {
    int lo = s_lo, hi = s_hi;   // answer in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Wave-wide partition point: the first p in [lo, hi) for which before(p) is false (hi if none), for
// a predicate that is true on a prefix of the range.  lo, hi and the predicate are wave-uniform and
// all 64 lanes take part: each round every lane probes the last position of one of 64 equal
// sub-ranges and a ballot keeps one of them, so 5,000 positions take three dependent loads where
// a binary search takes thirteen.  A predicate that is not a prefix (ids out of order) still ends,
// inside [lo, hi].
template <typename F>
__device__ __forceinline__ int64_t wave_partition_point(int64_t lo, int64_t hi, F before) {
    const int lane = lane_id();
    while (lo < hi) {
        const int64_t step = (hi - lo + WAVE - 1) / WAVE;
        const int64_t p = lo + (lane + 1) * step - 1;
        const bool b = p < hi && before(p);
        const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(b));
        const int64_t nlo = lo + c * step, nhi = nlo + step - 1;
        lo = nlo < hi ? nlo : hi;
        hi = nhi < hi ? nhi : hi;
        if (step == 1) break;
    }
    return lo;
}

// seg_of_row over all nseg >= 1 segments for a wave-uniform row, by the whole wave
__device__ __forceinline__ int wave_seg_of_row(const int64_t* __restrict__ seg_off, int nseg, int64_t r) {
    return (int)wave_partition_point(1, nseg, [&](int64_t j) { return seg_off[j] <= r; }) - 1;
}

// The link of a row with firm id `id`: a search of ids[w_lo, w_hi), a sub-range of the neighbouring
// segment (which starts at row t0) that holds the match if there is one.
__device__ __forceinline__ int32_t link_of(const int64_t* __restrict__ ids, int64_t id, int64_t t0, int64_t w_lo,
                                           int64_t w_hi) {
    const int64_t pos = lower_bound(ids, w_lo, w_hi, id);
    if (pos < w_hi && ids[pos] == id) return (int32_t)(pos - t0);
    return -1;
}

__global__ __launch_bounds__(HT) void month_links_kernel(const int64_t* __restrict__ ids,
                                                         const int64_t* __restrict__ seg_off,
                                                         const int32_t* __restrict__ month_index, int64_t nrows,
                                                         int32_t nseg, int32_t step, int32_t* __restrict__ link,
                                                         int32_t* __restrict__ bad) {
    const int lane = lane_id();
    const int64_t ntiles = (nrows + WAVE - 1) / WAVE;
    const int64_t wave0 = (int64_t)blockIdx.x * (HT / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int64_t nwaves = (int64_t)gridDim.x * (HT / WAVE);
    for (int64_t tile = wave0; tile < ntiles; tile += nwaves) {
        const int64_t r0 = tile * WAVE;
        const int64_t r1 = (r0 + WAVE < nrows ? r0 + WAVE : nrows) - 1;   // the tile's last row
        const int64_t i = r0 + lane;
        const bool live = i <= r1;
        // wave-uniform: the month of the tile's first row
        const int s0 = __builtin_amdgcn_readfirstlane(wave_seg_of_row(seg_off, nseg, r0));
        const int64_t s0_end = seg_off[s0 + 1];
        int32_t out = -1;
        int nbad = 0;
        if (r1 < s0_end) {
            // the whole tile lies in month s0
            const int t = s0 + step;
            const bool t_ok = t >= 0 && t < nseg && month_index[t] == month_index[s0] + step;
            const int64_t id = live ? ids[i] : 0;
            if (live && i > 0 && i > seg_off[s0]) nbad = ids[i - 1] >= id;
            if (t_ok) {
                int64_t t0, t1;
                month_rows(seg_off, t, nrows, &t0, &t1);
                // the window of the tile's ids in month t, from its first and last id
                const int64_t id_first = (int64_t)readlane_u64((uint64_t)id, 0);
                const int64_t id_last = (int64_t)readlane_u64((uint64_t)id, (int)(r1 - r0));
                int64_t w_lo = t0, w_hi = t1;
                if (id_first <= id_last) {
                    w_lo = wave_partition_point(t0, t1, [&](int64_t p) { return ids[p] < id_first; });
                    w_hi = wave_partition_point(w_lo, t1, [&](int64_t p) { return ids[p] < id_last; });
                    w_hi = w_hi < t1 ? w_hi + 1 : t1;
                }
                if (live) out = link_of(ids, id, t0, w_lo, w_hi);
            }
        } else if (live) {
            // the tile crosses a month boundary: per-lane months, the whole neighbour as the window
            const int s1 = seg_of_row(seg_off, s0, nseg - 1, r1);
            const int s = seg_of_row(seg_off, s0, s1, i);
            const int t = s + step;
            const bool t_ok = t >= 0 && t < nseg && month_index[t] == month_index[s] + step;
            const int64_t id = ids[i];
            if (i > 0 && i > seg_off[s]) nbad = ids[i - 1] >= id;
            if (t_ok) {
                int64_t t0, t1;
                month_rows(seg_off, t, nrows, &t0, &t1);
                out = link_of(ids, id, t0, t0, t1);
            }
        }
        if (live) link[i] = out;
        const int wbad = __builtin_popcountll(__builtin_amdgcn_ballot_w64(nbad != 0));
        if (wbad != 0 && lane == 0) atomicAdd(bad, wbad);
    }
}

// out[i] of a row of segment s (the definition in fm_hip.h); called with a wave-uniform s where
// the tile lies in one month, so that the months' bounds come by scalar loads
__device__ __forceinline__ double horizon_of(const double* __restrict__ ret, const int32_t* __restrict__ link,
                                             const int64_t* __restrict__ seg_off, int64_t nrows, int32_t nseg,
                                             int32_t horizon, int64_t i, int s) {
    int64_t row = i;
    double p = 1.0 + ret[row];
    for (int j = 1; j < horizon; ++j) {
        const int sj = s + j;
        if (sj >= nseg) return NAN;
        const int64_t b0 = seg_off[sj], b1 = seg_off[sj + 1];
        const int64_t l = link[row];
        if (l < 0 || l >= b1 - b0 || b0 < 0 || b0 + l >= nrows) return NAN;
        row = b0 + l;
        p = p * (1.0 + ret[row]);
    }
    return p - 1.0;
}

__global__ __launch_bounds__(HT) void horizon_return_kernel(const double* __restrict__ ret,
                                                            const int32_t* __restrict__ link,
                                                            const int64_t* __restrict__ seg_off, int64_t nrows,
                                                            int32_t nseg, int32_t horizon,
                                                            double* __restrict__ out) {
    const int lane = lane_id();
    const int64_t ntiles = (nrows + WAVE - 1) / WAVE;
    const int64_t wave0 = (int64_t)blockIdx.x * (HT / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int64_t nwaves = (int64_t)gridDim.x * (HT / WAVE);
    for (int64_t tile = wave0; tile < ntiles; tile += nwaves) {
        const int64_t r0 = tile * WAVE;
        const int64_t r1 = (r0 + WAVE < nrows ? r0 + WAVE : nrows) - 1;
        const int64_t i = r0 + lane;
        const int s0 = __builtin_amdgcn_readfirstlane(wave_seg_of_row(seg_off, nseg, r0));
        if (i > r1) continue;
        if (r1 < seg_off[s0 + 1]) {
            out[i] = horizon_of(ret, link, seg_off, nrows, nseg, horizon, i, s0);
        } else {
            const int s1 = seg_of_row(seg_off, s0, nseg - 1, r1);
            out[i] = horizon_of(ret, link, seg_off, nrows, nseg, horizon, i, seg_of_row(seg_off, s0, s1, i));
        }
    }
}

int tile_grid(int64_t nrows) {
    const int64_t blocks = (nrows + HT - 1) / HT;
    return (int)(blocks < H_MAX_GRID ? blocks : H_MAX_GRID);
}

}  // namespace
}  // namespace fm

extern "C" int fm_month_links(const fm_links_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_month_links: null args");
    const fm_links_args& a = *args;
    FM_REQUIRE(a.step == 1 || a.step == -1, "fm_month_links: step must be +1 or -1, got %d", a.step);
    FM_REQUIRE(a.nseg >= 0, "fm_month_links: nseg must not be negative");
    FM_REQUIRE(a.nrows >= 0, "fm_month_links: nrows must not be negative");
    FM_REQUIRE(a.seg_off != nullptr, "fm_month_links: seg_off is NULL");
    FM_REQUIRE(a.bad != nullptr, "fm_month_links: bad is NULL");
    if (a.nseg == 0 || a.nrows == 0) return FM_OK;
    FM_REQUIRE(a.ids != nullptr, "fm_month_links: ids is NULL");
    FM_REQUIRE(a.month_index != nullptr, "fm_month_links: month_index is NULL");
    FM_REQUIRE(a.link != nullptr, "fm_month_links: link is NULL");
    hipLaunchKernelGGL(month_links_kernel, dim3(tile_grid(a.nrows)), dim3(HT), 0, (hipStream_t)stream, a.ids,
                       a.seg_off, a.month_index, a.nrows, a.nseg, a.step, a.link, a.bad);
    FM_CHECK_LAUNCH("fm_month_links");
    return FM_OK;
}

extern "C" int fm_horizon_return(const fm_horizon_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_horizon_return: null args");
    const fm_horizon_args& a = *args;
    FM_REQUIRE(a.horizon >= 1 && a.horizon <= FM_MAX_HORIZON, "fm_horizon_return: horizon must be 1..%d, got %d",
               FM_MAX_HORIZON, a.horizon);
    FM_REQUIRE(a.nseg >= 0, "fm_horizon_return: nseg must not be negative");
    FM_REQUIRE(a.nrows >= 0, "fm_horizon_return: nrows must not be negative");
    FM_REQUIRE(a.seg_off != nullptr, "fm_horizon_return: seg_off is NULL");
    if (a.nseg == 0 || a.nrows == 0) return FM_OK;
    FM_REQUIRE(a.ret != nullptr, "fm_horizon_return: ret is NULL");
    FM_REQUIRE(a.link != nullptr, "fm_horizon_return: link is NULL");
    FM_REQUIRE(a.out != nullptr, "fm_horizon_return: out is NULL");
    FM_REQUIRE(!overlaps(a.out, 8 * a.nrows, a.ret, 8 * a.nrows), "fm_horizon_return: out must not overlap ret");
    FM_REQUIRE(!overlaps(a.out, 8 * a.nrows, a.link, 4 * a.nrows), "fm_horizon_return: out must not overlap link");
    hipLaunchKernelGGL(horizon_return_kernel, dim3(tile_grid(a.nrows)), dim3(HT), 0, (hipStream_t)stream, a.ret,
                       a.link, a.seg_off, a.nrows, a.nseg, a.horizon, a.out);
    FM_CHECK_LAUNCH("fm_horizon_return");
    return FM_OK;
}
