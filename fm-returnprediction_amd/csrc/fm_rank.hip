// fm_rank_transform: per-month cross-sectional ranks of the panel's columns (build-defined
// extension A13; pandas groupby(month)[x].rank, methods average / min / max).
// One workgroup per (month, column) unit, three phases:
//   1. every thread loads its rows' values once (wave w owns the rows [w * 64 R, (w + 1) * 64 R),
//      so row order = (wave, v, lane) order), maps the eligible ones to order-preserving keys
//      (zeros canonicalised, NaN / ineligible = SENT) and keeps them in registers; each wave
//      sorts a copy of its 64 R keys in registers (wave_sort64: DPP / permlane exchanges, no
//      LDS, no barrier) and writes the sorted run to LDS;
//   2. the runs are merged into one sorted array by the bitonic merge levels above the run
//      length, in the all-ascending form (the first stage of a level compares i with its
//      mirror i ^ (k - 1), the others i with i | j): only the stages whose distance reaches
//      across runs go through LDS with a barrier each (log2(runs) (log2(runs) + 1) / 2 of
//      them); the stages inside a run are finished by the run's wave in registers again.  The
//      array is not padded to a power of two: a partner past the end is a virtual SENT and
//      leaves its pair as it is;
//   3. every row finds `less` by a lower bound search of its own key in the sorted array, and
//      `less + eq` by an upper bound search only in the waves that hold a tied key (a key
//      whose successor differs has eq = 1), and writes its rank.
// No (key, row) pairs are sorted: the three methods need the two counts only.  The unit's
// values are read from HBM once and its ranks written once.
//
// Months of more than 16,384 rows (rank_long_kernel): the sorted keys of such a month do not fit
// one workgroup's LDS, but both counts are sums over any partition of the month's rows, so the
// month is cut into parts of 16,384 rows and a workgroup per (month, column, part) takes that
// part's rows as its own slice, sorts one part after another into LDS by phases 1-2 and adds up
// what phase 3 finds for its own rows' keys in each.  One launch, no workspace, no atomics, and
// no workgroup reads what another one writes; the price is that every slice's workgroup sorts
// every part: parts^2 part-sorts per unit, hence the 65,536-row limit.
//
// Both kernels run the phases through the same device functions below (RankRows::key,
// sort_runs, merge_runs, count_in_sorted, rank_value).
#include <math.h>

#include "fm_common.h"
#include "fm_select_dev.h"

// phase marks of rank_kernel (probe builds only, fm_common.h): 0 start, 1 runs sorted,
// 2 runs merged, 3 end
FM_PROBE_BUFFER(rank)

namespace fm {
namespace {

constexpr int RANK_MAX_ROWS = FM_RANK_MAX_ROWS;   // 4 parts: the long path's cost is quadratic in the part count
constexpr int RANK_PART = 16384;       // one workgroup's sort: 16 rows per thread of 1024 threads, 128 KB of keys
constexpr int RANK_SHORT_MAX = 8192;   // months up to here: 8 rows per thread

// ascending compare-exchange of buf[i], buf[l] (i < l)
__device__ __forceinline__ void cmpx(uint64_t* buf, int i, int l) {
    const uint64_t x = buf[i], y = buf[l];
    if (x > y) {
        buf[i] = y;
        buf[l] = x;
    }
}

// One column of one month, row by row as keys: SENT past the end, for a NaN and outside the
// universe (no eligible value maps to SENT: key != SENT is "the row is ranked")
struct RankRows {
    const double* __restrict__ X;
    const uint8_t* __restrict__ LV;
    int L, min_level;
    __device__ __forceinline__ uint64_t key(int idx) const {
        bool elig;
        return key(idx, elig);
    }
    __device__ __forceinline__ uint64_t key(int idx, bool& elig) const {
        const int ci = idx < L ? idx : L - 1;   // unconditional (clamped) load, masked after
        const double x = X[ci] + 0.0;           // -0.0 -> +0.0: the two zeros tie
        const int lv = LV != nullptr ? (int)LV[ci] : 255;
        elig = idx < L && !isnan(x) && lv >= min_level;
        return elig ? dkey(x) : SENT;
    }
};

// The sorted array of up to 1024 R rows: nrun runs of RUN = 64 R keys (one per wave that holds
// rows), Pact keys in all, P2 the power of two they would be padded to
struct Sorted {
    int nrun, Pact, P2;
};
template <int RUN>
__device__ __forceinline__ Sorted sorted_dims(int rows) {
    Sorted d;
    d.nrun = (rows + RUN - 1) / RUN;
    d.Pact = d.nrun * RUN;
    d.P2 = RUN;
    while (d.P2 < d.Pact) d.P2 <<= 1;
    return d;
}

// Phase 1 for the wave's R * 64 rows from `base` on, in (v, lane) order: their keys (all SENT in
// a wave w >= nrun, which holds none), a copy sorted in registers and stored as run w.  Returns
// the ranked rows of the NT-thread workgroup (s_cnt: a slot per wave); ends with a barrier.
template <int R>
__device__ __forceinline__ int sort_runs(uint64_t* rbuf, int* s_cnt, int NT, const Sorted& d, const RankRows& rows,
                                         int base, int w, int lane, uint64_t (&key)[R]) {
    constexpr int RUN = WAVE * R;
    int cnt = 0;
    if (w < d.nrun) {   // wave-uniform
#pragma unroll
        for (int v = 0; v < R; ++v) {
            bool elig;
            key[v] = rows.key(base + v * WAVE + lane, elig);
            cnt += elig ? 1 : 0;
        }
        uint64_t k[R];
#pragma unroll
        for (int v = 0; v < R; ++v) k[v] = key[v];
        wave_sort64<R>(k);
#pragma unroll
        for (int v = 0; v < R; ++v) rbuf[w * RUN + v * WAVE + lane] = k[v];
    } else {
#pragma unroll
        for (int v = 0; v < R; ++v) key[v] = SENT;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();
    int n = 0;
    for (int q = 0; q < NT / WAVE; ++q) n += s_cnt[q];
    return n;
}

// Phase 2: the runs in rbuf merged into one ascending array; every barrier is block-uniform
template <int R>
__device__ __forceinline__ void merge_runs(uint64_t* rbuf, int NT, const Sorted& d, int w, int lane) {
    constexpr int RUN = WAVE * R;
    const int tid = threadIdx.x;
    for (int k = 2 * RUN; k <= d.P2; k <<= 1) {   // block-uniform
        const int h = k >> 1;
        for (int t = tid; t < (d.P2 >> 1); t += NT) {
            const int i = ((t & ~(h - 1)) << 1) | (t & (h - 1));
            const int l = i ^ (k - 1);
            if (l < d.Pact) cmpx(rbuf, i, l);
        }
        __syncthreads();
        for (int j = h >> 1; j >= RUN; j >>= 1) {
            for (int t = tid; t < (d.P2 >> 1); t += NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                if (l < d.Pact) cmpx(rbuf, i, l);
            }
            __syncthreads();
        }
        if (w < d.nrun) {   // the stages inside the run: distances RUN / 2 .. 1, all ascending
            uint64_t m[R];
#pragma unroll
            for (int v = 0; v < R; ++v) m[v] = rbuf[w * RUN + v * WAVE + lane];
            bitonic_u64_stages<R, 2 * RUN, RUN / 2>(m);
#pragma unroll
            for (int v = 0; v < R; ++v) rbuf[w * RUN + v * WAVE + lane] = m[v];
        }
        __syncthreads();
    }
}

// Phase 3's searches for SG keys in step (that many LDS reads in flight): lt = #{sorted keys <
// key}, le = #{sorted keys <= key}; the keys past the eligible ones are SENT.  OWN: the keys are
// among the sorted ones, so an eligible key has lt < n <= P2 (the lower bound starts from
// P2 / 2) and its run of equals is not empty.  Otherwise every sorted key may be smaller (it
// starts from P2) and le = lt unless position lt holds the key.
template <int SG, bool OWN>
__device__ __forceinline__ void count_in_sorted(const uint64_t* rbuf, const Sorted& d, const uint64_t* key,
                                                int (&lt)[SG], int (&le)[SG]) {
    const int Pact = d.Pact, P2 = d.P2;
#pragma unroll
    for (int u = 0; u < SG; ++u) lt[u] = 0;
    for (int step = OWN ? P2 >> 1 : P2; step > 0; step >>= 1) {
#pragma unroll
        for (int u = 0; u < SG; ++u) {
            const int pa = lt[u] + step - 1;
            const uint64_t xa = rbuf[pa < Pact ? pa : Pact - 1];
            lt[u] += (pa < Pact && xa < key[u]) ? step : 0;
        }
    }
    // a key whose successor differs ends its run of equals at lt + 1 (at lt if it is absent):
    // only a wave that holds a tied key among these rows runs the upper bound search (the same
    // counts either way)
    bool tied = false;
#pragma unroll
    for (int u = 0; u < SG; ++u) {
        const int pc = lt[u], pn = lt[u] + 1;
        const uint64_t xn = rbuf[pn < Pact ? pn : Pact - 1];
        tied |= pn < Pact && xn == key[u] && key[u] != SENT;
        if constexpr (OWN) {
            le[u] = pn;
        } else {
            const uint64_t xc = rbuf[pc < Pact ? pc : Pact - 1];
            le[u] = lt[u] + ((pc < Pact && xc == key[u]) ? 1 : 0);
        }
    }
    if (__ballot(tied) != 0ull) {   // wave-uniform
#pragma unroll
        for (int u = 0; u < SG; ++u) le[u] = 0;
        for (int step = P2; step > 0; step >>= 1) {   // from P2: le reaches P2 in a full month
#pragma unroll
            for (int u = 0; u < SG; ++u) {
                const int pb = le[u] + step - 1;
                const uint64_t xb = rbuf[pb < Pact ? pb : Pact - 1];
                le[u] += (pb < Pact && xb <= key[u]) ? step : 0;
            }
        }
    }
}

// The rank of a row with lt smaller and le smaller-or-equal keys among the month's n eligible
// ones (dn = n, dn1 = n + 1): a multiple of 0.5 below 2^17, exact before the scaling
__device__ __forceinline__ double rank_value(int method, int scale, int lt, int le, double dn, double dn1) {
    double r;
    if (method == FM_RANK_MIN) r = (double)(lt + 1);
    else if (method == FM_RANK_MAX) r = (double)le;
    else r = 0.5 * (double)(lt + le + 1);
    double y = r;
    if (scale == FM_RANK_PCT) y = r / dn;
    else if (scale == FM_RANK_UNIFORM) y = r / dn1 - 0.5;
    return y;
}

template <int R>
__global__ __launch_bounds__(1024) void rank_kernel(fm_rank_args a) {
    constexpr int RUN = WAVE * R;          // keys per wave = the sorted run length
    constexpr int SG = R < 8 ? R : 8;      // rows searched in step
    extern __shared__ uint64_t rbuf[];     // blockDim.x * R keys
    __shared__ int s_cnt[1024 / WAVE];
    const int s = blockIdx.x, c = blockIdx.y;
    const int NT = blockDim.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the workgroup and its LDS were sized from max_seg_len
    FM_PROBE_AT(rank, 0);
    if (L <= 0) {   // block-uniform
        if (tid == 0 && a.nvalid != nullptr) a.nvalid[(int64_t)c * a.nseg + s] = 0;
        return;
    }
    const Sorted d = sorted_dims<RUN>(L);   // nrun <= the waves: waves nrun.. hold no row
    const RankRows rows{a.src + (int64_t)c * a.src_stride + r0, a.level != nullptr ? a.level + r0 : nullptr, L,
                        a.min_level};

    uint64_t key[R];
    const int n = sort_runs<R>(rbuf, s_cnt, NT, d, rows, w * RUN, w, lane, key);
    FM_PROBE_AT(rank, 1);
    merge_runs<R>(rbuf, NT, d, w, lane);
    FM_PROBE_AT(rank, 2);

    if (tid == 0 && a.nvalid != nullptr) a.nvalid[(int64_t)c * a.nseg + s] = n;
    double* __restrict__ D = a.dst + (int64_t)c * a.dst_stride + r0;
    const double dn = (double)n, dn1 = (double)(n + 1);
    const int method = a.method, scale = a.scale;
    if (w < d.nrun) {
#pragma unroll
        for (int v0 = 0; v0 < R; v0 += SG) {
            int lt[SG], le[SG];
            count_in_sorted<SG, true>(rbuf, d, key + v0, lt, le);
#pragma unroll
            for (int u = 0; u < SG; ++u) {
                const int idx = (w * R + v0 + u) * WAVE + lane;
                const double y = rank_value(method, scale, lt[u], le[u], dn, dn1);
                if (idx < L) D[idx] = key[v0 + u] != SENT ? y : NAN;
            }
        }
    }
    FM_PROBE_AT(rank, 3);
}

// Months of more than RANK_PART rows.  Workgroup (s, c, z) of 1024 threads ranks the slice
// [z * RANK_PART, (z + 1) * RANK_PART) of month s, column c (its own rows, laid out over the
// threads as a part's): it visits the month's parts of RANK_PART rows in turn, sorts each into
// LDS exactly as rank_kernel<16> does and adds its own keys' counts #{part keys < key} and
// #{part keys <= key} to two per-row sums.  Only the sums stay in registers across a part's
// sort: the own keys are made again from src for every part (the month's values come from
// cache after the first read), 8 rows at a time, which is what keeps a 16-row slice within
// 128 VGPRs.  A key need not occur in the visited part (count_in_sorted<.., false>).  L, the
// part count and every barrier are block-uniform.
__global__ __launch_bounds__(1024) void rank_long_kernel(fm_rank_args a) {
    constexpr int R = RANK_PART / 1024;    // rows per thread, of a visited part and of the own slice
    constexpr int RUN = WAVE * R;
    constexpr int SG = 8;
    extern __shared__ uint64_t rbuf[];     // RANK_PART keys
    __shared__ int s_cnt[1024 / WAVE];
    const int s = blockIdx.x, c = blockIdx.y;
    const int own0 = blockIdx.z * RANK_PART;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the grid's slices were counted from max_seg_len
    if (own0 >= L) {   // block-uniform: an empty month (slice 0 reports it) or a slice past the month's end
        if (own0 == 0 && tid == 0 && a.nvalid != nullptr) a.nvalid[(int64_t)c * a.nseg + s] = 0;
        return;
    }
    const RankRows rows{a.src + (int64_t)c * a.src_stride + r0, a.level != nullptr ? a.level + r0 : nullptr, L,
                        a.min_level};
    const bool own_rows = own0 + w * RUN < L;   // wave-uniform: this wave holds rows of the slice

    int lts[R], les[R];   // the own rows' counts over the parts visited so far
#pragma unroll
    for (int v = 0; v < R; ++v) lts[v] = les[v] = 0;
    int n = 0;

    for (int p0 = 0; p0 < L; p0 += RANK_PART) {   // block-uniform
        const Sorted d = sorted_dims<RUN>(L - p0 < RANK_PART ? L - p0 : RANK_PART);
        {
            uint64_t k[R];
            n += sort_runs<R>(rbuf, s_cnt, 1024, d, rows, p0 + w * RUN, w, lane, k);
        }
        merge_runs<R>(rbuf, 1024, d, w, lane);

#pragma unroll
        for (int v0 = 0; v0 < R; v0 += SG) {
            if (!own_rows) break;   // wave-uniform; no barrier below
            // the own keys are loop-invariant; an opaque base keeps the compiler from hoisting
            // their loads out of the part loop, which would hold all 16 in registers again
            int ob = own0;
            asm volatile("" : "+s"(ob));
            uint64_t key[SG];
            int lt[SG], le[SG];
#pragma unroll
            for (int u = 0; u < SG; ++u) key[u] = rows.key(ob + (w * R + v0 + u) * WAVE + lane);
            count_in_sorted<SG, false>(rbuf, d, key, lt, le);
#pragma unroll
            for (int u = 0; u < SG; ++u) {
                lts[v0 + u] += lt[u];
                les[v0 + u] += le[u];
            }
        }
        __syncthreads();   // the next part overwrites rbuf and s_cnt
    }

    if (blockIdx.z == 0 && tid == 0 && a.nvalid != nullptr) a.nvalid[(int64_t)c * a.nseg + s] = n;
    double* __restrict__ D = a.dst + (int64_t)c * a.dst_stride + r0;
    const double dn = (double)n, dn1 = (double)(n + 1);
    const int method = a.method, scale = a.scale;
#pragma unroll
    for (int v = 0; v < R; ++v) {
        if (!own_rows) break;
        const int idx = own0 + (w * R + v) * WAVE + lane;
        const double y = rank_value(method, scale, lts[v], les[v], dn, dn1);
        if (idx < L) D[idx] = rows.key(idx) != SENT ? y : NAN;
    }
}

template <int R>
int launch_rank(const fm_rank_args& a, hipStream_t st) {
    const int nw = (a.max_seg_len + WAVE * R - 1) / (WAVE * R);
    const size_t lds = 8 * (size_t)nw * WAVE * R;
    if (lds >= 64 * 1024 && raise_dynamic_lds<rank_kernel<R>>(8 * 1024 * R, "fm_rank_transform") != FM_OK) return FM_EHIP;
    hipLaunchKernelGGL((rank_kernel<R>), dim3(a.nseg, a.ncols), dim3(nw * WAVE), lds, st, a);
    return FM_OK;
}

int launch_rank_long(const fm_rank_args& a, hipStream_t st) {
    if (raise_dynamic_lds<rank_long_kernel>(8 * RANK_PART, "fm_rank_transform") != FM_OK) return FM_EHIP;
    const int nslice = (a.max_seg_len + RANK_PART - 1) / RANK_PART;
    hipLaunchKernelGGL(rank_long_kernel, dim3(a.nseg, a.ncols, nslice), dim3(1024), 8 * (size_t)RANK_PART, st, a);
    return FM_OK;
}

}  // namespace
}  // namespace fm

extern "C" int fm_rank_transform(const fm_rank_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_rank_transform: null args");
    const fm_rank_args& a = *args;
    FM_REQUIRE(a.nseg >= 0 && a.max_seg_len >= 0 && a.ncols >= 0 && a.ncols <= 65535, "fm_rank_transform: bad sizes");
    FM_REQUIRE(a.method >= FM_RANK_AVERAGE && a.method <= FM_RANK_MAX, "fm_rank_transform: method must be 0 (average), 1 (min) or 2 (max)");
    FM_REQUIRE(a.scale >= FM_RANK_RAW && a.scale <= FM_RANK_UNIFORM, "fm_rank_transform: scale must be 0 (raw), 1 (pct) or 2 (uniform)");
    FM_REQUIRE(a.min_level >= 0 && a.min_level <= 255, "fm_rank_transform: min_level must be 0..255");
    FM_REQUIRE(a.src == nullptr || (const void*)a.src != (const void*)a.dst, "fm_rank_transform: dst must not be src");
    if (a.max_seg_len > RANK_MAX_ROWS) {
        set_error("fm_rank_transform: %d-row months exceed %d", a.max_seg_len, RANK_MAX_ROWS);
        return FM_ETOOBIG;
    }
    if (a.nseg == 0 || a.ncols == 0 || a.max_seg_len == 0) {
        if (a.nvalid != nullptr && a.nseg > 0 && a.ncols > 0)
            if (hipMemsetAsync(a.nvalid, 0, sizeof(int32_t) * (size_t)a.nseg * a.ncols, (hipStream_t)stream) != hipSuccess) {
                set_error("fm_rank_transform: hipMemsetAsync failed");
                return FM_EHIP;
            }
        return FM_OK;
    }
    FM_REQUIRE(a.src && a.dst && a.seg_off, "fm_rank_transform: null pointer");
    FM_REQUIRE(a.src_stride >= 0 && a.dst_stride >= 0, "fm_rank_transform: bad strides");
    hipStream_t st = (hipStream_t)stream;
    const int rc = a.max_seg_len <= RANK_SHORT_MAX ? launch_rank<8>(a, st)
                   : a.max_seg_len <= RANK_PART    ? launch_rank<16>(a, st)
                                                   : launch_rank_long(a, st);
    if (rc != FM_OK) return rc;
    FM_CHECK_LAUNCH("fm_rank_transform");
    return FM_OK;
}
