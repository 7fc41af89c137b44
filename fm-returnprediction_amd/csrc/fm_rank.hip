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
#include <math.h>

#include "fm_common.h"
#include "fm_select_dev.h"

// phase marks of rank_kernel (probe builds only, fm_common.h): 0 start, 1 runs sorted,
// 2 runs merged, 3 end
FM_PROBE_BUFFER(rank)

namespace fm {
namespace {

constexpr int RANK_MAX_ROWS = 16384;   // 16 rows per thread of a 1024-thread workgroup
constexpr int RANK_SHORT_MAX = 8192;   // months up to here: 8 rows per thread

// ascending compare-exchange of buf[i], buf[l] (i < l)
__device__ __forceinline__ void cmpx(uint64_t* buf, int i, int l) {
    const uint64_t x = buf[i], y = buf[l];
    if (x > y) {
        buf[i] = y;
        buf[l] = x;
    }
}

template <int R>
__global__ __launch_bounds__(1024) void rank_kernel(fm_rank_args a) {
    constexpr int RUN = WAVE * R;          // keys per wave = the sorted run length
    constexpr int SG = R < 8 ? R : 8;      // rows searched in step (that many LDS reads in flight)
    extern __shared__ uint64_t rbuf[];     // blockDim.x * R keys
    __shared__ int s_cnt[1024 / WAVE];
    const int s = blockIdx.x, c = blockIdx.y;
    const int NT = blockDim.x, nw = NT / WAVE;
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
    const int nrun = (L + RUN - 1) / RUN;   // <= nw: waves nrun.. hold no row
    const int Pact = nrun * RUN;
    int P2 = RUN;
    while (P2 < Pact) P2 <<= 1;

    // ---- 1. load, keys, per-wave sorted runs -------------------------------------------------
    const double* __restrict__ X = a.src + (int64_t)c * a.src_stride + r0;
    const uint8_t* __restrict__ LV = a.level != nullptr ? a.level + r0 : nullptr;
    uint64_t key[R];
    int cnt = 0;
    if (w < nrun) {   // wave-uniform
        const int last = L - 1;
#pragma unroll
        for (int v = 0; v < R; ++v) {   // unconditional (clamped) loads, masked after
            const int idx = (w * R + v) * WAVE + lane;
            const int ci = idx < L ? idx : last;
            const double x = X[ci] + 0.0;   // -0.0 -> +0.0: the two zeros tie
            const int lv = LV != nullptr ? (int)LV[ci] : 255;
            const bool elig = idx < L && !isnan(x) && lv >= a.min_level;
            key[v] = elig ? dkey(x) : SENT;
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
    for (int q = 0; q < nw; ++q) n += s_cnt[q];
    FM_PROBE_AT(rank, 1);

    // ---- 2. merge the runs -------------------------------------------------------------------
    for (int k = 2 * RUN; k <= P2; k <<= 1) {   // block-uniform
        const int h = k >> 1;
        for (int t = tid; t < (P2 >> 1); t += NT) {
            const int i = ((t & ~(h - 1)) << 1) | (t & (h - 1));
            const int l = i ^ (k - 1);
            if (l < Pact) cmpx(rbuf, i, l);
        }
        __syncthreads();
        for (int j = h >> 1; j >= RUN; j >>= 1) {
            for (int t = tid; t < (P2 >> 1); t += NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                if (l < Pact) cmpx(rbuf, i, l);
            }
            __syncthreads();
        }
        if (w < nrun) {   // the stages inside the run: distances RUN / 2 .. 1, all ascending
            uint64_t m[R];
#pragma unroll
            for (int v = 0; v < R; ++v) m[v] = rbuf[w * RUN + v * WAVE + lane];
            bitonic_u64_stages<R, 2 * RUN, RUN / 2>(m);
#pragma unroll
            for (int v = 0; v < R; ++v) rbuf[w * RUN + v * WAVE + lane] = m[v];
        }
        __syncthreads();
    }
    FM_PROBE_AT(rank, 2);

    // ---- 3. less / less + eq by two bound searches, ranks ------------------------------------
    if (tid == 0 && a.nvalid != nullptr) a.nvalid[(int64_t)c * a.nseg + s] = n;
    double* __restrict__ D = a.dst + (int64_t)c * a.dst_stride + r0;
    const double dn = (double)n, dn1 = (double)(n + 1);
    const int method = a.method, scale = a.scale;
    if (w < nrun) {
#pragma unroll
        for (int v0 = 0; v0 < R; v0 += SG) {
            int lt[SG], le[SG];   // #{sorted keys < key}, #{<= key}: the keys past n are SENT
#pragma unroll
            for (int u = 0; u < SG; ++u) lt[u] = 0;
            for (int step = P2 >> 1; step > 0; step >>= 1) {   // an eligible key has lt < n <= P2
#pragma unroll
                for (int u = 0; u < SG; ++u) {
                    const int pa = lt[u] + step - 1;
                    const uint64_t xa = rbuf[pa < Pact ? pa : Pact - 1];
                    lt[u] += (pa < Pact && xa < key[v0 + u]) ? step : 0;
                }
            }
            // a key whose successor differs ends its run of equals at lt + 1: only a wave that
            // holds a tied key among these rows runs the upper bound search (the same counts
            // either way)
            bool tied = false;
#pragma unroll
            for (int u = 0; u < SG; ++u) {
                const int pn = lt[u] + 1;
                const uint64_t xn = rbuf[pn < Pact ? pn : Pact - 1];
                tied |= pn < Pact && xn == key[v0 + u] && key[v0 + u] != SENT;
                le[u] = pn;
            }
            if (__ballot(tied) != 0ull) {   // wave-uniform
#pragma unroll
                for (int u = 0; u < SG; ++u) le[u] = 0;
                for (int step = P2; step > 0; step >>= 1) {   // from P2: le reaches P2 in a full month
#pragma unroll
                    for (int u = 0; u < SG; ++u) {
                        const int pb = le[u] + step - 1;
                        const uint64_t xb = rbuf[pb < Pact ? pb : Pact - 1];
                        le[u] += (pb < Pact && xb <= key[v0 + u]) ? step : 0;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SG; ++u) {
                const int idx = (w * R + v0 + u) * WAVE + lane;
                double r;   // a multiple of 0.5 below 2^15: exact
                if (method == FM_RANK_MIN) r = (double)(lt[u] + 1);
                else if (method == FM_RANK_MAX) r = (double)le[u];
                else r = 0.5 * (double)(lt[u] + le[u] + 1);
                double y = r;
                if (scale == FM_RANK_PCT) y = r / dn;
                else if (scale == FM_RANK_UNIFORM) y = r / dn1 - 0.5;
                if (idx < L) D[idx] = key[v0 + u] != SENT ? y : NAN;
            }
        }
    }
    FM_PROBE_AT(rank, 3);
}

template <int R>
int launch_rank(const fm_rank_args& a, hipStream_t st) {
    const int nw = (a.max_seg_len + WAVE * R - 1) / (WAVE * R);
    const size_t lds = 8 * (size_t)nw * WAVE * R;
    if (lds >= 64 * 1024) {   // beyond the default dynamic-LDS limit: opt in (once)
        static bool attr_set = false;
        if (!attr_set) {
            if (hipFuncSetAttribute((const void*)rank_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    8 * 1024 * R) != hipSuccess) {
                set_error("fm_rank_transform: cannot raise the dynamic LDS limit");
                return FM_EHIP;
            }
            attr_set = true;
        }
    }
    hipLaunchKernelGGL((rank_kernel<R>), dim3(a.nseg, a.ncols), dim3(nw * WAVE), lds, st, a);
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
    const int rc = a.max_seg_len <= RANK_SHORT_MAX ? launch_rank<8>(a, st) : launch_rank<16>(a, st);
    if (rc != FM_OK) return rc;
    FM_CHECK_LAUNCH("fm_rank_transform");
    return FM_OK;
}
