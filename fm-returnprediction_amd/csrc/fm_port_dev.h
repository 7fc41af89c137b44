// What the per-month sort kernels of fm_port.hip and fm_dsort.hip share: the month limit and the
// three workgroup forms, the LDS bitonic sort, and the exact order statistics (order_stat_keys).
#pragma once

#include "fm_common.h"
#include "fm_select_dev.h"

namespace fm {
namespace {

constexpr int PORT_MAX_ROWS = 16384;   // 16 rows per thread of a 1024-thread workgroup

constexpr int PSLOTS = 2 * (FM_MAX_PORTS - 1);   // order statistics per month
constexpr int PCAP = 2 * WAVE;         // keys per candidate bucket (one wave sorts it)
constexpr int PORT_FAST_MIN = 2048;    // more breakpoint rows: the sample select

__host__ __device__ inline int pow2_ceil(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// In-place ascending bitonic sort of buf[0..P) (P a power of two) by the NT-thread workgroup;
// ends with a barrier.
template <int NT>
__device__ __forceinline__ void lds_bitonic(uint64_t* buf, int P) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const uint64_t x = buf[i], y = buf[l];
                if ((x > y) == ((i & k) == 0)) {
                    buf[i] = y;
                    buf[l] = x;
                }
            }
            __syncthreads();
        }
    }
}

// Dynamic LDS of a month of up to max_seg_len rows: the keys of the full sort; months that can
// reach the sample select hold its tables instead.
size_t port_lds_bytes(int max_seg_len) {
    size_t lds = 8 * (size_t)pow2_ceil(max_seg_len);
    const size_t fast = 13 * (size_t)(max_seg_len <= 512 * 10 ? 512 : 1024) + (size_t)PSLOTS * PCAP * 8;
    if (max_seg_len > PORT_FAST_MIN && lds < fast) lds = fast;
    return lds;
}

// The kernel's form by the longest month: f(threads, rows per thread) as compile-time constants
template <class F>
int with_form(int max_seg_len, F f) {
    using std::integral_constant;
    if (max_seg_len <= 256 * 4) return f(integral_constant<int, 256>{}, integral_constant<int, 4>{});
    if (max_seg_len <= 512 * 10) return f(integral_constant<int, 512>{}, integral_constant<int, 10>{});
    return f(integral_constant<int, 1024>{}, integral_constant<int, 16>{});
}

// Shared scratch of order_stat_keys for NW-wave workgroups: trank in, okey out
template <int NW>
struct OrderSh {
    uint64_t okey[PSLOTS];
    int trank[PSLOTS], tslot[PSLOTS], tbase[PSLOTS], ccnt[PSLOTS];
    int iscr[NW];
    int n, over;
};

// sh.okey[t] = the key at ascending rank sh.trank[t] (t < nt <= PSLOTS) among the n > 0 rows of
// this month marked in bpm (the thread's rows v with bit v set; fe[v] is then not NaN).  The caller
// has stored sh.trank and zeroed sh.n and sh.over (no barrier needed in between); ends with a
// barrier.  port_kernel's phase 2, statement for statement.
template <int NT, int VPT>
__device__ __forceinline__ void order_stat_keys(const double (&fe)[VPT], uint32_t bpm, int n, int nt,
                                                uint64_t* pbuf, OrderSh<NT / WAVE>& sh) {
    constexpr int NW = NT / WAVE;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    bool have = false;   // block-uniform: sh.okey holds the keys at the target ranks
    if constexpr (NT >= 512) {
        if (n > PORT_FAST_MIN) {
            uint64_t* samp = pbuf;
            uint32_t* hist = reinterpret_cast<uint32_t*>(samp + NT);
            uint8_t* slot = reinterpret_cast<uint8_t*>(hist + NT);
            uint64_t* cand = reinterpret_cast<uint64_t*>(slot + NT);
            {
                const int first = bpm != 0u ? __ffs((int)bpm) - 1 : -1;
                uint64_t key = SENT;
#pragma unroll
                for (int v = 0; v < VPT; ++v) key = v == first ? dkey(fe[v]) : key;
                samp[tid] = key;
                hist[tid] = 0u;
                if (tid < PSLOTS) sh.ccnt[tid] = 0;
            }
            __syncthreads();
            lds_bitonic<NT>(samp, NT);
            int bk[VPT];   // min(#{samples <= key}, NT - 1): monotone in the key
#pragma unroll
            for (int v = 0; v < VPT; ++v) bk[v] = 0;
            constexpr int SG = VPT <= 10 ? VPT : 1;
#pragma unroll
            for (int v0 = 0; v0 < VPT; v0 += SG) {
                if (SG == 1 && !((bpm >> v0) & 1u)) continue;
#pragma unroll
                for (int step = NT / 2; step > 0; step >>= 1) {
#pragma unroll
                    for (int v = v0; v < v0 + SG; ++v) {
                        const uint64_t key = ((bpm >> v) & 1u) ? dkey(fe[v]) : SENT;
                        bk[v] += samp[bk[v] + step - 1] <= key ? step : 0;
                    }
                }
                if (SG == 1) atomicAdd(&hist[bk[v0]], 1u);
            }
            if (SG > 1) {
#pragma unroll
                for (int v = 0; v < VPT; ++v)
                    if ((bpm >> v) & 1u) atomicAdd(&hist[bk[v]], 1u);
            }
            __syncthreads();
            const int x = (int)hist[tid];
            int tot;
            const int excl = block_excl_scan<NW>(x, sh.iscr, &tot);
            const int trv = lane < nt ? sh.trank[lane] : -1;   // lane t: target rank t
            int flag = 0;
            for (int t = 0; t < nt; ++t) {
                const int r = __builtin_amdgcn_readlane(trv, t);
                flag |= (r >= excl && r < excl + x) ? 1 : 0;
            }
            int nslots;
            const int sid = block_excl_scan<NW>(flag, sh.iscr, &nslots);
            slot[tid] = flag ? (uint8_t)sid : (uint8_t)255;
            if (flag) {
                if (x > PCAP) sh.over = 1;
                for (int t = 0; t < nt; ++t) {
                    const int r = sh.trank[t];   // (divergent here: no readlane)
                    if (r >= excl && r < excl + x) {
                        sh.tslot[t] = sid;
                        sh.tbase[t] = excl;
                    }
                }
            }
            __syncthreads();
            if (sh.over == 0) {   // block-uniform
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    if ((bpm >> v) & 1u) {
                        const int sl = slot[bk[v]];
                        if (sl != 255) cand[sl * PCAP + atomicAdd(&sh.ccnt[sl], 1)] = dkey(fe[v]);
                    }
                }
                __syncthreads();
                for (int sl = w; sl < nslots; sl += NW) wave_sort_lds<PCAP / WAVE>(cand + sl * PCAP, sh.ccnt[sl]);
                __syncthreads();
                if (tid < nt) sh.okey[tid] = cand[sh.tslot[tid] * PCAP + sh.trank[tid] - sh.tbase[tid]];
                have = true;
            }
        }
    }
    if (!have) {
        __syncthreads();
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const bool isbp = (bpm >> v) & 1u;
            const uint64_t m = __ballot(isbp);
            const int c = (int)__popcll(m);
            int base = 0;
            if (lane == 0 && c > 0) base = atomicAdd(&sh.n, c);
            base = __builtin_amdgcn_readfirstlane(base);
            if (isbp) pbuf[base + mask_rank(m)] = dkey(fe[v]);
        }
        const int P = pow2_ceil(n);
        for (int i = n + tid; i < P; i += NT) pbuf[i] = SENT;
        __syncthreads();
        lds_bitonic<NT>(pbuf, P);
        if (tid < nt) sh.okey[tid] = pbuf[sh.trank[tid]];
    }
    __syncthreads();
}

}  // namespace
}  // namespace fm
