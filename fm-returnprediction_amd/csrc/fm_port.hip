// fm_portfolio_sort: forecast-sorted portfolios (build-defined extension A12; paper Table 5).
// One workgroup per month, four phases:
//   1. every thread loads its rows' forecast / level / NYSE byte once (wave w owns the rows
//      [w * VPT * 64, (w + 1) * VPT * 64), so row order = (wave, v, lane) order) and keeps the
//      eligible forecasts in registers, with a bit per breakpoint row;
//   2. the 2 (nport - 1) exact order statistics of the breakpoint rows' order-preserving keys:
//      months of more than 2,048 such rows by a sample select (splitters from a sorted sample,
//      a counting pass over the buckets, then only the buckets that hold a target rank are
//      gathered and sorted), shorter months and months whose target buckets overfill (heavy
//      ties) by an LDS bitonic sort of all keys; then the numpy 'linear' breakpoints (qranks /
//      qlerp, mode 0).  Both ways give the same keys, so which one ran never shows;
//   3. every row is binned against the breakpoints in LDS, its portfolio byte written, and a
//      stable partition (ballot ranks; per-wave counts prefixed over the waves) gives each row
//      its place in its portfolio's list, in row order;
//   4. the rows' owners read return and weight (coalesced, once) and stage one term at a time
//      at the rows' list places in the LDS the keys have left; wave k sums portfolio k's
//      stretch (lane l takes entries l, l + 64, ...) and reduces with the fixed butterfly:
//      every sum's order depends on the month's rows alone, not on the grid, the thread count
//      or the other months.
// Forecast, return, weight, level and NYSE byte are each read from HBM once (months of more
// than 5,120 rows re-read return and weight per term, from the cache).
//
// fm_forecast_portfolio_sort runs the same four phases (the same kernel template, instantiated
// with PanelSrc) over a grid of (month, sort), with phase 1's load replaced by the forecast itself:
// F = c0 + sum_k c_k clip(x_k) from the panel's own layout (FP64 columns or the split planes),
// predictor k in the outer loop (the month's c_k and cuts are wave-uniform) and the thread's
// VPT rows in the inner one (VPT independent loads in flight), accumulated in the fe registers
// the sort keeps anyway; phase 4 reads the return column through the same layout.  No clipped
// panel and no forecast vector ever reach HBM.
//
// The forecast statistics -- fm_forecast_dist (A14; paper Table 3; fdist_kernel), fm_forecast_compare
// (A15; paper Table 4; fcmp_kernel, over a grid of (month, pair)) and fm_forecast_horizon (A17; paper
// Section 4, second approach; fhor_kernel) -- keep the month in registers as phase 1 leaves it and are
// written in terms of the device helpers above fdist_kernel: load_eligible (phase 1 from the same three
// sources), quantile_keys (phase 2), load_returns, and for every sum masked_sum / tile_sum, whose order
// depends on the month's rows alone; fit_rows is the regression of one row set on another built from
// them.  No list is staged and no row is partitioned.
#include <math.h>

#include "fm_common.h"
#include "fm_port_dev.h"
#include "fm_select_dev.h"

// phase marks of port_kernel (probe builds only, fm_common.h): 0 start, 1 rows loaded and
// counted, 2 sample sorted, 3 buckets counted and targets located, 4 order statistics,
// 5 rows partitioned, 6 sums, 7 end
FM_PROBE_BUFFER(port)

namespace fm {
namespace {

// What a month's workgroup sorts by.  PlainSrc: the caller's forecast and return vectors
// (fm_portfolio_sort).  PanelSrc<PL>: sort j of the fm_forecast_src that fm_fport_args,
// fm_fdist_args, fm_fcmp_args and fm_fhor_args embed as `src`, panel values from the FP64 columns or
// (PL) from the planes, two 4-byte loads joined in registers.
struct PlainSrc {
    static constexpr bool FUSED = false;
    __device__ static PlainSrc make(const fm_port_args&) { return {}; }
};

template <bool PL>
struct PanelSrc {
    static constexpr bool FUSED = true;
    const fm_forecast_src& a;
    int j;   // blockIdx.y
    template <class A>
    __device__ static PanelSrc make(const A& args) { return {args.src, (int)blockIdx.y}; }
    __device__ __forceinline__ double value(int col, int64_t row) const {
        if constexpr (PL) {
            const int64_t o = (int64_t)col * a.plane_stride + row;
            const uint32_t h = a.hi_plane[o], l = a.lo_plane[o];
            return __longlong_as_double((long long)(((uint64_t)h << 32) | l));
        } else {
            return a.cols[(int64_t)col * a.col_stride + row];
        }
    }
};

// The fused load of month s of nseg (L > 0 rows from r0) of sort src.j: fe[v] = the forecast of
// the thread's row (w * VPT + v) * 64 + lane (clamped to the month's last row), written to
// forecast_out at ro on request.  Predictor k outside (c_k and the month's cuts are
// wave-uniform), the thread's rows inside (VPT independent loads in flight); every product and
// every sum rounds on its own (-ffp-contract=off), in fm_forecast's order.
template <int VPT, class Src>
__device__ __forceinline__ void fused_forecast(const Src& src, int nseg, int s, int64_t so, int64_t ro,
                                               int64_t r0, int L, int w, int lane, double (&fe)[VPT]) {
    const fm_forecast_src& a = src.a;
    const int last = L - 1;
    const int K = a.sel_k[src.j];
    const double* __restrict__ c = a.coef + so * a.coef_stride;
    const double c0 = c[0];
#pragma unroll
    for (int v = 0; v < VPT; ++v) fe[v] = c0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const int col = a.sel_cols[src.j][k];
        const double ck = c[1 + k];
        const double lo = a.lo != nullptr ? a.lo[(int64_t)col * nseg + s] : NAN;
        const double hi = a.hi != nullptr ? a.hi[(int64_t)col * nseg + s] : NAN;
        double x[VPT];
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int idx = (w * VPT + v) * WAVE + lane;
            x[v] = src.value(col, r0 + (idx < L ? idx : last));
        }
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            double y = x[v];   // fm_clip: a NaN value stays NaN, a NaN bound is ignored
            if (y < lo) y = lo;
            if (y > hi) y = hi;
            fe[v] = fe[v] + ck * y;
        }
    }
    if (a.forecast_out != nullptr) {
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int idx = (w * VPT + v) * WAVE + lane;
            if (idx < L) a.forecast_out[ro + idx] = fe[v];
        }
    }
}

// One month (of one sort) by the NT-thread workgroup: A is fm_port_args with PlainSrc,
// fm_fport_args with PanelSrc (the fields both share have the same names; the forecast's own
// are those of the embedded fm_forecast_src, a.src).  The body stays in
// the kernel itself: behind an inlined device function the 1024 x 16 form allocates 18 more VGPRs
// (the fused load alone, fused_forecast above, leaves every form's allocation as it was).
template <int NT, int VPT, class Src = PlainSrc, class A = fm_port_args>
__global__ __launch_bounds__(NT, NT >= 512 ? 4 : 2) void port_kernel(A a) {
    constexpr int NW = NT / WAVE;
    constexpr bool FUSED = Src::FUSED;
    const Src src = Src::make(a);
    extern __shared__ uint64_t pbuf[];   // the keys; after the breakpoints the row lists
    __shared__ double s_bp[FM_MAX_PORTS];
    __shared__ double s_rec[FM_MAX_PORTS][4];
    __shared__ double s_sum[FM_MAX_PORTS][6];
    __shared__ int s_wcnt[NW][FM_MAX_PORTS], s_wbase[NW][FM_MAX_PORTS];
    __shared__ int s_start[FM_MAX_PORTS + 1];
    __shared__ double s_g[FM_MAX_PORTS];
    __shared__ uint64_t s_okey[PSLOTS];
    __shared__ int s_trank[PSLOTS], s_tslot[PSLOTS], s_tbase[PSLOTS], s_ccnt[PSLOTS];
    __shared__ int s_iscr[NW];
    __shared__ int s_n, s_over;
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int nport = a.nport, nm1 = nport - 1;
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the LDS was sized from max_seg_len
    // outputs: month s of sort j at [j][s], row vectors at [j][row]
    int64_t so = s, ro = r0;
    int min_level;
    if constexpr (FUSED) {
        so += (int64_t)src.j * a.nseg;
        ro += (int64_t)src.j * a.src.nrows;
        min_level = a.src.sel_level[src.j];
    } else {
        min_level = a.min_level;
    }
    const double* __restrict__ F = nullptr;   // PlainSrc: the month's forecasts
    if constexpr (!FUSED) F = a.forecast + r0;

    FM_PROBE_AT(port, 0);
    // ---- 1. load, eligibility, breakpoint rows -------------------------------------------
    double fe[VPT];     // the eligible rows' forecasts, NaN otherwise
    uint32_t bpm = 0;   // bit v: row v of this thread is a breakpoint row
    if (L > 0) {        // block-uniform
        const int last = L - 1;
        if constexpr (FUSED) {
            fused_forecast<VPT>(src, a.nseg, s, so, ro, r0, L, w, lane, fe);
        }
#pragma unroll
        for (int v = 0; v < VPT; ++v) {   // unconditional (clamped) loads, masked after
            const int idx = (w * VPT + v) * WAVE + lane;
            const int ci = idx < L ? idx : last;
            double f;
            if constexpr (FUSED) f = fe[v];
            else f = F[ci];
            const int lv = a.level != nullptr ? (int)a.level[r0 + ci] : 255;
            const int ny = a.nyse != nullptr ? (int)a.nyse[r0 + ci] : 1;
            const bool elig = idx < L && isfinite(f) && lv >= min_level;
            fe[v] = elig ? f : NAN;
            bpm |= (elig && (a.nyse_breakpoints == 0 || ny != 0)) ? 1u << v : 0u;
        }
    } else {
#pragma unroll
        for (int v = 0; v < VPT; ++v) fe[v] = NAN;
    }
    const int n = block_sum<NW>((int)__popc(bpm), s_iscr);
    FM_PROBE_AT(port, 1);
    uint8_t* port = a.port != nullptr ? a.port + ro : nullptr;
    double* rec = a.rec + so * (nport + 1) * 4;
    int32_t* cnt = a.cnt + so * nport;

    if (n < a.min_count) {   // block-uniform: the month is unsorted
        if (tid == 0) a.status[so] = 0u;
        if (tid < nm1 && a.bp != nullptr) a.bp[so * nm1 + tid] = NAN;
        if (tid < (nport + 1) * 4) rec[tid] = NAN;
        if (tid < nport) cnt[tid] = 0;
        if (port != nullptr) {
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
                const int idx = (w * VPT + v) * WAVE + lane;
                if (idx < L) port[idx] = 255;
            }
        }
        return;
    }

    // ---- 2. the 2 (nport - 1) order statistics, breakpoints ----------------------------------
    const int nt = 2 * nm1;   // targets: ranks (i, j) of each level
    if (tid < nm1) {
        int i, j;
        double g;
        qranks(n, a.q[tid], 0, i, j, g);
        s_trank[2 * tid] = i;
        s_trank[2 * tid + 1] = j;
        s_g[tid] = g;
    }
    if (tid == 0) {
        s_n = 0;
        s_over = 0;
    }
    bool have = false;   // block-uniform: s_okey holds the keys at the target ranks
    if constexpr (NT >= 512) {
        if (n > PORT_FAST_MIN) {
            // Sample select: NT sample keys (each thread's first breakpoint row) sorted into
            // splitters; every key is bucketed by binary search, the buckets counted and
            // scanned, and only the buckets that hold a target rank are gathered (<= PCAP keys
            // each, else the full sort below) and sorted, one wave per bucket.  Exact whatever
            // the sample: a poor one only overfills a bucket.
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
                if (tid < PSLOTS) s_ccnt[tid] = 0;
            }
            __syncthreads();
            lds_bitonic<NT>(samp, NT);
            FM_PROBE_AT(port, 2);
            int bk[VPT];   // min(#{samples <= key}, NT - 1): monotone in the key
#pragma unroll
            for (int v = 0; v < VPT; ++v) bk[v] = 0;
            // all rows in step (VPT reads in flight) where the registers allow, else row by row
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
            const int excl = block_excl_scan<NW>(x, s_iscr, &tot);
            const int trv = lane < nt ? s_trank[lane] : -1;   // lane t: target rank t
            int flag = 0;
            for (int t = 0; t < nt; ++t) {
                const int r = __builtin_amdgcn_readlane(trv, t);
                flag |= (r >= excl && r < excl + x) ? 1 : 0;
            }
            int nslots;
            const int sid = block_excl_scan<NW>(flag, s_iscr, &nslots);
            slot[tid] = flag ? (uint8_t)sid : (uint8_t)255;
            if (flag) {
                if (x > PCAP) s_over = 1;
                for (int t = 0; t < nt; ++t) {
                    const int r = s_trank[t];   // (divergent here: no readlane)
                    if (r >= excl && r < excl + x) {
                        s_tslot[t] = sid;
                        s_tbase[t] = excl;
                    }
                }
            }
            __syncthreads();
            FM_PROBE_AT(port, 3);
            if (s_over == 0) {   // block-uniform
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    if ((bpm >> v) & 1u) {
                        const int sl = slot[bk[v]];
                        if (sl != 255) cand[sl * PCAP + atomicAdd(&s_ccnt[sl], 1)] = dkey(fe[v]);
                    }
                }
                __syncthreads();
                for (int sl = w; sl < nslots; sl += NW) wave_sort_lds<PCAP / WAVE>(cand + sl * PCAP, s_ccnt[sl]);
                __syncthreads();
                if (tid < nt) s_okey[tid] = cand[s_tslot[tid] * PCAP + s_trank[tid] - s_tbase[tid]];
                have = true;
            }
        }
    }
    if (!have) {
        // Full sort (short months, or an overfull bucket: heavy ties): the keys compacted into
        // LDS (ballot + one integer LDS add per wave; their order does not matter), padded to a
        // power of two, bitonic-sorted.
        __syncthreads();
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const bool isbp = (bpm >> v) & 1u;
            const uint64_t m = __ballot(isbp);
            const int c = (int)__popcll(m);
            int base = 0;
            if (lane == 0 && c > 0) base = atomicAdd(&s_n, c);
            base = __builtin_amdgcn_readfirstlane(base);
            if (isbp) pbuf[base + mask_rank(m)] = dkey(fe[v]);
        }
        const int P = pow2_ceil(n);
        for (int i = n + tid; i < P; i += NT) pbuf[i] = SENT;
        __syncthreads();
        lds_bitonic<NT>(pbuf, P);
        if (tid < nt) s_okey[tid] = pbuf[s_trank[tid]];
    }
    __syncthreads();
    if (tid < nm1) {
        const double b = qlerp(kval(s_okey[2 * tid]), kval(s_okey[2 * tid + 1]), s_g[tid], 0);
        s_bp[tid] = b;
        if (a.bp != nullptr) a.bp[so * nm1 + tid] = b;
    }
    FM_PROBE_AT(port, 4);
    __syncthreads();   // the keys are dead from here: pbuf becomes the row lists

    // ---- 3. bin the rows, stable partition by portfolio ------------------------------------
    int pt[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) pt[v] = 0;
    constexpr int BG = VPT <= 10 ? VPT : VPT / 2;   // rows binned against one LDS read of a breakpoint
#pragma unroll
    for (int v0 = 0; v0 < VPT; v0 += BG) {
        for (int j = 0; j < nm1; ++j) {
            const double b = s_bp[j];
#pragma unroll
            for (int v = v0; v < v0 + BG; ++v) pt[v] += fe[v] > b ? 1 : 0;
        }
    }
    int pos[VPT];   // the row's place in its portfolio's list (row order), -1: in no portfolio
    int cvec = 0;   // lane k: this wave's rows of portfolio k so far
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int idx = (w * VPT + v) * WAVE + lane;
        const int p = isnan(fe[v]) ? 255 : pt[v];
        if (port != nullptr && idx < L) port[idx] = (uint8_t)p;
        int pp = -1;   // (place among this wave's rows of p) << 8 | p
        for (int k = 0; k < nport; ++k) {
            const uint64_t m = __ballot(p == k);
            const int before = __builtin_amdgcn_readlane(cvec, k);
            if (p == k) pp = ((before + mask_rank(m)) << 8) | k;
            cvec += lane == k ? (int)__popcll(m) : 0;
        }
        pos[v] = pp;
    }
    if (lane < nport) s_wcnt[w][lane] = cvec;
    __syncthreads();
    {
        int before = 0, tot = 0;
        if (lane < nport) {
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                const int c = s_wcnt[q][lane];
                before += q < w ? c : 0;
                tot += c;
            }
        }
        const int incl = wave_incl_scan(tot);
        if (lane < nport) s_wbase[w][lane] = incl - tot + before;   // this wave's first place in list k
        if (w == 0) {
            if (lane < nport) s_start[lane] = incl - tot;
            if (lane == nm1) s_start[nport] = incl;
        }
    }
    wave_sync();
#pragma unroll
    for (int v = 0; v < VPT; ++v)
        if (pos[v] >= 0) pos[v] = (pos[v] >> 8) + s_wbase[w][pos[v] & 255];

    FM_PROBE_AT(port, 5);
    // ---- 4. per-portfolio sums ----------------------------------------------------------------
    // return and weight: read once, coalesced, by the rows' owners; kept in registers where the
    // budget allows (HOLD), else re-read per term from the cache
    constexpr bool HOLD = VPT <= 10;
    const double* __restrict__ R = nullptr;   // PlainSrc: the month's returns
    if constexpr (!FUSED) R = a.ret + r0;
    const double* __restrict__ W = a.weight != nullptr ? a.weight + r0 : nullptr;
    double r[HOLD ? VPT : 1], x[HOLD ? VPT : 1];
    if constexpr (HOLD) {
        const int last = L - 1;   // L > 0: the month is sorted
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int idx = (w * VPT + v) * WAVE + lane;
            const int ci = idx < L ? idx : last;
            if constexpr (FUSED) r[v] = src.value(a.ret_col, r0 + ci);   // the same layout view
            else r[v] = R[ci];
            x[v] = W != nullptr ? W[ci] : NAN;
        }
    }
    // One term at a time: every row's term is staged at its list position (pbuf, 8 bytes a row),
    // then wave k sums portfolio k's stretch (lane l takes entries l, l + 64, ...; the fixed
    // butterfly across lanes).  Rows that do not count stage 0.  Pass 0 stages the two counts as
    // one exact double: 1 for a finite return + 2^20 for a usable weight as well.
    double* stage = reinterpret_cast<double*>(pbuf);
    const int npass = W != nullptr ? 6 : 3;
#pragma unroll 1
    for (int t = 0; t < npass; ++t) {   // block-uniform
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            if (pos[v] >= 0) {
                const int idx = (w * VPT + v) * WAVE + lane;   // < L: the row is eligible
                double rr, ww;
                if constexpr (HOLD) {
                    rr = r[v];
                    ww = x[v];
                } else {
                    if constexpr (FUSED) rr = src.value(a.ret_col, r0 + idx);
                    else rr = R[idx];
                    ww = W != nullptr ? W[idx] : NAN;
                }
                const bool okr = isfinite(rr), okw = okr && isfinite(ww) && ww > 0.0;
                // term t = 1: r, 2: f, 3: w, 4: w r, 5: w f (a factor 1.0 is exact); selected by t
                // here, so that nothing is hoisted out of the pass loop into registers
                const double m1 = (t == 1 || t == 4) ? rr : ((t == 2 || t == 5) ? fe[v] : 1.0);
                const double m2 = t >= 3 ? ww : 1.0;
                double y = (t >= 3 ? okw : okr) ? m1 * m2 : 0.0;
                if (t == 0) y = (okr ? 1.0 : 0.0) + (okw ? 1048576.0 : 0.0);
                stage[pos[v]] = y;
            }
        }
        __syncthreads();
        for (int k = w; k < nport; k += NW) {   // wave-uniform
            const int beg = s_start[k], end = s_start[k + 1];
            double acc = 0.0;
            for (int p0 = beg; p0 < end; p0 += 4 * WAVE) {   // four reads in flight, added in order
                double y[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int p = p0 + u * WAVE + lane;
                    const double z = stage[p < end ? p : end - 1];
                    y[u] = p < end ? z : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc += y[u];
            }
            acc = wave_sum(acc);
            if (lane == 0) s_sum[k][t] = acc;
        }
        __syncthreads();
    }
    FM_PROBE_AT(port, 6);
    if (tid < nport) {
        const int k = tid;
        const int64_t both = (int64_t)s_sum[k][0];
        const int c = (int)(both & 1048575), cw = (int)(both >> 20);
        const double e0 = c > 0 ? s_sum[k][1] / (double)c : NAN, e1 = c > 0 ? s_sum[k][2] / (double)c : NAN;
        const double v0 = cw > 0 ? s_sum[k][4] / s_sum[k][3] : NAN, v1 = cw > 0 ? s_sum[k][5] / s_sum[k][3] : NAN;
        s_rec[k][0] = e0;
        s_rec[k][1] = e1;
        s_rec[k][2] = v0;
        s_rec[k][3] = v1;
        rec[k * 4 + 0] = e0;
        rec[k * 4 + 1] = e1;
        rec[k * 4 + 2] = v0;
        rec[k * 4 + 3] = v1;
        cnt[k] = c;
    }
    __syncthreads();
    if (tid < 4) rec[nport * 4 + tid] = s_rec[nm1][tid] - s_rec[0][tid];   // NaN if an end is NaN
    FM_PROBE_AT(port, 7);
    if (tid == 0) a.status[so] = 1u;
}

// The NT x VPT form of entry point `who` over `grid` (each instantiation opts in to its LDS on its own)
template <int NT, int VPT, class Src, class A>
int launch(const A& a, dim3 grid, size_t lds, const char* who, hipStream_t st) {
    if (lds >= 64 * 1024 && raise_dynamic_lds<port_kernel<NT, VPT, Src, A>>(8 * pow2_ceil(NT * VPT), who) != FM_OK) return FM_EHIP;
    hipLaunchKernelGGL((port_kernel<NT, VPT, Src, A>), grid, dim3(NT), lds, st, a);
    return check_launch(who);
}

// Every entry point here gives a month one workgroup: the refusal of longer months
int check_max_rows(int max_seg_len, const char* who) {
    if (max_seg_len <= PORT_MAX_ROWS) return FM_OK;
    set_error("%s: %d-row months exceed %d", who, max_seg_len, PORT_MAX_ROWS);
    return FM_ETOOBIG;
}

// What fm_forecast_dist and fm_forecast_horizon ask of the arguments they share
int check_dist_args(int nq, const double* q, int min_count, int max_seg_len, const char* who) {
    FM_REQUIRE(max_seg_len >= 0, "%s: bad sizes", who);
    FM_REQUIRE(nq >= 0 && nq <= FM_MAX_DIST_Q, "%s: nq must be 0..%d", who, FM_MAX_DIST_Q);
    for (int i = 0; i < nq; ++i) {
        const double lo = i == 0 ? 0.0 : q[i - 1];
        FM_REQUIRE(q[i] > lo && q[i] < 1.0, "%s: q must be strictly ascending in (0, 1)", who);
    }
    FM_REQUIRE(min_count >= 1, "%s: min_count must be >= 1", who);
    return FM_OK;
}

// What both sorts' entry points ask of the arguments they share
template <class A>
int check_sort_args(const A& a, const char* who) {
    FM_REQUIRE(a.nport >= 2 && a.nport <= FM_MAX_PORTS, "%s: nport must be 2..%d", who, FM_MAX_PORTS);
    for (int j = 0; j < a.nport - 1; ++j) {
        const double lo = j == 0 ? 0.0 : a.q[j - 1];
        FM_REQUIRE(a.q[j] > lo && a.q[j] < 1.0, "%s: q must be strictly ascending in (0, 1)", who);
    }
    FM_REQUIRE(a.nyse_breakpoints == 0 || a.nyse != nullptr, "%s: nyse_breakpoints needs nyse", who);
    FM_REQUIRE(a.min_count >= 1, "%s: min_count must be >= 1", who);
    return check_max_rows(a.max_seg_len, who);
}

// What both fused entry points ask of their fm_forecast_src over nseg months; vec: the caller's
// own forecast vectors are the source (fm_forecast_dist), so f holds no panel
int check_forecast_src(const fm_forecast_src& f, int nseg, const char* who, bool vec = false) {
    FM_REQUIRE(nseg >= 0 && f.nrows >= 0, "%s: bad sizes", who);
    FM_REQUIRE(f.nsel >= 0 && f.nsel <= FM_MAX_SORTS, "%s: nsel must be 0..%d", who, FM_MAX_SORTS);
    if (nseg == 0 || f.nsel == 0) return FM_OK;   // nothing is read: an empty call has no pointers
    for (int j = 0; j < f.nsel; ++j)
        FM_REQUIRE(f.sel_level[j] >= 0 && f.sel_level[j] <= 255, "%s: sel_level must be 0..255", who);
    const bool f64 = f.cols != nullptr, pl = f.hi_plane != nullptr || f.lo_plane != nullptr;
    if (vec) {
        FM_REQUIRE(!f64 && !pl, "%s: exactly one of forecast, cols and the planes must be given", who);
        FM_REQUIRE(f.forecast_out == nullptr, "%s: forecast_out goes with a panel source", who);
        return FM_OK;
    }
    FM_REQUIRE(f64 != pl, "%s: exactly one of cols and the planes must be given", who);
    FM_REQUIRE(!pl || (f.hi_plane != nullptr && f.lo_plane != nullptr), "%s: both planes are needed", who);
    FM_REQUIRE((f64 ? f.col_stride : f.plane_stride) >= f.nrows, "%s: stride below the row count", who);
    FM_REQUIRE(f.ncols >= 1, "%s: ncols must be >= 1", who);
    FM_REQUIRE((f.lo == nullptr) == (f.hi == nullptr), "%s: lo and hi go together", who);
    for (int j = 0; j < f.nsel; ++j) {
        const int K = f.sel_k[j];
        FM_REQUIRE(K >= 1 && K <= FM_MAX_SORT_K, "%s: sort %d has K = %d, not 1..%d", who, j, K, FM_MAX_SORT_K);
        FM_REQUIRE(f.coef_stride >= K + 1, "%s: coef_stride %d below K + 1 = %d", who, f.coef_stride, K + 1);
        for (int k = 0; k < K; ++k)
            FM_REQUIRE(f.sel_cols[j][k] >= 0 && f.sel_cols[j][k] < f.ncols,
                       "%s: sort %d column %d outside the panel's %d", who, j, f.sel_cols[j][k], f.ncols);
    }
    FM_REQUIRE(f.coef != nullptr, "%s: null pointer", who);
    return FM_OK;
}

// ---- what the forecast statistics share ------------------------------------------------------
// Phases 1-2 are port_kernel's (the same loads, fused_forecast, the same sample select and full
// sort, here as the device function order_stat_keys: port_kernel keeps its own text for the
// register count noted above it, and tests/test_gpu_fdist.py holds the two to the same keys).
// Every sum over a month's rows goes through tile_sum, by way of masked_sum.

// The plain source of fm_forecast_dist and fm_forecast_horizon: sort j's forecasts are the caller's vector j
struct VecSrc {
    static constexpr bool FUSED = false;
    int j;   // blockIdx.y
    template <class A>
    __device__ static VecSrc make(const A&) { return {(int)blockIdx.y}; }
};

// The fixed-order sum of one term per row of the month (x[v] for the thread's row v; +0.0 for
// rows that do not count): each 64-row tile in row order by the wave butterfly (tile w * VPT + v
// is wave w's register v), then lane l of wave 0 adds the tile sums l, l + 64, ... in order and
// the butterfly runs again.  A tile past the month's end sums to +0.0 and adding it changes
// nothing (the lane's sum starts at +0.0, so it is never -0.0): the result does not depend on
// how many tiles the workgroup's form has.  Block-uniform result; two barriers.
template <int NW, int VPT>
__device__ __forceinline__ double tile_sum(const double (&x)[VPT], double* s_tile, int w, int lane) {
    constexpr int NTILE = NW * VPT;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const double t = wave_sum(x[v]);
        if (lane == 0) s_tile[w * VPT + v] = t;
    }
    __syncthreads();
    if (w == 0) {
        double acc = 0.0;
        for (int i = lane; i < NTILE; i += WAVE) acc += s_tile[i];
        acc = wave_sum(acc);
        if (lane == 0) s_tile[NTILE] = acc;
    }
    __syncthreads();
    return s_tile[NTILE];
}

// tile_sum of term(v) over the thread's rows whose bit of mask is set (+0.0 for the others); term
// is a lambda over the caller's registers
template <int NW, int VPT, class Term>
__device__ __forceinline__ double masked_sum(uint32_t mask, double* s_tile, int w, int lane, Term term) {
    double x[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) x[v] = ((mask >> v) & 1u) ? term(v) : 0.0;
    return tile_sum<NW, VPT>(x, s_tile, w, lane);
}

// The thread's row v of an L-row month: row_index is in the month when it is below L; every load
// goes to row_clamped (the month's last row beyond it), unconditionally, and is masked after
template <int VPT>
__device__ __forceinline__ int row_index(int w, int v, int lane) {
    return (w * VPT + v) * WAVE + lane;
}
__device__ __forceinline__ int row_clamped(int idx, int L) { return idx < L ? idx : L - 1; }
__device__ __forceinline__ int row_level(const uint8_t* level, int64_t row) {
    return level != nullptr ? (int)level[row] : 255;
}

// Phase 1 of month s of sort src.j (L rows from r0; A is fm_fdist_args or fm_fhor_args): fe[v] = the
// forecast of the thread's row v, fused or from the caller's vector, where the row is eligible (in
// the month, finite, at the sort's level), NaN elsewhere.  Returns the eligible rows' bit mask.
template <int VPT, class A, class Src>
__device__ __forceinline__ uint32_t load_eligible(const A& a, const Src& src, int s, int64_t so, int64_t ro,
                                                  int64_t r0, int L, int w, int lane, double (&fe)[VPT]) {
    uint32_t mask = 0;
    if (L > 0) {   // block-uniform
        const int min_level = a.src.sel_level[src.j];
        if constexpr (Src::FUSED) fused_forecast<VPT>(src, a.nseg, s, so, ro, r0, L, w, lane, fe);
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int idx = row_index<VPT>(w, v, lane), ci = row_clamped(idx, L);
            double f;
            if constexpr (Src::FUSED) f = fe[v];
            else f = a.forecast[ro + ci];
            const int lv = row_level(a.level, r0 + ci);   // loaded whatever f is, not behind the && below
            const bool elig = idx < L && isfinite(f) && lv >= min_level;
            fe[v] = elig ? f : NAN;
            mask |= elig ? 1u << v : 0u;
        }
    } else {
#pragma unroll
        for (int v = 0; v < VPT; ++v) fe[v] = NAN;
    }
    return mask;
}

// Phase 2: the 2 nq order statistics of the n rows of mask (their forecasts in fe) that the levels
// q need, as keys in sh.okey[2 i], sh.okey[2 i + 1] with the interpolation weight in s_g[i]; the
// caller's thread i < nq makes quantile i of them with qlerp.  nq > 0, block-uniform.
template <int NT, int VPT, class Sh>
__device__ __forceinline__ void quantile_keys(const double (&fe)[VPT], uint32_t mask, int n, int nq, const double* q,
                                              uint64_t* pbuf, Sh& sh, double* s_g) {
    const int tid = threadIdx.x;
    if (tid < nq) {
        int i, j;
        double g;
        qranks(n, q[tid], 0, i, j, g);
        sh.trank[2 * tid] = i;
        sh.trank[2 * tid + 1] = j;
        s_g[tid] = g;
    }
    if (tid == 0) {
        sh.n = 0;
        sh.over = 0;
    }
    order_stat_keys<NT, VPT>(fe, mask, n, 2 * nq, pbuf, sh);
}

// The thread's returns into x, get(row of the month) each, read once (when the registers are free).
// Returns the bit mask of set R: the rows of em with a finite return.
template <int VPT, class Get>
__device__ __forceinline__ uint32_t load_returns(uint32_t em, int L, int w, int lane, Get get, double (&x)[VPT]) {
    uint32_t rm = 0;
    if (L <= 0) return rm;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        x[v] = get(row_clamped(row_index<VPT>(w, v, lane), L));
        rm |= (((em >> v) & 1u) && isfinite(x[v])) ? 1u << v : 0u;
    }
    return rm;
}

// r regressed on g over the n rows of mask: both are centred in place on their means over the
// mask, then Sgg, Sgr, Srr.  NaN when n < 2 (block-uniform).
struct RowFit {
    double slope, icept, r2;
};
template <int NW, int VPT>
__device__ __forceinline__ RowFit fit_rows(uint32_t mask, int n, double (&g)[VPT], double (&r)[VPT], double* s_tile,
                                           int w, int lane) {
    if (n < 2) return {NAN, NAN, NAN};
    const double mg = masked_sum<NW, VPT>(mask, s_tile, w, lane, [&](int v) { return g[v]; }) / (double)n;
    const double mr = masked_sum<NW, VPT>(mask, s_tile, w, lane, [&](int v) { return r[v]; }) / (double)n;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        g[v] = g[v] - mg;
        r[v] = r[v] - mr;
    }
    const double Sgg = masked_sum<NW, VPT>(mask, s_tile, w, lane, [&](int v) { return g[v] * g[v]; });
    const double Sgr = masked_sum<NW, VPT>(mask, s_tile, w, lane, [&](int v) { return g[v] * r[v]; });
    const double Srr = masked_sum<NW, VPT>(mask, s_tile, w, lane, [&](int v) { return r[v] * r[v]; });
    const double slope = Sgr / Sgg;
    return {slope, mr - slope * mg, (Sgr * Sgr) / (Sgg * Srr)};
}

// ---- fm_forecast_dist (extension A14; paper Table 3) -----------------------------------------
// Per (month, sort): the count, mean, ddof-1 standard deviation and nq quantiles of the eligible
// forecasts.  Neither return nor weight is read.
template <int NT, int VPT, class Src>
__global__ __launch_bounds__(NT, NT >= 512 ? 4 : 2) void fdist_kernel(fm_fdist_args a) {
    constexpr int NW = NT / WAVE;
    const Src src = Src::make(a);
    extern __shared__ uint64_t pbuf[];   // the keys of the order statistics
    __shared__ OrderSh<NW> sh;
    __shared__ double s_g[FM_MAX_DIST_Q];
    __shared__ double s_tile[NW * VPT + 1];
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int nq = a.nq, nrec = 2 + nq;
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the LDS was sized from max_seg_len
    const int64_t so = s + (int64_t)src.j * a.nseg, ro = r0 + (int64_t)src.j * a.src.nrows;

    double fe[VPT];   // the eligible rows' forecasts, NaN otherwise
    const uint32_t bpm = load_eligible<VPT>(a, src, s, so, ro, r0, L, w, lane, fe);
    const int n = block_sum<NW>((int)__popc(bpm), sh.iscr);
    double* rec = a.rec + so * nrec;
    if (tid == 0) a.cnt[so] = n;
    if (n < a.min_count) {   // block-uniform
        if (tid == 0) a.status[so] = 0u;
        if (tid < nrec) rec[tid] = NAN;
        return;
    }
    if (nq > 0) {   // block-uniform
        quantile_keys<NT, VPT>(fe, bpm, n, nq, a.q, pbuf, sh, s_g);
        if (tid < nq) rec[2 + tid] = qlerp(kval(sh.okey[2 * tid]), kval(sh.okey[2 * tid + 1]), s_g[tid], 0);
    }
    // the mean, then the squared deviations from it
    const double mean = masked_sum<NW, VPT>(bpm, s_tile, w, lane, [&](int v) { return fe[v]; }) / (double)n;
    const double ss = masked_sum<NW, VPT>(bpm, s_tile, w, lane, [&](int v) {
        const double d = fe[v] - mean;
        return d * d;
    });
    if (tid == 0) {
        rec[0] = mean;
        rec[1] = n > 1 ? sqrt(ss / (double)(n - 1)) : NAN;
        a.status[so] = 1u;
    }
}

template <int NT, int VPT, class Src>
int launch_fdist(const fm_fdist_args& a, size_t lds, hipStream_t st) {
    const char* who = "fm_forecast_dist";
    if (lds >= 64 * 1024 && raise_dynamic_lds<fdist_kernel<NT, VPT, Src>>(8 * pow2_ceil(NT * VPT), who) != FM_OK) return FM_EHIP;
    hipLaunchKernelGGL((fdist_kernel<NT, VPT, Src>), dim3(a.nseg, a.src.nsel), dim3(NT), lds, st, a);
    return check_launch(who);
}

// ---- fm_forecast_compare (extension A15; paper Table 4) --------------------------------------
// Per (month, pair): forecast b regressed on forecast a over the rows where both are finite, then
// the realised return regressed on that regression's residual (fit_rows).  Phase 1 loads two
// forecasts (fused_forecast for the pair's two sorts, or the caller's two vectors), so it keeps its
// own shape; no order statistics follow, so there are no keys: the month stays in registers and
// eleven masked_sums (2 + 3 + 1 + 5) reduce it.  The register budget of the 1024 x 16 form (128
// VGPRs) holds two row sets of 16 doubles, not three: the deviations replace the forecasts, the
// residual replaces F_b's deviation, and the return is loaded only then, into the registers F_a's
// deviation has left.  Each forecast column is read from HBM once per pair, the return once.

// The plain source of fm_forecast_compare: the caller's forecast vectors and return vector
struct CmpVecSrc {
    static constexpr bool FUSED = false;
};

// The fused 1024 x 16 form: F_a, F_b and the load's 16 panel values in flight are three row sets, so
// F_a waits in dynamic LDS (8 bytes a row, 128 KB: the form has one workgroup per CU anyway)
template <int VPT, class Src>
constexpr bool fcmp_parks() {
    return Src::FUSED && VPT > 10;
}

template <int NT, int VPT, class Src>
__global__ __launch_bounds__(NT, NT >= 512 ? 4 : 2) void fcmp_kernel(fm_fcmp_args a) {
    constexpr int NW = NT / WAVE;
    constexpr bool FUSED = Src::FUSED;
    constexpr bool PARK = fcmp_parks<VPT, Src>();
    extern __shared__ double s_park[];   // PARK: F_a while F_b's load has the registers
    __shared__ double s_tile[NW * VPT + 1];
    __shared__ int s_iscr[NW];
    const int s = blockIdx.x, p = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int ja = a.pair_a[p], jb = a.pair_b[p], min_level = a.pair_level[p];
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the workgroup's form was chosen from max_seg_len
    const int64_t so = s + (int64_t)p * a.nseg;
    double* rec = a.rec + so * FM_FCMP_NREC;
    auto sum = [&](uint32_t mask, auto term) { return masked_sum<NW, VPT>(mask, s_tile, w, lane, term); };

    // ---- 1. the two forecasts, set E ----------------------------------------------------------
    double fa[VPT], fb[VPT];   // F_a, F_b; then their deviations; fb then the residual, fa the return
    uint32_t em = 0;           // bit v: row v of this thread is in E
    if (L > 0) {               // block-uniform
        if constexpr (FUSED) {
            const Src sa{a.src, ja}, sb{a.src, jb};
            fused_forecast<VPT>(sa, a.nseg, s, s + (int64_t)ja * a.nseg, r0 + (int64_t)ja * a.src.nrows, r0, L, w, lane, fa);
            if constexpr (PARK) {   // each thread parks and fetches its own rows: no barrier
#pragma unroll
                for (int v = 0; v < VPT; ++v) s_park[row_index<VPT>(w, v, lane)] = fa[v];
            }
            fused_forecast<VPT>(sb, a.nseg, s, s + (int64_t)jb * a.nseg, r0 + (int64_t)jb * a.src.nrows, r0, L, w, lane, fb);
            if constexpr (PARK) {
#pragma unroll
                for (int v = 0; v < VPT; ++v) fa[v] = s_park[row_index<VPT>(w, v, lane)];
            }
        }
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int idx = row_index<VPT>(w, v, lane), ci = row_clamped(idx, L);
            if constexpr (!FUSED) {
                fa[v] = a.forecast[(int64_t)ja * a.src.nrows + r0 + ci];
                fb[v] = a.forecast[(int64_t)jb * a.src.nrows + r0 + ci];
            }
            const int lv = row_level(a.level, r0 + ci);
            em |= (idx < L && isfinite(fa[v]) && isfinite(fb[v]) && lv >= min_level) ? 1u << v : 0u;
        }
    }
    const int nE = block_sum<NW>((int)__popc(em), s_iscr);
    const int need = a.min_count > 2 ? a.min_count : 2;
    auto ret_of = [&](int ci) {
        if constexpr (FUSED) return Src{a.src, 0}.value(a.ret_col, r0 + ci);   // the same layout view
        else return a.ret[r0 + ci];
    };
    if (nE < need) {   // block-uniform: the month has no regression
        const uint32_t rm = load_returns<VPT>(em, L, w, lane, ret_of, fa);
        const int nR = block_sum<NW>((int)__popc(rm), s_iscr);
        if (tid == 0) {
            a.cnt[so * 2] = nE;
            a.cnt[so * 2 + 1] = nR;
            a.status[so] = 0u;
        }
        if (tid < FM_FCMP_NREC) rec[tid] = NAN;
        return;
    }

    // ---- 2. b on a over E: means, centered moments, the residual's own sum ---------------------
    const double ma = sum(em, [&](int v) { return fa[v]; }) / (double)nE;
    const double mb = sum(em, [&](int v) { return fb[v]; }) / (double)nE;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        fa[v] = fa[v] - ma;   // da
        fb[v] = fb[v] - mb;   // db
    }
    const double Saa = sum(em, [&](int v) { return fa[v] * fa[v]; });
    const double Sbb = sum(em, [&](int v) { return fb[v] * fb[v]; });
    const double Sab = sum(em, [&](int v) { return fa[v] * fb[v]; });
    const double beta = Sab / Saa;
#pragma unroll
    for (int v = 0; v < VPT; ++v) fb[v] = fb[v] - beta * fa[v];   // e
    const double See0 = sum(em, [&](int v) { return fb[v] * fb[v]; });

    // ---- 3. the return (into F_a's registers) on the residual over R ---------------------------
    const uint32_t rm = load_returns<VPT>(em, L, w, lane, ret_of, fa);
    const int nR = block_sum<NW>((int)__popc(rm), s_iscr);
    const RowFit fit = fit_rows<NW, VPT>(rm, nR, fb, fa, s_tile, w, lane);
    if (tid == 0) {
        rec[0] = Sab / sqrt(Saa * Sbb);
        rec[1] = beta;
        rec[2] = mb - beta * ma;
        rec[3] = sqrt(See0 / (double)(nE - 1));
        rec[4] = fit.slope;
        rec[5] = fit.icept;
        rec[6] = fit.r2;
        a.cnt[so * 2] = nE;
        a.cnt[so * 2 + 1] = nR;
        a.status[so] = 1u;
    }
}

template <int NT, int VPT, class Src>
int launch_fcmp(const fm_fcmp_args& a, hipStream_t st) {
    const char* who = "fm_forecast_compare";
    const size_t lds = fcmp_parks<VPT, Src>() ? 8 * (size_t)NT * VPT : 0;
    if (lds >= 64 * 1024 && raise_dynamic_lds<fcmp_kernel<NT, VPT, Src>>(lds, who) != FM_OK) return FM_EHIP;
    hipLaunchKernelGGL((fcmp_kernel<NT, VPT, Src>), dim3(a.nseg, a.npair), dim3(NT), lds, st, a);
    return check_launch(who);
}

// ---- fm_forecast_horizon (extension A17; the paper's Section 4, second approach) --------------
// Per (month, sort): the monthly forecast F scaled to G = a m + g (F - m) around the month's mean
// m, G's mean, standard deviation and quantiles, and the realised long-horizon return regressed on
// G (fit_rows).  The order statistics are F's (G is non-decreasing in F, so F's mapped to G are
// G's); the mean comes first, since the mapping needs it.  Then G replaces F in the fe registers,
// and eight sums in all reduce the month (three in the body, five in fit_rows).  The return vector
// is read last, once, into registers of its own: with fe and the term being summed that is
// fcmp_kernel's budget of two row sets and a transient third.

// G of one forecast: three operations, each rounded on its own
__device__ __forceinline__ double fhor_scale(double f, double m, double base, double g) {
    const double d = f - m;
    return base + g * d;
}

template <int NT, int VPT, class Src>
__global__ __launch_bounds__(NT, NT >= 512 ? 4 : 2) void fhor_kernel(fm_fhor_args a) {
    constexpr int NW = NT / WAVE;
    const Src src = Src::make(a);
    extern __shared__ uint64_t pbuf[];   // the keys of the order statistics
    __shared__ OrderSh<NW> sh;
    __shared__ double s_g[FM_MAX_DIST_Q];
    __shared__ double s_tile[NW * VPT + 1];
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int nq = a.nq, nrec = FM_FHOR_NREC + nq;
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the LDS was sized from max_seg_len
    const int64_t so = s + (int64_t)src.j * a.nseg, ro = r0 + (int64_t)src.j * a.src.nrows;

    // ---- 1. load, set E -------------------------------------------------------------------------
    double fe[VPT];   // the rows' forecasts F, NaN outside E; from phase 3 on G, then G - mg
    const uint32_t em = load_eligible<VPT>(a, src, s, so, ro, r0, L, w, lane, fe);
    const int nE = block_sum<NW>((int)__popc(em), sh.iscr);
    double* rec = a.rec + so * nrec;
    double* gout = a.scaled_out != nullptr ? a.scaled_out + ro : nullptr;
    auto ret_of = [&](int ci) { return a.ret[r0 + ci]; };
    if (nE < a.min_count) {   // block-uniform: the month has no scaled forecast
        double x[VPT];
        const uint32_t rm = load_returns<VPT>(em, L, w, lane, ret_of, x);
        const int nR = block_sum<NW>((int)__popc(rm), sh.iscr);
        if (tid == 0) {
            a.cnt[so * 2] = nE;
            a.cnt[so * 2 + 1] = nR;
            a.status[so] = 0u;
        }
        if (tid < nrec) rec[tid] = NAN;
        if (gout != nullptr) {
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
                const int idx = row_index<VPT>(w, v, lane);
                if (idx < L) gout[idx] = NAN;
            }
        }
        return;
    }

    // ---- 2. the mean of F, then the quantiles of G from F's order statistics -------------------
    // masked_sum's text in the body, here and twice in phase 3: through the helper these three sums
    // cost the launch 0.2-0.5 %
    double x[VPT];
#pragma unroll
    for (int v = 0; v < VPT; ++v) x[v] = ((em >> v) & 1u) ? fe[v] : 0.0;
    const double m = tile_sum<NW, VPT>(x, s_tile, w, lane) / (double)nE;
    const double g = a.gain, base = a.level_mult * m;
    if (nq > 0) {   // block-uniform
        quantile_keys<NT, VPT>(fe, em, nE, nq, a.q, pbuf, sh, s_g);
        if (tid < nq)
            rec[FM_FHOR_NREC + tid] = qlerp(fhor_scale(kval(sh.okey[2 * tid]), m, base, g),
                                            fhor_scale(kval(sh.okey[2 * tid + 1]), m, base, g), s_g[tid], 0);
    }

    // ---- 3. G in place of F; its mean and standard deviation over E ----------------------------
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        fe[v] = ((em >> v) & 1u) ? fhor_scale(fe[v], m, base, g) : NAN;
        const int idx = row_index<VPT>(w, v, lane);
        if (gout != nullptr && idx < L) gout[idx] = fe[v];
    }
    // (the two sums below keep their own text, not masked_sum: see phase 2)
#pragma unroll
    for (int v = 0; v < VPT; ++v) x[v] = ((em >> v) & 1u) ? fe[v] : 0.0;
    const double mG = tile_sum<NW, VPT>(x, s_tile, w, lane) / (double)nE;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const double d = fe[v] - mG;
        x[v] = ((em >> v) & 1u) ? d * d : 0.0;
    }
    const double ss = tile_sum<NW, VPT>(x, s_tile, w, lane);

    // ---- 4. the return on G over R ----------------------------------------------------------------
    double r[VPT];
    const uint32_t rm = load_returns<VPT>(em, L, w, lane, ret_of, r);
    const int nR = block_sum<NW>((int)__popc(rm), sh.iscr);
    const RowFit fit = fit_rows<NW, VPT>(rm, nR, fe, r, s_tile, w, lane);
    if (tid == 0) {
        rec[0] = mG;
        rec[1] = nE > 1 ? sqrt(ss / (double)(nE - 1)) : NAN;
        rec[2] = fit.slope;
        rec[3] = fit.icept;
        rec[4] = fit.r2;
        rec[5] = m;
        a.cnt[so * 2] = nE;
        a.cnt[so * 2 + 1] = nR;
        a.status[so] = 1u;
    }
}

template <int NT, int VPT, class Src>
int launch_fhor(const fm_fhor_args& a, size_t lds, hipStream_t st) {
    const char* who = "fm_forecast_horizon";
    if (lds >= 64 * 1024 && raise_dynamic_lds<fhor_kernel<NT, VPT, Src>>(8 * pow2_ceil(NT * VPT), who) != FM_OK) return FM_EHIP;
    hipLaunchKernelGGL((fhor_kernel<NT, VPT, Src>), dim3(a.nseg, a.src.nsel), dim3(NT), lds, st, a);
    return check_launch(who);
}

}  // namespace
}  // namespace fm

extern "C" int fm_portfolio_sort(const fm_port_args* args, void* stream) {
    using namespace fm;
    FM_REQUIRE(args != nullptr, "fm_portfolio_sort: null args");
    const fm_port_args& a = *args;
    FM_REQUIRE(a.nseg >= 0 && a.max_seg_len >= 0, "fm_portfolio_sort: bad sizes");
    FM_REQUIRE(a.min_level >= 0 && a.min_level <= 255, "fm_portfolio_sort: min_level must be 0..255");
    if (const int rc = check_sort_args(a, "fm_portfolio_sort")) return rc;
    if (a.nseg == 0) return FM_OK;
    FM_REQUIRE(a.forecast && a.ret && a.seg_off && a.rec && a.cnt && a.status, "fm_portfolio_sort: null pointer");
    const char* who = "fm_portfolio_sort";
    const size_t lds = port_lds_bytes(a.max_seg_len);
    return with_form(a.max_seg_len, [&](auto nt, auto vpt) {
        return launch<nt, vpt, PlainSrc>(a, dim3(a.nseg), lds, who, (hipStream_t)stream);
    });
}

extern "C" int fm_forecast_portfolio_sort(const fm_fport_args* args, void* stream) {
    using namespace fm;
    const char* who = "fm_forecast_portfolio_sort";
    FM_REQUIRE(args != nullptr, "%s: null args", who);
    const fm_fport_args& a = *args;
    FM_REQUIRE(a.max_seg_len >= 0, "%s: bad sizes", who);
    if (const int rc = check_sort_args(a, who)) return rc;
    if (const int rc = check_forecast_src(a.src, a.nseg, who)) return rc;
    if (a.nseg == 0 || a.src.nsel == 0) return FM_OK;   // nothing is read: an empty panel has no pointers
    FM_REQUIRE(a.ret_col >= 0 && a.ret_col < a.src.ncols, "%s: ret_col outside the panel", who);
    FM_REQUIRE(a.seg_off && a.rec && a.cnt && a.status, "%s: null pointer", who);
    const bool pl = a.src.hi_plane != nullptr;
    const dim3 grid(a.nseg, a.src.nsel);
    const size_t lds = port_lds_bytes(a.max_seg_len);
    return with_form(a.max_seg_len, [&](auto nt, auto vpt) {
        return pl ? launch<nt, vpt, PanelSrc<true>>(a, grid, lds, who, (hipStream_t)stream)
                  : launch<nt, vpt, PanelSrc<false>>(a, grid, lds, who, (hipStream_t)stream);
    });
}

extern "C" int fm_forecast_dist(const fm_fdist_args* args, void* stream) {
    using namespace fm;
    const char* who = "fm_forecast_dist";
    FM_REQUIRE(args != nullptr, "%s: null args", who);
    const fm_fdist_args& a = *args;
    if (const int rc = check_dist_args(a.nq, a.q, a.min_count, a.max_seg_len, who)) return rc;
    if (const int rc = check_max_rows(a.max_seg_len, who)) return rc;
    const bool vec = a.forecast != nullptr;
    if (const int rc = check_forecast_src(a.src, a.nseg, who, vec)) return rc;
    if (a.nseg == 0 || a.src.nsel == 0) return FM_OK;   // nothing is read: an empty call has no pointers
    FM_REQUIRE(a.seg_off && a.rec && a.cnt && a.status, "%s: null pointer", who);
    const bool pl = a.src.hi_plane != nullptr;
    const size_t lds = port_lds_bytes(a.max_seg_len);
    const hipStream_t st = (hipStream_t)stream;
    return with_form(a.max_seg_len, [&](auto nt, auto vpt) {
        if (vec) return launch_fdist<nt, vpt, VecSrc>(a, lds, st);
        return pl ? launch_fdist<nt, vpt, PanelSrc<true>>(a, lds, st) : launch_fdist<nt, vpt, PanelSrc<false>>(a, lds, st);
    });
}

extern "C" int fm_forecast_horizon(const fm_fhor_args* args, void* stream) {
    using namespace fm;
    const char* who = "fm_forecast_horizon";
    FM_REQUIRE(args != nullptr, "%s: null args", who);
    const fm_fhor_args& a = *args;
    if (const int rc = check_dist_args(a.nq, a.q, a.min_count, a.max_seg_len, who)) return rc;
    FM_REQUIRE(isfinite(a.gain) && a.gain > 0.0, "%s: gain must be finite and > 0", who);
    FM_REQUIRE(isfinite(a.level_mult), "%s: level_mult must be finite", who);
    if (const int rc = check_max_rows(a.max_seg_len, who)) return rc;
    const bool vec = a.forecast != nullptr;
    if (const int rc = check_forecast_src(a.src, a.nseg, who, vec)) return rc;
    if (a.nseg == 0 || a.src.nsel == 0) return FM_OK;   // nothing is read: an empty call has no pointers
    FM_REQUIRE(a.ret != nullptr, "%s: ret is needed (the realised return is always a vector)", who);
    FM_REQUIRE(a.seg_off && a.rec && a.cnt && a.status, "%s: null pointer", who);
    const bool pl = a.src.hi_plane != nullptr;
    const size_t lds = port_lds_bytes(a.max_seg_len);
    const hipStream_t st = (hipStream_t)stream;
    return with_form(a.max_seg_len, [&](auto nt, auto vpt) {
        if (vec) return launch_fhor<nt, vpt, VecSrc>(a, lds, st);
        return pl ? launch_fhor<nt, vpt, PanelSrc<true>>(a, lds, st) : launch_fhor<nt, vpt, PanelSrc<false>>(a, lds, st);
    });
}

extern "C" int fm_forecast_compare(const fm_fcmp_args* args, void* stream) {
    using namespace fm;
    const char* who = "fm_forecast_compare";
    FM_REQUIRE(args != nullptr, "%s: null args", who);
    const fm_fcmp_args& a = *args;
    FM_REQUIRE(a.max_seg_len >= 0, "%s: bad sizes", who);
    FM_REQUIRE(a.npair >= 0 && a.npair <= FM_MAX_PAIRS, "%s: npair must be 0..%d", who, FM_MAX_PAIRS);
    FM_REQUIRE(a.min_count >= 1, "%s: min_count must be >= 1", who);
    if (const int rc = check_max_rows(a.max_seg_len, who)) return rc;
    const bool vec = a.forecast != nullptr;
    if (const int rc = check_forecast_src(a.src, a.nseg, who, vec)) return rc;
    for (int p = 0; p < a.npair; ++p) {
        FM_REQUIRE(a.pair_a[p] >= 0 && a.pair_a[p] < a.src.nsel && a.pair_b[p] >= 0 && a.pair_b[p] < a.src.nsel,
                   "%s: pair %d (%d, %d) outside the %d forecasts", who, p, a.pair_a[p], a.pair_b[p], a.src.nsel);
        FM_REQUIRE(a.pair_level[p] >= 0 && a.pair_level[p] <= 255, "%s: pair_level must be 0..255", who);
    }
    if (a.nseg == 0 || a.npair == 0) return FM_OK;   // nothing is read: an empty call has no pointers
    if (vec) {
        FM_REQUIRE(a.ret != nullptr, "%s: forecast vectors need ret", who);
    } else {
        FM_REQUIRE(a.ret == nullptr, "%s: ret goes with forecast vectors (the panel's return is ret_col)", who);
        FM_REQUIRE(a.ret_col >= 0 && a.ret_col < a.src.ncols, "%s: ret_col outside the panel", who);
    }
    FM_REQUIRE(a.seg_off && a.rec && a.cnt && a.status, "%s: null pointer", who);
    const bool pl = a.src.hi_plane != nullptr;
    const hipStream_t st = (hipStream_t)stream;
    return with_form(a.max_seg_len, [&](auto nt, auto vpt) {
        if (vec) return launch_fcmp<nt, vpt, CmpVecSrc>(a, st);
        return pl ? launch_fcmp<nt, vpt, PanelSrc<true>>(a, st) : launch_fcmp<nt, vpt, PanelSrc<false>>(a, st);
    });
}
