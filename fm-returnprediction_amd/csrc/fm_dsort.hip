// fm_portfolio_double_sort: two-way sorted portfolios (build-defined extension A21).
// Three launches on the caller's stream, each one workgroup per (month, sort) in
// fm_portfolio_sort's three forms; wave w owns the rows [w * VPT * 64, (w + 1) * VPT * 64), so row
// order = (wave, v, lane) order:
//   A. dsort_bp_kernel<.., false>: the eligible rows' a in registers and a bit per breakpoint
//      row, the na - 1 breakpoints of a by order_stat_keys (the single sort's exact selection).
//      An unsorted month gets all its outputs here and is skipped by B and C;
//   B. dsort_bp_kernel<.., true> over a grid of (month, sort, a-bin): every row's a-bin against
//      A's breakpoints, b of the bin's breakpoint rows in the registers (independent mode: one
//      "bin" of all breakpoint rows), the nb - 1 breakpoints of b by order_stat_keys;
//   C. dsort_sum_kernel: every row's cell = pa * nb + pb against the breakpoints in LDS, its byte
//      written, and a stable partition by cell: ballot ranks within the wave (one ballot per
//      distinct cell among the 64 rows, the wave's counts so far in two registers: lane k holds
//      cells k and 64 + k), the per-wave counts prefixed over the waves and the cells.  Then
//      eight terms (the two counts as one exact double, ret, a, b, w, w ret, w a, w b), one at a
//      time: each row's term is staged at its list place in LDS, wave k sums the stretches of
//      cells k, k + NW, ... (lane l takes entries l, l + 64, ...; the fixed butterfly); ret, a, b
//      and weight are re-read per term, from the cache.  Last the cell means into the two record
//      views in LDS, the neutral slabs added in bin order, every slab's spread, one write.
// One selection per workgroup and launch: in a loop over the bins, or inlined twice, the index
// arithmetic of order_stat_keys (invariant from one selection to the next) is kept in registers
// across the selections and the 1024 x 16 form spills.  Between the launches the breakpoints wait in
// the month's own records (rec_a slab 0: a's, rec_b slab i: b's of bin i), which C overwrites
// last: no workspace, and a month still depends on its own rows alone.  The bins of a
// conditional sort run side by side, not one after the other.
#include <math.h>

#include "fm_common.h"
#include "fm_port_dev.h"
#include "fm_select_dev.h"

namespace fm {
namespace {

constexpr int DS = FM_MAX_DSORT;
constexpr int DCELLS = DS * DS;

// Where month s of sort js keeps its records
struct DsortOut {
    int64_t so;           // [js][s]
    int nrb, nra;         // doubles of one month of one slab of rec_b / rec_a
    int64_t sb, sa;       // doubles between the slabs
    double *rec_b, *rec_a;   // slab 0 of the month
    __device__ DsortOut(const fm_dsort_args& a, int s, int js) {
        so = s + (int64_t)js * a.nseg;
        nrb = (a.nb + 1) * 4;
        nra = (a.na + 1) * 4;
        sb = (int64_t)a.nseg * nrb;
        sa = (int64_t)a.nseg * nra;
        rec_b = a.rec_b + ((int64_t)js * (a.na + 1) * a.nseg + s) * nrb;
        rec_a = a.rec_a + ((int64_t)js * (a.nb + 1) * a.nseg + s) * nra;
    }
};

// Launch A (BROUND false): a's breakpoints of month blockIdx.x of sort blockIdx.y, or the whole
// output of an unsorted month.  Launch B (BROUND true): b's breakpoints of a-bin blockIdx.z.
template <int NT, int VPT, bool BROUND>
__global__ __launch_bounds__(NT, NT >= 512 ? 4 : 2) void dsort_bp_kernel(fm_dsort_args a) {
    constexpr int NW = NT / WAVE;
    extern __shared__ uint64_t pbuf[];   // the keys of the order statistics
    __shared__ OrderSh<NW> sh;
    __shared__ double s_g[DS];
    const int s = blockIdx.x, js = blockIdx.y, bin = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int na = a.na, nb = a.nb;
    const DsortOut o(a, s, js);
    if constexpr (BROUND) {
        if (a.status[o.so] == 0u) return;   // block-uniform: launch A found the month unsorted
    }
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the LDS was sized from max_seg_len
    const int last = L - 1;
    const double* __restrict__ A = a.a + (int64_t)js * a.a_sort_stride + r0;
    const double* __restrict__ B = a.b + (int64_t)js * a.b_sort_stride + r0;

    // ---- 1. load, eligibility, this selection's rows ---------------------------------------------
    double fe[VPT];     // the selection's values: a (A) or b (B) of its rows, NaN otherwise
    uint32_t bpm = 0;   // bit v: row v of this thread is one of the selection's rows
    if (L > 0) {        // block-uniform
        uint32_t bm = 0, nm = 0;   // bit v: b is finite and the level passes / an NYSE row (or all rows)
#pragma unroll
        for (int v = 0; v < VPT; ++v) {   // unconditional (clamped) loads, masked after
            const int idx = (w * VPT + v) * WAVE + lane;
            const int ci = idx < L ? idx : last;
            const double fb = B[ci];
            const int lv = a.level != nullptr ? (int)a.level[r0 + ci] : 255;
            const int ny = a.nyse != nullptr ? (int)a.nyse[r0 + ci] : 1;
            bm |= (idx < L && isfinite(fb) && lv >= a.min_level) ? 1u << v : 0u;
            nm |= (a.nyse_breakpoints == 0 || ny != 0) ? 1u << v : 0u;
        }
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const int idx = (w * VPT + v) * WAVE + lane;
            const double fa = A[idx < L ? idx : last];
            const bool isbp = ((bm >> v) & 1u) && ((nm >> v) & 1u) && isfinite(fa);
            fe[v] = isbp ? fa : NAN;
            bpm |= isbp ? 1u << v : 0u;
        }
        if constexpr (BROUND) {
            if (a.conditional != 0) {   // keep the rows of a-bin `bin`
                int pa[VPT];
#pragma unroll
                for (int v = 0; v < VPT; ++v) pa[v] = 0;
                for (int k = 0; k < na - 1; ++k) {
                    const double bp = o.rec_a[k];   // launch A's breakpoint k
#pragma unroll
                    for (int v = 0; v < VPT; ++v) pa[v] += fe[v] > bp ? 1 : 0;
                }
#pragma unroll
                for (int v = 0; v < VPT; ++v) bpm &= pa[v] == bin ? ~0u : ~(1u << v);
            }
#pragma unroll
            for (int v = 0; v < VPT; ++v) {   // b in a's place (re-read: the cache has it)
                const int idx = (w * VPT + v) * WAVE + lane;
                const double fb = B[idx < L ? idx : last];
                fe[v] = ((bpm >> v) & 1u) ? fb : NAN;
            }
        }
    } else {
#pragma unroll
        for (int v = 0; v < VPT; ++v) fe[v] = NAN;
    }
    const int n = block_sum<NW>((int)__popc(bpm), sh.iscr);

    if constexpr (!BROUND) {
        if (n < a.min_count) {   // block-uniform: the month is unsorted
            const int ncell = na * nb;
            if (tid == 0) a.status[o.so] = 0u;
            if (tid < na - 1 && a.bpa != nullptr) a.bpa[o.so * (na - 1) + tid] = NAN;
            if (tid < na * (nb - 1) && a.bpb != nullptr) a.bpb[o.so * na * (nb - 1) + tid] = NAN;
            if (tid < ncell) a.cnt[o.so * ncell + tid] = 0;
            for (int e = tid; e < (na + 1) * o.nrb; e += NT) o.rec_b[(e / o.nrb) * o.sb + e % o.nrb] = NAN;
            for (int e = tid; e < (nb + 1) * o.nra; e += NT) o.rec_a[(e / o.nra) * o.sa + e % o.nra] = NAN;
            if (a.cell != nullptr) {
                uint8_t* cell = a.cell + (int64_t)js * a.nrows + r0;
#pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const int idx = (w * VPT + v) * WAVE + lane;
                    if (idx < L) cell[idx] = 255;
                }
            }
            return;
        }
        if (tid == 0) a.status[o.so] = 1u;
    }
    const int nq = BROUND ? nb - 1 : na - 1;
    double* out = BROUND ? o.rec_b + bin * o.sb : o.rec_a;   // where the breakpoints wait for launch C
    if constexpr (BROUND) {
        if (a.conditional != 0 && n < a.min_count_bin) {   // block-uniform: the a-bin is not sorted on b
            if (tid < nq) out[tid] = NAN;
            return;
        }
    }

    // ---- 2. the 2 nq order statistics, breakpoints ---------------------------------------------------
    if (tid < nq) {
        int i, j;
        double g;
        qranks(n, BROUND ? a.qb[tid] : a.qa[tid], 0, i, j, g);
        sh.trank[2 * tid] = i;
        sh.trank[2 * tid + 1] = j;
        s_g[tid] = g;
    }
    if (tid == 0) {
        sh.n = 0;
        sh.over = 0;
    }
    order_stat_keys<NT, VPT>(fe, bpm, n, 2 * nq, pbuf, sh);
    if (tid < nq) out[tid] = qlerp(kval(sh.okey[2 * tid]), kval(sh.okey[2 * tid + 1]), s_g[tid], 0);
}

// Launch C: cells, partition, sums and records of month blockIdx.x of sort blockIdx.y
template <int NT, int VPT>
__global__ __launch_bounds__(NT, NT >= 512 ? 4 : 2) void dsort_sum_kernel(fm_dsort_args a) {
    constexpr int NW = NT / WAVE;
    static_assert(NT >= DCELLS + 1, "one thread per cell");
    extern __shared__ double stage[];    // one term of every row, at the row's list place
    __shared__ double s_bpa[DS], s_bpb[DS][DS];
    __shared__ int s_wcnt[NW][DCELLS];   // per wave and cell: the count, then the wave's first place
    __shared__ int s_start[DCELLS + 1];
    __shared__ double s_sum[DCELLS][8];
    __shared__ double s_rb[DS + 1][DS + 1][4], s_ra[DS + 1][DS + 1][4];
    const int s = blockIdx.x, js = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int na = a.na, nb = a.nb, ncell = na * nb;
    const bool cond = a.conditional != 0;
    const DsortOut o(a, s, js);
    if (a.status[o.so] == 0u) return;   // block-uniform: launch A wrote the unsorted month
    const int64_t r0 = a.seg_off[s];
    int L = (int)(a.seg_off[s + 1] - r0);
    L = L < a.max_seg_len ? L : a.max_seg_len;   // the LDS was sized from max_seg_len
    const int last = L - 1;   // L > 0: the month is sorted
    const double* __restrict__ A = a.a + (int64_t)js * a.a_sort_stride + r0;
    const double* __restrict__ B = a.b + (int64_t)js * a.b_sort_stride + r0;
    uint8_t* cell = a.cell != nullptr ? a.cell + (int64_t)js * a.nrows + r0 : nullptr;

    // ---- 1. the breakpoints of launches A and B, out of the records they waited in -------------------
    if (tid < na - 1) {
        const double bp = o.rec_a[tid];
        s_bpa[tid] = bp;
        if (a.bpa != nullptr) a.bpa[o.so * (na - 1) + tid] = bp;
    }
    if (tid >= WAVE && tid < WAVE + na * (nb - 1)) {
        const int e = tid - WAVE, i = e / (nb - 1), j = e - i * (nb - 1);
        const double bp = o.rec_b[(cond ? i : 0) * o.sb + j];   // independent: bin 0's row for every i
        s_bpb[i][j] = bp;   // NaN: a-bin i is not sorted on b
        if (a.bpb != nullptr) a.bpb[o.so * na * (nb - 1) + e] = bp;
    }
    __syncthreads();

    // ---- 2. every row's cell, stable partition by cell ---------------------------------------
    int pos[VPT];          // the row's place in its cell's list (row order), -1: in no cell
    int c0 = 0, c1 = 0;    // lane k: this wave's rows of cell k / cell 64 + k so far
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int idx = (w * VPT + v) * WAVE + lane;
        const int ci = idx < L ? idx : last;
        const double fa = A[ci], fb = B[ci];
        const int lv = a.level != nullptr ? (int)a.level[r0 + ci] : 255;
        const bool elig = idx < L && isfinite(fa) && isfinite(fb) && lv >= a.min_level;
        int pa = 0, pb = 0;
        for (int i = 0; i < na - 1; ++i) pa += fa > s_bpa[i] ? 1 : 0;
        for (int j = 0; j < nb - 1; ++j) pb += fb > s_bpb[pa][j] ? 1 : 0;
        const int c = (elig && !isnan(s_bpb[pa][0])) ? pa * nb + pb : 255;
        if (cell != nullptr && idx < L) cell[idx] = (uint8_t)c;
        int pp = -1;   // (place among this wave's rows of c) << 8 | c
        uint64_t todo = __ballot(c != 255);
        while (todo != 0ull) {   // wave-uniform: one round per distinct cell among the 64 rows
            const int src = __builtin_amdgcn_readfirstlane((int)__ffsll((unsigned long long)todo) - 1);
            const int k = __builtin_amdgcn_readlane(c, src);
            const uint64_t mk = __ballot(c == k);
            const int before = k < WAVE ? __builtin_amdgcn_readlane(c0, k) : __builtin_amdgcn_readlane(c1, k - WAVE);
            if (c == k) pp = ((before + mask_rank(mk)) << 8) | k;
            const int add = (int)__popcll(mk);
            c0 += lane == k ? add : 0;
            c1 += lane + WAVE == k ? add : 0;
            todo &= ~mk;
        }
        pos[v] = pp;
    }
    if (lane < ncell) s_wcnt[w][lane] = c0;
    if (lane + WAVE < ncell) s_wcnt[w][lane + WAVE] = c1;
    __syncthreads();
    if (tid < ncell) {   // this cell's rows of the earlier waves; the total
        int run = 0;
        for (int q = 0; q < NW; ++q) {
            const int c = s_wcnt[q][tid];
            s_wcnt[q][tid] = run;
            run += c;
        }
        s_start[tid + 1] = run;
    }
    __syncthreads();
    if (w == 0) {   // inclusive scan of the totals over the cells, in place
        const int t0 = lane < ncell ? s_start[lane + 1] : 0;
        const int t1 = lane + WAVE < ncell ? s_start[lane + WAVE + 1] : 0;
        const int i0 = wave_incl_scan(t0);
        const int i1 = wave_incl_scan(t1) + __builtin_amdgcn_readlane(i0, WAVE - 1);
        if (lane < ncell) s_start[lane + 1] = i0;
        if (lane + WAVE < ncell) s_start[lane + WAVE + 1] = i1;
        if (lane == 0) s_start[0] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < VPT; ++v)
        if (pos[v] >= 0) pos[v] = (pos[v] >> 8) + s_wcnt[w][pos[v] & 255] + s_start[pos[v] & 255];

    // ---- 3. per-cell sums --------------------------------------------------------------------------
    const double* __restrict__ R = a.ret + r0;
    const double* __restrict__ W = a.weight != nullptr ? a.weight + r0 : nullptr;
    uint32_t okr = 0, okw = 0;   // bit v: the row counts (finite return) / counts in the weighted sums
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
        const int idx = (w * VPT + v) * WAVE + lane;
        const int ci = idx < L ? idx : last;
        const double rr = R[ci], ww = W != nullptr ? W[ci] : NAN;
        const bool r_ok = pos[v] >= 0 && isfinite(rr);
        okr |= r_ok ? 1u << v : 0u;
        okw |= (r_ok && isfinite(ww) && ww > 0.0) ? 1u << v : 0u;
    }
    // One term at a time: every row's term is staged at its list position (8 bytes a row), then
    // wave k sums the stretches of cells k, k + NW, ...  Rows that do not count stage 0.  Term 0
    // is the two counts as one exact double: 1 for a finite return + 2^20 for a usable weight as
    // well; 1: ret, 2: a, 3: b; 4 .. 7: the weight times 1, ret, a, b.
    const int npass = W != nullptr ? 8 : 4;
#pragma unroll 1
    for (int t = 0; t < npass; ++t) {   // block-uniform
        const int what = t & 3;
        // (the row index behind an opaque copy of the lane: else the VPT row addresses of each of the
        // four vectors, invariant in this loop, are computed before it and held in registers)
        int ol = lane;
        asm volatile("" : "+v"(ol));
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            if (pos[v] >= 0) {
                const int idx = (w * VPT + v) * WAVE + ol;   // < L: the row is eligible
                const bool r_ok = (okr >> v) & 1u, w_ok = (okw >> v) & 1u;
                double m1 = 1.0, m2 = 1.0;
                if (what == 1) m1 = R[idx];
                if (what == 2) m1 = A[idx];
                if (what == 3) m1 = B[idx];
                if (t >= 4) m2 = W[idx];
                double y = (t >= 4 ? w_ok : r_ok) ? m1 * m2 : 0.0;   // (a factor 1.0 is exact)
                if (t == 0) y = (r_ok ? 1.0 : 0.0) + (w_ok ? 1048576.0 : 0.0);
                stage[pos[v]] = y;
            }
        }
        __syncthreads();
        for (int k = w; k < ncell; k += NW) {   // wave-uniform
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

    // ---- 4. the two record views ---------------------------------------------------------------------
    if (tid < ncell) {
        const int i = tid / nb, j = tid - i * nb;
        const int64_t both = (int64_t)s_sum[tid][0];
        const int c = (int)(both & 1048575), cw = (int)(both >> 20);
        const double er = c > 0 ? s_sum[tid][1] / (double)c : NAN;
        const double ea = c > 0 ? s_sum[tid][2] / (double)c : NAN;
        const double eb = c > 0 ? s_sum[tid][3] / (double)c : NAN;
        double vr = NAN, va = NAN, vb = NAN;
        if (cw > 0) {   // (weight NULL: cw = 0, and terms 4 .. 7 were never summed)
            const double sw = s_sum[tid][4];
            vr = s_sum[tid][5] / sw;
            va = s_sum[tid][6] / sw;
            vb = s_sum[tid][7] / sw;
        }
        s_rb[i][j][0] = er;
        s_rb[i][j][1] = eb;
        s_rb[i][j][2] = vr;
        s_rb[i][j][3] = vb;
        s_ra[j][i][0] = er;
        s_ra[j][i][1] = ea;
        s_ra[j][i][2] = vr;
        s_ra[j][i][3] = va;
        a.cnt[o.so * ncell + tid] = c;
    }
    __syncthreads();
    // the neutral slabs: the na (nb) slabs' entries added in bin order, then one division
    if (tid < nb * 4) {
        const int j = tid >> 2, c = tid & 3;
        double acc = s_rb[0][j][c];
        for (int i = 1; i < na; ++i) acc += s_rb[i][j][c];
        s_rb[na][j][c] = acc / (double)na;
    }
    if (tid >= WAVE && tid < WAVE + na * 4) {
        const int i = (tid - WAVE) >> 2, c = tid & 3;
        double acc = s_ra[0][i][c];
        for (int j = 1; j < nb; ++j) acc += s_ra[j][i][c];
        s_ra[nb][i][c] = acc / (double)nb;
    }
    __syncthreads();
    // every slab's spread row: its last row minus its first (NaN if an end is NaN)
    if (tid < (na + 1) * 4) {
        const int i = tid >> 2, c = tid & 3;
        s_rb[i][nb][c] = s_rb[i][nb - 1][c] - s_rb[i][0][c];
    }
    if (tid >= WAVE && tid < WAVE + (nb + 1) * 4) {
        const int j = (tid - WAVE) >> 2, c = tid & 3;
        s_ra[j][na][c] = s_ra[j][na - 1][c] - s_ra[j][0][c];
    }
    __syncthreads();
    for (int e = tid; e < (na + 1) * o.nrb; e += NT) {
        const int i = e / o.nrb, x = e - i * o.nrb;
        o.rec_b[i * o.sb + x] = s_rb[i][x >> 2][x & 3];
    }
    for (int e = tid; e < (nb + 1) * o.nra; e += NT) {
        const int j = e / o.nra, x = e - j * o.nra;
        o.rec_a[j * o.sa + x] = s_ra[j][x >> 2][x & 3];
    }
}

template <int NT, int VPT>
int launch_dsort(const fm_dsort_args& a, hipStream_t st) {
    const char* who = "fm_portfolio_double_sort";
    const size_t lds = port_lds_bytes(a.max_seg_len), big = 8 * (size_t)pow2_ceil(NT * VPT);
    const size_t lds_c = 8 * (size_t)(a.max_seg_len > 0 ? a.max_seg_len : 1);   // launch C stages 8 bytes a row
    if (lds >= 32 * 1024) {   // (with the static tables the launches can pass the default 64 KB)
        if (raise_dynamic_lds<dsort_bp_kernel<NT, VPT, false>>(big, who) != FM_OK) return FM_EHIP;
        if (raise_dynamic_lds<dsort_bp_kernel<NT, VPT, true>>(big, who) != FM_OK) return FM_EHIP;
        if (raise_dynamic_lds<dsort_sum_kernel<NT, VPT>>(big, who) != FM_OK) return FM_EHIP;
    }
    const dim3 grid(a.nseg, a.nsel), grid_b(a.nseg, a.nsel, a.conditional != 0 ? a.na : 1);
    hipLaunchKernelGGL((dsort_bp_kernel<NT, VPT, false>), grid, dim3(NT), lds, st, a);
    if (const int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL((dsort_bp_kernel<NT, VPT, true>), grid_b, dim3(NT), lds, st, a);
    if (const int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL((dsort_sum_kernel<NT, VPT>), grid, dim3(NT), lds_c, st, a);
    return check_launch(who);
}

}  // namespace
}  // namespace fm

extern "C" int fm_portfolio_double_sort(const fm_dsort_args* args, void* stream) {
    using namespace fm;
    const char* who = "fm_portfolio_double_sort";
    FM_REQUIRE(args != nullptr, "%s: null args", who);
    const fm_dsort_args& a = *args;
    FM_REQUIRE(a.nseg >= 0 && a.max_seg_len >= 0 && a.nrows >= 0, "%s: bad sizes", who);
    FM_REQUIRE(a.nsel >= 0 && a.nsel <= 65535, "%s: nsel must be 0..65535", who);
    FM_REQUIRE(a.a_sort_stride >= 0 && a.b_sort_stride >= 0, "%s: negative sort stride", who);
    FM_REQUIRE(a.na >= 2 && a.na <= FM_MAX_DSORT, "%s: na must be 2..%d", who, FM_MAX_DSORT);
    FM_REQUIRE(a.nb >= 2 && a.nb <= FM_MAX_DSORT, "%s: nb must be 2..%d", who, FM_MAX_DSORT);
    for (int i = 0; i < a.na - 1; ++i) {
        const double lo = i == 0 ? 0.0 : a.qa[i - 1];
        FM_REQUIRE(a.qa[i] > lo && a.qa[i] < 1.0, "%s: qa must be strictly ascending in (0, 1)", who);
    }
    for (int j = 0; j < a.nb - 1; ++j) {
        const double lo = j == 0 ? 0.0 : a.qb[j - 1];
        FM_REQUIRE(a.qb[j] > lo && a.qb[j] < 1.0, "%s: qb must be strictly ascending in (0, 1)", who);
    }
    FM_REQUIRE(a.min_level >= 0 && a.min_level <= 255, "%s: min_level must be 0..255", who);
    FM_REQUIRE(a.nyse_breakpoints == 0 || a.nyse != nullptr, "%s: nyse_breakpoints needs nyse", who);
    FM_REQUIRE(a.min_count >= 1, "%s: min_count must be >= 1", who);
    FM_REQUIRE(a.conditional == 0 || a.min_count_bin >= 1, "%s: min_count_bin must be >= 1", who);
    if (a.max_seg_len > PORT_MAX_ROWS) {
        set_error("%s: %d-row months exceed %d", who, a.max_seg_len, PORT_MAX_ROWS);
        return FM_ETOOBIG;
    }
    if (a.nseg == 0 || a.nsel == 0) return FM_OK;   // nothing is read: an empty call has no pointers
    FM_REQUIRE(a.a && a.b && a.ret && a.seg_off && a.rec_b && a.rec_a && a.cnt && a.status, "%s: null pointer", who);
    return with_form(a.max_seg_len, [&](auto nt, auto vpt) { return launch_dsort<nt, vpt>(a, (hipStream_t)stream); });
}
