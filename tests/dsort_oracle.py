"""numpy restatement of fm_portfolio_double_sort's definition (include/fm_hip.h): a
loop over months with np.quantile, np.searchsorted(side="left"), masked sums in row order and the
margin sums in the stated order.  The reference has no double sort, so this restatement is what
the device is pinned to."""
import numpy as np


def _rsum(x):
    """The sum of x in row order (np.sum adds pairwise)."""
    return float(np.cumsum(x)[-1]) if len(x) else 0.0


def _margins(cells):
    """cells [n1, n2, 4] -> [n1+1, n2+1, 4]: every slab's last-minus-first row, and the neutral slab
    (x_0 + x_1 + ... + x_{n1-1}) / n1 added in that order, with its own last-minus-first row."""
    n1, n2, _ = cells.shape
    out = np.full((n1 + 1, n2 + 1, 4), np.nan)
    out[:n1, :n2] = cells
    acc = cells[0].copy()
    for i in range(1, n1):
        acc = acc + cells[i]
    out[n1, :n2] = acc / float(n1)
    with np.errstate(invalid="ignore"):
        out[:, n2] = out[:, n2 - 1] - out[:, 0]
    return out


def double_sort(seg_off, A, B, R, W=None, level=None, nyse=None, na=5, nb=5, qa=None, qb=None,
                conditional=False, min_level=0, nyse_breakpoints=False, min_count=None, min_count_bin=None):
    """One sort -> dict(rec_b [na+1, T, nb+1, 4], rec_a [nb+1, T, na+1, 4], cnt [T, na, nb] int32,
    cell [rows] uint8, bpa [T, na-1], bpb [T, na, nb-1], status [T] int32)."""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    A, B, R = (np.asarray(x, dtype=np.float64) for x in (A, B, R))
    T = len(seg_off) - 1
    qa = np.arange(1, na) / na if qa is None else np.asarray(qa, dtype=np.float64)
    qb = np.arange(1, nb) / nb if qb is None else np.asarray(qb, dtype=np.float64)
    min_count = na * nb if min_count is None else min_count
    min_count_bin = nb if min_count_bin is None else min_count_bin
    rec_b = np.full((na + 1, T, nb + 1, 4), np.nan)
    rec_a = np.full((nb + 1, T, na + 1, 4), np.nan)
    cnt = np.zeros((T, na, nb), dtype=np.int32)
    cell = np.full(len(A), 255, dtype=np.uint8)
    bpa = np.full((T, na - 1), np.nan)
    bpb = np.full((T, na, nb - 1), np.nan)
    status = np.zeros(T, dtype=np.int32)
    for t in range(T):
        r0, r1 = int(seg_off[t]), int(seg_off[t + 1])
        a, b, r = A[r0:r1], B[r0:r1], R[r0:r1]
        elig = np.isfinite(a) & np.isfinite(b)
        if level is not None:
            elig &= np.asarray(level[r0:r1]) >= min_level
        brk = elig & (np.asarray(nyse[r0:r1]) != 0) if nyse_breakpoints else elig
        if brk.sum() < min_count:
            continue
        status[t] = 1
        bpa[t] = np.quantile(a[brk], qa)
        pa = np.searchsorted(bpa[t], a, side="left")   # (rows that are not eligible are masked below)
        c = np.full(r1 - r0, 255, dtype=np.uint8)
        for i in range(na):
            if conditional:
                rows = brk & (pa == i)
                if rows.sum() < min_count_bin:
                    continue   # NaN breakpoints, the bin's rows stay 255
                bpb[t, i] = np.quantile(b[rows], qb)
            else:
                bpb[t, i] = np.quantile(b[brk], qb)
            m = elig & (pa == i)
            c[m] = i * nb + np.searchsorted(bpb[t, i], b[m], side="left")
        cell[r0:r1] = c
        w = None if W is None else np.asarray(W[r0:r1], dtype=np.float64)
        cb = np.full((na, nb, 4), np.nan)   # ew ret, ew b, vw ret, vw b
        ca = np.full((nb, na, 4), np.nan)   # ew ret, ew a, vw ret, vw a
        for i in range(na):
            for j in range(nb):
                m = (c == i * nb + j) & np.isfinite(r)
                k = int(m.sum())
                cnt[t, i, j] = k
                if k:
                    er, ea, eb = _rsum(r[m]) / k, _rsum(a[m]) / k, _rsum(b[m]) / k
                    cb[i, j, 0], cb[i, j, 1] = er, eb
                    ca[j, i, 0], ca[j, i, 1] = er, ea
                if w is not None:
                    with np.errstate(invalid="ignore"):
                        mw = m & np.isfinite(w) & (w > 0)
                    if mw.any():
                        sw = _rsum(w[mw])
                        vr, va, vb = _rsum(w[mw] * r[mw]) / sw, _rsum(w[mw] * a[mw]) / sw, _rsum(w[mw] * b[mw]) / sw
                        cb[i, j, 2], cb[i, j, 3] = vr, vb
                        ca[j, i, 2], ca[j, i, 3] = vr, va
        rec_b[:, t] = _margins(cb)
        rec_a[:, t] = _margins(ca)
    return dict(rec_b=rec_b, rec_a=rec_a, cnt=cnt, cell=cell, bpa=bpa, bpb=bpb, status=status)


def double_sort_batch(seg_off, A, B, R, **kw):
    """nsel sorts: A and B are [n] (shared) or [nsel, n].  -> the same dict with a leading [nsel]."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    S = max(A.shape[0] if A.ndim == 2 else 1, B.shape[0] if B.ndim == 2 else 1)
    outs = [double_sort(seg_off, A[s] if A.ndim == 2 else A, B[s] if B.ndim == 2 else B, R, **kw) for s in range(S)]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def integer_panel(seed=11, T=6, lo=120, hi=180, vals=41):
    """The integer-valued fixture: signals, returns and weights are small integers, so every sum is
    exact in any order and every mean is one correctly rounded division."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=T)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    A = rng.integers(-vals, vals + 1, n).astype(np.float64)
    B = rng.integers(-vals, vals + 1, (3, n)).astype(np.float64)
    R = rng.integers(-20, 21, n).astype(np.float64)
    W = rng.integers(1, 50, n).astype(np.float64)
    A[rng.random(n) < 0.03] = np.nan
    B[rng.random((3, n)) < 0.03] = np.nan
    R[rng.random(n) < 0.03] = np.nan
    W[rng.random(n) < 0.03] = 0.0
    level = rng.integers(0, 3, n).astype(np.uint8)
    nyse = (rng.random(n) < 0.5).astype(np.uint8)
    return dict(seg_off=seg_off, A=A, B=B, R=R, W=W, level=level, nyse=nyse)


def ragged_panel(seed=5, T=36, lo=300, hi=420):
    """The real-valued ragged panel: NaN and +-inf signals, NaN returns, NaN / zero / negative
    weights, three universe levels."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=T)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    A = rng.normal(5.0, 2.0, n)
    B = 0.3 * (A - 5.0) * 0.01 + rng.normal(0.01, 0.02, n)
    for x in (A, B):
        x[rng.random(n) < 0.02] = np.nan
        x[rng.random(n) < 0.002] = np.inf
        x[rng.random(n) < 0.002] = -np.inf
    R = rng.normal(0.01, 0.15, n)
    R[rng.random(n) < 0.02] = np.nan
    W = np.exp(rng.normal(5.0, 2.0, n))
    W[rng.random(n) < 0.01] = np.nan
    W[rng.random(n) < 0.01] = 0.0
    W[rng.random(n) < 0.01] = -1.0
    level = rng.integers(0, 3, n).astype(np.uint8)
    nyse = (rng.random(n) < 0.4).astype(np.uint8)
    return dict(seg_off=seg_off, A=A, B=B, R=R, W=W, level=level, nyse=nyse)
