"""numpy restatement of fm_portfolio_hold (extension A19; include/fm_hip.h), an independent
formulation without links (firm x calendar-month tables, shifted), and the hand-made panel the
tests run on.  Test infrastructure only.

Sums are taken in longdouble (np.add.at, from +0.0) and rounded to float64 once, then divided in
float64; the k-cohort average and the turnover use the definition's operation order.  On the
integer-valued fixture every sum is exact, so the device must give the same bits."""
import numpy as np


def ancestors(seg_off, link_prev, hold):
    """anc [hold+1, rows] int64: the row reached after a hops over the step -1 links, -1 where a hop
    is missing (every row at once per hop)."""
    so = np.asarray(seg_off, dtype=np.int64)
    link = np.asarray(link_prev, dtype=np.int64)
    n = int(so[-1])
    lens = np.diff(so)
    seg = np.searchsorted(so, np.arange(n), side="right") - 1
    anc = np.full((hold + 1, n), -1, dtype=np.int64)
    row = np.arange(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    anc[0] = row
    for a in range(1, hold + 1):
        s = seg - a
        alive &= s >= 0
        sc = np.maximum(s, 0)
        l = link[row]
        alive &= (l >= 0) & (l < lens[sc])
        row = np.where(alive, so[sc] + l, 0)
        anc[a] = np.where(alive, row, -1)
    return anc


def _complete(status, mi, t, depth):
    """status [T] of one sort: months t - depth .. t are sorted and consecutive in the calendar."""
    if t - depth < 0:
        return False
    return all(status[t - x] == 1 and mi[t - x] == mi[t] - x for x in range(depth + 1))


def _records(seg_off, month_index, status, member_port, own_port, ret, weight, nport, hold, sort_rec):
    """Everything after the membership: ``member_port`` [S, hold+1, rows] int (the portfolio of the
    row's ancestor at each age, >= nport or < 0: no member), ``own_port`` [S, rows]."""
    so = np.asarray(seg_off, dtype=np.int64)
    mi = np.asarray(month_index, dtype=np.int64)
    T, n = len(so) - 1, int(so[-1])
    S, k, P = member_port.shape[0], hold, nport
    ret = np.asarray(ret, dtype=np.float64)
    seg = np.searchsorted(so, np.arange(n), side="right") - 1
    f0 = np.isfinite(ret)
    if weight is None:
        f1 = np.zeros(n, dtype=bool)
        w = np.zeros(n)
    else:
        w = np.asarray(weight, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            f1 = f0 & np.isfinite(w) & (w > 0)
    members = np.zeros((S, T, k + 1, P), dtype=np.int64)
    stay = np.zeros((S, T, k + 1, P), dtype=np.int64)
    cohort_n = np.zeros((S, T, k, P, 2), dtype=np.int64)
    sums = np.zeros((S, T, k, P, 3), dtype=np.longdouble)
    ld = np.longdouble
    with np.errstate(all="ignore"):
        wr = np.where(f1, w, 0.0) * np.where(f1, ret, 0.0)
    for j in range(S):
        for a in range(k + 1):
            q = member_port[j, a]
            m = (q >= 0) & (q < P)
            np.add.at(members[j, :, a], (seg[m], q[m]), 1)
            s = m & (own_port[j] == q)
            np.add.at(stay[j, :, a], (seg[s], q[s]), 1)
            if a == k:
                continue
            m0, m1 = m & f0, m & f1
            np.add.at(cohort_n[j, :, a, :, 0], (seg[m0], q[m0]), 1)
            np.add.at(cohort_n[j, :, a, :, 1], (seg[m1], q[m1]), 1)
            np.add.at(sums[j, :, a, :, 0], (seg[m0], q[m0]), ret[m0].astype(ld))
            np.add.at(sums[j, :, a, :, 1], (seg[m1], q[m1]), wr[m1].astype(ld))
            np.add.at(sums[j, :, a, :, 2], (seg[m1], q[m1]), w[m1].astype(ld))
    s64 = sums.astype(np.float64)
    cohort = np.full((S, T, k, P, 2), np.nan)
    with np.errstate(all="ignore"):
        e = cohort_n[..., 0] > 0
        cohort[..., 0][e] = s64[..., 0][e] / cohort_n[..., 0][e].astype(np.float64)
        v = cohort_n[..., 1] > 0
        cohort[..., 1][v] = s64[..., 1][v] / s64[..., 2][v]
    status = np.asarray(status).reshape(S, T)
    status_out = np.zeros((S, T), dtype=np.int32)
    rec = np.full((S, T, P + 1, 4), np.nan)
    turnover = np.full((S, T, P), np.nan)
    with np.errstate(all="ignore"):
        for j in range(S):
            for t in range(T):
                if not _complete(status[j], mi, t, k - 1):
                    continue
                status_out[j, t] = 1
                for col in range(4):
                    if col % 2 == 0:
                        terms = [cohort[j, t, a, :, col // 2] for a in range(k)]
                    elif sort_rec is None:
                        terms = [np.full(P, np.nan)] * k
                    else:
                        terms = [np.asarray(sort_rec, dtype=np.float64)[j, t - a, :P, col] for a in range(k)]
                    x = terms[0].copy()
                    for a in range(1, k):
                        x = x + terms[a]
                    rec[j, t, :P, col] = x / np.float64(k)
                rec[j, t, P] = rec[j, t, P - 1] - rec[j, t, 0]
                if _complete(status[j], mi, t, k):
                    m0 = members[j, t, 0].astype(np.float64)
                    ok = members[j, t, 0] > 0
                    tv = (1.0 - stay[j, t, k].astype(np.float64) / m0) / np.float64(k)
                    turnover[j, t, ok] = tv[ok]
    return dict(members=members.astype(np.int32), stay=stay.astype(np.int32), cohort_n=cohort_n.astype(np.int32),
                cohort=cohort, status=status_out, rec=rec, turnover=turnover)


def portfolio_hold(seg_off, month_index, link_prev, port, status, ret, weight=None, nport=5, hold=1, sort_rec=None):
    """The definition, hop by hop over the links -> dict(members, stay [S, T, k+1, P] int32, cohort_n
    [S, T, k, P, 2] int32, cohort [S, T, k, P, 2], status [S, T] int32, rec [S, T, P+1, 4], turnover
    [S, T, P]).  ``port`` [S, rows] uint8, ``status`` [S, T]."""
    port = np.asarray(port).reshape(-1, int(np.asarray(seg_off)[-1])).astype(np.int64)
    anc = ancestors(seg_off, link_prev, hold)
    mp = np.where(anc[None] >= 0, port[:, np.maximum(anc, 0)], -1)
    return _records(seg_off, month_index, status, mp, port, ret, weight, nport, hold, sort_rec)


def pivot_hold(ids, seg_off, month_index, port, status, ret, weight=None, nport=5, hold=1, sort_rec=None):
    """The same without links: per sort a firm x calendar-month table of the port bytes (every month
    of the range a column), shifted by the age; a member's firm is present in every month between."""
    import pandas as pd
    so = np.asarray(seg_off, dtype=np.int64)
    n = int(so[-1])
    port = np.asarray(port).reshape(-1, n).astype(np.int64)
    month = np.repeat(np.asarray(month_index, dtype=np.int64), np.diff(so))
    S = port.shape[0]
    mp = np.full((S, hold + 1, n), -1, dtype=np.int64)
    if n:
        cal = np.arange(month.min(), month.max() + 1)
        fi = None
        for j in range(S):
            df = pd.DataFrame({"id": np.asarray(ids), "m": month, "p": port[j].astype(np.float64), "one": 1.0})
            Pt = df.pivot(index="id", columns="m", values="p").reindex(columns=cal)
            here = df.pivot(index="id", columns="m", values="one").reindex(columns=cal).notna()
            if fi is None:
                fi = Pt.index.get_indexer(np.asarray(ids))
            chain = here.copy()
            for a in range(hold + 1):
                if a > 0:
                    chain &= here.shift(a, axis=1, fill_value=False)
                tab = Pt.shift(a, axis=1).where(chain).fillna(-1.0).to_numpy()
                mp[j, a] = tab[fi, month - cal[0]].astype(np.int64)
    return _records(seg_off, month_index, status, mp, port, ret, weight, nport, hold, sort_rec)


def sum_bounds(seg_off, link_prev, port, ret, weight, nport, hold):
    """For the forward error bounds of real-valued data: per (sort, month, age, portfolio) the term
    counts [.., 2] and sum |ret|, sum |w ret|, sum w [.., 3] of the cohort sums (float64)."""
    so = np.asarray(seg_off, dtype=np.int64)
    n, T = int(so[-1]), len(so) - 1
    port = np.asarray(port).reshape(-1, n).astype(np.int64)
    anc = ancestors(seg_off, link_prev, hold)
    seg = np.searchsorted(so, np.arange(n), side="right") - 1
    ret = np.asarray(ret, dtype=np.float64)
    f0 = np.isfinite(ret)
    w = np.zeros(n) if weight is None else np.asarray(weight, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        f1 = f0 & np.isfinite(w) & (w > 0) & (weight is not None)
    S = port.shape[0]
    cnt = np.zeros((S, T, hold, nport, 2), dtype=np.int64)
    mag = np.zeros((S, T, hold, nport, 3))
    for j in range(S):
        for a in range(hold):
            q = np.where(anc[a] >= 0, port[j, np.maximum(anc[a], 0)], -1)
            m = (q >= 0) & (q < nport)
            m0, m1 = m & f0, m & f1
            np.add.at(cnt[j, :, a, :, 0], (seg[m0], q[m0]), 1)
            np.add.at(cnt[j, :, a, :, 1], (seg[m1], q[m1]), 1)
            np.add.at(mag[j, :, a, :, 0], (seg[m0], q[m0]), np.abs(ret[m0]))
            np.add.at(mag[j, :, a, :, 1], (seg[m1], q[m1]), np.abs(w[m1] * ret[m1]))
            np.add.at(mag[j, :, a, :, 2], (seg[m1], q[m1]), w[m1])
    return cnt, mag


# ------------------------------------------------------------------------------------------------
# The fixture: 32 months, 11,276 rows.  Months shorter than a wave, of exactly one, two, three and
# four waves and one row either side, a stretch of months of several workgroup rounds (a round is
# 256 rows), an empty month, months shorter than the number of portfolios, a long month between
# short ones, and a two-month calendar step.
HOLD_LENS = [65, 1, 64, 0, 63, 2, 130, 129, 191, 192, 193, 255, 256, 257,
             300, 320, 1025, 700, 500, 400, 2100, 333, 640, 511, 513, 384,
             90, 450, 128, 600, 64, 420]
HOLD_GAP_SEG = HOLD_LENS.index(90)     # a two-month calendar step into this segment
HOLD_NPORT = 5
HOLD_NSORT = 3
HOLD_EXTRA_UNSORTED = (1, 9)           # (sort, month): one more unsorted month
HOLD_SEED = 11


def hold_panel(seed=HOLD_SEED):
    """-> dict(ids, seg_off, month_index, link_prev, port [3, rows] uint8, status [3, T] int32, ret,
    weight, sort_rec [3, T, 6, 4]).  Each month keeps about 97 % of the previous month's firms where
    the lengths allow; the rest enter from one pool of int64 ids, some above 2^40.  Returns are
    m / 64 with |m| <= 8 and weights whole numbers in 1..199 (plus a few NaN, infinite, zero and
    negative entries), so every sum of the definition is exact in any order."""
    import horizon_oracle as HO
    rng = np.random.default_rng(seed)
    uni = np.unique(np.concatenate([rng.integers(1, 1 << 20, 8000), rng.integers(1 << 40, 1 << 62, 4000)]))
    parts, prev = [], np.zeros(0, dtype=np.int64)
    for n in HOLD_LENS:
        keep = rng.choice(prev, size=min(int(round(0.97 * len(prev))), n), replace=False) if len(prev) else prev
        new = rng.choice(np.setdiff1d(uni, keep), size=n - len(keep), replace=False)
        cur = np.sort(np.concatenate([keep, new]).astype(np.int64))
        assert len(cur) == n and len(np.unique(cur)) == n
        parts.append(cur)
        prev = cur
    T = len(HOLD_LENS)
    seg_off = np.zeros(T + 1, dtype=np.int64)
    np.cumsum(HOLD_LENS, out=seg_off[1:])
    steps = np.ones(T, dtype=np.int64)
    steps[HOLD_GAP_SEG] = 2
    month_index = (900 + np.cumsum(steps)).astype(np.int32)
    ids = np.concatenate(parts)
    n = len(ids)
    link_prev = HO.month_links(ids, seg_off, month_index, -1)
    ret = rng.integers(-8, 9, n) / 64.0
    for v in (np.nan, np.inf, -np.inf):
        ret[rng.choice(n, size=12, replace=False)] = v
    weight = rng.integers(1, 200, n).astype(np.float64)
    for v in (np.nan, 0.0, -3.0, np.inf):
        weight[rng.choice(n, size=15, replace=False)] = v
    seg = np.searchsorted(seg_off, np.arange(n), side="right") - 1
    port = rng.integers(0, HOLD_NPORT, (HOLD_NSORT, n)).astype(np.uint8)
    port[rng.random((HOLD_NSORT, n)) < 0.08] = 255
    status = np.ones((HOLD_NSORT, T), dtype=np.int32)
    status[:, np.asarray(HOLD_LENS) < HOLD_NPORT] = 0
    status[HOLD_EXTRA_UNSORTED] = 0
    port[status[:, seg] == 0] = 255
    sort_rec = rng.normal(0.01, 0.02, (HOLD_NSORT, T, HOLD_NPORT + 1, 4))
    sort_rec[status == 0] = np.nan
    return dict(ids=ids, seg_off=seg_off, month_index=month_index, link_prev=link_prev, port=port, status=status,
                ret=ret, weight=weight, sort_rec=sort_rec)


def real_values(p, seed=5):
    """Real-valued returns and weights on the rows of ``p`` (NaN / infinite entries kept where the
    fixture has them)."""
    rng = np.random.default_rng(seed)
    n = len(p["ret"])
    ret = np.where(np.isfinite(p["ret"]), rng.normal(0.01, 0.1, n), p["ret"])
    w = p["weight"]
    with np.errstate(invalid="ignore"):
        weight = np.where(np.isfinite(w) & (w > 0), np.exp(rng.normal(5.0, 2.0, n)), w)
    return ret, weight
