"""numpy restatement of fm_month_links and fm_horizon_return (extension A16; include/fm_hip.h),
an independent pandas formulation of the compounded returns, and the hand-made panel the GPU
tests run on.  Test infrastructure only."""
import numpy as np


def month_links(ids, seg_off, month_index, step):
    """link [rows] int32: per month a searchsorted of its ids in the neighbouring month's ids."""
    ids = np.asarray(ids, dtype=np.int64)
    so = np.asarray(seg_off, dtype=np.int64)
    mi = np.asarray(month_index, dtype=np.int64)
    T = len(so) - 1
    link = np.full(len(ids), -1, dtype=np.int32)
    for s in range(T):
        t = s + step
        if t < 0 or t >= T or mi[t] != mi[s] + step:
            continue
        mine, other = ids[so[s]:so[s + 1]], ids[so[t]:so[t + 1]]
        if len(other) == 0:
            continue
        pos = np.searchsorted(other, mine)
        hit = pos < len(other)
        hit[hit] = other[pos[hit]] == mine[hit]
        link[so[s]:so[s + 1]] = np.where(hit, pos, -1)
    return link


def count_bad(ids, seg_off):
    """Rows whose id is not greater than their predecessor's in the month."""
    ids = np.asarray(ids, dtype=np.int64)
    so = np.asarray(seg_off, dtype=np.int64)
    return int(sum(np.count_nonzero(np.diff(ids[so[s]:so[s + 1]]) <= 0) for s in range(len(so) - 1)))


def horizon_return(ret, link, seg_off, h):
    """out [rows]: the hop loop of the definition, every row at once per hop; each sum and product
    is one IEEE operation."""
    ret = np.asarray(ret, dtype=np.float64)
    link = np.asarray(link, dtype=np.int64)
    so = np.asarray(seg_off, dtype=np.int64)
    n, T = len(ret), len(so) - 1
    seg = np.searchsorted(so, np.arange(n), side="right") - 1
    row = np.arange(n)
    alive = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        p = 1.0 + ret
        for j in range(1, h):
            sj = seg + j
            alive &= sj < T
            sjc = np.minimum(sj, T - 1)
            l = link[row]
            alive &= (l >= 0) & (l < so[sjc + 1] - so[sjc])
            row = np.where(alive, so[sjc] + l, 0)
            p = p * (1.0 + ret[row])
        out = p - 1.0
    out[~alive] = np.nan
    return out


def pandas_horizon(ids, month, ret, h):
    """The same returns without links or segments: pivot to a firm x calendar-month matrix (every
    month of the range a column), shift(-j), multiply in the same order, mask by presence.
    ``month``: each row's calendar month number."""
    import pandas as pd
    ids, month, ret = np.asarray(ids), np.asarray(month, dtype=np.int64), np.asarray(ret, dtype=np.float64)
    if len(ids) == 0:
        return np.zeros(0)
    cal = np.arange(month.min(), month.max() + 1)
    df = pd.DataFrame({"id": ids, "m": month, "r": ret, "one": 1.0})
    R = df.pivot(index="id", columns="m", values="r").reindex(columns=cal)
    P = df.pivot(index="id", columns="m", values="one").reindex(columns=cal).notna()
    with np.errstate(all="ignore"):
        prod = 1.0 + R
        ok = P.copy()
        for j in range(1, h):
            prod = prod * (1.0 + R.shift(-j, axis=1))
            ok &= P.shift(-j, axis=1, fill_value=False)
        out = (prod - 1.0).where(ok)
    fi = R.index.get_indexer(ids)
    return out.to_numpy()[fi, month - cal[0]]


def assert_same_bits(got, exp, what):
    """Equal NaN masks, and equal bits everywhere else (infinities and the sign of zero included)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), (what, "NaN masks differ at", np.nonzero(gn != en)[0][:8])
    a, b = got[~gn].view(np.uint64), exp[~en].view(np.uint64)
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, (what, len(bad), "values differ, first", got[~gn][bad[:4]], exp[~en][bad[:4]])


# ------------------------------------------------------------------------------------------------
# The hand-made panel of the GPU tests: every tile shape of the kernels (a wave takes 64 rows; a
# tile inside one month, tiles that cross one or several month boundaries, an empty month, months
# far longer than 16,384 rows), ids that need all 64 bits, and a calendar with gaps.
EDGE_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000, 20000]
EDGE_GAPS = {5: 2, 8: 3}          # month_index steps into segments 5 and 8: one and two months missing
ID_X = 123456 + (1 << 41)         # ID_X and ID_Y differ only above bit 32
ID_Y = ID_X + (1 << 32)
SEG_X, SEG_Y = 10, 11             # ID_X only in segment 10, ID_Y only in segment 11: equal low words


def edge_panel(seed=3):
    """-> dict(ids, seg_off, month_index, ret): months of EDGE_LENS rows; each month keeps about 90 %
    of the previous month's firms where the lengths allow it, the rest enter from one universe of
    int64 ids, a third of them above 2^40."""
    rng = np.random.default_rng(seed)
    uni = np.unique(np.concatenate([rng.integers(1, 1 << 20, 30000), rng.integers(1 << 40, 1 << 62, 15000)]))
    uni = uni[(uni != ID_X) & (uni != ID_Y)]
    parts, prev = [], np.zeros(0, dtype=np.int64)
    for s, n in enumerate(EDGE_LENS):
        forced = np.array([ID_X] if s == SEG_X else [ID_Y] if s == SEG_Y else [ID_X, ID_Y] if s > SEG_Y else [],
                          dtype=np.int64)
        room = n - len(forced)
        keep = rng.choice(prev, size=min(int(round(0.9 * len(prev))), room), replace=False) if len(prev) else prev
        keep = keep[(keep != ID_X) & (keep != ID_Y)]
        pool = np.setdiff1d(uni, keep)
        new = rng.choice(pool, size=room - len(keep), replace=False)
        cur = np.sort(np.concatenate([keep, new, forced]).astype(np.int64))
        assert len(cur) == n and len(np.unique(cur)) == n
        parts.append(cur)
        prev = cur
    seg_off = np.zeros(len(EDGE_LENS) + 1, dtype=np.int64)
    np.cumsum(EDGE_LENS, out=seg_off[1:])
    steps = np.array([EDGE_GAPS.get(s, 1) for s in range(len(EDGE_LENS))])
    month_index = (700 + np.cumsum(steps)).astype(np.int32)
    ids = np.concatenate(parts)
    ret = rng.normal(0.01, 0.1, len(ids))
    special = [np.nan, np.inf, -np.inf, -1.0, -0.0]
    at = rng.choice(len(ids), size=40 * len(special), replace=False)
    for k, v in enumerate(special):
        ret[at[k::len(special)]] = v
    return dict(ids=ids, seg_off=seg_off, month_index=month_index, ret=ret)
