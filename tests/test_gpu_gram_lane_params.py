"""fm_gram's per-lane, per-chunk clip parameters (16-wide kernels): each lane reads the cuts, the
shift and the scale of its own operand column once per chunk and clips the MFMA operand with
them, so what can go wrong is a parameter of the wrong column, of the previous chunk's month, or
a default where a month's value belongs.

Panel: 16 months of 63, 1, 130, 3, 64, 4, 65, 5 rows and the same lengths backwards, under a
balanced plan of 240 rows per workgroup: three workgroups running over 5, 10 and 3
months, two months (one of 64, one of 130 rows) cut by a workgroup boundary and the others whole.
Integer-valued columns as in tests/gram_cases.py, so every defined entry must equal the int64
reference (tests/gram_oracle.py) bit for bit.  Cuts and shifts of every column differ between
any two consecutive months, so a stale parameter changes the column's sums.  Month 2 has its last
regressor all NaN and NaN cuts for it (its rows fall into the smaller models' patterns); month
6 holds +-inf in regressor 0 and in y under finite cuts, which bring them back to integers; a
quarter of the other bounds are NaN (no bound).

Variants: 15 columns (nest5 x 3 levels, the Table-2 instantiation, ncols == ZW - 1), 14 columns
(the same instantiation without FULLC: z column 15 is a column past ncols with default
parameters) and 3 columns (nest2 x 3, NB 8: twelve operand lanes past ncols), FP64 columns and
planes, unscaled and with a power-of-two scale per (column, month).

tests/gram_cases.py already runs 15 columns with a scale under a balanced plan whose first
workgroup runs over months 0-6 (zw16-NB15-nest5x3-c15F-both-bal137-scale), +-inf under finite
cuts under its other plans (the infcut cases) and the 32-wide kernels, which keep the clip at
the scatter; those are not repeated here.  New here: the month lengths 3, 4 and 130, parameters
that provably change at every chunk boundary of a workgroup, the all-NaN column with NaN cuts, and
infinities and a scale under a balanced plan with fewer than 15 columns.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import pytest
import torch

import gram_cases as GC
import gram_oracle as GO

MONTHS = (63, 1, 130, 3, 64, 4, 65, 5, 5, 65, 4, 64, 3, 130, 1, 63)
SEG_OFF = np.concatenate([[0], np.cumsum(MONTHS)]).astype(np.int64)
NSEG = len(MONTHS)
ROWS_PER_WG = 240
M_NAN_COL, M_INF = 2, 6
NLEVELS = 3

Case = namedtuple("Case", "ncols cons layout scaled")
CASES = [Case(ncols, cons, layout, scaled)
         for ncols, cons in ((15, "nest5"), (14, "nest5"), (3, "nest2"))
         for layout in ("f64", "planes") for scaled in (False, True)]


def case_id(c):
    zw, NB, _, full = GC.dispatch_class(c.ncols, GC.NPATTERNS[c.cons] * NLEVELS, c.layout)
    return f"zw{zw}-NB{NB}-{c.cons}x{NLEVELS}-c{c.ncols}{'F' if full else ''}-{c.layout}-{'scale' if c.scaled else 'cuts'}"


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


@lru_cache(maxsize=None)
def plan():
    from fmcore import engine
    seg, rows, off, wg = engine.make_chunks_balanced(SEG_OFF, ROWS_PER_WG, 0)
    return seg, rows, off, wg


@lru_cache(maxsize=None)
def panel_data(ncols, cons):
    """(cols [ncols, n], level [n], models, masks, lut, pats)."""
    from fmcore import engine
    models = GC.model_set(cons, ncols, NLEVELS)
    masks = [m.mask for m in models]
    lut, pats = engine.plan_patterns(models)
    rng = np.random.default_rng([ncols, 7919])
    n = int(SEG_OFF[-1])
    cols = np.empty((ncols, n))
    for c in range(ncols):
        cols[c] = rng.integers(-(c + 2) * 7, (c + 2) * 11 + 1, n)
    level = rng.integers(0, NLEVELS, n).astype(np.uint8)
    rate = 0.3 * (rng.permutation(ncols) / max(ncols - 1, 1)) ** 2
    nan = rng.random((ncols, n)) < rate[:, None]
    s = slice(int(SEG_OFF[M_INF]), int(SEG_OFF[M_INF + 1]))
    for c in (0, ncols - 1):
        u = rng.random(n)
        cols[c, s] = np.where(u[s] < 0.2, np.inf, np.where(u[s] > 0.8, -np.inf, cols[c, s]))
    cols[nan] = np.nan
    cols[ncols - 2, int(SEG_OFF[M_NAN_COL]):int(SEG_OFF[M_NAN_COL + 1])] = np.nan
    return cols, level, models, masks, lut, pats


@lru_cache(maxsize=None)
def transform(ncols, scaled):
    """lo, hi, shift, inv_scale [ncols, NSEG], all exact on the integer panel."""
    rng = np.random.default_rng([ncols, 104729])
    c = np.arange(ncols)[:, None]
    t = np.arange(NSEG)[None, :]
    shape = (ncols, NSEG)
    # consecutive months differ by construction: the month's term moves by one step (mod 5 / 7 / 9)
    lo = (-(c + 2) * 3 - (t % 5)).astype(np.float64)
    hi = ((c + 2) * 5 + (t % 7)).astype(np.float64)
    shift = (rng.integers(-4, 5, (ncols, 1)) * 9 + (t % 9) - 4).astype(np.float64)
    for a in (lo, hi, shift):
        assert (np.diff(a, axis=1) != 0).all()
    drop_lo, drop_hi = rng.random(shape) < 0.25, rng.random(shape) < 0.25
    drop_lo[:, M_INF] = drop_hi[:, M_INF] = False      # finite cuts where the infinities are
    lo[drop_lo] = np.nan
    hi[drop_hi] = np.nan
    lo[ncols - 2, M_NAN_COL] = hi[ncols - 2, M_NAN_COL] = np.nan   # the cuts of an all-NaN column
    inv = 2.0 ** rng.integers(-3, 4, shape) if scaled else None
    return lo, hi, shift, inv


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_plan_shape():
    """The plan this file relies on: every workgroup runs over at least three months, and the
    chunk lengths hold every month length of the list."""
    seg, rows, off, wg = plan()
    assert len(wg) - 1 == 3
    for b in range(len(wg) - 1):
        assert len(set(seg[wg[b]:wg[b + 1]].tolist())) >= 3
    lens = set(np.diff(rows.reshape(-1, 2), axis=1).ravel().tolist())
    assert {1, 3, 4, 5, 63, 64, 65, 130} <= lens


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lane_params_exact(E, case):
    cols_h, level, models, masks, lut, pats = panel_data(case.ncols, case.cons)
    lo, hi, shift, inv = transform(case.ncols, case.scaled)
    seg, rows, off, wg = plan()
    dev = E.require_device()
    host = np.ascontiguousarray(cols_h)
    cols = planes = None
    if case.layout == "f64":
        cols = torch.from_numpy(host).to(dev)
    else:
        w = host.view(np.uint32).reshape(case.ncols, -1, 2)       # little-endian: [..., 1] = high word
        planes = torch.from_numpy(np.ascontiguousarray(np.stack([w[:, :, 1], w[:, :, 0]])).view(np.int32)).to(dev)
    panel = E.DevicePanel(cols=cols, names=[f"c{j}" for j in range(case.ncols)],
                          seg_off=torch.from_numpy(SEG_OFF).to(dev), seg_off_h=SEG_OFF.copy(),
                          months=np.arange(NSEG), planes=planes, chunk_policy=("balanced", ROWS_PER_WG),
                          chunk_split=None, row_origin=0)
    p = E._chunk_plan(panel)
    assert np.array_equal(p.chunk_seg.cpu().numpy(), seg) and np.array_equal(p.chunk_row.cpu().numpy(), rows)
    assert p.wg_off is not None and np.array_equal(p.wg_off.cpu().numpy(), wg)
    nb = len(pats) * NLEVELS
    zw = GO.zwidth(case.ncols)
    buf = torch.full((len(seg) + 2, nb, zw * (zw + 1) // 2), float("nan"), dtype=torch.float64, device=dev)
    before = buf.cpu().numpy().view(np.uint64).copy()
    out = E.gram_partials(panel, models, level=_dev(level, dev), nlevels=NLEVELS,
                          cuts=E.Cuts(_dev(lo, dev), _dev(hi, dev), None), shift=_dev(shift, dev),
                          inv_scale=_dev(inv, dev), partial_out=buf[1:-1])
    torch.cuda.synchronize()
    assert len(out) == 1 and out[0].partial.data_ptr() == buf[1].data_ptr() and out[0].zw == zw
    after = buf.cpu().numpy()
    got = after[1:-1]
    assert np.array_equal(after.view(np.uint64)[[0, -1]], before[[0, -1]]), "a chunk next to the partials was written"

    ref = GO.gram_reference(cols_h, SEG_OFF, seg, rows, lo, hi, shift, inv, level, NLEVELS, masks, lut,
                            len(pats), exact=True)
    # the month of the all-NaN column has rows, none of them in a pattern of the largest model;
    # the month of the infinities has none left after the cuts
    pid, _ = GO.row_buckets(cols_h, level, NLEVELS, masks, lut)
    pm = pid[SEG_OFF[M_NAN_COL]:SEG_OFF[M_NAN_COL + 1]]
    assert (pm >= 0).any() and all(not (pats[q] >> (len(models) - 1)) & 1 for q in pm[pm >= 0])
    s = slice(int(SEG_OFF[M_INF]), int(SEG_OFF[M_INF + 1]))
    assert np.isinf(cols_h[:, s]).any() and not np.isinf(ref.Z[s]).any() and (ref.bucket[s] >= 0).any()
    dm = GO.defined_mask(masks, pats, NLEVELS, zw)
    assert got.shape == ref.gram.shape
    want = np.where(dm[None], ref.gram, 0.0)
    have = np.where(dm[None], got, 0.0)
    bad = np.argwhere(_bits(have) != _bits(want))
    if len(bad):
        I, J = GO.packed_pairs(zw)
        k, b, e = bad[0]
        pytest.fail(f"{len(bad)} defined entries differ; first: chunk {k} (month {seg[k]}) bucket {b} entry "
                    f"({I[e]}, {J[e]}): got {got[k, b, e]!r}, expected {ref.gram[k, b, e]!r} "
                    f"(rows in bucket: {ref.n[k, b]})")
    assert np.array_equal(got[:, :, 0], ref.n.astype(np.float64))
    empty = ref.n == 0
    assert empty.any() and (~empty).any()
    for b in range(nb):
        assert (_bits(got[empty[:, b], b][:, dm[b]]) == 0).all()
