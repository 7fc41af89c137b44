"""CPU checks of the Gram tests' reference (tests/gram_oracle.py) and fixtures
(tests/gram_cases.py): that the oracle's buckets combine into the Gram of the rows pandas would
keep, and that the fixtures reach every fm_gram instantiation, chunk plan and tile shape
tests/test_gpu_gram.py is meant to cover.
"""
import numpy as np
import pytest

from fmcore import engine as E

import gram_cases as GC
import gram_oracle as GO

ALL_CASES = GC.CASES + GC.REAL_CASES + GC.INF_CASES + GC.MOMENT_CASES
MODEL_SETS = sorted({(c.cons, c.ncols, c.nlevels) for c in ALL_CASES})
INT_CASES = [c for c in GC.CASES + GC.MOMENT_CASES]


# ------------------------------------------------------------------------------------ packed index
@pytest.mark.parametrize("zw", [16, 32])
def test_packed_index_round_trip(zw):
    I, J = GO.packed_pairs(zw)
    assert len(I) == zw * (zw + 1) // 2
    for e, (i, j) in enumerate(zip(I, J)):
        assert GO.packed_index(i, j, zw) == e and GO.packed_index(j, i, zw) == e
    assert sorted({GO.packed_index(i, j, zw) for i in range(zw) for j in range(zw)}) == list(range(len(I)))


# ------------------------------------------------------------------------------------ buckets combine
@pytest.mark.parametrize("cons,ncols,nlevels", MODEL_SETS)
def test_buckets_combine_to_dropna_gram(cons, ncols, nlevels):
    """Per month and problem (model, u): the reference buckets summed by fm_solve's rule (patterns
    that contain the model, levels >= u, the problem's columns) equal, exactly, the Gram of the
    month's rows without a NaN in the model's columns and with level >= u."""
    d = GC.panel_data(cons, ncols, nlevels)
    seg, rows, off, _, _ = GC.plan_arrays("m100")
    ref = GC.reference(d, "m100", "shift")
    _, _, shift, _ = GC.transform("shift", ncols)
    Z = GO.z_values(d.cols, GC.SEG_OFF, shift=shift)
    lvl = np.zeros(GC.NROWS, dtype=np.int64) if d.level is None else d.level.astype(np.int64)
    fitted = 0
    for t in range(GC.NSEG):
        chunks = np.arange(off[t], off[t + 1])
        assert (seg[chunks] == t).all()
        r = np.arange(GC.SEG_OFF[t], GC.SEG_OFF[t + 1])
        for mi, m in enumerate(d.models):
            zidx = [0] + [1 + x for x in m.xs] + [1 + m.y]
            use = np.array(m.xs + [m.y])
            for u in range(nlevels):
                keep = r[~np.isnan(d.cols[use][:, r]).any(axis=0) & (lvl[r] >= u)]
                Zi = np.rint(Z[keep][:, zidx]).astype(np.int64)
                G, n, _, _ = GO.problem_gram(ref, d.pats, nlevels, chunks, mi, u, zidx)
                assert n == len(keep)
                assert np.array_equal(G.astype(np.int64), Zi.T @ Zi), (t, mi, u)
                fitted += n > len(zidx)
    assert fitted > 0


# ------------------------------------------------------------------------------------ dispatch
def test_model_sets_give_the_table():
    for rows, ncols, cap in ((GC.ROWS16, (7, 15), 16), (GC.ROWS32, (16, 31), 8)):
        for cons, nl, nb, NB in rows:
            for nc in ncols:
                models = GC.model_set(cons, nc, nl)
                lut, pats = E.plan_patterns(models)
                assert len(pats) * nl == nb
                assert GC.dispatch_class(nc, nb, "f64")[1] == NB
                assert E.group_models(models, nl, cap) == [list(range(len(models)))]


@pytest.mark.parametrize("case", ALL_CASES, ids=GC.case_id)
def test_case_reaches_its_instantiation(case):
    d = GC.panel_data(case.cons, case.ncols, case.nlevels, case.kind)
    zw, NB, pl, full = GC.dispatch_class(case.ncols, len(d.pats) * case.nlevels, case.layout)
    assert GC.case_id(case).startswith(f"zw{zw}-NB{NB}-")
    assert zw == (16 if case.ncols <= 15 else 32) == GO.zwidth(case.ncols)
    cap = 16 if zw == 16 else 8
    assert len(d.pats) * case.nlevels <= cap
    assert E.group_models(d.models, case.nlevels, cap) == [list(range(len(d.models)))]
    assert (d.level is None) == (case.nlevels == 1)
    assert full == (case.ncols in (15, 31)) and pl == (case.layout in ("planes", "both"))
    union = 0
    for m in d.masks:
        union |= m
    assert union == (1 << case.ncols) - 1          # every column is some model's


def test_every_instantiation_is_reached():
    """All 36: (ZW 16: NB 1, 4, 8, 12, 15, 16; ZW 32: NB 1, 4, 8) x (FP64 columns, planes) x
    (ncols == ZW - 1 or fewer); the both-layout panels, every table row, every ncols and every
    plan x transform occur too."""
    got = {GC.dispatch_class(c.ncols, GC.NPATTERNS[c.cons] * c.nlevels, c.layout) for c in GC.CASES}
    want = {(16, NB, pl, f) for NB in (1, 4, 8, 12, 15, 16) for pl in (False, True) for f in (False, True)} | \
           {(32, NB, pl, f) for NB in (1, 4, 8) for pl in (False, True) for f in (False, True)}
    assert got == want and len(want) == 36
    rows = {(c.cons, c.nlevels, c.ncols <= 15) for c in GC.CASES}
    assert {(a, b, True) for a, b, _, _ in GC.ROWS16} | {(a, b, False) for a, b, _, _ in GC.ROWS32} <= rows
    assert {c.ncols for c in GC.CASES} >= {1, 7, 14, 15, 16, 23, 31}
    assert {c.layout for c in GC.CASES} == {"f64", "planes", "both"}
    assert {(c.plan, c.xf) for c in GC.CASES} == {(p, x) for p in GC.PLANS for x in GC.XFORMS}
    for zw in (16, 32):
        for cases in (GC.REAL_CASES, GC.INF_CASES, GC.MOMENT_CASES):
            assert {c.layout for c in cases if GO.zwidth(c.ncols) == zw} >= {"f64", "planes"}


# ------------------------------------------------------------------------------------ plans
def test_panel_months():
    assert sorted(GC.MONTHS) == [0, 1, 2, 5, 63, 64, 65, 127, 255, 256, 257, 320, 513, 700]
    assert GC.NROWS < 3000 and GC.MONTHS[GC.M_EMPTY] == 0


@pytest.mark.parametrize("plan", list(GC.PLANS))
def test_plans(plan):
    seg, rows, off, order, wg = GC.plan_arrays(plan)
    rows = rows.reshape(-1, 2)
    n = len(seg)
    assert off[-1] == n and (np.diff(off) >= 1).all()          # every month has a chunk, the empty one too
    for t in range(GC.NSEG):                                    # a month's chunks tile it in order
        r = rows[off[t]:off[t + 1]]
        assert (seg[off[t]:off[t + 1]] == t).all()
        assert r[0, 0] == GC.SEG_OFF[t] and r[-1, 1] == GC.SEG_OFF[t + 1] and (r[1:, 0] == r[:-1, 1]).all()
    lens = rows[:, 1] - rows[:, 0]
    e = off[GC.M_EMPTY]
    assert lens[e] == 0 and off[GC.M_EMPTY + 1] == e + 1
    if plan == "whole":
        assert n == GC.NSEG and set(lens) >= {0, 1, 63, 65, 257}
    if plan == "m100":
        assert n > 2 * GC.NSEG and lens.max() <= 100
    if plan == "split":
        assert sorted(order) == list(range(n)) and list(order) != list(range(n - 1, -1, -1))
        assert n == GC.NSEG + sum(m >= 256 for m in GC.MONTHS)
    if plan.startswith("bal"):
        assert wg[0] == 0 and wg[-1] == n and (np.diff(wg) >= 1).all()
        per = np.diff(wg)
        crosses = [len(set(seg[wg[b]:wg[b + 1]])) > 1 for b in range(len(per))]
        assert per.max() > 1 and any(crosses)                  # several chunks, across a month boundary
        b = np.searchsorted(wg, e, side="right") - 1
        assert wg[b + 1] - wg[b] > 1                           # the empty month's chunk has company
        origin = GC.PLANS[plan][2]
        assert ((rows[lens > 0, 0] + origin) // 300 == (rows[lens > 0, 1] - 1 + origin) // 300).all()
    else:
        assert wg is None


# ------------------------------------------------------------------------------------ tiles
def _tiles(case):
    d = GC.panel_data(case.cons, case.ncols, case.nlevels, case.kind)
    nb = len(d.pats) * case.nlevels
    _, bucket = GO.row_buckets(d.cols, d.level, d.nlevels, d.masks, d.lut)
    _, rows, _, _, _ = GC.plan_arrays(case.plan)
    return d, nb, bucket, rows, GC.tile_stats(bucket, rows, nb)


@pytest.mark.parametrize("case", [c for c in GC.CASES if c.kind != "dense"], ids=GC.case_id)
def test_tile_residues(case):
    d, nb, bucket, rows, (counts, tb) = _tiles(case)
    assert {int(x) for x in np.unique(counts[counts > 0] % 4)} == {0, 1, 2, 3}
    occupied = counts > 0
    assert (~occupied.any(axis=1)).any()                                  # a tile with no valid row
    valid = tb >= 0
    assert (valid[:, 63] & (valid.sum(axis=1) == 1)).any()                # only its last row is valid
    assert (counts.max(axis=1) == 64).any()                               # 64 rows in one bucket
    if nb >= 3:                                                           # an empty bucket between two occupied
        gap = [any(o[a] and o[c] and not o[a + 1:c].any() and c > a + 1 for a in range(nb) for c in range(a + 2, nb))
               for o in occupied]
        assert any(gap)
    # every bucket is occupied in some chunk and empty in some other
    rows = rows.reshape(-1, 2)
    per_chunk = np.array([np.bincount(bucket[r0:r1][bucket[r0:r1] >= 0], minlength=nb) for r0, r1 in rows])
    assert (per_chunk > 0).any(axis=0).all() and (per_chunk == 0).any(axis=0).all()


@pytest.mark.parametrize("case", [c for c in GC.CASES if c.kind == "dense"], ids=GC.case_id)
def test_dense_panels_define_every_entry(case):
    d, nb, bucket, rows, (counts, tb) = _tiles(case)
    assert not np.isnan(d.cols).any() and (bucket >= 0).all()
    dm = GO.defined_mask(d.masks, d.pats, d.nlevels, GO.zwidth(case.ncols))
    assert (dm.sum(axis=1) == (case.ncols + 1) * (case.ncols + 2) // 2).all()


# ------------------------------------------------------------------------------------ exactness, coverage
@pytest.mark.parametrize("case", INT_CASES, ids=GC.case_id)
def test_integer_fixtures_are_exact(case):
    """rows_per_chunk * max |z|^2 < 2^53 with room to spare (2^40), and z is integer-valued up to
    a power of two wherever it is defined (gram_reference asserts it when it scales z)."""
    d = GC.panel_data(case.cons, case.ncols, case.nlevels, case.kind)
    ref = GC.reference(d, case.plan, case.xf)
    used = ref.Z[ref.bucket >= 0]
    dm = GO.defined_mask(d.masks, d.pats, d.nlevels, ref.zw)
    zmax = 0.0
    for b in range(ref.nb):
        zcols = np.flatnonzero(dm[b][[GO.packed_index(0, j, ref.zw) for j in range(ref.zw)]])
        zb = ref.Z[ref.bucket == b][:, zcols]
        assert np.isfinite(zb).all()
        zmax = max(zmax, float(np.abs(zb).max(initial=0.0)))
    assert len(used) and 700 * zmax ** 2 < 2.0 ** 40
    assert ref.n.sum() == (ref.bucket >= 0).sum()


@pytest.mark.parametrize("cons,ncols,nlevels", MODEL_SETS)
def test_defined_mask_covers_what_the_models_read(cons, ncols, nlevels):
    d = GC.panel_data(cons, ncols, nlevels)
    zw = GO.zwidth(ncols)
    dm = GO.defined_mask(d.masks, d.pats, nlevels, zw)
    for mi, m in enumerate(d.models):
        zidx = [0] + [1 + x for x in m.xs] + [1 + m.y]
        need = [GO.packed_index(a, b, zw) for a in zidx for b in zidx]
        for q, P in enumerate(d.pats):
            if (P >> mi) & 1:
                assert dm[q * nlevels:(q + 1) * nlevels][:, need].all()
    top = len(d.pats) - 1                      # the pattern of all models: every panel column
    assert d.pats[top] == (1 << len(d.models)) - 1
    assert dm[top * nlevels].sum() == (ncols + 1) * (ncols + 2) // 2
