"""Fixtures of the Gram tests (tests/test_gram_host.py checks them on the CPU,
tests/test_gpu_gram.py runs them): the panel, the model sets, the chunk plans, the transforms and
the list of cases with the fm_gram instantiation each one is meant to reach.

Panel: 14 months of 0 .. 700 rows (2,628 in all), month-major.  Column c holds integers from
[-(c+2)*7, (c+2)*11] (a different range per column, so no two Gram entries coincide), NaN at a
per-column rate between 0 and 40 %.  Some months are structured: 63 rows without y and then one
complete row; every row without y; every row complete and of the top level (one bucket); the
buckets in round-robin order; and the months of 1, 2 and 5 rows hold bucket counts of 1, 2 and 3.
The last column is y.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from fmcore import engine as E

import gram_oracle as GO

MONTHS = (64, 1, 65, 0, 2, 5, 63, 127, 255, 256, 257, 320, 513, 700)
M_ONLY_LAST, M_ONE, M_NO_Y, M_EMPTY, M_TWO, M_FIVE, M_ONE_BUCKET, M_ROUND_ROBIN = 0, 1, 2, 3, 4, 5, 9, 11
SEG_OFF = np.concatenate([[0], np.cumsum(MONTHS)]).astype(np.int64)
NROWS = int(SEG_OFF[-1])
NSEG = len(MONTHS)

# name -> (panel.chunk_policy, panel.chunk_split, panel.row_origin)
PLANS = {
    "whole": (("months", 1024), None, 0),
    "m100": (("months", 100), None, 0),
    "split": (None, True, 0),
    "bal0": (("balanced", 300), None, 0),
    "bal137": (("balanced", 300), None, 137),
}
XFORMS = ("raw", "shift", "cuts", "scale", "infcut")


# ------------------------------------------------------------------------------------ model sets
def model_set(cons, ncols, nlevels):
    """The model list of a construction over ``ncols`` panel columns (y = the last one): "one",
    "nest<k>" (k nested models), "ind<k>" (k models, none inside another) and "chains" (a in b, c in
    d, the chains independent).  Together the models use every column."""
    y = ncols - 1
    reg = list(range(ncols - 1))
    lv = tuple(range(nlevels))
    if cons == "one":
        xs = [reg]
    elif cons.startswith("nest"):
        k = int(cons[4:])
        cut = [((i + 1) * len(reg)) // k for i in range(k)]
        xs = [reg[:c] for c in cut]
    elif cons.startswith("ind"):
        k = int(cons[3:])
        xs = [reg[i::k] for i in range(k)]
    elif cons == "chains":
        xs = [reg[0:1], reg[0::2], reg[1:2], reg[1::2]]
    else:
        raise ValueError(cons)
    assert all(len(x) >= 1 for x in xs) or cons == "one", (cons, ncols)
    return [E.Model(f"{cons}{i}", y=y, xs=list(x), levels=lv) for i, x in enumerate(xs)]


# construction -> pattern count under plan_patterns
NPATTERNS = {"one": 1, "nest2": 2, "nest4": 4, "nest5": 5, "ind2": 3, "ind3": 7, "chains": 8}


def dispatch_class(ncols, nb, layout):
    """(ZW, NB, planes, FULLC) of the fm_gram instantiation these sizes reach (fm_gram.hip)."""
    if ncols <= 15:
        zw = 16
        NB = next(b for b in (1, 4, 8, 12, 15, 16) if nb <= b)
    else:
        zw = 32
        NB = next(b for b in (1, 4, 8) if nb <= b)
    return zw, NB, layout != "f64", ncols == zw - 1


# ------------------------------------------------------------------------------------ the data
Data = namedtuple("Data", "cols level models masks lut pats nlevels ncols kind")


@lru_cache(maxsize=None)
def panel_data(cons, ncols, nlevels, kind="int"):
    """Host columns [ncols, n] and levels of one model set.  kind: "int" (above), "dense" (no NaN
    and no structured month: every row in the top pattern), "inf" (+-inf in regressor 0 and in y,
    for cuts to bring back), "infx" (+-inf in regressor 0 only), "real" (normals far from 0)."""
    models = model_set(cons, ncols, nlevels)
    masks = [m.mask for m in models]
    lut, pats = E.plan_patterns(models)
    assert len(pats) == NPATTERNS[cons]
    rng = np.random.default_rng([ncols, nlevels, sum(map(ord, cons)), sum(map(ord, kind))])
    n = NROWS
    cols = np.empty((ncols, n), dtype=np.float64)
    for c in range(ncols):
        if kind == "real":
            cols[c] = 1000.0 * (c + 1) + (c + 1) * rng.standard_normal(n)
        else:
            cols[c] = rng.integers(-(c + 2) * 7, (c + 2) * 11 + 1, n)
    level = rng.integers(0, nlevels, n).astype(np.uint8)
    if kind == "dense":
        return Data(cols, level if nlevels > 1 else None, models, masks, lut, pats, nlevels, ncols, kind)
    rate = 0.4 * (rng.permutation(ncols) / max(ncols - 1, 1)) ** 3    # 0 .. 40 %, most of them small
    nan = rng.random((ncols, n)) < rate[:, None]
    seg = lambda t: slice(int(SEG_OFF[t]), int(SEG_OFF[t + 1]))   # noqa: E731
    y = ncols - 1
    s = seg(M_ONLY_LAST)
    nan[:, s] = False
    nan[y, s.start:s.stop - 1] = True
    s = seg(M_NO_Y)
    nan[y, s] = True
    s = seg(M_ONE_BUCKET)
    nan[:, s] = False
    level[s] = nlevels - 1
    nb = len(pats) * nlevels
    union = GO.pattern_columns(masks, pats)

    def put(r, b):   # row r into bucket b (-1: dropped)
        level[r] = max(b, 0) % nlevels
        for c in range(ncols):
            nan[c, r] = b < 0 or not (union[b // nlevels] >> c) & 1

    s = seg(M_ROUND_ROBIN)
    for i, r in enumerate(range(s.start, s.stop)):
        put(r, i % nb)
    # the tiny months are one tile under every plan: bucket counts of 1, 2 and 3, and in the
    # 5-row month the first and the last bucket with the ones between them empty
    put(seg(M_ONE).start, nb - 1)
    for r in range(seg(M_TWO).start, seg(M_TWO).stop):
        put(r, nb // 2)
    for i, r in enumerate(range(seg(M_FIVE).start, seg(M_FIVE).stop)):
        put(r, 0 if i < 3 else (nb - 1 if nb > 1 else -1))
    if kind in ("inf", "infx") and ncols >= 2:
        for c in ([0, y] if kind == "inf" else [0]):
            u = rng.random(n)
            cols[c][u < 0.03] = np.inf
            cols[c][u > 0.97] = -np.inf
    cols[nan] = np.nan
    return Data(cols, level if nlevels > 1 else None, models, masks, lut, pats, nlevels, ncols, kind)


@lru_cache(maxsize=None)
def transform(xf, ncols):
    """lo, hi, shift, inv_scale as [ncols, NSEG] arrays or None, all exact on the integer panels:
    "raw" nothing; "shift" integer shifts; "cuts" integer bounds (a quarter of them NaN = none,
    one column with lo == hi) and shifts; "scale" shifts and power-of-two scales; "infcut"
    finite bounds everywhere (they bring +-inf back); "real": bounds, pivots near the columns'
    means and scales that are no powers of two, for the real-valued panel."""
    rng = np.random.default_rng([ncols, XFORMS.index(xf) if xf in XFORMS else 99])
    c = np.arange(ncols)[:, None]
    shape = (ncols, NSEG)
    lo = hi = shift = inv = None
    if xf in ("shift", "cuts", "scale"):
        shift = rng.integers(-40, 41, shape).astype(np.float64)
    if xf in ("cuts", "infcut"):
        lo = (-(c + 2) * 3 + rng.integers(-3, 4, shape)).astype(np.float64)
        hi = ((c + 2) * 5 + rng.integers(-3, 4, shape)).astype(np.float64)
    if xf == "cuts":
        lo[rng.random(shape) < 0.25] = np.nan
        hi[rng.random(shape) < 0.25] = np.nan
        k = min(2, ncols - 1)
        lo[k] = hi[k] = 3.0
    if xf == "scale":
        inv = 2.0 ** rng.integers(-3, 4, shape)
    if xf == "real":
        mean, sd = 1000.0 * (c + 1), (c + 1.0)
        shift = mean + sd * rng.uniform(-0.5, 0.5, shape)
        lo = mean - sd * rng.uniform(1.0, 2.5, shape)
        hi = mean + sd * rng.uniform(1.0, 2.5, shape)
        lo[rng.random(shape) < 0.2] = np.nan
        inv = 1.0 / (sd * rng.uniform(0.7, 1.9, shape))
    return lo, hi, shift, inv


def plan_arrays(plan, seg_off=SEG_OFF):
    """(chunk_seg, chunk_row, seg_chunk_off, order or None, wg_off or None) as engine._chunk_plan
    makes them for a panel with this plan's settings."""
    pol, split, origin = PLANS[plan]
    if split:
        return E.make_chunks_split(seg_off) + (None,)
    if pol[0] == "balanced":
        seg, rows, off, wg = E.make_chunks_balanced(seg_off, pol[1], origin)
        return seg, rows, off, None, wg
    return E.make_chunks(seg_off, pol[1]) + (None, None)


def reference(data, plan, xf, exact=True):
    seg, rows, _, _, _ = plan_arrays(plan)
    lo, hi, shift, inv = transform(xf, data.ncols)
    return GO.gram_reference(data.cols, SEG_OFF, seg, rows, lo, hi, shift, inv, data.level, data.nlevels,
                             data.masks, data.lut, len(data.pats), exact=exact)


# ------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "cons nlevels ncols layout plan xf kind")


def case_id(c):
    zw, NB, pl, full = dispatch_class(c.ncols, NPATTERNS[c.cons] * c.nlevels, c.layout)
    return (f"zw{zw}-NB{NB}-{c.cons}x{c.nlevels}-c{c.ncols}{'F' if full else ''}-{c.layout}-{c.plan}-{c.xf}"
            + ("" if c.kind == "int" else f"-{c.kind}"))


# (construction, levels, nb, NB) in the order of the variant table
ROWS16 = (("one", 1, 1, 1), ("one", 3, 3, 4), ("nest2", 2, 4, 4), ("ind2", 2, 6, 8), ("chains", 1, 8, 8),
          ("ind2", 3, 9, 12), ("nest4", 3, 12, 12), ("ind3", 2, 14, 15), ("nest5", 3, 15, 15), ("chains", 2, 16, 16))
ROWS32 = (("one", 1, 1, 1), ("one", 3, 3, 4), ("nest2", 2, 4, 4), ("ind2", 2, 6, 8), ("chains", 1, 8, 8))


def _cases():
    out = []
    plans = list(PLANS)
    i = 0

    def add(cons, nl, ncols, layout, kind="int"):
        nonlocal i
        xf = XFORMS[(i + i // 5) % 5]
        if kind == "dense":
            xf = XFORMS[i % 4]
        elif xf == "infcut" and ncols >= 2:
            kind = "inf"
        elif xf == "infcut":
            xf = "shift"
        out.append(Case(cons, nl, ncols, layout, plans[i % 5], xf, kind))
        i += 1

    for r, (cons, nl, _, _) in enumerate(ROWS16):
        small = (1, 7, 14)[r % 3] if cons == "one" else (7, 14)[r % 2]
        for ncols in (15, small):
            for layout in ("f64", "planes"):
                add(cons, nl, ncols, layout)
        add(cons, nl, (15, small)[r % 2], "both")
    for r, (cons, nl, _, _) in enumerate(ROWS32):
        small = (16, 23)[r % 2]
        for ncols in (31, small):
            for layout in ("f64", "planes"):
                add(cons, nl, ncols, layout)
        add(cons, nl, (31, small)[r % 2], "both")
    # ncols 1 (y alone) with levels, and the NaN-free panels: one bucket per level holds every entry
    add("one", 3, 1, "planes")
    for ncols in (7, 15, 23, 31):
        for layout in ("f64", "planes"):
            add("one", (1, 3)[len(out) % 2], ncols, layout, kind="dense")
    # the Table-2 shape under every plan x transform
    for p in plans:
        for k, xf in enumerate(XFORMS):
            out.append(Case("nest5", 3, 15, ("f64", "planes", "both")[(len(out) + k) % 3], p, xf,
                            "inf" if xf == "infcut" else "int"))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()

# real-valued and infinity cases: one 16-wide and one 32-wide, on both layouts
REAL_CASES = [Case("nest5", 3, 15, lay, "m100", "real", "real") for lay in ("f64", "planes")] + \
             [Case("chains", 1, 23, lay, "bal137", "real", "real") for lay in ("f64", "planes")]
INF_CASES = [Case("nest4", 3, 14, lay, "split", "raw", "infx") for lay in ("f64", "planes")] + \
            [Case("ind2", 2, 31, lay, "whole", "raw", "infx") for lay in ("f64", "planes")]
# the solve's moments: 16-wide and 32-wide model lists
MOMENT_CASES = [Case("nest5", 3, 15, "f64", "whole", "shift", "int"), Case("ind3", 2, 7, "planes", "bal137", "shift", "int"),
                Case("nest2", 2, 23, "f64", "m100", "shift", "int"), Case("chains", 1, 31, "planes", "split", "raw", "int")]


# ------------------------------------------------------------------------------------ tiles
def tile_stats(bucket, chunk_row, nb):
    """Per 64-row tile, counted from each chunk's first row: counts [ntiles, nb], the bucket of
    every row (-1 dropped) padded to 64 with -2."""
    counts, rows = [], []
    for r0, r1 in np.asarray(chunk_row).reshape(-1, 2):
        for t0 in range(int(r0), int(r1), 64):
            b = bucket[t0:min(t0 + 64, int(r1))]
            counts.append(np.bincount(b[b >= 0], minlength=nb))
            rows.append(np.concatenate([b, np.full(64 - len(b), -2)]))
    return np.array(counts).reshape(-1, nb), np.array(rows).reshape(-1, 64)
