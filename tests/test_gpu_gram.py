"""fm_gram's packed per-(chunk, bucket) partial Grams against exact references, through
engine.gram_partials (the launch path of fm_pass), and the solve's moments against the problem
Gram of the same reference.

A Gram of integer-valued data is exact in FP64 in any summation order, on the FP64 MFMA too, so
on the integer panels of tests/gram_cases.py every defined entry must equal the int64 reference
(tests/gram_oracle.py) bit for bit: for all 36 fm_gram instantiations (ZW 16 / 32, bucket bound,
FP64 columns or planes, ncols == ZW - 1 or fewer), under whole-month, many-chunk, split-month and
balanced plans, raw and with exact shifts, cuts and power-of-two scales.  tests/test_gram_host.py
shows on the CPU that the cases reach those instantiations, plans and tile shapes.  The partials
are written into a slice of a NaN-filled buffer: a store that is skipped (an empty bucket must be
stored as zeros) or that lands in a neighbouring chunk shows.

Real-valued panels are held to n * 2^-53 * sum |z_i z_j| (n fused multiply-adds in any order)
against a longdouble reference; panels with +-inf to the class of every entry.
"""
import numpy as np
import pytest
import torch

import gram_cases as GC
import gram_oracle as GO

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _panel(E, case, data):
    """The DevicePanel of a case, built directly (panel_from_arrays has no empty month)."""
    dev = E.require_device()
    host = np.ascontiguousarray(data.cols)
    cols = planes = None
    if case.layout != "planes":
        cols = torch.from_numpy(host).to(dev)
    if case.layout != "f64":
        w = host.view(np.uint32).reshape(data.ncols, -1, 2)       # little-endian: [..., 1] = high word
        planes = torch.from_numpy(np.ascontiguousarray(np.stack([w[:, :, 1], w[:, :, 0]])).view(np.int32)).to(dev)
    pol, split, origin = GC.PLANS[case.plan]
    p = E.DevicePanel(cols=cols, names=[f"c{j}" for j in range(data.ncols)],
                      seg_off=torch.from_numpy(GC.SEG_OFF).to(dev), seg_off_h=GC.SEG_OFF.copy(),
                      months=np.arange(GC.NSEG), planes=planes, chunk_policy=pol, chunk_split=split,
                      row_origin=origin)
    if cols is not None and planes is not None:
        p.planes_version = cols._version
    return p


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _launch(E, case):
    """Run the case: (data, partial [nchunks, nb, PK] host, the NaN guards' bits before and after)."""
    data = GC.panel_data(case.cons, case.ncols, case.nlevels, case.kind)
    panel = _panel(E, case, data)
    dev = panel.device
    lo, hi, shift, inv = GC.transform(case.xf, case.ncols)
    cuts = E.Cuts(_dev(lo, dev), _dev(hi, dev), None) if lo is not None else None
    seg, rows, off, order, wg = GC.plan_arrays(case.plan)
    plan = E._chunk_plan(panel)
    assert np.array_equal(plan.chunk_seg.cpu().numpy(), seg) and np.array_equal(plan.chunk_row.cpu().numpy(), rows)
    assert (plan.order is None) == (order is None) and (plan.wg_off is None) == (wg is None)
    nb = len(data.pats) * data.nlevels
    zw = GO.zwidth(case.ncols)
    buf = torch.full((len(seg) + 2, nb, zw * (zw + 1) // 2), float("nan"), dtype=torch.float64, device=dev)
    before = buf.cpu().numpy().view(np.uint64).copy()
    out = E.gram_partials(panel, data.models, level=_dev(data.level, dev), nlevels=data.nlevels, cuts=cuts,
                          shift=_dev(shift, dev), inv_scale=_dev(inv, dev), partial_out=buf[1:-1])
    torch.cuda.synchronize()
    assert len(out) == 1 and out[0].partial.data_ptr() == buf[1].data_ptr() and out[0].zw == zw
    assert out[0].group.npatterns == len(data.pats)
    after = buf.cpu().numpy()
    guards_ok = np.array_equal(after.view(np.uint64)[[0, -1]], before[[0, -1]])
    return data, after[1:-1], guards_ok


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("case", GC.CASES, ids=GC.case_id)
def test_partials_exact(E, case):
    """Integer panels: guards untouched, every defined entry of every (chunk, bucket) equal to
    the int64 reference bit for bit (so entry (0, 0) is the row count and an empty bucket or
    chunk is +0.0 throughout)."""
    data, got, guards_ok = _launch(E, case)
    ref = GC.reference(data, case.plan, case.xf)
    assert guards_ok, "a chunk next to the partials was written"
    dm = GO.defined_mask(data.masks, data.pats, data.nlevels, ref.zw)
    assert got.shape == ref.gram.shape
    want = np.where(dm[None], ref.gram, 0.0)
    have = np.where(dm[None], got, 0.0)
    bad = np.argwhere(_bits(have) != _bits(want))
    if len(bad):
        I, J = GO.packed_pairs(ref.zw)
        k, b, e = bad[0]
        pytest.fail(f"{len(bad)} defined entries differ; first: chunk {k} bucket {b} entry ({I[e]}, {J[e]}): "
                    f"got {got[k, b, e]!r}, expected {ref.gram[k, b, e]!r} (rows in bucket: {ref.n[k, b]})")
    assert np.array_equal(got[:, :, 0], ref.n.astype(np.float64))
    empty = ref.n == 0
    assert empty.any() and (~empty).any()
    for b in range(ref.nb):
        assert (_bits(got[empty[:, b], b][:, dm[b]]) == 0).all()


def test_partial_out_is_checked(E):
    """A buffer of another shape, or a strided view, is refused before anything is launched."""
    case = GC.CASES[0]
    data = GC.panel_data(case.cons, case.ncols, case.nlevels, case.kind)
    panel = _panel(E, case, data)
    nch, nb, pk = len(GC.plan_arrays(case.plan)[0]), len(data.pats) * data.nlevels, 16 * 17 // 2
    good = torch.zeros((nch, nb, pk), dtype=torch.float64, device=panel.device)
    assert E.gram_partials(panel, data.models, partial_out=good)[0].partial is good
    for bad in (torch.zeros((nch + 1, nb, pk), dtype=torch.float64, device=panel.device),
                torch.zeros((nch, nb, 2 * pk), dtype=torch.float64, device=panel.device)[:, :, ::2],
                torch.zeros((nch, nb, pk), dtype=torch.float32, device=panel.device)):
        with pytest.raises(ValueError, match="partial_out"):
            E.gram_partials(panel, data.models, partial_out=bad)
    with pytest.raises(ValueError, match="partial_out"):
        E.gram_partials(panel, data.models, partial_out=[good, good])


@pytest.mark.parametrize("case", GC.REAL_CASES, ids=GC.case_id)
def test_partials_real_valued(E, case):
    """Normals with mean >> spread, shifted by a nearby pivot, cut and scaled by a non-power of two:
    |entry - longdouble reference| <= 1.01 * n * 2^-53 * sum |z_i z_j| per (chunk, bucket)."""
    data, got, guards_ok = _launch(E, case)
    ref = GC.reference(data, case.plan, case.xf, exact=False)
    assert guards_ok
    dm = np.broadcast_to(GO.defined_mask(data.masks, data.pats, data.nlevels, ref.zw)[None], got.shape)
    err = np.abs(got.astype(np.longdouble) - ref.gram)
    bound = 1.01 * ref.n[:, :, None].astype(np.longdouble) * U * ref.absum
    assert np.isfinite(got[dm]).all()
    ratio = (err[dm] / np.maximum(bound[dm], np.longdouble(1e-300))).max()
    print(f"{GC.case_id(case)}: worst error / bound = {float(ratio):.3f}")
    assert (err[dm] <= bound[dm]).all()
    assert np.array_equal(got[:, :, 0], ref.n.astype(np.float64))


@pytest.mark.parametrize("case", GC.INF_CASES, ids=GC.case_id)
def test_partials_with_infinities(E, case):
    """+inf and -inf in one regressor, no cuts: every defined entry has the reference's class
    (NaN, +inf, -inf, or finite and equal); the class does not depend on the summation order."""
    data, got, guards_ok = _launch(E, case)
    assert guards_ok
    ref = GC.reference(data, case.plan, case.xf)      # counts, buckets and z
    assert np.isinf(ref.Z[ref.bucket >= 0]).any()
    dm = GO.defined_mask(data.masks, data.pats, data.nlevels, ref.zw)
    _, rows, _, _, _ = GC.plan_arrays(case.plan)
    seen = set()
    for k, (r0, r1) in enumerate(rows.reshape(-1, 2)):
        for b in range(ref.nb):
            r = r0 + np.flatnonzero(ref.bucket[r0:r1] == b)
            cls, val = GO.gram_classes(ref.Z, r, ref.zw)
            g = got[k, b]
            assert np.array_equal(GO.classify(g)[dm[b]], cls[dm[b]]), (k, b)
            fin = dm[b] & (cls == GO.CLASS_FINITE)
            assert np.array_equal(_bits(g[fin]), _bits(val[fin])), (k, b)
            seen |= set(cls[dm[b]].tolist())
    assert seen == {GO.CLASS_FINITE, GO.CLASS_NAN, GO.CLASS_PINF, GO.CLASS_NINF}


@pytest.mark.parametrize("case", GC.MOMENT_CASES, ids=GC.case_id)
def test_solve_moments(E, case):
    """fm_pass(..., moments=True) on the integer panels: per fitted (month, problem) the moments
    against the reference's problem Gram: n exactly, the means within 2 * 2^-53 * |mean|, each
    centered moment within 4 * 2^-53 * (|G_ij| + |G0i G0j| / n): four roundings in
    G_ij - G0i * G0j * (1 / n), the Gram itself being exact."""
    data = GC.panel_data(case.cons, case.ncols, case.nlevels, case.kind)
    panel = _panel(E, case, data)
    dev = panel.device
    _, _, shift, _ = GC.transform(case.xf, case.ncols)
    shift_h = np.zeros((case.ncols, GC.NSEG)) if shift is None else shift
    res = E.fm_pass(panel, data.models, level=_dev(data.level, dev), nlevels=data.nlevels,
                    shift=_dev(shift_h, dev), moments=True)
    st = res.status.cpu().numpy()
    mom = res.moments.cpu().numpy()
    ref = GC.reference(data, case.plan, case.xf)
    _, _, off, _, _ = GC.plan_arrays(case.plan)
    nfit = 0
    for t in range(GC.NSEG):
        chunks = np.arange(off[t], off[t + 1])
        for k, p in enumerate(res.problems):
            m = data.models[p.model]
            zidx = [0] + [1 + x for x in m.xs] + [1 + m.y]
            G, n, mean, cen = GO.problem_gram(ref, data.pats, data.nlevels, chunks, p.model, p.level, zidx)
            K1 = p.K + 1
            assert ((st[t, k] & E.L.FM_ST_SKIPPED) != 0) == (n < K1), (t, k)   # fitted: n >= K + 1 rows
            if n < K1:
                continue
            assert (st[t, k] & E.L.FM_ST_FITTED) != 0, (t, k)
            nfit += 1
            mo = mom[t, k]
            assert mo[0] == n, (t, k)
            gm = mo[1:1 + K1].astype(np.longdouble)
            assert (np.abs(gm - mean) <= 2 * U * np.abs(mean)).all(), (t, k)
            gc = mo[1 + K1:1 + K1 + K1 * K1].reshape(K1, K1).astype(np.longdouble)
            tol = 4 * U * (np.abs(G[1:, 1:]) + np.abs(np.outer(G[0, 1:], G[0, 1:])) / n)
            assert (np.abs(gc - cen) <= tol).all(), (t, k)
    assert nfit >= len(res.problems) * 5
