"""The two-wave high-word select with several units per workgroup.

A workgroup of select_pair_hk_kernel takes units (month, column) blockIdx.x, + gridDim.x, ...;
from its second unit on, the unit's values are loaded inside the loop, behind the kernel's own
global stores (the month bounds through vector loads made wave-uniform, the value loads
issued ahead during the previous unit's sorts).  The small select tests have fewer units than
workgroup slots, so only a panel with more than 3 * CUs * (workgroups per CU) units sends
every workgroup through that path at least twice.  Consecutive units of a workgroup differ in
length here and include an empty month and months with no row for the second wave."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
NCOLS = 4
QS = ((1, 99), (0, 100))


@pytest.fixture(scope="module")
def E():
    from fmcore import engine
    engine.require_device()
    return engine


def _same(a, b):
    """Bit-exact up to NaN payloads, the sign of zeros included."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return np.array_equal(a[m], b[m]) and np.array_equal(np.signbit(a[m]), np.signbit(b[m]))


def _panel(E, wgs_per_cu, long_month, seed):
    """More than 3 * CUs * wgs_per_cu units of NCOLS columns; month lengths cycle through
    LENGTHS (one month of ``long_month`` rows sets the kernel's instantiation)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    nseg = (3 * ncu * wgs_per_cu) // NCOLS + 97   # 97: the cycle of lengths is not aligned to the grid
    lens = np.array([LENGTHS[i % len(LENGTHS)] for i in range(nseg)], dtype=np.int64)
    if long_month:
        lens[nseg // 2] = long_month
    seg_off = np.zeros(nseg + 1, dtype=np.int64)
    np.cumsum(lens, out=seg_off[1:])
    n = int(seg_off[-1])
    rng = np.random.default_rng(seed)
    vals = rng.standard_normal((NCOLS, n))
    vals[rng.random((NCOLS, n)) < 0.02] = np.nan
    for c in range(NCOLS):
        ix = rng.choice(n, 6, replace=False)
        vals[c, ix] = [np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf]
    dev = E.require_device()
    p = E.DevicePanel(cols=torch.from_numpy(vals).to(dev), names=[f"c{c}" for c in range(NCOLS)],
                      seg_off=torch.from_numpy(seg_off).to(dev), seg_off_h=seg_off, months=np.arange(nseg))
    assert nseg * NCOLS > 3 * ncu * wgs_per_cu
    return p, vals, seg_off


@pytest.mark.parametrize("wgs_per_cu,long_month", [(12, 0), (8, 5000)], ids=["vph8", "vph40"])
def test_pair_select_many_units_per_workgroup(E, wgs_per_cu, long_month):
    panel, vals, seg_off = _panel(E, wgs_per_cu, long_month, 900 + long_month)
    assert panel.max_seg_len == (long_month or max(LENGTHS))
    ref = [E.select_cuts(panel, a / 100, b / 100, 1, E.LERP_NUMPY, center=True) for a, b in QS]
    ref = [{f: getattr(r, f).cpu().numpy() for f in ("lo", "hi", "center", "nvalid")} for r in ref]
    E.split_planes(panel)
    for (qa, qb), r in zip(QS, ref):
        g = E.select_cuts(panel, qa / 100, qb / 100, 1, E.LERP_NUMPY, center=True)
        got = {f: getattr(g, f).cpu().numpy() for f in ("lo", "hi", "center", "nvalid")}
        for f in ("lo", "hi", "center"):
            assert _same(got[f], r[f]), (qa, qb, f)
        assert np.array_equal(got["nvalid"], r["nvalid"])
        exp_lo = np.full(got["lo"].shape, np.nan)
        exp_hi = np.full(got["hi"].shape, np.nan)
        exp_n = np.zeros(got["nvalid"].shape, dtype=got["nvalid"].dtype)
        with np.errstate(invalid="ignore"):
            for c in range(NCOLS):
                for t in range(len(seg_off) - 1):
                    s = vals[c, seg_off[t]:seg_off[t + 1]]
                    v = s[~np.isnan(s)]
                    exp_n[c, t] = len(v)
                    if len(v):
                        exp_lo[c, t], exp_hi[c, t] = np.percentile(v, (qa, qb))
        assert np.array_equal(got["nvalid"], exp_n), (qa, qb)
        assert _same(got["lo"], exp_lo), (qa, qb)
        assert _same(got["hi"], exp_hi), (qa, qb)
