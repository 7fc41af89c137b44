"""Host-side checks of the rank transform's long-month path (months of more than 16,384 rows,
up to FM_RANK_MAX_ROWS = 65,536): the limit's constant in the header, the engine and the
library's refusal, the order of the argument checks, and the additivity the long kernel relies
on: the two counts of a row's key, taken per 16,384-row part and summed, give pandas' ranks bit
for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART = 16384


def test_limit_constant():
    from fmcore import engine as E
    text = open(os.path.join(ROOT, "include", "fm_hip.h")).read()
    m = re.search(r"^#define\s+FM_RANK_MAX_ROWS\s+(\d+)\s*$", text, re.M)
    assert m is not None, "FM_RANK_MAX_ROWS is not defined in include/fm_hip.h"
    assert E.RANK_MAX_ROWS == 65536 == int(m.group(1))


def _rc(lib, **kw):
    from fmcore import _lib as L
    buf = (ctypes.c_double * 8)()
    other = (ctypes.c_double * 8)()
    a = L.RankArgs()
    a.src, a.dst = ctypes.addressof(buf), ctypes.addressof(other)
    a.src_stride = a.dst_stride = 8
    a.ncols, a.nseg, a.max_seg_len = 1, 1, 8
    for k, v in kw.items():
        setattr(a, k, v)
    return lib.fm_rank_transform(ctypes.byref(a), None)


def test_refusal_names_the_limit():
    from fmcore import _lib as L
    lib = L.load()
    assert _rc(lib, max_seg_len=65537) == -3
    assert b"65536" in lib.fm_last_error()


def test_argument_checks_come_first():
    """A long month with a bad method is FM_EINVAL, not FM_ETOOBIG and not a launch (the
    pointers are host memory)."""
    from fmcore import _lib as L
    lib = L.load()
    assert _rc(lib, max_seg_len=20000, method=3) == -1
    assert _rc(lib, max_seg_len=65537, method=3) == -1


def _rank_by_parts(x, method, scale):
    """One month's ranks from per-part counts, as the long kernel takes them: for every row's
    key the part's #{keys < key} and #{keys <= key} (a searchsorted pair in the part's sorted
    eligible keys), summed over the parts, then the three formulas."""
    with np.errstate(invalid="ignore"):   # signalling NaNs among the values
        v = x + 0.0                       # -0.0 -> +0.0: the two zeros tie
    ok = ~np.isnan(v)
    lt = np.zeros(len(v), dtype=np.int64)
    le = np.zeros(len(v), dtype=np.int64)
    n = 0
    for p0 in range(0, len(v), PART):
        part = np.sort(v[p0:p0 + PART][ok[p0:p0 + PART]])
        n += len(part)
        lt[ok] += np.searchsorted(part, v[ok], side="left")
        le[ok] += np.searchsorted(part, v[ok], side="right")
    r = {"average": 0.5 * (lt + le + 1), "min": lt + 1.0, "max": le + 0.0}[method]
    y = {"raw": r, "pct": r / n, "uniform": r / (n + 1.0) - 0.5}[scale]
    return np.where(ok, y, np.nan)


@pytest.fixture(scope="module")
def long_month():
    return RO.tie_heavy(40000, np.random.default_rng(19))


@pytest.mark.parametrize("method,scale", RO.COMBOS)
def test_part_counts_add_up_to_pandas(long_month, method, scale):
    x = long_month
    seg_off = np.array([0, len(x)], dtype=np.int64)
    assert len(x) > 2 * PART and np.isinf(x).any() and np.isnan(x).any()
    RO.assert_same_bits(_rank_by_parts(x, method, scale), RO.pandas_rank(x, seg_off, method, scale),
                        f"{method}/{scale}")
