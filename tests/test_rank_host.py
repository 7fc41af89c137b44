"""Host-side checks of the per-month rank transform (A13): the binding's ABI, the counting
restatement of the definition against pandas bit for bit, the drop-in and engine signatures
and the pipeline switch's default."""
import ctypes
import inspect

import numpy as np
import pytest

import rank_oracle as RO


def test_binding_has_rank_transform():
    from fmcore import _lib as L
    assert "fm_rank_transform" in L.EXPORTED
    lib = L.load()
    assert hasattr(lib, "fm_rank_transform")
    assert lib.fm_struct_size(b"fm_rank_args") == ctypes.sizeof(L.RankArgs)
    assert (L.FM_RANK_AVERAGE, L.FM_RANK_MIN, L.FM_RANK_MAX) == (0, 1, 2)
    assert (L.FM_RANK_RAW, L.FM_RANK_PCT, L.FM_RANK_UNIFORM) == (0, 1, 2)


def test_argument_checks_need_no_device():
    """The argument checks run before any HIP call: bad method / scale, dst == src and a month
    past the limit are refused with the documented codes."""
    from fmcore import _lib as L
    from fmcore import engine as E
    lib = L.load()
    buf = (ctypes.c_double * 8)()
    other = (ctypes.c_double * 8)()

    def rc(**kw):
        a = L.RankArgs()
        a.src, a.dst = ctypes.addressof(buf), ctypes.addressof(other)
        a.src_stride = a.dst_stride = 8
        a.ncols, a.nseg, a.max_seg_len = 1, 1, 8
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.fm_rank_transform(ctypes.byref(a), None)

    assert rc(method=3) == -1 and rc(scale=-1) == -1 and rc(min_level=256) == -1
    assert rc(dst=ctypes.addressof(buf)) == -1
    assert b"dst must not be src" in lib.fm_last_error()
    assert rc(max_seg_len=E.RANK_MAX_ROWS + 1) == -3
    assert E.RANK_MAX_ROWS >= 16384


@pytest.mark.parametrize("method,scale", RO.COMBOS)
def test_restatement_equals_pandas(method, scale):
    rng = np.random.default_rng(17)
    lens = np.array([0, 1, 2, 3, 64, 65, 130, 257, 400])
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg_off[-1])
    x = RO.tie_heavy(n, rng)
    x[seg_off[5]:seg_off[6]] = np.nan                     # an all-NaN month
    x[seg_off[6]:seg_off[7]] = 0.25                       # an all-equal month
    assert np.isinf(x).any() and (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
    level = rng.integers(0, 3, n).astype(np.uint8)
    for lv, ml in ((None, 0), (level, 1), (level, 2)):
        RO.assert_same_bits(RO.counting_rank(x, seg_off, method, scale, lv, ml),
                            RO.pandas_rank(x, seg_off, method, scale, lv, ml), f"{method}/{scale}/min_level {ml}")
    y = rng.normal(size=n)
    RO.assert_same_bits(RO.counting_rank(y, seg_off, method, scale), RO.pandas_rank(y, seg_off, method, scale),
                        f"{method}/{scale} tie-free")


def test_signatures():
    from fmdrop import bind
    from fmdrop import calc_Lewellen_2014 as CL
    from fmcore import engine as E
    sig = inspect.signature(CL.rank_transform)
    assert list(sig.parameters) == ["crsp_comp", "varlist", "date_col", "method", "scale", "universe"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(date_col="mthcaldt", method="average", scale="pct", universe=None)
    assert "rank_transform" not in bind.HOT["calc_Lewellen_2014"]   # the reference has no such name
    sig = inspect.signature(E.rank_transform)
    assert list(sig.parameters) == ["panel", "cols", "method", "scale", "level", "min_level", "out"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(cols=None, method="average", scale="pct", level=None, min_level=0, out=None)


def test_pipeline_config_default():
    import dataclasses
    from fmcore import lewellen as LW
    assert LW.PipelineConfig().rank is None
    assert dataclasses.fields(LW.PipelineConfig)[-1].name == "rank"   # a trailing field
    assert LW.PipelineConfig(rank="uniform").rank == "uniform"
