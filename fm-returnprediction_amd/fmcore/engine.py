"""Device-resident Fama-MacBeth engine: host orchestration of libfm_hip kernels.

torch (ROCm) only provides device buffers and the stream; every computation on the hot
path is a libfm_hip kernel.  There is no CPU fallback: without a HIP device the
functions raise.

Layout in HBM (``DevicePanel``): the panel's C columns with rows sorted by (month, input
order) -- month segments are CSR ``seg_off[T+1]`` -- as an FP64 SoA block ``cols[C, n]``
and/or the split layout ``planes[2, C, n]`` (uint32 high / low words: the selects read the
high plane, the Gram both), plus optional ``me`` (FP64), ``nyse`` (uint8) and ``group`` (int32
group / industry code) rows and a uint8 universe ``level`` per row.  A panel built with
``layout="planes"`` holds no FP64 columns at all (half the HBM): the whole Table-2 pass reads
the planes, and consumers of FP64 columns (clip, forecasts, moments) get them from ``values()``.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

# statsmodels/numpy quantile modes
LERP_NUMPY = 0
LERP_PANDAS = 1


def require_device():
    if not torch.cuda.is_available():
        raise RuntimeError("fmcore needs a HIP device (MI355X); none is visible and there is "
                           "no CPU fallback")
    L.load()
    return torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    return None if t is None else t.data_ptr()


class KernelTimer:
    """Records HIP events on the current stream around every libfm_hip launch made by
    this module while active (bench.py uses it for the per-kernel roofline)."""

    def __init__(self):
        self.events = {}

    def __enter__(self):
        global _TIMER
        _TIMER = self
        return self

    def __exit__(self, *exc):
        global _TIMER
        _TIMER = None

    def avg_ms(self, name):
        torch.cuda.synchronize()
        ev = self.events.get(name, [])
        if not ev:
            return float("nan")
        return float(np.mean([a.elapsed_time(b) for a, b in ev]))

    def names(self):
        return list(self.events)


_TIMER = None

# The latest argument struct of each struct-taking entry point, with the tensors it points
# to kept alive, so one kernel can be re-issued in isolation (time_launch).
LAST_LAUNCH = {}


def _remember(tag, name, struct, *keep):
    LAST_LAUNCH[tag] = (name, struct, keep)


def time_launch(tag, reps=20):
    """Average device milliseconds of the latest `tag` launch, re-issued `reps` times back
    to back on the current stream.  The host stays ahead of the device, so unlike events
    around single launches of a host-bound pipeline this excludes launch gaps.  The
    re-issued launches rewrite the same outputs with the same values."""
    name, struct, keep = LAST_LAUNCH[tag]
    st = _stream()
    args = (L.C.byref(struct),) if struct is not None else keep[1]
    L.call(name, *args, st)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        L.call(name, *args, st)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _kcall(tag, name, *args):
    t = _TIMER
    if t is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
    L.call(name, *args)
    if t is not None:
        e1.record()
        t.events.setdefault(tag, []).append((e0, e1))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------
# Panel
# ------------------------------------------------------------------------------------------
@dataclass
class DevicePanel:
    cols: Optional[torch.Tensor]       # [C, n] float64, contiguous (None: a planes-only panel)
    names: List[str]
    seg_off: torch.Tensor              # [T+1] int64 (device)
    seg_off_h: np.ndarray              # [T+1] int64 (host)
    months: object = None              # segment labels (host)
    me: Optional[torch.Tensor] = None  # [n] float64
    nyse: Optional[torch.Tensor] = None  # [n] uint8
    order: Optional[np.ndarray] = None   # sorted row -> original positional row
    chunk_rows: Optional[int] = None     # Gram chunking override (sharded runs: global policy)
    chunk_split: Optional[bool] = None   # split-month Gram plan (make_chunks_split) override
    planes: Optional[torch.Tensor] = None   # [2, C, n] int32: the values' high / low words
    chunk_policy: Optional[tuple] = None    # Gram plan of the GLOBAL panel (chunk_policy()), sharded runs
    row_origin: int = 0                     # global row of this panel's row 0 (balanced plans)
    planes_version: int = -1                # cols._version when the planes were made from cols
    group: Optional[torch.Tensor] = None    # [n] int32: each row's group (industry) code, month-major; < 0: none
    ngroups: int = 0                        # codes 0 .. ngroups-1 (at most MAX_GROUPS)
    ids: Optional[torch.Tensor] = None      # [n] int64: each row's firm id, month-major, ascending within a month
    month_index: Optional[np.ndarray] = None   # [T] int32 (host): each segment's calendar month number, ascending

    @property
    def device(self):
        return (self.cols if self.cols is not None else self.planes).device

    def month_index_device(self):
        """``month_index`` on the device (int32 [T]), uploaded once and kept."""
        t = self.__dict__.get("_month_index_dev")
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(self.month_index, dtype=np.int32)).to(self.device)
            self.__dict__["_month_index_dev"] = t
        return t

    def values(self):
        """The FP64 columns [C, n]: ``cols``, or for a planes-only panel a device merge of the
        planes (fm_merge_planes), made once and kept.  Off the Table-2 hot path (clip,
        forecasts, moments, the standardize variant)."""
        if self.cols is not None:
            return self.cols
        m = self.__dict__.get("_merged")
        if m is None:
            C, n = self.planes.shape[1], self.planes.shape[2]
            m = torch.empty((C, n), dtype=torch.float64, device=self.planes.device)
            _kcall("fm_merge_planes", "fm_merge_planes", self.planes[0].data_ptr(), self.planes[1].data_ptr(),
                   self.planes.stride(1), C, n, m.data_ptr(), m.stride(0), _stream())
            self.__dict__["_merged"] = m
        return m

    def column_host(self, i, n=None):
        """Column i (its first n rows) as a host float64 array, from the planes without an
        FP64 device copy when the panel has none."""
        n = self.nrows if n is None else n
        if self.cols is not None:
            return self.cols[i, :n].cpu().numpy()
        hi = self.planes[0, i, :n].cpu().numpy().astype(np.uint32).astype(np.uint64)
        lo = self.planes[1, i, :n].cpu().numpy().astype(np.uint32).astype(np.uint64)
        return ((hi << np.uint64(32)) | lo).view(np.float64)

    def check_planes(self):
        """The planes must still be the FP64 columns' words: an in-place write to ``cols``
        after the planes were made (torch bumps the tensor's version counter) is refused."""
        if self.planes is not None and self.cols is not None and self.planes_version >= 0 and \
                self.cols._version != self.planes_version:
            raise RuntimeError("panel.cols was modified in place after its planes were made: call "
                               "split_planes(panel) again (or build a new panel)")

    @property
    def nrows(self):
        return int(self.seg_off_h[-1])

    @property
    def nseg(self):
        return len(self.seg_off_h) - 1

    @property
    def ncols(self):
        return self.cols.shape[0] if self.cols is not None else self.planes.shape[1]

    @property
    def stride(self):
        return self.values().stride(0)

    @property
    def max_seg_len(self):
        return int(np.diff(self.seg_off_h).max()) if self.nseg else 0

    def col(self, name):
        return self.names.index(name)


def month_segments(labels):
    """Factorize month labels (sorted) -> (codes, uniques, stable order of valid rows,
    seg_off).  Rows with a missing label are excluded (pandas groupby/dropna drop them)."""
    import pandas as pd
    codes, uniq = pd.factorize(labels, sort=True)
    codes = np.asarray(codes)
    if len(uniq) < 32767:
        # numpy sorts 16-bit keys stably by radix (vs a merge sort on int64): ~4x at 3M rows
        codes = codes.astype(np.int16)
    order = np.argsort(codes, kind="stable")
    order = order[codes[order] >= 0]
    counts = np.bincount(codes[codes >= 0], minlength=len(uniq))
    seg_off = np.zeros(len(uniq) + 1, dtype=np.int64)
    np.cumsum(counts, out=seg_off[1:])
    return codes, uniq, order, seg_off


def month_index(labels):
    """The calendar month number of each segment label -> int32 [T], strictly ascending:
    datetime64 labels map to year * 12 + month - 1, integer labels are taken as they are (a count
    of months).  Anything else, a missing date, or two labels of one month (or labels out of
    order) raise ValueError: the month links compare these numbers to tell neighbouring months
    from a gap in the calendar."""
    a = np.asarray(labels)
    if a.dtype.kind == "M":
        if np.isnat(a).any():
            raise ValueError("month_index: a month label is NaT")
        m = a.astype("datetime64[M]").astype(np.int64) + 1970 * 12
    elif a.dtype.kind in "iu":
        m = a.astype(np.int64)
    else:
        raise ValueError(f"month_index: month labels must be datetime64 or integers, not {a.dtype}")
    if m.ndim != 1:
        raise ValueError("month_index: month labels must be one-dimensional")
    if len(m) and (m.min() < -(2 ** 31) or m.max() >= 2 ** 31):
        raise ValueError("month_index: month numbers must fit 32 bits")
    if len(m) > 1 and not bool(np.all(np.diff(m) > 0)):
        raise ValueError("month_index: two segment labels fall in the same calendar month (or the labels "
                         "do not ascend)")
    return m.astype(np.int32)


def _set_ids(panel, ids_t):
    """Firm identity of a freshly built panel: the month-major ids and the segments' calendar
    month numbers (host and device)."""
    panel.ids = ids_t
    panel.month_index = month_index(panel.months)
    panel.month_index_device()
    return panel


def gather_layout(raw, perm, layout="f64"):
    """The device gather of an ingest: FP64 columns ``raw`` [C, n_in] (input row order) ->
    month-major rows in the panel's layout, (cols, planes): "f64" the FP64 columns, "planes"
    the high / low 32-bit words gathered straight from the raw words (no FP64 panel copy),
    "both"."""
    if layout not in PANEL_LAYOUTS:
        raise ValueError(f"layout must be one of {PANEL_LAYOUTS}")
    cols = planes = None
    if layout != "planes":
        cols = raw.index_select(1, perm).contiguous()
    if layout != "f64":
        C = raw.shape[0]
        words = raw.contiguous().view(torch.int32).view(C, -1, 2)   # little-endian: [..., 1] = high word
        planes = torch.empty((2, C, max(perm.numel(), 1)), dtype=torch.int32, device=raw.device)
        planes[0, :, :perm.numel()] = words[:, :, 1].index_select(1, perm)
        planes[1, :, :perm.numel()] = words[:, :, 0].index_select(1, perm)
    return cols, planes


def _check_group(who, group, ngroups, n_in):
    """Host group codes of an ingest -> (int32 [n_in], ngroups); ``ngroups`` None: max code + 1."""
    group = np.asarray(group)
    if group.dtype.kind not in "iu" or group.shape != (n_in,):
        raise ValueError(f"{who}: group must hold one integer code per input row")
    if len(group) and (group.min() < -(2 ** 31) or group.max() >= 2 ** 31):
        raise ValueError(f"{who}: group codes must fit 32 bits")
    if ngroups is None:
        ngroups = max(int(group.max()) + 1 if len(group) else 1, 1)
    ngroups = int(ngroups)
    if ngroups < 1 or ngroups > MAX_GROUPS:
        raise ValueError(f"{who}: ngroups must be 1..{MAX_GROUPS}, got {ngroups}")
    return group.astype(np.int32), ngroups


def panel_from_arrays(arrays: Sequence[np.ndarray], names, labels, me=None, nyse=None,
                      device=None, layout="f64", ids=None, group=None, ngroups=None):
    """Upload host columns (original row order) and permute them month-major on device, into
    the panel's ``layout`` ("f64", "planes": the split layout only, "both").  ``ids``: each input
    row's integer firm id; the panel then carries firm identity (``ids``, ``month_index``), which
    the month links and the multi-month returns need: the labels must then be datetime64 or
    integer month numbers (``month_index``), and a month's rows must arrive in ascending id order
    (``month_links`` checks it).  ``group``: one integer group (industry) code per input row
    (``group_codes`` makes them from labels; a negative code: no group), permuted month-major like
    ``nyse``, with ``ngroups`` (default: the largest code + 1; more than MAX_GROUPS: ValueError) --
    what ``group_adjust`` reads."""
    if group is not None:
        group, ngroups = _check_group("panel_from_arrays", group, ngroups, len(labels))
    device = device or require_device()
    _, uniq, order, seg_off = month_segments(labels)
    if ids is not None:
        month_index(uniq)   # refuse labels without a calendar before any upload
        ids = np.asarray(ids)
        if ids.dtype.kind not in "iu" or ids.shape != (len(labels),):
            raise ValueError("panel_from_arrays: ids must hold one integer firm id per input row")
    n_in = len(labels)
    host = np.empty((len(arrays), n_in), dtype=np.float64)
    for i, a in enumerate(arrays):
        host[i] = np.asarray(a, dtype=np.float64)
    raw = torch.from_numpy(host).to(device, non_blocking=False)
    perm = torch.from_numpy(order.astype(np.int64)).to(device)
    cols, planes = gather_layout(raw, perm, layout)
    me_t = nyse_t = None
    if me is not None:
        me_t = torch.from_numpy(np.asarray(me, dtype=np.float64)).to(device).index_select(0, perm)
    if nyse is not None:
        nyse_t = torch.from_numpy(np.asarray(nyse, dtype=np.uint8)).to(device).index_select(0, perm)
    p = DevicePanel(cols=cols, names=list(names), seg_off=torch.from_numpy(seg_off).to(device),
                    seg_off_h=seg_off, months=uniq, me=me_t, nyse=nyse_t, order=order, planes=planes)
    if cols is not None and planes is not None:
        p.planes_version = cols._version
    if group is not None:
        p.group = torch.from_numpy(group).to(device).index_select(0, perm)
        p.ngroups = ngroups
    if ids is not None:
        _set_ids(p, torch.from_numpy(ids.astype(np.int64)).to(device).index_select(0, perm))
    return p


def split_planes(panel: DevicePanel):
    """The panel's FP64 columns as two 32-bit planes (fm_split_planes), kept beside cols:
    the selects then order values by their high words (half the bytes) and the Gram reads
    both planes (the high plane the select just streamed is still in the Infinity Cache).
    A device pass over the panel, done once at ingest."""
    C, n = panel.cols.shape
    planes = torch.empty((2, C, max(n, 1)), dtype=torch.int32, device=panel.cols.device)
    _kcall("fm_split_planes", "fm_split_planes", panel.cols.data_ptr(), panel.stride, C, n, planes[0].data_ptr(),
           planes[1].data_ptr(), planes.stride(1), _stream())
    panel.planes = planes
    panel.planes_version = panel.cols._version
    return panel


@dataclass
class _Src:
    """What a panel kernel reads: FP64 columns (``f64``) and/or the panel's planes."""
    f64: Optional[torch.Tensor]
    hp: Optional[int]
    lp: Optional[int]
    pstride: int
    ncols: int
    device: object

    @property
    def ptr(self):
        return None if self.f64 is None else self.f64.data_ptr()

    @property
    def stride(self):
        return self.f64.stride(0) if self.f64 is not None else self.pstride


def _source(panel: DevicePanel, cols=None):
    """``cols`` given: those FP64 columns only.  Else the panel's own values: its FP64
    columns, its planes, or both (a planes-only panel: no FP64 pointer at all)."""
    if cols is not None:
        cols = cols.view(1, -1) if cols.dim() == 1 else cols
        return _Src(cols, None, None, 0, cols.shape[0], cols.device)
    panel.check_planes()
    hp = lp = None
    ps = 0
    if panel.planes is not None:
        hp, lp, ps = panel.planes[0].data_ptr(), panel.planes[1].data_ptr(), panel.planes.stride(1)
    return _Src(panel.cols, hp, lp, ps, panel.ncols, panel.device)


PANEL_LAYOUTS = ("f64", "planes", "both")


def panel_synthetic(nmonths, nfirms, seed, month0=0, nan_rate=0.02, nyse_rate=0.4, device=None, layout="f64"):
    """Generate a balanced synthetic panel directly in HBM (fm_gen_panel; identical to
    fmcore.synth.synth_arrays with present_rate=1).  ``layout``: "f64" the FP64 columns,
    "planes" only the split layout (fm_gen_panel_planes writes the high / low words itself:
    no FP64 columns, no layout pass), "both".  The firm ids are 10000 + the position in the
    month, the month numbers month0, month0 + 1, ..."""
    from .synth import WINSOR_VARS
    if layout not in PANEL_LAYOUTS:
        raise ValueError(f"layout must be one of {PANEL_LAYOUTS}")
    device = device or require_device()
    n = nmonths * nfirms
    C = len(WINSOR_VARS)
    cols = planes = None
    if layout != "planes":
        cols = torch.empty((C, n), dtype=torch.float64, device=device)
    if layout != "f64":
        planes = torch.empty((2, C, max(n, 1)), dtype=torch.int32, device=device)
    me = torch.empty(n, dtype=torch.float64, device=device)
    nyse = torch.empty(n, dtype=torch.uint8, device=device)
    if planes is None:
        _kcall("fm_gen_panel", "fm_gen_panel", seed, month0, nmonths, nfirms, nan_rate, nyse_rate, cols.data_ptr(),
               cols.stride(0), me.data_ptr(), nyse.data_ptr(), _stream())
    else:
        _kcall("fm_gen_panel", "fm_gen_panel_planes", seed, month0, nmonths, nfirms, nan_rate, nyse_rate, _ptr(cols),
               cols.stride(0) if cols is not None else 0, planes[0].data_ptr(), planes[1].data_ptr(),
               planes.stride(1), me.data_ptr(), nyse.data_ptr(), _stream())
    seg_off = np.arange(nmonths + 1, dtype=np.int64) * nfirms
    p = DevicePanel(cols=cols, names=list(WINSOR_VARS), seg_off=torch.from_numpy(seg_off).to(device),
                    seg_off_h=seg_off, months=np.arange(month0, month0 + nmonths), me=me, nyse=nyse,
                    planes=planes)
    if cols is not None and planes is not None:
        p.planes_version = cols._version
    _set_ids(p, _balanced_ids(nmonths, nfirms, device))
    return p


def _balanced_ids(nmonths, nfirms, device):
    """The ids of a balanced panel, 10000 + the position in the month, for every month: one month
    uploaded, then doubled by contiguous device copies (memcpys only, so generating a panel still
    loads no kernel but the generator's)."""
    n = nmonths * nfirms
    ids = torch.empty(n, dtype=torch.int64, device=device)
    if n:
        ids[:nfirms].copy_(torch.from_numpy(np.arange(nfirms, dtype=np.int64) + 10000))
    k = nfirms
    while 0 < k < n:
        m = min(k, n - k)
        ids[k:k + m].copy_(ids[:m])
        k += m
    return ids


# ------------------------------------------------------------------------------------------
# Order statistics, clipping, universes
# ------------------------------------------------------------------------------------------
@dataclass
class Cuts:
    lo: torch.Tensor      # [C, T]
    hi: torch.Tensor
    nvalid: torch.Tensor  # [C, T] int32
    mean: Optional[torch.Tensor] = None
    sd: Optional[torch.Tensor] = None
    center: Optional[torch.Tensor] = None   # Gram pivot (midpoint of the cuts)


_SELECT_WS = {}   # device -> the zeroed fm_select work buffer (the library leaves it zeroed)
_SELECT_WS_OLD = []   # outgrown buffers stay alive: captured HIP graphs may still use them


def select_ws(nseg, ncols, max_seg_len, device):
    """fm_select_args.ws: the fix-up worklist (+ zero-sign replay slots for > 6,144-row
    months), zeroed once; every fm_select call leaves it zeroed, so one buffer per device
    serves all calls on the stream (grown on demand, never freed while graphs may use it)."""
    need = int(L.load().fm_select_ws_bytes(int(nseg), int(ncols), int(max_seg_len)))
    if need < 0:
        raise ValueError("fm_select_ws_bytes: bad sizes")
    key = str(device)
    buf = _SELECT_WS.get(key)
    if buf is None or buf.numel() < need:
        if buf is not None:
            _SELECT_WS_OLD.append(buf)
        buf = torch.zeros(max(need, 1 << 16), dtype=torch.uint8, device=device)
        _SELECT_WS[key] = buf
    return buf


def select_cuts(panel: DevicePanel, q_lo, q_hi, min_count, mode=LERP_NUMPY, cols=None,
                row_mask=None, moments=False, center=False, level=None, tag="fm_select_cuts",
                universe=None):
    """Per (column, month) quantile cuts.  ``cols`` defaults to panel.cols.  ``moments``:
    also the clipped mean / sd; ``center``: also a Gram pivot inside the data; ``level``
    (uint8 [rows], one column): every row's (x >= lo) + (x >= hi) (fm_select).
    ``universe`` = (q_a, q_b): also get_subsets' NYSE breakpoints and level bytes of the
    panel's me / nyse rows in the same call (fm_select_universe: sharing the select fix-up's
    launch for months of <= 5,120 rows, riding the long-month kernel's launch for
    6,145-20,480-row months without the histogram (MID) variant, its own launch first
    otherwise); returns (Cuts, (cut_a, cut_b, level)) then."""
    if cols is not None:
        src = _source(panel, cols)
    elif row_mask is not None or moments:   # the row-masked and moments paths read FP64 columns
        src = _source(panel, panel.values())
    else:
        src = _source(panel)
    C, T = src.ncols, panel.nseg
    dev = src.device
    lo = torch.empty((C, T), dtype=torch.float64, device=dev)
    hi = torch.empty_like(lo)
    nv = torch.empty((C, T), dtype=torch.int32, device=dev)
    mean = sd = cen = None
    if moments:
        mean = torch.empty_like(lo)
        sd = torch.empty_like(lo)
    if center:
        cen = torch.empty_like(lo)
    msl = max(panel.max_seg_len, 1)
    ws = select_ws(T, C, msl, dev)
    sa = L.SelectArgs(cols=src.ptr, col_stride=src.stride if src.f64 is not None else 0, ncols=C,
                      seg_off=panel.seg_off.data_ptr(),
                      nseg=T, max_seg_len=msl, row_mask=_ptr(row_mask), q_lo=float(q_lo),
                      q_hi=float(q_hi), min_count=int(min_count), lerp_mode=int(mode), lo=lo.data_ptr(),
                      hi=hi.data_ptr(), nvalid=nv.data_ptr(), mean=_ptr(mean), sd=_ptr(sd), center=_ptr(cen),
                      level=_ptr(level), ws=ws.data_ptr(), hi_plane=src.hp, plane_stride=src.pstride,
                      lo_plane=src.lp)
    if universe is None:
        _kcall(tag, "fm_select", L.C.byref(sa), _stream())
        _remember(tag, "fm_select", sa, src, panel.planes, lo, hi, nv, mean, sd, cen, row_mask, panel.seg_off, level)
        return Cuts(lo, hi, nv, mean, sd, cen)
    ca = torch.empty(T, dtype=torch.float64, device=dev)
    cb = torch.empty_like(ca)
    ulev = torch.empty(panel.nrows, dtype=torch.uint8, device=dev)
    ua = L.UniverseArgs(me=panel.me.data_ptr(), nyse=panel.nyse.data_ptr(), q_a=float(universe[0]),
                        q_b=float(universe[1]), cut_a=ca.data_ptr(), cut_b=cb.data_ptr(), level=ulev.data_ptr())
    _kcall(tag, "fm_select_universe", L.C.byref(sa), L.C.byref(ua), _stream())
    # re-issued by time_launch with both structs (keep[1] holds the argument tuple)
    LAST_LAUNCH[tag] = ("fm_select_universe", None,
                        ((sa, ua, src, panel.planes, lo, hi, nv, mean, sd, cen, row_mask, panel.seg_off, panel.me, panel.nyse,
                          ca, cb, ulev), (L.C.byref(sa), L.C.byref(ua))))
    return Cuts(lo, hi, nv, mean, sd, cen), (ca, cb, ulev)


def clip(panel: DevicePanel, cuts: Cuts, out=None):
    v = panel.values()
    out = torch.empty_like(v) if out is None else out
    _kcall("fm_clip", "fm_clip", v.data_ptr(), out.data_ptr(), v.stride(0), panel.ncols,
           panel.seg_off.data_ptr(), panel.nseg, panel.nrows, cuts.lo.data_ptr(), cuts.hi.data_ptr(),
           _stream())
    return out


def standardize(panel: DevicePanel, mean, sd, src=None, out=None):
    src = panel.values() if src is None else src
    out = torch.empty_like(src) if out is None else out
    _kcall("fm_standardize", "fm_standardize", src.data_ptr(), out.data_ptr(), src.stride(0), src.shape[0],
           panel.seg_off.data_ptr(), panel.nseg, panel.nrows, mean.data_ptr(), sd.data_ptr(),
           _stream())
    return out


def nyse_breakpoints(panel: DevicePanel, q_a=0.2, q_b=0.5, level=None):
    """me_20 / me_50 per month over NYSE rows (pandas groupby.quantile lerp); with ``level``
    (uint8 [rows]) also every row's universe level from them, in the same call."""
    cuts = select_cuts(panel, q_a, q_b, 1, LERP_PANDAS, cols=panel.me.view(1, -1), row_mask=panel.nyse,
                       level=level, tag="fm_select_cuts[nyse]")
    return cuts.lo[0], cuts.hi[0]


def universe_level(panel: DevicePanel, cut_a, cut_b):
    level = torch.empty(panel.nrows, dtype=torch.uint8, device=panel.device)
    _kcall("fm_universe_level", "fm_universe_level", panel.me.data_ptr(), panel.seg_off.data_ptr(), panel.nseg,
           panel.nrows, cut_a.data_ptr(), cut_b.data_ptr(), level.data_ptr(), _stream())
    return level


def universe(panel: DevicePanel, q_a=0.2, q_b=0.5):
    """get_subsets on the device (reference src/calc_Lewellen_2014.py:69-105): the NYSE
    me_20 / me_50 breakpoints and the nested universe level byte of every row, one launch
    (fm_universe); months longer than its register budget take fm_select (row mask, the
    level bytes written by the same call).  Returns (cut_a [T], cut_b [T], level [rows] uint8)."""
    if panel.max_seg_len > UNIVERSE_MAX_ROWS:
        level = torch.empty(panel.nrows, dtype=torch.uint8, device=panel.device)
        a, b = nyse_breakpoints(panel, q_a, q_b, level=level)
        return a, b, level
    dev = panel.device
    a = torch.empty(panel.nseg, dtype=torch.float64, device=dev)
    b = torch.empty_like(a)
    level = torch.empty(panel.nrows, dtype=torch.uint8, device=dev)
    args = (panel.me.data_ptr(), panel.nyse.data_ptr(), panel.seg_off.data_ptr(), panel.nseg,
            max(panel.max_seg_len, 0), float(q_a), float(q_b), a.data_ptr(), b.data_ptr(), level.data_ptr())
    _kcall("fm_universe", "fm_universe", *args, _stream())
    _remember("fm_universe", "fm_universe", None, (panel.me, panel.nyse, panel.seg_off, a, b, level), args)
    return a, b, level


UNIVERSE_MAX_ROWS = 64 * 256   # fm_universe's register budget (one workgroup per month)
# fm_select's long-month kernel: months of SELECT_LONG_MIN + 1 .. SELECT_LONG_MAX rows (no row
# mask, no moments); fm_select_universe puts the universe months into its launch
SELECT_LONG_MIN, SELECT_LONG_MAX = 24 * 256, 40 * 512


def pilot_shift(panel: DevicePanel, cols=None):
    src = panel.values() if cols is None else cols
    sh = torch.empty((src.shape[0], panel.nseg), dtype=torch.float64, device=src.device)
    _kcall("fm_pilot_shift", "fm_pilot_shift", src.data_ptr(), src.stride(0), src.shape[0], panel.seg_off.data_ptr(),
           panel.nseg, sh.data_ptr(), _stream())
    return sh


# ------------------------------------------------------------------------------------------
# Models, problems, the batched Gram pass
# ------------------------------------------------------------------------------------------
@dataclass
class Model:
    name: str
    y: int                       # panel column of the dependent variable
    xs: List[int]                # panel columns of the regressors (order = output order)
    levels: Sequence[int] = (0,)  # universe levels to solve (0 all, 1 all-but-tiny, 2 large)
    const_check: bool = True     # add_constant(has_constant='skip') semantics (regressions.py)

    @property
    def mask(self):
        m = 1 << self.y
        for x in self.xs:
            m |= 1 << x
        return m


@dataclass
class Problem:
    model: int
    level: int
    K: int


@dataclass
class FMResult:
    problems: List[Problem]
    rec: torch.Tensor            # [T, nprob, pmax+2]
    status: torch.Tensor         # [T, nprob] int32 (FM_ST_* bits)
    pmax: int
    moments: Optional[torch.Tensor] = None   # [T, nprob, mom_stride]
    mom_stride: int = 0

    @property
    def nprob(self):
        return len(self.problems)


def plan_patterns(models: Sequence[Model]):
    """Validity patterns that can occur: if model a's columns are a subset of model b's,
    every row valid for b is valid for a.  Returns (lut[1<<M] uint8, pattern_models)."""
    M = len(models)
    masks = [m.mask for m in models]
    pats = []
    for P in range(1, 1 << M):
        ok = True
        for a, b in itertools.permutations(range(M), 2):
            if (masks[a] & masks[b]) == masks[a] and (P >> b) & 1 and not (P >> a) & 1:
                ok = False
                break
        if ok:
            pats.append(P)
    lut = np.full(1 << M, 255, dtype=np.uint8)
    for i, P in enumerate(pats):
        lut[P] = i
    return lut, pats


def group_models(models: Sequence[Model], nlevels, cap):
    """Split models into groups whose bucket count (patterns x levels) fits ``cap``."""
    groups, cur = [], []
    for i, m in enumerate(models):
        trial = cur + [i]
        if len(trial) > L.FM_MAX_MODELS or len(plan_patterns([models[j] for j in trial])[1]) * nlevels > cap:
            if not cur:
                raise ValueError("a single model exceeds the bucket budget")
            groups.append(cur)
            cur = [i]
        else:
            cur = trial
    if cur:
        groups.append(cur)
    return groups


def default_chunk_rows(total_rows, nseg, max_seg_len, target_chunks=512):
    """Rows per Gram workgroup: whole months when there are enough months to fill the chip
    (fm_gram keeps 3 workgroups per CU resident, 768 slots: one month per workgroup means one
    prologue and one cross-wave epilogue per month), else months split into
    ~target_chunks/nseg pieces.  Callers that shard months across ranks pass the GLOBAL sizes
    so every rank chunks (and sums) identically."""
    if nseg == 0:
        return 256
    per = max(1, -(-target_chunks // nseg))
    ch = -(-max(int(max_seg_len), 1) // per)
    return max(256, ((ch + 255) // 256) * 256)


GRAM_SLOTS_PER_CU = 3   # fm_gram workgroups resident per CU (3 waves / SIMD)
# The plan's slot count is a constant of the plan, not a query of the local device: a plan
# (and so every month's FP64 partial-sum order) must not change with the GPU a rank runs on.
GRAM_PLAN_SLOTS = 256 * GRAM_SLOTS_PER_CU   # MI355X: 256 CUs


def chunk_policy(total_rows, nseg, max_seg_len, slots=None, min_rows=2048):
    """The Gram's chunk plan for a panel of these GLOBAL sizes (sharded callers pass the
    global panel's, so every rank cuts, and sums, every month identically):

    * ("balanced", R): when the months are too few to even out over the resident workgroup
      slots (fewer than 4 rounds of them), every workgroup takes R consecutive rows of the
      global row space, cut at month boundaries into chunks (a workgroup can end one month and
      start the next), so every CU gets the same rows.  At the bench's 600 x 5,000 panel a
      grid of whole months leaves 88 CUs a third month to finish while the rest idle
      (profiles/r04/v1_size_scan.log: 600 months cost what 768 do).
    * ("months", chunk_rows): otherwise months split into ceil(L / chunk_rows) chunks
      (default_chunk_rows), one per workgroup.

    ``slots`` defaults to GRAM_PLAN_SLOTS (a constant, never the local device's CU count)."""
    slots = slots or GRAM_PLAN_SLOTS
    if nseg > 0 and nseg < 4 * slots:
        R = -(-int(total_rows) // slots)
        if R >= min_rows:
            return ("balanced", int(R))
    return ("months", default_chunk_rows(total_rows, nseg, max_seg_len))


def make_chunks_balanced(seg_off_h, rows_per_wg, row_origin=0):
    """Chunks = the row space cut at month boundaries and at global row multiples of
    rows_per_wg (row_origin = global row of local row 0); the chunks of one R-block go to one
    workgroup.  Returns (seg, rows, off, wg_off): chunk month, (r0, r1) pairs, a month's chunk
    range (fm_solve sums them in order) and each workgroup's chunk range.  A function of the
    global row space only, so a month's chunks (and sums) do not depend on the sharding."""
    so = np.asarray(seg_off_h, dtype=np.int64)
    T = len(so) - 1
    total = int(so[-1])
    R = int(rows_per_wg)
    first = (-int(row_origin)) % R
    blk = np.arange(first, total, R, dtype=np.int64)
    cuts = np.unique(np.concatenate([so, blk[blk > 0]]))
    starts, ends = cuts[:-1], cuts[1:]
    seg_of = np.searchsorted(so, starts, side="right") - 1
    # empty months keep one empty chunk (fm_solve then sums nothing for them)
    empty = np.nonzero(np.diff(so) == 0)[0]
    if len(empty):
        starts = np.concatenate([starts, so[empty]])
        ends = np.concatenate([ends, so[empty]])
        seg_of = np.concatenate([seg_of, empty])
        order = np.lexsort((seg_of, starts))   # by row, then month (an empty month before the next)
        starts, ends, seg_of = starts[order], ends[order], seg_of[order]
    seg = seg_of.astype(np.int32)
    rows = np.stack([starts, ends], axis=1).reshape(-1).astype(np.int64)
    off = np.zeros(T + 1, dtype=np.int32)
    np.cumsum(np.bincount(seg, minlength=T), out=off[1:])
    blk_of = (int(row_origin) + starts) // R
    brk = np.nonzero(np.diff(blk_of))[0] + 1
    wg_off = np.concatenate([[0], brk, [len(seg)]]).astype(np.int32)
    return seg, rows, off, wg_off


def split_policy(nseg):
    """Whether the Gram takes the split-month plan (make_chunks_split) by default.  A grid of
    whole months that is a few rounds of the chip's resident workgroup slots leaves the CUs
    unevenly loaded (600 months cost as much as 768: profiles/r04/v1_size_scan.log), but the
    3/4 + 1/4 split with the big chunks launched first measured -2 us on the Gram and +2 us on
    the solve at the bench's 600 months (profiles/r04/v3_split_scan.log: -10 us at 512
    months, +5 us at 768), so it is off; callers opt in with panel.chunk_split = True.
    Callers that shard months pass the GLOBAL month count, like default_chunk_rows, so every
    rank plans (and sums) identically."""
    return False


def make_chunks_split(seg_off_h, num=3, den=4, min_rows=256):
    """Every month of >= min_rows rows as two chunks, rows [0, L*num/den) and the rest (a
    function of the month's own length only, so sharding does not change its sums), else one.
    Returns (seg, rows, off, order): the chunk arrays in month order (fm_solve sums a month's
    chunks from seg_chunk_off) and the launch order for fm_gram's chunk_order -- every big
    chunk first (last month first), then the small ones, which fill the slots the big ones
    leave (longest-first scheduling evens the per-CU load)."""
    T = len(seg_off_h) - 1
    lens = np.diff(seg_off_h).astype(np.int64)
    two = lens >= min_rows
    nch = np.where(two, 2, 1).astype(np.int64)
    off = np.zeros(T + 1, dtype=np.int32)
    np.cumsum(nch, out=off[1:])
    n = int(off[-1])
    seg = np.repeat(np.arange(T, dtype=np.int32), nch)
    rows = np.empty((n, 2), dtype=np.int64)
    first = off[:-1].astype(np.int64)
    cut = seg_off_h[:-1] + (lens * num) // den
    rows[first, 0] = seg_off_h[:-1]
    rows[first, 1] = np.where(two, cut, seg_off_h[1:])
    sec = first[two] + 1
    rows[sec, 0] = cut[two]
    rows[sec, 1] = seg_off_h[1:][two]
    order = np.concatenate([first[::-1], sec[::-1]]).astype(np.int32)
    return seg, rows.reshape(-1), off, order


def make_chunks(seg_off_h, chunk_rows):
    """Split every month into ceil(L / chunk_rows) near-equal chunks (depends only on the
    month's own length, so per-month arithmetic is independent of sharding)."""
    T = len(seg_off_h) - 1
    lens = np.diff(seg_off_h).astype(np.int64)
    nch = np.maximum(1, -(-lens // chunk_rows)).astype(np.int64)
    seg = np.repeat(np.arange(T, dtype=np.int32), nch)
    k = np.arange(len(seg)) - np.repeat(np.cumsum(nch) - nch, nch)
    L = lens[seg]
    n = nch[seg]
    r0 = seg_off_h[seg] + (k * L) // n
    r1 = seg_off_h[seg] + ((k + 1) * L) // n
    rows = np.stack([r0, r1], axis=1).reshape(-1).astype(np.int64)
    off = np.zeros(T + 1, dtype=np.int32)
    np.cumsum(nch, out=off[1:])
    return seg, rows, off


@dataclass
class _Plan:
    chunk_seg: torch.Tensor
    chunk_row: torch.Tensor
    seg_chunk_off: torch.Tensor
    nchunks: int
    order: Optional[torch.Tensor] = None   # fm_gram launch order (split plan) or None
    wg_off: Optional[torch.Tensor] = None  # balanced plan: each workgroup's chunk range
    nwg: int = 0


def _chunk_plan(panel: DevicePanel):
    cache = getattr(panel, "_chunk_cache", None)
    if cache is not None:
        return cache
    pol = panel.chunk_policy
    if pol is None and panel.chunk_rows is not None:   # a sharded caller's global months policy
        pol = ("months", panel.chunk_rows)
    split = panel.chunk_split
    if split is None:
        split = pol is None and split_policy(panel.nseg)
    if pol is None and not split:
        pol = chunk_policy(panel.nrows, panel.nseg, panel.max_seg_len)
    order = wg = None
    if split:
        seg, rows, off, order = make_chunks_split(panel.seg_off_h)
    elif pol[0] == "balanced":
        seg, rows, off, wg = make_chunks_balanced(panel.seg_off_h, pol[1], panel.row_origin)
    else:
        seg, rows, off = make_chunks(panel.seg_off_h, pol[1])
    dev = panel.device
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    plan = _Plan(t(seg), t(rows), t(off), len(seg), t(order), t(wg), 0 if wg is None else len(wg) - 1)
    panel._chunk_cache = plan
    return plan


@dataclass
class _GroupPlan:
    """Device-resident description of one model group (built once per model set)."""
    nmodels: int
    npatterns: int
    nprob: int
    mm: torch.Tensor     # [nmodels] column masks
    ym: torch.Tensor     # [nmodels] y-column bit
    lut: torch.Tensor    # [1<<nmodels] validity pattern -> pattern index
    patm: torch.Tensor   # [npatterns] model set of each pattern
    pm: torch.Tensor     # [nprob] group-local model of each problem
    pl: torch.Tensor     # [nprob] universe level
    pf: torch.Tensor     # [nprob] const-check flag
    pz: torch.Tensor     # [nprob, 32] z columns (0 = intercept, 1+c = panel column c)
    pnz: torch.Tensor    # [nprob]
    idx: torch.Tensor    # [nprob] global problem index


def _group_plans(panel, models, problems, nlevels, cap, const_check, dev):
    key = (tuple((m.y, tuple(m.xs), tuple(m.levels), bool(m.const_check)) for m in models),
           nlevels, cap, bool(const_check), str(dev))
    cache = panel.__dict__.setdefault("_group_cache", {})
    if key in cache:
        return cache[key]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    plans = []
    for g in group_models(models, nlevels, cap):
        gm = [models[i] for i in g]
        lut, pats = plan_patterns(gm)
        gp = [(k, p) for k, p in enumerate(problems) if p.model in g]
        local = {mi: j for j, mi in enumerate(g)}
        pz = np.zeros((len(gp), 32), dtype=np.int32)
        pnz = np.zeros(len(gp), dtype=np.int32)
        for j, (_, p) in enumerate(gp):
            m = models[p.model]
            z = [0] + [1 + x for x in m.xs] + [1 + m.y]
            pz[j, :len(z)] = z
            pnz[j] = len(z)
        plans.append(_GroupPlan(
            nmodels=len(gm), npatterns=len(pats), nprob=len(gp),
            mm=t(np.array([m.mask for m in gm], dtype=np.int64).astype(np.int32)),
            ym=t(np.array([1 << m.y for m in gm], dtype=np.int32)),
            lut=t(lut),
            patm=t(np.array(pats, dtype=np.int64).astype(np.uint32).view(np.int32)),
            pm=t(np.array([local[p.model] for _, p in gp], dtype=np.int32)),
            pl=t(np.array([p.level for _, p in gp], dtype=np.int32)),
            pf=t(np.array([1 if (models[p.model].const_check and const_check) else 0 for _, p in gp],
                          dtype=np.int32)),
            pz=t(pz), pnz=t(pnz),
            idx=t(np.array([k for k, _ in gp], dtype=np.int64))))
    cache[key] = plans
    return plans


def solve_fix_inline(zw, pmax):
    """True where fm_solve does the statsmodels fix-ups inside its own launch (the 16-wide solve of
    at most 15 columns); elsewhere fm_solve_fixup follows it."""
    return zw == 16 and pmax + 1 <= 16


def _solve_group(panel, src, gpl, partial, seg_chunk_off, zw, nlevels, T, pmax, mom_stride, lo, hi,
                 shift, inv_scale, add_back, level, const_check, keep):
    """fm_solve + the statsmodels fix-ups (inf in y, nonzero constant columns) for one
    model group; returns (rec, status, moments) [T, ng, ...]."""
    dev = src.device
    ng = gpl.nprob
    rs = pmax + 2
    grec = torch.empty((T, ng, rs), dtype=torch.float64, device=dev)
    gst = torch.empty((T, ng), dtype=torch.int32, device=dev)   # the solve writes every entry
    # centered moments are always produced: the inf-in-y fix reads them
    gmom = torch.empty((T, ng, mom_stride), dtype=torch.float64, device=dev)
    sa = L.SolveArgs(
        partial=partial.data_ptr(), seg_chunk_off=seg_chunk_off.data_ptr(), nseg=T, zw=zw,
        nlevels=nlevels, npatterns=gpl.npatterns, pattern_models=gpl.patm.data_ptr(), nprob=ng,
        prob_model=gpl.pm.data_ptr(), prob_level=gpl.pl.data_ptr(), prob_z=gpl.pz.data_ptr(),
        prob_nz=gpl.pnz.data_ptr(), prob_flags=gpl.pf.data_ptr(), add_back=_ptr(add_back),
        gram_flags=None, nmodels=gpl.nmodels, pmax=pmax, rec=grec.data_ptr(),
        status=gst.data_ptr(), moments=_ptr(gmom), mom_stride=mom_stride, ab_ncols=src.ncols)
    # statsmodels fix-ups: the exact nonzero-constant test where the solve saw a near-zero
    # variance (CONST_SUSPECT), inf in y (pinv(X) @ y gives +-inf / NaN coefficients) and the
    # QR + SVD refit of ill-conditioned / rank-deficient problems (FM_ST_REFIT).  The 16-wide
    # solve does them inside its own launch (each month's workgroup, right after its solve);
    # the 32-wide one is followed by fm_solve_fixup, which scans the status on the device: no
    # host round trip either way.  Both read the fix_* fields of the one struct.
    inline_fix = solve_fix_inline(zw, pmax)
    if not inline_fix and src.f64 is None:   # fm_solve_fixup reads FP64 columns
        src = _source(panel, panel.values())

    def set_fix():
        # the fix-ups' rows: the FP64 columns, else the planes of a planes-only panel
        sa.fix_cols, sa.fix_stride, sa.fix_seg_off = src.ptr, src.stride, panel.seg_off.data_ptr()
        if src.f64 is None:
            sa.fix_hi_plane, sa.fix_lo_plane = src.hp, src.lp
        sa.fix_lo, sa.fix_hi, sa.fix_shift, sa.fix_inv_scale = _ptr(lo), _ptr(hi), _ptr(shift), _ptr(inv_scale)
        sa.fix_level, sa.fix_check_const = _ptr(level), int(bool(const_check))

    if inline_fix:
        set_fix()
    _kcall("fm_solve", "fm_solve", L.C.byref(sa), _stream())
    # (a copy: the struct as this launch saw it, whatever fm_solve_fixup gets set below)
    _remember("fm_solve", "fm_solve", L.SolveArgs.from_buffer_copy(sa), partial, seg_chunk_off, gpl, add_back,
              grec, gst, gmom, src.f64, panel.planes, lo, hi, shift, inv_scale, level, *keep)
    if not inline_fix:
        set_fix()
        _kcall("fm_solve_fixup", "fm_solve_fixup", L.C.byref(sa), _stream())
    return grec, gst, gmom


def _problems(models, nlevels):
    problems = []
    for mi, m in enumerate(models):
        for u in m.levels:
            if u >= nlevels:
                raise ValueError("model level beyond the universe levels provided")
            problems.append(Problem(mi, u, len(m.xs)))
    return problems


@dataclass
class GramGroup:
    """One model group's Gram launch: its plan, the chunk plan it ran under and what it wrote."""
    group: _GroupPlan
    plan: _Plan
    partial: torch.Tensor   # [nchunks, nb, zw*(zw+1)/2], nb = group.npatterns * nlevels
    flags: torch.Tensor     # [T, nmodels] int32, reserved: never read
    zw: int


def gram_partials(panel: DevicePanel, models: Sequence[Model], level=None, nlevels=1, cuts: Cuts = None,
                  shift=None, inv_scale=None, cols=None, const_check=True, partial_out=None, problems=None):
    """The Gram half of fm_pass: one fm_gram launch per model group, under the panel's chunk plan.
    Returns a GramGroup per model group.  ``partial[chunk, pattern * nlevels + level]`` is the packed
    upper triangle (entry (i, j >= i) at i*zw - i*(i-1)/2 + (j-i)) of Z'Z over the chunk's rows of
    that validity pattern and universe level, z = [1, (clip(x) - shift) * inv_scale ...]; a bucket
    without rows is stored as zeros (fm_solve sums every image).  ``shift`` / ``inv_scale`` None:
    0 / 1 (fm_pass passes its pivot).  ``partial_out``: the caller's own contiguous FP64 buffer
    [nchunks, nb, PK] to write into (a list of them, one per group, when there are several)."""
    src = _source(panel, cols)
    ncols = src.ncols
    if ncols > L.FM_MAX_COLS:
        raise ValueError(f"at most {L.FM_MAX_COLS} columns per pass")
    dev = src.device
    T = panel.nseg
    zw = 16 if ncols <= 15 else 32
    cap = 16 if zw == 16 else 8
    if problems is None:
        problems = _problems(models, nlevels)
    plan = _chunk_plan(panel)
    lo = cuts.lo if cuts is not None else None
    hi = cuts.hi if cuts is not None else None
    groups = _group_plans(panel, models, problems, nlevels, cap, const_check, dev)
    if partial_out is not None and not isinstance(partial_out, (list, tuple)):
        partial_out = [partial_out]
    if partial_out is not None and len(partial_out) != len(groups):
        raise ValueError(f"partial_out: {len(groups)} model groups need as many buffers")
    out = []
    for k, gpl in enumerate(groups):
        nb = gpl.npatterns * nlevels
        shape = (plan.nchunks, nb, zw * (zw + 1) // 2)
        if partial_out is None:
            partial = torch.empty(shape, dtype=torch.float64, device=dev)
        else:
            partial = partial_out[k]
            if tuple(partial.shape) != shape or partial.dtype != torch.float64 or \
                    not partial.is_contiguous() or partial.device != dev:
                raise ValueError(f"partial_out: group {k} needs a contiguous float64 {shape} tensor on {dev}")
        flags = torch.empty((T, gpl.nmodels), dtype=torch.int32, device=dev)   # reserved: never read
        ga = L.GramArgs(
            cols=src.ptr, col_stride=src.stride if src.f64 is not None else 0, ncols=ncols, nseg=T,
            seg_off=panel.seg_off.data_ptr(), chunk_seg=plan.chunk_seg.data_ptr(),
            chunk_row=plan.chunk_row.data_ptr(), nchunks=plan.nchunks,
            lo=_ptr(lo), hi=_ptr(hi), shift=_ptr(shift), inv_scale=_ptr(inv_scale),
            level=_ptr(level), nlevels=nlevels, model_mask=gpl.mm.data_ptr(),
            model_ymask=gpl.ym.data_ptr(), nmodels=gpl.nmodels, pattern_id=gpl.lut.data_ptr(),
            npatterns=gpl.npatterns, partial=partial.data_ptr(), flags=flags.data_ptr(),
            chunk_order=_ptr(plan.order), hi_plane=src.hp, lo_plane=src.lp, plane_stride=src.pstride,
            wg_chunk_off=_ptr(plan.wg_off), nwg=plan.nwg)
        _kcall("fm_gram", "fm_gram", L.C.byref(ga), _stream())
        _remember("fm_gram", "fm_gram", ga, src.f64, panel.planes, partial, flags, lo, hi, shift, inv_scale, level,
                  plan, gpl)
        out.append(GramGroup(gpl, plan, partial, flags, zw))
    return out


def fm_pass(panel: DevicePanel, models: Sequence[Model], level=None, nlevels=1, cuts: Cuts = None,
            shift=None, inv_scale=None, add_back=None, moments=False, cols=None, const_check=True):
    """One batched cross-sectional pass: every (model, universe level) problem for every
    month from one read of the panel per model group.  Returns an FMResult."""
    src = _source(panel, cols)
    dev = src.device
    T = panel.nseg
    if src.ncols > L.FM_MAX_COLS:
        raise ValueError(f"at most {L.FM_MAX_COLS} columns per pass")
    if shift is None:
        shift = pilot_shift(panel, cols)
    if add_back is None and inv_scale is None:
        add_back = shift
    problems = _problems(models, nlevels)
    pmax = max(2, max(p.K + 1 for p in problems))
    nprob = len(problems)
    rs = pmax + 2
    mom_stride = 1 + (pmax + 1) + (pmax + 1) ** 2
    rec = torch.empty((T, nprob, rs), dtype=torch.float64, device=dev)
    status = torch.empty((T, nprob), dtype=torch.int32, device=dev)   # every problem is in one group
    mom = torch.empty((T, nprob, mom_stride), dtype=torch.float64, device=dev) if moments else None
    lo = cuts.lo if cuts is not None else None
    hi = cuts.hi if cuts is not None else None
    grams = gram_partials(panel, models, level, nlevels, cuts, shift, inv_scale, cols, const_check,
                          problems=problems)
    for g in grams:
        gpl, plan = g.group, g.plan
        grec, gst, gmom = _solve_group(panel, src, gpl, g.partial, plan.seg_chunk_off, g.zw, nlevels, T, pmax,
                                       mom_stride, lo, hi, shift, inv_scale, add_back, level,
                                       const_check, (src.f64, panel.planes, g.flags, lo, hi, shift, inv_scale,
                                                     level, plan))
        if len(grams) == 1:
            rec, status = grec, gst
            mom = gmom if moments else None
        else:
            rec.index_copy_(1, gpl.idx, grec)
            status.index_copy_(1, gpl.idx, gst)
            if moments:
                mom.index_copy_(1, gpl.idx, gmom)
    return FMResult(problems=problems, rec=rec, status=status, pmax=pmax, moments=mom,
                    mom_stride=mom_stride)


def wls_weight(panel: DevicePanel, weight):
    """The [rows] FP64 weight vector ``fm_pass_wls`` reads: None or "me" the panel's market equity,
    another string a panel column by name, anything else a float64 [rows] tensor on the panel's device."""
    if weight is None or (isinstance(weight, str) and weight == "me"):
        if panel.me is None:
            raise ValueError("fm_pass_wls: the panel has no market equity (me) to weight by")
        return panel.me
    if isinstance(weight, str):
        if weight not in panel.names:
            raise ValueError(f"fm_pass_wls: the panel has no column {weight!r} to weight by")
        return column_vector(panel, weight)
    return _row_vector("fm_pass_wls", weight, torch.float64, panel.nrows, panel.device, "weight")


def _wls_tables(panel, models, problems, dev):
    """The problem tables fm_wls reads (fm_solve's prob_level / prob_z / prob_nz), made once per
    model set and kept with the panel."""
    key = (tuple((m.y, tuple(m.xs)) for m in models), tuple((p.model, p.level) for p in problems), str(dev))
    cache = panel.__dict__.setdefault("_wls_cache", {})
    if key not in cache:
        pz = np.zeros((len(problems), 32), dtype=np.int32)
        pnz = np.zeros(len(problems), dtype=np.int32)
        for j, p in enumerate(problems):
            m = models[p.model]
            z = [0] + [1 + x for x in m.xs] + [1 + m.y]
            pz[j, :len(z)] = z
            pnz[j] = len(z)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        cache[key] = (t(np.array([p.level for p in problems], dtype=np.int32)), t(pz), t(pnz))
    return cache[key]


def fm_pass_wls(panel: DevicePanel, models: Sequence[Model], weight=None, level=None, nlevels=1, cuts: Cuts = None,
                shift=None, moments=False):
    """The weighted counterpart of fm_pass (A22, fm_wls): per month and (model, universe level)
    problem the weighted least-squares fit of y on [1, x], the weights ``weight`` (see wls_weight;
    usually market equity), in one launch.  Rows of NaN, +-inf, zero or negative weight are dropped.
    Returns an FMResult laid out as fm_pass lays it out, so every later stage runs on it unchanged.
    FP64 columns, at most 15 of them; ``shift`` [C, T] is only the pivot of the kernel's first pass."""
    if panel.cols is None:
        raise ValueError("fm_pass_wls: a planes-only panel is not supported (fm_wls reads FP64 columns)")
    src = panel.cols
    dev = src.device
    T = panel.nseg
    if src.shape[0] > L.FM_WLS_MAX_COLS:
        raise ValueError(f"fm_pass_wls: at most {L.FM_WLS_MAX_COLS} columns per pass")
    wv = wls_weight(panel, weight)
    problems = _problems(models, nlevels)
    pmax = max(2, max(p.K + 1 for p in problems))
    nprob = len(problems)
    mom_stride = 1 + (pmax + 1) + (pmax + 1) ** 2
    rec = torch.empty((T, nprob, pmax + 2), dtype=torch.float64, device=dev)
    status = torch.empty((T, nprob), dtype=torch.int32, device=dev)   # the kernel writes every entry
    mom = torch.empty((T, nprob, mom_stride), dtype=torch.float64, device=dev) if moments else None
    lo = cuts.lo if cuts is not None else None
    hi = cuts.hi if cuts is not None else None
    pl, pz, pnz = _wls_tables(panel, models, problems, dev)
    wa = L.WlsArgs(
        cols=src.data_ptr(), col_stride=src.stride(0), nrows=panel.nrows, ncols=src.shape[0], nseg=T,
        seg_off=panel.seg_off.data_ptr(), lo=_ptr(lo), hi=_ptr(hi), shift=_ptr(shift), level=_ptr(level),
        weight=wv.data_ptr(), nprob=nprob, pmax=pmax, prob_level=pl.data_ptr(), prob_z=pz.data_ptr(),
        prob_nz=pnz.data_ptr(), rec=rec.data_ptr(), status=status.data_ptr(), moments=_ptr(mom),
        mom_stride=mom_stride)
    _kcall("fm_wls", "fm_wls", L.C.byref(wa), _stream())
    _remember("fm_wls", "fm_wls", wa, src, wv, lo, hi, shift, level, pl, pz, pnz, rec, status, mom)
    return FMResult(problems=problems, rec=rec, status=status, pmax=pmax, moments=mom, mom_stride=mom_stride)


def firm_codes(panel: DevicePanel):
    """Dense firm codes of the panel's rows: (int32 [rows] tensor, nfirms), code = the rank of the
    row's ``panel.ids`` among the panel's distinct ids, so the codes ascend inside a month where the
    ids do.  Made once and kept with the panel."""
    if panel.ids is None:
        raise ValueError("firm_codes: the panel has no firm ids (DevicePanel.ids)")
    cache = panel.__dict__.get("_firm_codes")
    if cache is None:
        uniq, inv = torch.unique(panel.ids, return_inverse=True)
        cache = (inv.to(torch.int32).contiguous(), int(uniq.numel()))
        panel.__dict__["_firm_codes"] = cache
    return cache


@dataclass
class PooledResult:
    problems: List[Problem]
    coef: torch.Tensor            # [nprob, pmax]: a, b_1 .. b_K, NaN pad (a is NaN under month FE)
    se: torch.Tensor              # [nprob, 5, pmax]: classical, White, month, firm, two-way
    cov: Optional[torch.Tensor]   # [nprob, 5, pmax, pmax]
    stat: torch.Tensor            # [nprob, 8]: N, G_t, G_f, R2, SSR, s2, classical dof, 0
    status: torch.Tensor          # [nprob] int32 (FM_ST_* bits)
    resid: Optional[torch.Tensor]   # [nprob, rows], NaN on unused rows
    pmax: int

    @property
    def nprob(self):
        return len(self.problems)

    def tstat(self, kind="twoway"):
        """coef / se of one covariance kind ("classical", "white", "month", "firm", "twoway" or 0..4)."""
        k = L.FM_POOL_SE_NAMES.index(kind) if isinstance(kind, str) else int(kind)
        return self.coef / self.se[:, k, :]


_POOL_WS = {}   # device -> the fm_pool workspace (grown on demand; every call rewrites what it reads)


def pooled_regressions(panel: DevicePanel, models: Sequence[Model], level=None, nlevels=1, cuts: Cuts = None,
                       month_fe=False, small_sample=True, seg_lo=0, seg_hi=None, cov=False, resid=False, shift=None,
                       firm=None):
    """Pooled panel OLS of every (model, universe level) problem over the months [seg_lo, seg_hi)
    with classical, White, month-clustered, firm-clustered and two-way clustered standard errors
    (A23, fm_pool), with or without month fixed effects.  Models of at most 15 regressors; the panel
    may have any number of FP64 columns.  ``firm``: (int32 [rows] codes, nfirms) in place of
    firm_codes(panel).  Raises ValueError when the firm codes do not ascend inside every month."""
    if panel.cols is None:
        raise ValueError("pooled_regressions: a planes-only panel is not supported (fm_pool reads FP64 columns)")
    src = panel.cols
    dev = src.device
    T = panel.nseg
    seg_hi = T if seg_hi is None else int(seg_hi)
    codes, nfirms = firm_codes(panel) if firm is None else firm
    codes = _row_vector("pooled_regressions", codes, torch.int32, panel.nrows, dev, "firm")
    problems = _problems(models, nlevels)
    if any(p.K > L.FM_POOL_MAX_K for p in problems):
        raise ValueError(f"pooled_regressions: at most {L.FM_POOL_MAX_K} regressors per model")
    pmax = max(2, max(p.K + 1 for p in problems))
    nprob = len(problems)
    nan = float("nan")
    coef = torch.full((nprob, pmax), nan, dtype=torch.float64, device=dev)
    se = torch.full((nprob, 5, pmax), nan, dtype=torch.float64, device=dev)
    cv = torch.full((nprob, 5, pmax, pmax), nan, dtype=torch.float64, device=dev) if cov else None
    stat = torch.zeros((nprob, 8), dtype=torch.float64, device=dev)
    status = torch.full((nprob,), L.FM_ST_SKIPPED, dtype=torch.int32, device=dev)   # an empty call fits nothing
    rs = torch.full((nprob, panel.nrows), nan, dtype=torch.float64, device=dev) if resid else None
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(L.load().fm_pool_ws_bytes(T, nprob, pmax, int(nfirms)))
    if need < 0:
        raise ValueError("fm_pool_ws_bytes: bad sizes")
    ws = _POOL_WS.get(str(dev))
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        _POOL_WS[str(dev)] = ws
    lo = cuts.lo if cuts is not None else None
    hi = cuts.hi if cuts is not None else None
    pl, pz, pnz = _wls_tables(panel, models, problems, dev)
    pa = L.PoolArgs(
        cols=src.data_ptr(), col_stride=src.stride(0), nrows=panel.nrows, ncols=src.shape[0], nseg=T,
        seg_off=panel.seg_off.data_ptr(), lo=_ptr(lo), hi=_ptr(hi), shift=_ptr(shift), level=_ptr(level),
        firm=codes.data_ptr(), nfirms=int(nfirms), seg_lo=int(seg_lo), seg_hi=seg_hi, month_fe=int(bool(month_fe)),
        small_sample=int(bool(small_sample)), nprob=nprob, pmax=pmax, prob_level=pl.data_ptr(), prob_z=pz.data_ptr(),
        prob_nz=pnz.data_ptr(), coef=coef.data_ptr(), se=se.data_ptr(), cov=_ptr(cv), stat=stat.data_ptr(),
        status=status.data_ptr(), resid=_ptr(rs), bad=bad.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
    _kcall("fm_pool", "fm_pool", L.C.byref(pa), _stream())
    _remember("fm_pool", "fm_pool", pa, src, lo, hi, shift, level, codes, pl, pz, pnz, coef, se, cv, stat, status, rs,
              bad, ws)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"pooled_regressions: {nbad} rows have a firm code outside 0..{int(nfirms) - 1} or not above "
                         "the previous row's in their month (rows must be sorted by (month, firm))")
    return PooledResult(problems=problems, coef=coef, se=se, cov=cv, stat=stat, status=status, resid=rs, pmax=pmax)


def drop_degenerate_months(res: FMResult, models: Sequence[Model], sd):
    """Standardized passes (A9): a month in which a regressor has fewer than two values or
    zero dispersion has an all-NaN z-score column, so every row drops out and the month is
    not fitted for the models using it; clear FM_ST_FITTED there.  ``sd`` [C, T]."""
    bad = ~(sd > 0)                                              # NaN sd -> True
    C = sd.shape[0]
    use = np.zeros((res.nprob, C), dtype=np.float64)
    for k, p in enumerate(res.problems):
        use[k, models[p.model].xs] = 1.0
    hit = _small_tensor(tuple(map(tuple, use)), torch.float64, sd.device) @ bad.to(torch.float64)
    res.status &= ~((hit.t() > 0).to(torch.int32) * L.FM_ST_FITTED)
    return res


# ------------------------------------------------------------------------------------------
# Time-series stage
# ------------------------------------------------------------------------------------------
@dataclass
class TSIndex:
    idx: torch.Tensor     # [nprob, T] int32: fitted months in order
    count: torch.Tensor   # [nprob] int32


def ts_compact(status, s_seg, s_prob, nseg, nprob):
    dev = status.device
    idx = torch.empty((nprob, nseg), dtype=torch.int32, device=dev)
    cnt = torch.empty(nprob, dtype=torch.int32, device=dev)
    _kcall("fm_ts_compact", "fm_ts_compact", status.data_ptr(), s_seg, s_prob, nseg, nprob, idx.data_ptr(),
           cnt.data_ptr(), _stream())
    return TSIndex(idx, cnt)


def compact_result(res: FMResult):
    T, P = res.status.shape
    return ts_compact(res.status, P, 1, T, P)


@dataclass
class Summary:
    mean: torch.Tensor   # [nprob, kmax]
    se: torch.Tensor
    tstat: torch.Tensor
    nobs: torch.Tensor


def _sum_outputs(nprob, kmax, dev, sum_range):
    """Summary output buffers; with a problem range (sharded runs) pre-filled with the -0.0 /
    0 that the SUM-combine across ranks needs for the problems this rank does not summarize."""
    if sum_range is None:
        mean = torch.empty((nprob, kmax), dtype=torch.float64, device=dev)
        se, ts = torch.empty_like(mean), torch.empty_like(mean)
        nobs = torch.empty((nprob, kmax), dtype=torch.int32, device=dev)
    else:
        mean = torch.full((nprob, kmax), -0.0, dtype=torch.float64, device=dev)
        se, ts = mean.clone(), mean.clone()
        nobs = torch.zeros((nprob, kmax), dtype=torch.int32, device=dev)
    return mean, se, ts, nobs


def ts_summary(rec, r_seg, r_prob, ix: TSIndex, nseg, nprob, kmax, nw_lags=4, sum_range=None):
    """FM means / NW standard errors of every (problem, coefficient).  ``sum_range`` = (p0, p1):
    problems [p0, p1) only (pointer offsets into the same buffers), -0.0 / 0 elsewhere."""
    dev = rec.device
    mean, se, ts, nobs = _sum_outputs(nprob, kmax, dev, sum_range)
    p0, p1 = (0, nprob) if sum_range is None else sum_range
    n = p1 - p0
    if n <= 0:
        return Summary(mean, se, ts, nobs)
    # the series [n][kmax][nseg] and the long-series chunk partials (fm_hip.h)
    work = torch.empty(n * kmax * (max(nseg, 1) + -(-nseg // 2048) * 28), dtype=torch.float64, device=dev)
    _kcall("fm_ts_summary", "fm_ts_summary", rec.data_ptr() + 8 * p0 * r_prob, r_seg, r_prob,
           ix.idx[p0].data_ptr(), ix.count[p0:].data_ptr(), nseg, n, kmax, nw_lags, mean[p0].data_ptr(),
           se[p0].data_ptr(), ts[p0].data_ptr(), nobs[p0].data_ptr(), work.data_ptr(), _stream())
    return Summary(mean, se, ts, nobs)


def summarize_result(res: FMResult, ix: TSIndex = None, nw_lags=4, sum_range=None):
    ix = ix or compact_result(res)
    T, P, rs = res.rec.shape
    return ts_summary(res.rec, P * rs, rs, ix, T, P, rs, nw_lags, sum_range), ix


def rolling_result(res: FMResult, ix: TSIndex, window=120, min_periods=60, own=None):
    """Rolling means [P, T, pmax] of the fitted-month series.  ``own`` = (seg_lo, seg_hi, lag)
    (sharded runs): only the rows a predictive stage of those months reads, the same bits
    (fm_rolling_mean_own); other rows are left unwritten."""
    T, P, rs = res.rec.shape
    out = torch.empty((P, T, res.pmax), dtype=torch.float64, device=res.rec.device)
    if own is None:
        _kcall("fm_rolling_mean", "fm_rolling_mean", res.rec.data_ptr(), P * rs, rs, ix.idx.data_ptr(),
               ix.count.data_ptr(), T, P, res.pmax, window, min_periods, out.data_ptr(), _stream())
    else:
        _kcall("fm_rolling_mean", "fm_rolling_mean_own", res.rec.data_ptr(), P * rs, rs, ix.idx.data_ptr(),
               ix.count.data_ptr(), T, P, res.pmax, window, min_periods, int(own[0]), int(own[1]), int(own[2]),
               out.data_ptr(), _stream())
    return out


_SMALL = {}


def _small_tensor(values, dtype, dev):
    """Cached device copy of a small constant list (no per-call host-to-device copy)."""
    key = (values, dtype, str(dev))
    t = _SMALL.get(key)
    if t is None:
        t = _SMALL[key] = torch.tensor(list(values), dtype=dtype, device=dev)
    return t


def predictive_result(res: FMResult, ix: TSIndex, roll, lag=1, seg_lo=0, seg_hi=None, moments=None):
    """A7/A8 per (problem, fitted-month row): slope, R2, N of y on the lagged-rolling
    forecast, from the month's centered moments.  In sharded runs ``res`` holds the
    gathered global records and ``moments`` the local months [seg_lo, seg_hi) only."""
    T, P, _ = res.rec.shape
    dev = res.rec.device
    mom = res.moments if moments is None else moments
    seg_hi = T if seg_hi is None else seg_hi
    pk = _small_tensor(tuple(p.K for p in res.problems), torch.int32, dev)
    pred = torch.empty((P, T, 4), dtype=torch.float64, device=dev)
    pst = torch.empty((P, T), dtype=torch.int32, device=dev)
    _kcall("fm_predictive", "fm_predictive", mom.data_ptr(), res.mom_stride, T, P, pk.data_ptr(),
           ix.idx.data_ptr(), ix.count.data_ptr(), roll.data_ptr(), res.pmax, lag, seg_lo, seg_hi,
           pred.data_ptr(), pst.data_ptr(), _stream())
    return pred, pst


def summarize_predictive(pred, pst, nw_lags=4, sum_range=None):
    """FM summary of the predictive records (slope, R^2, n).  ``sum_range`` (sharded runs):
    problems [p0, p1) only, -0.0 / 0 elsewhere (combined across ranks by a SUM)."""
    P, T, _ = pred.shape
    if not ts_fused_fits(T):
        p0, p1 = (0, P) if sum_range is None else sum_range
        ix = TSIndex(torch.empty((P, T), dtype=torch.int32, device=pred.device),
                     torch.zeros(P, dtype=torch.int32, device=pred.device))
        if p1 > p0:
            _kcall("fm_ts_compact", "fm_ts_compact", pst[p0].data_ptr(), 1, T, T, p1 - p0, ix.idx[p0].data_ptr(),
                   ix.count[p0:].data_ptr(), _stream())
        return ts_summary(pred, 4, T * 4, ix, T, P, 3, nw_lags, sum_range), ix
    ix, summ, _, _, _ = ts_fused(pred, 4, T * 4, pst, 1, T, T, P, 3, nw_lags, tag="fm_ts_fused[pred]",
                                 sum_range=sum_range)
    return summ, ix


def ts_fused_fits(nseg, pmax=0, window=None, lag=1, predictive=False):
    """Whether fm_ts_fused can stage this series in LDS (else the per-stage kernels run)."""
    need = L.load().fm_ts_fused_lds_bytes(nseg, pmax, window or 0, lag, int(window is not None),
                                           int(bool(predictive)))
    return need <= L.FM_TS_FUSED_MAX_LDS


def ts_fused(rec, r_seg, r_prob, status, s_seg, s_prob, nseg, nprob, kmax, nw_lags=4,
             window=None, min_periods=None, pmax=None, moments=None, mom_stride=0, prob_k=None,
             lag=1, seg_lo=0, seg_hi=None, predictive=False, tag="fm_ts_fused", sum_range=None,
             roll_own=False):
    """The whole time-series stage in one launch (fm_ts_fused): TSIndex, Summary and, when
    ``window`` is given, the rolling means [P, T, pmax]; with ``predictive`` also the
    predictive records [P, T, 4] and status [P, T].  Returns (ix, summ, roll, pred, pst).
    Sharded runs: ``sum_range`` = (p0, p1) summarizes problems [p0, p1) only (-0.0 / 0
    elsewhere), ``roll_own`` rolls only the rows the months [seg_lo, seg_hi) read."""
    dev = rec.device
    idx = torch.empty((nprob, nseg), dtype=torch.int32, device=dev)
    cnt = torch.empty(nprob, dtype=torch.int32, device=dev)
    mean = torch.empty((nprob, kmax), dtype=torch.float64, device=dev)
    se, ts = torch.empty_like(mean), torch.empty_like(mean)
    nobs = torch.empty((nprob, kmax), dtype=torch.int32, device=dev)
    roll = pred = pst = None
    if window is not None:
        roll = torch.empty((nprob, nseg, pmax), dtype=torch.float64, device=dev)
    if predictive:
        pred = torch.empty((nprob, nseg, 4), dtype=torch.float64, device=dev)
        pst = torch.empty((nprob, nseg), dtype=torch.int32, device=dev)
    # problem range of the summaries: (0, 0) = every problem; an empty range of a sharded rank
    # (more ranks than problems) = (nprob, nprob): the kernel then summarizes none
    sp_lo, sp_hi = 0, 0
    if sum_range is not None:
        sp_lo, sp_hi = int(sum_range[0]), int(sum_range[1])
        if sp_hi <= sp_lo:
            sp_lo = sp_hi = nprob
    ta = L.TsArgs(rec=rec.data_ptr(), r_seg=r_seg, r_prob=r_prob, status=status.data_ptr(), s_seg=s_seg,
                  s_prob=s_prob, nseg=nseg, nprob=nprob, kmax=kmax, nw_lags=nw_lags, idx=idx.data_ptr(),
                  count=cnt.data_ptr(), mean=mean.data_ptr(), se=se.data_ptr(), tstat=ts.data_ptr(),
                  nobs=nobs.data_ptr(), work=None, window=window or 0,
                  min_periods=min_periods or 0, pmax=pmax or 0, roll=_ptr(roll), moments=_ptr(moments),
                  mom_stride=mom_stride, prob_k=_ptr(prob_k), lag=lag, seg_lo=seg_lo,
                  seg_hi=nseg if seg_hi is None else seg_hi, pred=_ptr(pred), pred_status=_ptr(pst),
                  sum_p_lo=sp_lo, sum_p_hi=sp_hi, roll_own=int(bool(roll_own)))
    _kcall(tag, "fm_ts_fused", L.C.byref(ta), _stream())
    _remember(tag, "fm_ts_fused", ta, rec, status, idx, cnt, mean, se, ts, nobs, roll,
              moments, prob_k, pred, pst)
    return TSIndex(idx, cnt), Summary(mean, se, ts, nobs), roll, pred, pst


def time_series_result(res: FMResult, nw_lags=4, window=120, min_periods=60, lag=1, seg_lo=0,
                       seg_hi=None, moments=None, rolling=True, predictive=True, sum_range=None,
                       roll_own=False):
    """compact_result + summarize_result + rolling_result + predictive_result in one launch.
    Returns (ix, summ, roll, pred, pst).  Sharded runs (every rank on the gathered series):
    ``sum_range`` = this rank's problems for the FM summaries, ``roll_own`` = rolling means only
    where this rank's predictive records [seg_lo, seg_hi) read them."""
    T, P, rs = res.rec.shape
    mom = res.moments if moments is None else moments
    window = window if (rolling or predictive) else None
    if not ts_fused_fits(T, res.pmax, window, lag, predictive):
        ix = compact_result(res)
        summ, _ = summarize_result(res, ix, nw_lags, sum_range)
        roll = pred = pst = None
        if window is not None:
            own = None
            if roll_own:
                own = (seg_lo, T if seg_hi is None else seg_hi, lag if predictive else 0)
            roll = rolling_result(res, ix, window, min_periods, own)
        if predictive:
            pred, pst = predictive_result(res, ix, roll, lag, seg_lo, seg_hi, moments)
        return ix, summ, roll, pred, pst
    pk = _small_tensor(tuple(p.K for p in res.problems), torch.int32, res.rec.device) if predictive else None
    return ts_fused(res.rec, P * rs, rs, res.status, P, 1, T, P, rs, nw_lags,
                    window=window, min_periods=min_periods,
                    pmax=res.pmax, moments=mom if predictive else None, mom_stride=res.mom_stride,
                    prob_k=pk, lag=lag, seg_lo=seg_lo, seg_hi=seg_hi, predictive=predictive,
                    sum_range=sum_range, roll_own=roll_own)


def forecast(panel: DevicePanel, coef, cols=None):
    """A7 per-row forecasts F = c0[t] + sum_k c_k[t] x_k for coef [T, K+1] (NaN propagates)."""
    src = panel.values() if cols is None else cols
    coef = coef.contiguous()
    out = torch.empty(panel.nrows, dtype=torch.float64, device=src.device)
    _kcall("fm_forecast", "fm_forecast", src.data_ptr(), src.stride(0), src.shape[0], panel.seg_off.data_ptr(),
           panel.nseg, panel.nrows, coef.data_ptr(), coef.stride(0), out.data_ptr(), _stream())
    return out


PORT_MAX_ROWS = 16384   # fm_portfolio_sort's month limit (one workgroup per month, keys in LDS)


@dataclass
class Portfolios:
    bp: torch.Tensor       # [T, nport-1] float64 breakpoints (NaN: unsorted month)
    port: torch.Tensor     # [rows] uint8 portfolio 0..nport-1, 255 = none
    rec: torch.Tensor      # [T, nport+1, 4] float64: ew ret, ew forecast, vw ret, vw forecast; last = H-L
    cnt: torch.Tensor      # [T, nport] int32 rows with a finite return
    status: torch.Tensor   # [T] int32: 1 = sorted month
    forecast: Optional[torch.Tensor] = None   # [nsel, rows] float64 (forecast_portfolio_sort, on request)
    # forecast_portfolio_sort returns every tensor with a leading [nsel] dimension


def _row_vector(who, t, dtype, n, dev, what, required=False):
    """Argument ``what`` of ``who``, a ``dtype`` [n] tensor on ``dev`` (``n`` a tuple: of that shape),
    made contiguous; None passes through unless ``required``."""
    if t is None and not required:
        return None
    sh = tuple(n) if isinstance(n, tuple) else (n,)
    if t is None or t.dtype != dtype or tuple(t.shape) != sh or t.device != dev:
        raise ValueError(f"{who}: {what} must be a {dtype} {list(sh)} tensor on {dev}")
    return t.contiguous()


def _months(who, seg_off, dev, what):
    """The month offsets every row-vector entry point takes -> (seg_off contiguous, T); ``what``: whose
    device ``dev`` is, for the message ("forecast's", "returns'", ...)."""
    if seg_off.dtype != torch.int64 or seg_off.dim() != 1 or seg_off.shape[0] < 1 or seg_off.device != dev:
        raise ValueError(f"{who}: seg_off must be an int64 [T+1] tensor on the {what} device")
    return seg_off.contiguous(), int(seg_off.shape[0]) - 1


def _longest_month(seg_off, T, max_seg_len):
    """``max_seg_len`` if the caller knows it, else read from ``seg_off`` (one host sync)."""
    if max_seg_len is not None:
        return int(max_seg_len)
    return int((seg_off[1:] - seg_off[:-1]).max().item()) if T > 0 else 0


def _outputs(who, cls, shapes, out, dev):
    """The result dataclass ``cls`` of ``who`` with the tensors ``shapes`` = {field: (shape, dtype)}:
    allocated on ``dev``, or the caller's ``out`` checked tensor by tensor."""
    if out is None:
        return cls(**{k: torch.empty(sh, dtype=dt, device=dev) for k, (sh, dt) in shapes.items()})
    for k, (sh, dt) in shapes.items():
        t = getattr(out, k)
        if t is None or tuple(t.shape) != sh or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{who}: out.{k} must be a contiguous {dt} {list(sh)} tensor on {dev}")
    return out


def _new_or_filled(empty, shape, dtype, fill, dev):
    """An output a launch will write; an ``empty`` call launches nothing, so its outputs are then
    filled with what a launch would have written."""
    if empty:
        return torch.full(shape, fill, dtype=dtype, device=dev)
    return torch.empty(shape, dtype=dtype, device=dev)


def _rec_summary(rec, status, nw_lags):
    """FM mean, Newey-West s.e., t and nobs of the monthly series of ``rec`` [S, T, ...] over the months
    with ``status`` [S, T] 1, NaN entries dropped per series: every leading index is one problem of
    two launches -> ``Summary`` with [S, k] tensors, k the series per problem."""
    S, T = int(rec.shape[0]), int(rec.shape[1])
    k = int(np.prod(rec.shape[2:], dtype=np.int64))
    ix = ts_compact(status, 1, T, T, S)
    return ts_summary(rec, k, T * k, ix, T, S, k, nw_lags)


def _sort_plan(who, lead, T, n, nport, q, nyse_breakpoints, min_count):
    """What the two portfolio sorts share: ``fill(a)`` sets an argument struct's ``nport``, ``q`` (default
    k / nport), ``nyse_breakpoints`` and ``min_count`` (default nport) and returns it; ``shapes``: the
    ``Portfolios`` tensors' (shape, dtype) under the leading dimensions ``lead``."""
    qs = list(q) if q is not None else [k / nport for k in range(1, max(nport, 1))]
    if q is not None and len(qs) != nport - 1:
        raise ValueError(f"{who}: q must hold nport - 1 = {nport - 1} levels, got {len(qs)}")

    def fill(a):
        a.nport, a.nyse_breakpoints = nport, int(bool(nyse_breakpoints))
        a.min_count = nport if min_count is None else int(min_count)
        for j, v in enumerate(qs[:L.FM_MAX_PORTS - 1]):
            a.q[j] = float(v)
        return a

    np_ = min(max(nport, 2), L.FM_MAX_PORTS)   # output shapes of a call the library will refuse
    shapes = dict(bp=(lead + (T, np_ - 1), torch.float64), port=(lead + (n,), torch.uint8),
                  rec=(lead + (T, np_ + 1, 4), torch.float64), cnt=(lead + (T, np_), torch.int32),
                  status=(lead + (T,), torch.int32))
    return fill, shapes


def portfolio_sort(seg_off, forecast, ret, weight=None, level=None, nyse=None, nport=10, q=None,
                   min_level=0, nyse_breakpoints=False, min_count=None, max_seg_len=None):
    """A12: per month (``seg_off`` int64 [T+1] device, rows sorted by month) sort the rows into
    ``nport`` portfolios by ``forecast`` and average each portfolio's ``ret`` and forecast,
    equal- and ``weight``-weighted, plus the high-minus-low spread (fm_portfolio_sort; the
    definition is in fm_hip.h).  Plain device tensors in, ``Portfolios`` of device tensors out.
    ``q``: the nport-1 breakpoint levels (default k / nport); ``max_seg_len``: the longest
    month if the caller knows it (otherwise read from ``seg_off``, one host sync)."""
    dev = forecast.device
    n = int(forecast.shape[0])
    who = "portfolio_sort"
    seg_off, T = _months(who, seg_off, dev, "forecast's")
    forecast = _row_vector(who, forecast, torch.float64, n, dev, "forecast")
    ret = _row_vector(who, ret, torch.float64, n, dev, "ret")
    weight = _row_vector(who, weight, torch.float64, n, dev, "weight")
    level = _row_vector(who, level, torch.uint8, n, dev, "level")
    nyse = _row_vector(who, nyse, torch.uint8, n, dev, "nyse")
    fill, shapes = _sort_plan(who, (), T, n, int(nport), q, nyse_breakpoints, min_count)
    max_seg_len = _longest_month(seg_off, T, max_seg_len)
    a = fill(L.PortArgs())
    a.forecast, a.ret, a.weight, a.level, a.nyse = _ptr(forecast), _ptr(ret), _ptr(weight), _ptr(level), _ptr(nyse)
    a.seg_off, a.nseg, a.max_seg_len, a.min_level = seg_off.data_ptr(), T, max_seg_len, int(min_level)
    out = _outputs(who, Portfolios, shapes, None, dev)
    for k in shapes:
        setattr(a, k, getattr(out, k).data_ptr())
    _kcall("fm_portfolio_sort", "fm_portfolio_sort", L.C.byref(a), _stream())
    _remember("fm_portfolio_sort", "fm_portfolio_sort", a, seg_off, forecast, ret, weight, level, nyse, out)
    return out


def lagged_coefficients(roll, ix: TSIndex, problems, lag=1):
    """The coefficient tables [nsel, T, pmax] of ``forecast_portfolio_sort`` from the time-series
    stage's outputs (``roll`` [P, T, pmax], ``ix``), without a host sync on the fitted-month
    counts (fm_lagged_coef): for problem p = problems[j], month ``ix.idx[p, i]`` of the fitted
    rows i in [lag, count[p]) gets ``roll[p, i - lag]`` -- the row fm_predictive reads for that
    month -- and every other month NaN."""
    P, T, pmax = roll.shape
    problems = tuple(int(p) for p in problems)
    if any(p < 0 or p >= P for p in problems):
        raise ValueError(f"lagged_coefficients: problems must lie in 0..{P - 1}")
    if lag < 0:
        raise ValueError("lagged_coefficients: lag must be >= 0")
    roll = roll.contiguous()
    dev = roll.device
    out = torch.empty((len(problems), T, pmax), dtype=torch.float64, device=dev)
    if not problems or T == 0:
        return out
    pj = _small_tensor(problems, torch.int32, dev)
    idx, cnt = ix.idx.contiguous(), ix.count.contiguous()
    _kcall("fm_lagged_coef", "fm_lagged_coef", roll.data_ptr(), idx.data_ptr(), cnt.data_ptr(), T, P, pmax,
           pj.data_ptr(), len(problems), int(lag), out.data_ptr(), _stream())
    return out


def _forecast_plan(who, panel, coef, sel, cuts):
    """What the fused-forecast functions do before their loop: the panel's source, ``sel`` with its
    columns resolved to indices, ``coef`` and the cuts' tables checked -> (src, sel, coef, lo, hi)."""
    src = _source(panel)
    T, C, nsel = panel.nseg, src.ncols, len(sel)
    sel = [([panel.col(c) if isinstance(c, str) else int(c) for c in xs], int(lv)) for xs, lv in sel]
    coef = coef.contiguous()
    if coef.dtype != torch.float64 or coef.dim() != 3 or coef.shape[0] != nsel or coef.shape[1] != T or \
            coef.device != src.device:
        raise ValueError(f"{who}: coef must be a float64 [{nsel}, {T}, >= K+1] tensor on {src.device}")
    lo = hi = None
    if cuts is not None:
        lo, hi = cuts.lo.contiguous(), cuts.hi.contiguous()
        if tuple(lo.shape) != (C, T) or tuple(hi.shape) != (C, T):
            raise ValueError(f"{who}: the cuts must be [{C}, {T}] tables")
    return src, sel, coef, lo, hi


def _fill_forecast_src(f, n, part, j0=0, src=None, coef=None, lo=None, hi=None, forecast_out=None):
    """Fill the fm_forecast_src ``f`` for the sorts ``part`` = sel[j0:j0 + m] of an ``n``-row panel:
    the sorts' columns and levels, then from ``src`` the one layout the kernel reads (FP64 columns if
    the panel has them, else its planes), the cuts, ``coef[j0:]`` and ``forecast_out[j0:]``.
    ``src`` None (the caller's own forecast vectors): the sorts' count and levels only."""
    f.nrows, f.nsel = n, len(part)
    for j, (xs, lv) in enumerate(part):
        f.sel_k[j], f.sel_level[j] = len(xs), lv
        for k, c in enumerate(xs[:L.FM_MAX_SORT_K]):
            f.sel_cols[j][k] = c
    if src is None:
        return
    if src.f64 is not None:
        f.cols, f.col_stride = src.ptr, src.stride
    else:
        f.hi_plane, f.lo_plane, f.plane_stride = src.hp, src.lp, src.pstride
    f.ncols, f.lo, f.hi = src.ncols, _ptr(lo), _ptr(hi)
    nsel = coef.shape[0]
    f.coef, f.coef_stride = coef[j0:].data_ptr() if nsel else None, coef.stride(1)
    f.forecast_out = forecast_out[j0:].data_ptr() if forecast_out is not None and nsel else None


def forecast_portfolio_sort(panel: DevicePanel, coef, sel, cuts: Cuts = None, ret="retx", weight=None, level=None,
                            nyse=None, nport=10, q=None, nyse_breakpoints=False, min_count=None,
                            forecast_out=False, out: "Portfolios" = None):
    """A12 fused with its forecast: for every sort j of ``sel`` = [(xs, min_level), ...] (``xs`` the
    predictors' panel columns, names or indices, in coefficient order) and every month t, each row's
    F = c0 + sum_k c_k clip(x_k) with c = ``coef[j, t]`` ([nsel, T, >= K+1], e.g. from
    ``lagged_coefficients``) and the ``cuts`` (None: no clipping) is computed inside the sort
    kernel's load phase, from whichever layout the panel holds (FP64 columns, else its planes; no
    merged copy, no clipped panel, no forecast vector), then sorted as ``portfolio_sort`` sorts
    with the panel column ``ret`` as the realised return (fm_forecast_portfolio_sort; the
    definition is in fm_hip.h).  One launch per FM_MAX_SORTS sorts.  Returns ``Portfolios`` whose
    tensors carry a leading [nsel] dimension; ``forecast_out``: also the forecasts [nsel, rows];
    ``out``: a ``Portfolios`` of that shape to write into (else allocated)."""
    who = "forecast_portfolio_sort"
    src, sel, coef, lo, hi = _forecast_plan(who, panel, coef, sel, cuts)
    dev = src.device
    n, T, nsel = panel.nrows, panel.nseg, len(sel)
    weight = _row_vector(who, weight, torch.float64, n, dev, "weight")
    level = _row_vector(who, level, torch.uint8, n, dev, "level")
    nyse = _row_vector(who, nyse, torch.uint8, n, dev, "nyse")
    fill, shapes = _sort_plan(who, (nsel,), T, n, int(nport), q, nyse_breakpoints, min_count)
    if forecast_out:
        shapes["forecast"] = ((nsel, n), torch.float64)
    out = _outputs(who, Portfolios, shapes, out, dev)
    for j0 in range(0, max(nsel, 1), L.FM_MAX_SORTS):
        a = fill(L.FPortArgs())
        _fill_forecast_src(a.src, n, sel[j0:j0 + L.FM_MAX_SORTS], j0, src, coef, lo, hi,
                           out.forecast if forecast_out else None)
        a.ret_col = panel.col(ret) if isinstance(ret, str) else int(ret)
        a.weight, a.level, a.nyse = _ptr(weight), _ptr(level), _ptr(nyse)
        a.seg_off, a.nseg, a.max_seg_len = panel.seg_off.data_ptr(), T, panel.max_seg_len
        if nsel:
            a.bp, a.port, a.rec = out.bp[j0:].data_ptr(), out.port[j0:].data_ptr(), out.rec[j0:].data_ptr()
            a.cnt, a.status = out.cnt[j0:].data_ptr(), out.status[j0:].data_ptr()
        _kcall("fm_forecast_portfolio_sort", "fm_forecast_portfolio_sort", L.C.byref(a), _stream())
        _remember("fm_forecast_portfolio_sort", "fm_forecast_portfolio_sort", a, src, panel.planes, panel.seg_off,
                  coef, lo, hi, weight, level, nyse, out)
    return out


def portfolio_summary(p: Portfolios, nw_lags=4):
    """FM mean, Newey-West s.e., t and nobs of the (nport+1) * 4 monthly series of ``p.rec`` over
    the sorted months (status 1), NaN entries dropped per series -> ``Summary`` with
    [nport+1, 4] tensors; for the batched ``Portfolios`` of ``forecast_portfolio_sort`` every sort
    is one problem of the same two launches, and the tensors are [nsel, nport+1, 4]."""
    if p.rec.dim() == 4:
        S, T, n1, k = p.rec.shape
        s = _rec_summary(p.rec, p.status, nw_lags)
        return Summary(s.mean.view(S, n1, k), s.se.view(S, n1, k), s.tstat.view(S, n1, k), s.nobs.view(S, n1, k))
    T, n1, k = p.rec.shape
    ix = ts_compact(p.status.view(T, 1), 1, 1, T, 1)
    s = ts_summary(p.rec, n1 * k, n1 * k, ix, T, 1, n1 * k, nw_lags)
    return Summary(s.mean.view(n1, k), s.se.view(n1, k), s.tstat.view(n1, k), s.nobs.view(n1, k))


@dataclass
class PortfolioAlphas:
    # leading dimensions [nport+1, 2 (ew, vw), M]; [nsel, nport+1, 2, M] for a batched Portfolios
    coef: torch.Tensor     # [..., K+1] float64: alpha, then the loading on factor column f at 1 + f (NaN: not in the model)
    se: torch.Tensor       # [..., K+1] float64 classical standard errors
    se_hac: torch.Tensor   # [..., K+1] float64 Newey-West standard errors
    stat: torch.Tensor     # [..., 4] float64: R2, residual s, mean and ddof-1 sd of the dependent series
    nobs: torch.Tensor     # [...] int32 months used

    @property
    def tstat(self):
        return self.coef / self.se

    @property
    def tstat_hac(self):
        return self.coef / self.se_hac


def alpha_model_masks(models, K):
    """The bit masks of ``models`` (sequences of factor columns; None: CAPM on column 0 and, when
    K > 1, all K factors).  ValueError for an empty model, a repeated column or one outside 0..K-1."""
    if models is None:
        models = [[0]] + ([list(range(K))] if K > 1 else [])
    masks = []
    for cols in models:
        cols = [int(c) for c in cols]
        if not cols or len(set(cols)) != len(cols) or min(cols) < 0 or max(cols) >= K:
            raise ValueError(f"portfolio_alphas: a model must name distinct factor columns in 0..{K - 1}, got {cols}")
        masks.append(sum(1 << c for c in cols))
    if not 1 <= len(masks) <= L.FM_MAX_ALPHA_MODELS:
        raise ValueError(f"portfolio_alphas: 1..{L.FM_MAX_ALPHA_MODELS} models per call, got {len(masks)}")
    return masks


def portfolio_alphas(ports: Portfolios, factors, models=None, rf=None, nw_lags=0):
    """A18: the factor-model alphas of forecast-sorted portfolios -- every row of ``ports.rec``
    (the portfolios and the high-minus-low spread), equal- and value-weighted, regressed over the
    sorted months on each of ``models``' factor returns, with classical and Newey-West(``nw_lags``)
    standard errors, R2, and the mean and standard deviation of the series, in one launch
    (fm_portfolio_alpha; the definition is in fm_hip.h).  ``ports``: a ``Portfolios`` of
    ``portfolio_sort`` (rec [T, nport+1, 4]) or the batched one of ``forecast_portfolio_sort``;
    ``factors`` float64 [T, K] on its device, K <= 6, a NaN row dropping the month; ``rf`` float64
    [T] or None, subtracted from the portfolios' returns (not from the spread); ``models``: up to 4
    sequences of factor columns, default CAPM on column 0 plus, when K > 1, all K factors.
    Returns ``PortfolioAlphas``.  No host sync."""
    rec, status = ports.rec, ports.status
    dev = rec.device
    batched = rec.dim() == 4
    if rec.dtype != torch.float64 or rec.dim() not in (3, 4) or rec.shape[-1] != 4 or rec.shape[-2] < 1:
        raise ValueError("portfolio_alphas: ports.rec must be a float64 [T, nport+1, 4] or [nsel, T, nport+1, 4] tensor")
    S = int(rec.shape[0]) if batched else 1
    T, nrow = int(rec.shape[-3]), int(rec.shape[-2])
    if status.dtype != torch.int32 or tuple(status.shape) != tuple(rec.shape[:-2]) or status.device != dev:
        raise ValueError(f"portfolio_alphas: ports.status must be an int32 {list(rec.shape[:-2])} tensor on {dev}")
    if factors.dtype != torch.float64 or factors.dim() != 2 or factors.shape[0] != T or factors.device != dev:
        raise ValueError(f"portfolio_alphas: factors must be a float64 [{T}, K] tensor on {dev}")
    K = int(factors.shape[1])
    if not 1 <= K <= L.FM_MAX_FACTORS:
        raise ValueError(f"portfolio_alphas: 1..{L.FM_MAX_FACTORS} factor columns, got {K}")
    if rf is not None and (rf.dtype != torch.float64 or rf.dim() != 1 or rf.shape[0] != T or rf.device != dev):
        raise ValueError(f"portfolio_alphas: rf must be a float64 [{T}] tensor on {dev}")
    masks = alpha_model_masks(models, K)
    M = len(masks)
    factors = factors.contiguous()
    rf = None if rf is None else rf.contiguous()
    lead = ((S,) if batched else ()) + (nrow, 2, M)
    out = PortfolioAlphas(coef=torch.empty(lead + (K + 1,), dtype=torch.float64, device=dev),
                          se=torch.empty(lead + (K + 1,), dtype=torch.float64, device=dev),
                          se_hac=torch.empty(lead + (K + 1,), dtype=torch.float64, device=dev),
                          stat=torch.empty(lead + (L.FM_ALPHA_NSTAT,), dtype=torch.float64, device=dev),
                          nobs=torch.empty(lead, dtype=torch.int32, device=dev))
    # rec and status are read in place, whatever their strides
    a = L.AlphaArgs(rec=rec.data_ptr(), rec_month=rec.stride(-3), rec_sort=rec.stride(0) if batched else 0,
                    rec_row=rec.stride(-2), rec_col=rec.stride(-1), status=status.data_ptr(),
                    st_month=status.stride(-1), st_sort=status.stride(0) if batched else 0,
                    nsel=S, nrow=nrow, T=T, K=K, M=M,
                    nw_lags=int(nw_lags), factors=factors.data_ptr(), rf=_ptr(rf), spread_row=nrow - 1,
                    coef=out.coef.data_ptr(), se=out.se.data_ptr(), se_hac=out.se_hac.data_ptr(),
                    stat=out.stat.data_ptr(), nobs=out.nobs.data_ptr())
    for m, v in enumerate(masks):
        a.model_mask[m] = v
    _kcall("fm_portfolio_alpha", "fm_portfolio_alpha", L.C.byref(a), _stream())
    _remember("fm_portfolio_alpha", "fm_portfolio_alpha", a, rec, status, factors, rf, out)
    return out


@dataclass
class ForecastDist:
    rec: torch.Tensor      # [nsel, T, 2+nq] float64: mean, sd (ddof 1), the nq quantiles (NaN: status 0)
    cnt: torch.Tensor      # [nsel, T] int32 eligible rows
    status: torch.Tensor   # [nsel, T] int32: 1 = the month has at least min_count eligible rows
    forecast: Optional[torch.Tensor] = None   # [nsel, rows] float64 (forecast_dist, on request)


def _dist_plan(who, nsel, T, n, q, min_count, forecast_out, out, dev):
    """What the two forecast-distribution entry points share: the levels, the ``ForecastDist`` to fill
    (``out`` checked, else allocated) and ``fill(a, j0)``, which sets the fields of an argument
    struct outside its ``src`` for the sorts from j0."""
    qs = [float(v) for v in q]
    nq = min(len(qs), L.FM_MAX_DIST_Q)   # output shapes of a call the library will refuse
    shapes = dict(rec=((nsel, T, 2 + nq), torch.float64), cnt=((nsel, T), torch.int32),
                  status=((nsel, T), torch.int32))
    if forecast_out:
        shapes["forecast"] = ((nsel, n), torch.float64)
    out = _outputs(who, ForecastDist, shapes, out, dev)

    def fill(a, j0):
        a.nq, a.min_count, a.nseg = len(qs), int(min_count), T
        for i, v in enumerate(qs[:L.FM_MAX_DIST_Q]):
            a.q[i] = v
        if nsel:
            a.rec, a.cnt, a.status = out.rec[j0:].data_ptr(), out.cnt[j0:].data_ptr(), out.status[j0:].data_ptr()
        return a

    return out, fill


def forecast_dist(panel: DevicePanel, coef, sel, cuts: Cuts = None, level=None, q=(0.1, 0.9), min_count=1,
                  forecast_out=False, out: "ForecastDist" = None):
    """A14: for every sort j of ``sel`` = [(xs, min_level), ...] and every month, the count, mean,
    ddof-1 standard deviation and ``q`` quantiles of the eligible rows' forecasts -- the forecast
    of ``forecast_portfolio_sort`` (``coef`` [nsel, T, >= K+1], ``cuts``, ``level`` as there), bit
    for bit, computed in the kernel's load phase from whichever layout the panel holds
    (fm_forecast_dist; the definition is in fm_hip.h).  One launch per FM_MAX_SORTS sorts.  Returns
    ``ForecastDist``; ``forecast_out``: also the forecasts [nsel, rows]; ``out``: a
    ``ForecastDist`` of that shape to write into (else allocated)."""
    src, sel, coef, lo, hi = _forecast_plan("forecast_dist", panel, coef, sel, cuts)
    dev = src.device
    n, T, nsel = panel.nrows, panel.nseg, len(sel)
    level = _row_vector("forecast_dist", level, torch.uint8, n, dev, "level")
    out, fill = _dist_plan("forecast_dist", nsel, T, n, q, min_count, forecast_out, out, dev)
    for j0 in range(0, max(nsel, 1), L.FM_MAX_SORTS):
        a = fill(L.FDistArgs(), j0)
        _fill_forecast_src(a.src, n, sel[j0:j0 + L.FM_MAX_SORTS], j0, src, coef, lo, hi,
                           out.forecast if forecast_out else None)
        a.level, a.seg_off, a.max_seg_len = _ptr(level), panel.seg_off.data_ptr(), panel.max_seg_len
        _kcall("fm_forecast_dist", "fm_forecast_dist", L.C.byref(a), _stream())
        _remember("fm_forecast_dist", "fm_forecast_dist", a, src, panel.planes, panel.seg_off, coef, lo, hi, level, out)
    return out


def _forecast_vectors(who, forecast, seg_off, level, min_level, max_seg_len):
    """What the entry points on the caller's own forecast vectors share: ``forecast`` as a contiguous
    [nsel, rows] block (a 1-D forecast is one vector), the months, ``level`` checked, ``min_level`` as
    one level per vector and the longest month -> (forecast, seg_off, T, level, levels, max_seg_len)."""
    dev = forecast.device
    if forecast.dtype != torch.float64 or forecast.dim() not in (1, 2):
        raise ValueError(f"{who}: forecast must be a float64 [rows] or [nsel, rows] tensor")
    forecast = forecast.view(1, -1) if forecast.dim() == 1 else forecast
    forecast = forecast.contiguous()
    nsel, n = int(forecast.shape[0]), int(forecast.shape[1])
    seg_off, T = _months(who, seg_off, dev, "forecast's")
    level = _row_vector(who, level, torch.uint8, n, dev, "level")
    levels = [int(min_level)] * nsel if np.ndim(min_level) == 0 else [int(v) for v in min_level]
    if len(levels) != nsel:
        raise ValueError(f"{who}: min_level must be one value or {nsel}")
    return forecast, seg_off, T, level, levels, _longest_month(seg_off, T, max_seg_len)


def forecast_dist_vector(seg_off, forecast, level=None, min_level=0, q=(0.1, 0.9), min_count=1, max_seg_len=None):
    """A14 on forecast vectors the caller holds: ``forecast`` float64 [rows] or [nsel, rows] on the
    device, months ``seg_off`` int64 [T+1]; eligible rows are the finite forecasts with ``level`` >=
    ``min_level`` (one value, or one per vector).  Returns ``ForecastDist`` with a leading [nsel]
    dimension (1 for a 1-D forecast).  ``max_seg_len``: the longest month if the caller knows it
    (otherwise read from ``seg_off``, one host sync)."""
    who = "forecast_dist_vector"
    forecast, seg_off, T, level, levels, max_seg_len = _forecast_vectors(who, forecast, seg_off, level, min_level,
                                                                         max_seg_len)
    dev, (nsel, n) = forecast.device, forecast.shape
    out, fill = _dist_plan(who, nsel, T, n, q, min_count, False, None, dev)
    for j0 in range(0, max(nsel, 1), L.FM_MAX_SORTS):
        a = fill(L.FDistArgs(), j0)
        _fill_forecast_src(a.src, n, [((), lv) for lv in levels[j0:j0 + L.FM_MAX_SORTS]])
        a.forecast = forecast[j0:].data_ptr() if nsel else None
        a.level, a.seg_off, a.max_seg_len = _ptr(level), seg_off.data_ptr(), max_seg_len
        _kcall("fm_forecast_dist", "fm_forecast_dist", L.C.byref(a), _stream())
        _remember("fm_forecast_dist", "fm_forecast_dist", a, seg_off, forecast, level, out)
    return out


def forecast_dist_summary(d: ForecastDist, nw_lags=4):
    """FM mean, Newey-West s.e., t and nobs of the 2 + nq monthly series of ``d.rec`` over the
    months with status 1, NaN entries dropped per series (the sd of a one-row month) ->
    ``Summary`` with [nsel, 2+nq] tensors: every sort is one problem of the two launches
    ``portfolio_summary`` issues."""
    return _rec_summary(d.rec, d.status, nw_lags)


@dataclass
class ForecastCompare:
    rec: torch.Tensor      # [npair, T, 7] float64: correlation, slope, intercept, residual sd (ddof 1) of
    #                        F_b on F_a; slope, intercept, R2 of the return on the residual (NaN: status 0)
    cnt: torch.Tensor      # [npair, T, 2] int32: rows with both forecasts; those with a return as well
    status: torch.Tensor   # [npair, T] int32: 1 = the month has at least max(min_count, 2) such rows
    forecast: Optional[torch.Tensor] = None   # [nsel, rows] float64 (forecast_compare, on request)


def _pair_batches(who, pairs, nsel):
    """``pairs`` = [(a, b, min_level), ...] cut greedily, in order, into launches of at most
    FM_MAX_PAIRS pairs over at most FM_MAX_SORTS distinct forecasts -> (pairs, [(p0, part, js)]):
    ``part`` the launch's pairs from pair p0 on with a and b as indices into ``js``, the launch's
    forecasts in ascending order."""
    pairs = [(int(a), int(b), int(lv)) for a, b, lv in pairs]
    for a, b, _ in pairs:
        if not (0 <= a < nsel and 0 <= b < nsel):
            raise ValueError(f"{who}: pair ({a}, {b}) outside the {nsel} forecasts")
    cuts, p0, js = [], 0, set()
    for p, (a, b, _) in enumerate(pairs):
        if p - p0 == L.FM_MAX_PAIRS or len(js | {a, b}) > L.FM_MAX_SORTS:
            cuts.append((p0, p, sorted(js)))
            p0, js = p, set()
        js |= {a, b}
    cuts.append((p0, len(pairs), sorted(js)))
    return pairs, [(p0, [(js.index(a), js.index(b), lv) for a, b, lv in pairs[p0:p1]], js) for p0, p1, js in cuts]


def _compare_plan(who, npair, T, nsel, n, forecast_out, out, dev):
    """The ``ForecastCompare`` to fill (``out`` checked, else allocated) and ``fill(a, p0, part)``,
    which sets an argument struct's pairs and its outputs from pair p0 on."""
    shapes = dict(rec=((npair, T, L.FM_FCMP_NREC), torch.float64), cnt=((npair, T, 2), torch.int32),
                  status=((npair, T), torch.int32))
    if forecast_out:
        shapes["forecast"] = ((nsel, n), torch.float64)
    out = _outputs(who, ForecastCompare, shapes, out, dev)

    def fill(a, p0, part):
        a.npair, a.nseg = len(part), T
        for i, (ja, jb, lv) in enumerate(part):
            a.pair_a[i], a.pair_b[i], a.pair_level[i] = ja, jb, lv
        if npair:
            a.rec, a.cnt, a.status = out.rec[p0:].data_ptr(), out.cnt[p0:].data_ptr(), out.status[p0:].data_ptr()
        return a

    return out, fill


def _rows_of(t, js):
    """Rows ``js`` (ascending) of ``t`` as one contiguous block: a view where they are consecutive."""
    if js and js[-1] - js[0] + 1 == len(js):
        return t[js[0]:js[-1] + 1]
    return t[js].contiguous()


def forecast_compare(panel: DevicePanel, coef, sel, pairs, cuts: Cuts = None, ret="retx", level=None, min_count=1,
                     forecast_out=False, out: "ForecastCompare" = None):
    """A15 (paper Table 4, model comparison): for every pair (a, b, min_level) of ``pairs`` -- a and b
    indices into ``sel``, the forecasts of ``forecast_dist`` (``sel`` = [(xs, level), ...] whose level
    is not read here, ``coef`` [nsel, T, >= K+1], ``cuts`` as there) -- and every month: forecast b
    regressed on forecast a across the rows of the universe ``min_level`` where both are finite
    (correlation, slope, intercept, residual standard deviation), then the panel column ``ret`` on
    that residual (slope, intercept, R2).  Both forecasts are computed in the kernel's load phase,
    bit for bit ``forecast_dist``'s (fm_forecast_compare; the definition is in fm_hip.h).  One launch
    per FM_MAX_PAIRS pairs over at most FM_MAX_SORTS distinct forecasts, cut greedily in the pairs'
    order.  Returns ``ForecastCompare`` with a leading [npair] dimension; ``forecast_out``: also the
    forecasts [nsel, rows] (the rows of a forecast no pair names are NaN); ``out``: a
    ``ForecastCompare`` of that shape to write into (else allocated)."""
    src, sel, coef, lo, hi = _forecast_plan("forecast_compare", panel, coef, sel, cuts)
    dev = src.device
    n, T, nsel = panel.nrows, panel.nseg, len(sel)
    pairs, batches = _pair_batches("forecast_compare", pairs, nsel)
    level = _row_vector("forecast_compare", level, torch.uint8, n, dev, "level")
    out, fill = _compare_plan("forecast_compare", len(pairs), T, nsel, n, forecast_out, out, dev)
    if forecast_out:
        unused = sorted(set(range(nsel)) - {j for a, b, _ in pairs for j in (a, b)})
        if unused:
            out.forecast[unused] = float("nan")
    for p0, part, js in batches:
        a = fill(L.FCmpArgs(), p0, part)
        cj = _rows_of(coef, js)
        fj = _rows_of(out.forecast, js) if forecast_out else None
        _fill_forecast_src(a.src, n, [sel[j] for j in js], 0, src, cj, lo, hi, fj)
        a.ret_col = panel.col(ret) if isinstance(ret, str) else int(ret)
        a.level, a.seg_off, a.max_seg_len, a.min_count = _ptr(level), panel.seg_off.data_ptr(), panel.max_seg_len, int(min_count)
        _kcall("fm_forecast_compare", "fm_forecast_compare", L.C.byref(a), _stream())
        _remember("fm_forecast_compare", "fm_forecast_compare", a, src, panel.planes, panel.seg_off, cj, fj, lo, hi, level, out)
        if js and fj is not None and fj.data_ptr() != out.forecast[js[0]].data_ptr():   # a gathered copy
            out.forecast[js] = fj
    return out


def forecast_compare_vector(seg_off, forecast, ret, pairs, level=None, min_count=1, max_seg_len=None):
    """A15 on forecast vectors the caller holds: ``forecast`` float64 [nsel, rows] and the realised
    return ``ret`` float64 [rows] on the device, months ``seg_off`` int64 [T+1]; ``pairs`` =
    [(a, b, min_level), ...] regresses vector b on vector a over the rows with ``level`` >=
    min_level where both are finite.  Returns ``ForecastCompare`` with a leading [npair] dimension.
    ``max_seg_len``: the longest month if the caller knows it (otherwise read from ``seg_off``, one
    host sync)."""
    dev = forecast.device
    if forecast.dtype != torch.float64 or forecast.dim() != 2:
        raise ValueError("forecast_compare_vector: forecast must be a float64 [nsel, rows] tensor")
    forecast = forecast.contiguous()
    nsel, n = int(forecast.shape[0]), int(forecast.shape[1])
    seg_off, T = _months("forecast_compare_vector", seg_off, dev, "forecast's")
    ret = _row_vector("forecast_compare_vector", ret, torch.float64, n, dev, "ret")
    level = _row_vector("forecast_compare_vector", level, torch.uint8, n, dev, "level")
    pairs, batches = _pair_batches("forecast_compare_vector", pairs, nsel)
    max_seg_len = _longest_month(seg_off, T, max_seg_len)
    out, fill = _compare_plan("forecast_compare_vector", len(pairs), T, nsel, n, False, None, dev)
    for p0, part, js in batches:
        a = fill(L.FCmpArgs(), p0, part)
        fj = _rows_of(forecast, js)
        _fill_forecast_src(a.src, n, [((), 0)] * len(js))
        a.forecast, a.ret = fj.data_ptr() if js else None, _ptr(ret)
        a.level, a.seg_off, a.max_seg_len, a.min_count = _ptr(level), seg_off.data_ptr(), max_seg_len, int(min_count)
        _kcall("fm_forecast_compare", "fm_forecast_compare", L.C.byref(a), _stream())
        _remember("fm_forecast_compare", "fm_forecast_compare", a, seg_off, fj, ret, level, out)
    return out


def forecast_compare_summary(c: ForecastCompare, nw_lags=4):
    """FM mean, Newey-West s.e., t and nobs of the 7 monthly series of ``c.rec`` over the months with
    status 1, NaN entries dropped per series (a constant forecast, a zero residual, a month without
    returns) -> ``Summary`` with [npair, 7] tensors: every pair is one problem of the two launches
    ``forecast_dist_summary`` issues."""
    return _rec_summary(c.rec, c.status, nw_lags)


@dataclass
class ForecastHorizon:
    rec: torch.Tensor      # [nsel, T, 6+nq] float64: mean and sd (ddof 1) of the scaled forecast G; slope, intercept
    #                        and R2 of the k-month return on G; the mean of the monthly forecast; G's nq quantiles
    cnt: torch.Tensor      # [nsel, T, 2] int32: eligible rows; those with a k-month return as well
    status: torch.Tensor   # [nsel, T] int32: 1 = the month has at least min_count eligible rows
    scaled: Optional[torch.Tensor] = None     # [nsel, rows] float64 G (on request; NaN: the row is not eligible)
    forecast: Optional[torch.Tensor] = None   # [nsel, rows] float64 (forecast_horizon, on request)


def extrapolation_gain(k, decay):
    """g = 1 + decay + ... + decay^(k-1) in double, terms added in that order: the factor that
    scales a monthly forecast's deviation from the cross-sectional mean to k months when it decays
    geometrically (the paper's Section 4: decay 0.9; decay 1 gives k exactly)."""
    g, p = 1.0, 1.0
    for _ in range(int(k) - 1):
        p = p * float(decay)
        g = g + p
    return g


def _horizon_plan(who, nsel, T, n, q, min_count, level_mult, gain, scaled_out, forecast_out, out, dev):
    """What the two forecast-horizon entry points share: the ``ForecastHorizon`` to fill (``out``
    checked, else allocated) and ``fill(a, j0)``, which sets the fields of an argument struct
    outside its ``src`` for the sorts from j0."""
    qs = [float(v) for v in q]
    nq = min(len(qs), L.FM_MAX_DIST_Q)   # output shapes of a call the library will refuse
    shapes = dict(rec=((nsel, T, L.FM_FHOR_NREC + nq), torch.float64), cnt=((nsel, T, 2), torch.int32),
                  status=((nsel, T), torch.int32))
    if scaled_out:
        shapes["scaled"] = ((nsel, n), torch.float64)
    if forecast_out:
        shapes["forecast"] = ((nsel, n), torch.float64)
    out = _outputs(who, ForecastHorizon, shapes, out, dev)

    def fill(a, j0):
        a.nq, a.min_count, a.nseg = len(qs), int(min_count), T
        a.level_mult, a.gain = float(level_mult), float(gain)
        for i, v in enumerate(qs[:L.FM_MAX_DIST_Q]):
            a.q[i] = v
        if nsel:
            a.rec, a.cnt, a.status = out.rec[j0:].data_ptr(), out.cnt[j0:].data_ptr(), out.status[j0:].data_ptr()
            a.scaled_out = out.scaled[j0:].data_ptr() if scaled_out else None
        return a

    return out, fill


def forecast_horizon(panel: DevicePanel, coef, sel, ret, level_mult, gain, cuts: Cuts = None, level=None,
                     q=(0.1, 0.9), min_count=1, scaled_out=False, forecast_out=False, out: "ForecastHorizon" = None):
    """A17 (the paper's Section 4, second approach): for every sort j of ``sel`` = [(xs, min_level), ...]
    and every month, the monthly forecast of ``forecast_dist`` (``coef`` [nsel, T, >= K+1], ``cuts``,
    ``level`` as there; bit for bit, computed in the kernel's load phase) is scaled around its
    cross-sectional mean m to G = ``level_mult`` * m + ``gain`` * (F - m); the month's mean, ddof-1
    standard deviation and ``q`` quantiles of G, and the regression of ``ret`` -- a float64 [rows]
    device vector, e.g. ``horizon_return``'s k-month return -- on G (slope, intercept, R2) follow
    (fm_forecast_horizon; the definition is in fm_hip.h).  With ``level_mult`` = k and ``gain`` =
    ``extrapolation_gain(k, 0.9)`` G is the paper's extrapolated k-month forecast.  One launch per
    FM_MAX_SORTS sorts.  Returns ``ForecastHorizon``; ``scaled_out``: also G [nsel, rows];
    ``forecast_out``: also the monthly forecasts [nsel, rows]; ``out``: a ``ForecastHorizon`` of that
    shape to write into (else allocated)."""
    src, sel, coef, lo, hi = _forecast_plan("forecast_horizon", panel, coef, sel, cuts)
    dev = src.device
    n, T, nsel = panel.nrows, panel.nseg, len(sel)
    ret = _row_vector("forecast_horizon", ret, torch.float64, n, dev, "ret")
    level = _row_vector("forecast_horizon", level, torch.uint8, n, dev, "level")
    out, fill = _horizon_plan("forecast_horizon", nsel, T, n, q, min_count, level_mult, gain, scaled_out,
                              forecast_out, out, dev)
    for j0 in range(0, max(nsel, 1), L.FM_MAX_SORTS):
        a = fill(L.FHorArgs(), j0)
        _fill_forecast_src(a.src, n, sel[j0:j0 + L.FM_MAX_SORTS], j0, src, coef, lo, hi,
                           out.forecast if forecast_out else None)
        a.ret, a.level, a.seg_off, a.max_seg_len = _ptr(ret), _ptr(level), panel.seg_off.data_ptr(), panel.max_seg_len
        _kcall("fm_forecast_horizon", "fm_forecast_horizon", L.C.byref(a), _stream())
        _remember("fm_forecast_horizon", "fm_forecast_horizon", a, src, panel.planes, panel.seg_off, coef, lo, hi,
                  ret, level, out)
    return out


def forecast_horizon_vector(seg_off, forecast, ret, level_mult, gain, level=None, min_level=0, q=(0.1, 0.9),
                            min_count=1, max_seg_len=None, scaled_out=False):
    """A17 on forecast vectors the caller holds: ``forecast`` float64 [rows] or [nsel, rows] and the
    realised return ``ret`` float64 [rows] on the device, months ``seg_off`` int64 [T+1]; eligible rows
    are the finite forecasts with ``level`` >= ``min_level`` (one value, or one per vector).  Returns
    ``ForecastHorizon`` with a leading [nsel] dimension (1 for a 1-D forecast).  ``max_seg_len``: the
    longest month if the caller knows it (otherwise read from ``seg_off``, one host sync)."""
    who = "forecast_horizon_vector"
    forecast, seg_off, T, level, levels, max_seg_len = _forecast_vectors(who, forecast, seg_off, level, min_level,
                                                                         max_seg_len)
    dev, (nsel, n) = forecast.device, forecast.shape
    ret = _row_vector(who, ret, torch.float64, n, dev, "ret")
    out, fill = _horizon_plan(who, nsel, T, n, q, min_count, level_mult, gain, scaled_out, False, None, dev)
    for j0 in range(0, max(nsel, 1), L.FM_MAX_SORTS):
        a = fill(L.FHorArgs(), j0)
        _fill_forecast_src(a.src, n, [((), lv) for lv in levels[j0:j0 + L.FM_MAX_SORTS]])
        a.forecast = forecast[j0:].data_ptr() if nsel else None
        a.ret, a.level, a.seg_off, a.max_seg_len = _ptr(ret), _ptr(level), seg_off.data_ptr(), max_seg_len
        _kcall("fm_forecast_horizon", "fm_forecast_horizon", L.C.byref(a), _stream())
        _remember("fm_forecast_horizon", "fm_forecast_horizon", a, seg_off, forecast, ret, level, out)
    return out


def forecast_horizon_summary(h: ForecastHorizon, nw_lags=4):
    """FM mean, Newey-West s.e., t and nobs of the 6 + nq monthly series of ``h.rec`` over the months
    with status 1, NaN entries dropped per series (a constant forecast, a month without k-month
    returns, the sd of a one-row month) -> ``Summary`` with [nsel, 6+nq] tensors: every sort is one
    problem of the two launches ``forecast_compare_summary`` issues."""
    return _rec_summary(h.rec, h.status, nw_lags)


# fm_rank_transform's month limit (FM_RANK_MAX_ROWS): up to 16,384 rows one workgroup per (month,
# column) sorts the month's keys in LDS; a longer month is ranked in parts of 16,384 rows, at a cost
# quadratic in the part count, so four parts are the limit
RANK_MAX_ROWS = 65536
RANK_METHODS = {"average": L.FM_RANK_AVERAGE, "min": L.FM_RANK_MIN, "max": L.FM_RANK_MAX}
RANK_SCALES = {"raw": L.FM_RANK_RAW, "pct": L.FM_RANK_PCT, "uniform": L.FM_RANK_UNIFORM}


def rank_transform(panel: DevicePanel, cols=None, method="average", scale="pct", level=None, min_level=0,
                   out=None):
    """A13: the chosen columns (names or indices; default all) replaced by their cross-sectional
    ranks within each month (fm_rank_transform; pandas ``groupby(month)[x].rank(method,
    pct)``, the exact definition is in fm_hip.h), every other column copied unchanged.
    ``scale``: "raw" r, "pct" r / n, "uniform" r / (n + 1) - 0.5.  ``level`` (uint8 per row) with
    ``min_level`` ranks within that universe and gives NaN outside it.  Returns a new f64-layout
    ``DevicePanel`` that shares the input's segments, ``me``, ``nyse``, ``months``, ``order``, ``ids``
    and ``month_index`` (``out``: its [C, n] float64 column block, not the input's); the [len(cols), T] int32 table
    of ranked rows per month is its ``rank_nvalid`` attribute."""
    if method not in RANK_METHODS:
        raise ValueError(f"rank_transform: method must be one of {sorted(RANK_METHODS)} "
                         "('first' and 'dense' are out of scope)")
    if scale not in RANK_SCALES:
        raise ValueError(f"rank_transform: scale must be one of {sorted(RANK_SCALES)}")
    src = panel.values()
    C, n, T = panel.ncols, panel.nrows, panel.nseg
    idx = list(range(C)) if cols is None else [panel.col(c) if isinstance(c, str) else int(c) for c in cols]
    if any(i < 0 or i >= C for i in idx) or len(set(idx)) != len(idx):
        raise ValueError("rank_transform: cols must be distinct columns of the panel")
    if out is None:
        out = torch.empty_like(src)
    elif out.dtype != torch.float64 or out.shape != src.shape or out.device != src.device or out.stride(1) != 1:
        raise ValueError("rank_transform: out must be a float64 tensor of the panel's [C, n] shape on its device")
    if out.data_ptr() == src.data_ptr():
        raise ValueError("rank_transform: out must not be the panel's own columns")
    if level is not None:
        if level.dtype != torch.uint8 or level.dim() != 1 or level.shape[0] != n or level.device != src.device:
            raise ValueError(f"rank_transform: level must be a uint8 [{n}] tensor on {src.device}")
        level = level.contiguous()
    for i in sorted(set(range(C)) - set(idx)):
        out[i].copy_(src[i])
    nvalid = torch.empty((len(idx), T), dtype=torch.int32, device=src.device)
    # consecutive columns go in one launch (all 14 predictors of the pipeline: one)
    runs, k = [], 0
    while k < len(idx):
        e = k + 1
        while e < len(idx) and idx[e] == idx[e - 1] + 1:
            e += 1
        runs.append((k, e))
        k = e
    for k, e in runs:
        a = L.RankArgs()
        a.src, a.src_stride = src[idx[k]].data_ptr(), src.stride(0)
        a.dst, a.dst_stride = out[idx[k]].data_ptr(), out.stride(0)
        a.ncols, a.nseg, a.seg_off = e - k, T, panel.seg_off.data_ptr()
        a.max_seg_len, a.min_level, a.level = panel.max_seg_len, int(min_level), _ptr(level)
        a.method, a.scale = RANK_METHODS[method], RANK_SCALES[scale]
        a.nvalid = nvalid[k].data_ptr()
        _kcall("fm_rank_transform", "fm_rank_transform", L.C.byref(a), _stream())
        _remember("fm_rank_transform", "fm_rank_transform", a, src, out, nvalid, level, panel.seg_off)
    res = DevicePanel(cols=out, names=list(panel.names), seg_off=panel.seg_off, seg_off_h=panel.seg_off_h,
                      months=panel.months, me=panel.me, nyse=panel.nyse, order=panel.order,
                      chunk_rows=panel.chunk_rows, chunk_split=panel.chunk_split, chunk_policy=panel.chunk_policy,
                      row_origin=panel.row_origin, group=panel.group, ngroups=panel.ngroups, ids=panel.ids,
                      month_index=panel.month_index)
    _share_links(panel, res)
    res.rank_nvalid = nvalid
    return res


# ------------------------------------------------------------------------------------------
# Multi-month return horizons (A16): firm links between neighbouring months, compounded returns
# ------------------------------------------------------------------------------------------
MAX_HORIZON = L.FM_MAX_HORIZON


def _share_links(src: DevicePanel, dst: DevicePanel):
    """A panel built from ``src`` with the same rows and ids keeps the links ``src`` has."""
    links = src.__dict__.get("_links")
    if links is not None:
        dst.__dict__["_links"] = links


def month_links(panel: DevicePanel, step=1):
    """A16: for every row, the position inside the neighbouring calendar month (``step`` +1: the
    following one, -1: the preceding one) of the same firm's row, -1 where there is none -- no such
    segment, a gap in the calendar (``panel.month_index``), or the firm is absent there
    (fm_month_links; the definition is in fm_hip.h).  int32 [rows] on the device, computed once per
    panel and step and kept.  The panel needs ``ids``, strictly ascending inside every month:
    ValueError otherwise (one host sync on the order check, at ingest)."""
    if step not in (1, -1):
        raise ValueError(f"month_links: step must be +1 or -1, got {step!r}")
    if panel.ids is None or panel.month_index is None:
        raise ValueError("month_links: the panel carries no firm ids (build it with ids=...)")
    cache = panel.__dict__.setdefault("_links", {})
    if step in cache:
        return cache[step]
    _check_ids(panel.ids)
    n, T = panel.nrows, panel.nseg
    if panel.ids.shape[0] != n or len(panel.month_index) != T:
        raise ValueError("month_links: ids / month_index do not match the panel's rows / months")
    dev = panel.device
    link = torch.empty(n, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    mi = panel.month_index_device()
    a = L.LinksArgs(ids=panel.ids.data_ptr(), seg_off=panel.seg_off.data_ptr(), month_index=mi.data_ptr(),
                    nrows=n, nseg=T, step=int(step), link=link.data_ptr(), bad=bad.data_ptr())
    _kcall("fm_month_links", "fm_month_links", L.C.byref(a), _stream())
    _remember("fm_month_links", "fm_month_links", a, panel.ids, panel.seg_off, mi, link, bad)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"month_links: {nbad} rows have a firm id that is not greater than the previous row's "
                         "in the same month (ids must be unique and ascending inside a month)")
    cache[step] = link
    return link


def horizon_return(seg_off, ret, link, horizon, out=None):
    """A16: the compounded ``horizon``-month return of every row, (1 + r_t)(1 + r_t+1) ... - 1 over the
    firm's rows of the following months, found through ``link`` (``month_links`` with step +1); NaN
    where a month of the chain is missing (fm_horizon_return; the definition, exact to the bit, is
    in fm_hip.h).  Plain device tensors: ``seg_off`` int64 [T+1], ``ret`` float64 [rows], ``link``
    int32 [rows]; returns (or fills ``out``) float64 [rows]."""
    n = int(ret.shape[0])
    dev = ret.device
    seg_off, T = _months("horizon_return", seg_off, dev, "returns'")
    ret = _row_vector("horizon_return", ret, torch.float64, n, dev, "ret", required=True)
    link = _row_vector("horizon_return", link, torch.int32, n, dev, "link", required=True)
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.shape != (n,) or out.device != dev or not out.is_contiguous():
        raise ValueError(f"horizon_return: out must be a contiguous float64 [{n}] tensor on {dev}")
    a = L.HorizonArgs(ret=ret.data_ptr(), link=link.data_ptr(), seg_off=seg_off.data_ptr(), nrows=n,
                      nseg=T, horizon=int(horizon), out=out.data_ptr())
    _kcall("fm_horizon_return", "fm_horizon_return", L.C.byref(a), _stream())
    _remember("fm_horizon_return", "fm_horizon_return", a, ret, link, seg_off, out)
    return out


def horizon_panel(panel: DevicePanel, h, ret="retx", name=None):
    """A16: the panel with one more column, the compounded ``h``-month return of column ``ret``
    (``horizon_return`` over ``month_links(panel, +1)``), named ``f"{ret}_{h}m"`` unless ``name`` is
    given and appended last; every other column is copied unchanged.  Returns a new f64-layout
    ``DevicePanel`` that shares the input's segments, ``me``, ``nyse``, ``months``, ``order``, ``ids`` and
    ``month_index``, as ``rank_transform`` returns its panel.  This is an ingest-time copy of the whole
    panel (one more [C+1, n] block in HBM), made once per horizon, not a per-step stage.  The panel
    needs ``ids``; ValueError for a horizon outside 1..MAX_HORIZON, a column name that exists
    already, or more than FM_MAX_COLS columns."""
    h = int(h)
    if h < 1 or h > MAX_HORIZON:
        raise ValueError(f"horizon_panel: the horizon must be 1..{MAX_HORIZON}, got {h}")
    ci = panel.col(ret) if isinstance(ret, str) else int(ret)
    name = f"{panel.names[ci]}_{h}m" if name is None else str(name)
    if name in panel.names:
        raise ValueError(f"horizon_panel: the panel already has a column {name!r}")
    if panel.ncols + 1 > L.FM_MAX_COLS:
        raise ValueError(f"horizon_panel: at most {L.FM_MAX_COLS} columns per panel")
    link = month_links(panel, 1)
    src = panel.values()
    C, n = panel.ncols, panel.nrows
    out = torch.empty((C + 1, n), dtype=torch.float64, device=src.device)
    out[:C].copy_(src[:, :n])
    horizon_return(panel.seg_off, src[ci], link, h, out=out[C])
    res = DevicePanel(cols=out, names=list(panel.names) + [name], seg_off=panel.seg_off, seg_off_h=panel.seg_off_h,
                      months=panel.months, me=panel.me, nyse=panel.nyse, order=panel.order,
                      chunk_rows=panel.chunk_rows, chunk_split=panel.chunk_split, chunk_policy=panel.chunk_policy,
                      row_origin=panel.row_origin, group=panel.group, ngroups=panel.ngroups, ids=panel.ids,
                      month_index=panel.month_index)
    _share_links(panel, res)
    return res


def column_vector(panel: DevicePanel, col):
    """Column ``col`` (name or index) as a contiguous float64 [rows] device vector: a view of the FP64
    columns, or for a planes-only panel a merge of that column's two planes alone (fm_merge_planes)."""
    i = panel.col(col) if isinstance(col, str) else int(col)
    n = panel.nrows
    if panel.cols is not None:
        return panel.cols[i, :n]
    out = torch.empty(n, dtype=torch.float64, device=panel.planes.device)
    _kcall("fm_merge_planes", "fm_merge_planes", panel.planes[0, i].data_ptr(), panel.planes[1, i].data_ptr(),
           panel.planes.stride(1), 1, n, out.data_ptr(), n, _stream())
    return out


MAX_HOLD = L.FM_MAX_HOLD


@dataclass
class HeldPortfolios:
    # ``rec`` and ``status`` have ``Portfolios``' shapes and dtypes: portfolio_summary and
    # portfolio_alphas read a HeldPortfolios as they read a Portfolios.  Every tensor carries a leading
    # [nsel] dimension when the port bytes did.
    rec: torch.Tensor        # [T, nport+1, 4] float64: the k-cohort average of ew ret, predicted, vw ret, predicted; last = H-L
    status: torch.Tensor     # [T] int32: 1 = a complete month (k sorted consecutive months end here)
    cohort: torch.Tensor     # [T, k, nport, 2] float64: month-t ew / vw return of the cohort formed a months earlier
    cohort_n: torch.Tensor   # [T, k, nport, 2] int32: its rows with a finite return / also a finite weight > 0
    members: torch.Tensor    # [T, k+1, nport] int32: rows whose age-a ancestor was in portfolio q
    stay: torch.Tensor       # [T, k+1, nport] int32: those that are in portfolio q themselves
    turnover: torch.Tensor   # [T, nport] float64: share of names replaced in month t
    hold: int = 1


def portfolio_hold(seg_off, month_index, link_prev, port, status, ret, weight=None, nport=10, hold=1, sort_rec=None):
    """A19: the sorted portfolios held for ``hold`` = k months as overlapping cohorts -- in month t
    the k cohorts formed in months t, t-1, .., t-k+1, each followed through the firm links -- as a
    monthly record with ``Portfolios``' layout, plus the cohorts' returns and sizes, how many of a
    cohort's names are still in the same portfolio at every age, and the monthly name turnover
    (fm_portfolio_hold; the definition is in fm_hip.h).  Plain device tensors in, ``HeldPortfolios``
    out: ``seg_off`` int64 [T+1], ``month_index`` int32 [T], ``link_prev`` int32 [rows]
    (``month_links`` with step -1), ``port`` uint8 [rows] or [nsel, rows] and ``status`` int32 [T] or
    [nsel, T] of a sort, ``ret`` and ``weight`` float64 [rows], ``sort_rec`` the sort's own ``rec``
    (for the predicted columns; None: they are NaN).  One launch, no host sync."""
    dev = ret.device
    n = int(ret.shape[0])
    who = "portfolio_hold"
    seg_off, T = _months(who, seg_off, dev, "returns'")
    nport, hold = int(nport), int(hold)
    if not 2 <= nport <= L.FM_MAX_PORTS:
        raise ValueError(f"portfolio_hold: nport must be 2..{L.FM_MAX_PORTS}, got {nport}")
    if not 1 <= hold <= L.FM_MAX_HOLD:
        raise ValueError(f"portfolio_hold: hold must be 1..{L.FM_MAX_HOLD}, got {hold}")
    batched = port.dim() == 2
    S = int(port.shape[0]) if batched else 1
    lead = (S,) if batched else ()
    if S > L.FM_MAX_SORTS:
        raise ValueError(f"portfolio_hold: at most {L.FM_MAX_SORTS} sorts per call, got {S}")
    month_index = _row_vector(who, month_index, torch.int32, T, dev, "month_index", required=True)
    link_prev = _row_vector(who, link_prev, torch.int32, n, dev, "link_prev", required=True)
    port = _row_vector(who, port, torch.uint8, lead + (n,), dev, "port", required=True)
    status = _row_vector(who, status, torch.int32, lead + (T,), dev, "status", required=True)
    ret = _row_vector(who, ret, torch.float64, n, dev, "ret", required=True)
    weight = _row_vector(who, weight, torch.float64, n, dev, "weight")
    sort_rec = _row_vector(who, sort_rec, torch.float64, lead + (T, nport + 1, 4), dev, "sort_rec")

    empty, nan, f64, i32 = not (n and T and S), float("nan"), torch.float64, torch.int32
    out = HeldPortfolios(rec=_new_or_filled(empty, lead + (T, nport + 1, 4), f64, nan, dev),
                         status=_new_or_filled(empty, lead + (T,), i32, 0, dev),
                         cohort=_new_or_filled(empty, lead + (T, hold, nport, 2), f64, nan, dev),
                         cohort_n=_new_or_filled(empty, lead + (T, hold, nport, 2), i32, 0, dev),
                         members=_new_or_filled(empty, lead + (T, hold + 1, nport), i32, 0, dev),
                         stay=_new_or_filled(empty, lead + (T, hold + 1, nport), i32, 0, dev),
                         turnover=_new_or_filled(empty, lead + (T, nport), f64, nan, dev), hold=hold)
    a = L.HoldArgs(seg_off=seg_off.data_ptr(), month_index=month_index.data_ptr(), link_prev=link_prev.data_ptr(),
                   port=port.data_ptr(), status=status.data_ptr(), ret=ret.data_ptr(), weight=_ptr(weight),
                   sort_rec=_ptr(sort_rec), nrows=n, nseg=T, nsel=S, nport=nport, hold=hold,
                   members=out.members.data_ptr(), stay=out.stay.data_ptr(), cohort_n=out.cohort_n.data_ptr(),
                   cohort=out.cohort.data_ptr(), status_out=out.status.data_ptr(), rec=out.rec.data_ptr(),
                   turnover=out.turnover.data_ptr())
    _kcall("fm_portfolio_hold", "fm_portfolio_hold", L.C.byref(a), _stream())
    _remember("fm_portfolio_hold", "fm_portfolio_hold", a, seg_off, month_index, link_prev, port, status, ret, weight,
              sort_rec, out)
    return out


def held_portfolios(panel: DevicePanel, ports: Portfolios, hold, ret="retx", weight=None):
    """A19 on a panel: ``portfolio_hold`` of the sorted ``ports`` (``portfolio_sort`` or the batched
    ``forecast_portfolio_sort``) with the panel's segments, calendar and step -1 firm links
    (``month_links``), the panel column ``ret`` and the sort's own records for the predicted columns.
    The panel needs ``ids``: ValueError otherwise."""
    if panel.ids is None or panel.month_index is None:
        raise ValueError("held_portfolios: the panel carries no firm ids (build it with ids=...)")
    nport = int(ports.rec.shape[-2]) - 1
    return portfolio_hold(panel.seg_off, panel.month_index_device(), month_links(panel, -1), ports.port, ports.status,
                          column_vector(panel, ret), weight=weight, nport=nport, hold=hold, sort_rec=ports.rec)


# ------------------------------------------------------------------------------------------
# Double-sorted portfolios and the factor returns built from them (A21)
# ------------------------------------------------------------------------------------------
MAX_DSORT = L.FM_MAX_DSORT


@dataclass
class DoubleSort:
    # nsel sorts of na x nb cells; ``batched`` False: the call had one [n] signal pair (nsel = 1)
    rec_b: torch.Tensor    # [nsel, na+1, T, nb+1, 4] float64: per a-bin (last slab: a-neutral) the b portfolios'
    #                        ew ret, ew mean b, vw ret, vw mean b; last row = H-L
    rec_a: torch.Tensor    # [nsel, nb+1, T, na+1, 4] float64: the same with the roles swapped (ew / vw mean a)
    cnt: torch.Tensor      # [nsel, T, na, nb] int32 rows with a finite return
    cell: torch.Tensor     # [nsel, rows] uint8: pa * nb + pb, 255 = none
    bpa: torch.Tensor      # [nsel, T, na-1] float64 breakpoints of a (NaN: unsorted month)
    bpb: torch.Tensor      # [nsel, T, na, nb-1] float64 breakpoints of b per a-bin (independent: the same row)
    status: torch.Tensor   # [nsel, T] int32: 1 = sorted month
    na: int = 5
    nb: int = 5
    conditional: bool = False

    def _view(self, rec, nslab):
        S, T = int(self.status.shape[0]), int(self.status.shape[1])
        status = self.status[:, None, :].repeat(1, nslab, 1).view(S * nslab, T)   # (a copy: consumers read it by stride)
        return Portfolios(bp=None, port=None, rec=rec.view(S * nslab, T, rec.shape[-2], 4), cnt=None, status=status)

    @property
    def by_b(self):
        """The b portfolios within every a-bin and a-neutral, as a batched ``Portfolios`` whose sort axis
        is nsel * (na+1) (sort s, slab i at s * (na+1) + i), for ``portfolio_summary`` / ``portfolio_alphas``."""
        return self._view(self.rec_b, self.na + 1)

    @property
    def by_a(self):
        """The a portfolios within every b-bin and b-neutral: sort axis nsel * (nb+1)."""
        return self._view(self.rec_a, self.nb + 1)


def _dsort_levels(who, name, nbin, q):
    if not 2 <= nbin <= L.FM_MAX_DSORT:
        raise ValueError(f"{who}: n{name} must be 2..{L.FM_MAX_DSORT}, got {nbin}")
    qs = [float(v) for v in q] if q is not None else [k / nbin for k in range(1, nbin)]
    if len(qs) != nbin - 1:
        raise ValueError(f"{who}: q{name} must hold n{name} - 1 = {nbin - 1} levels, got {len(qs)}")
    if any(not (lo < v < 1.0) for lo, v in zip([0.0] + qs[:-1], qs)):
        raise ValueError(f"{who}: q{name} must be strictly ascending in (0, 1), got {qs}")
    return qs


def double_sort(seg_off, a, b, ret, weight=None, level=None, nyse=None, na=5, nb=5, qa=None, qb=None,
                conditional=False, min_level=0, nyse_breakpoints=False, min_count=None, min_count_bin=None,
                max_seg_len=None):
    """A21: per month (``seg_off`` int64 [T+1], rows sorted by month) sort the rows two ways, on ``a``
    into ``na`` bins and on ``b`` into ``nb`` -- independently, or with ``conditional`` b within each
    a-bin -- and average every cell's ``ret``, a and b, equal- and ``weight``-weighted, with each
    row's and column's high-minus-low spread and the a-neutral / b-neutral averages across the
    rows / columns (fm_portfolio_double_sort; the definition is in fm_hip.h).  ``a`` and ``b``: float64
    [n], or [nsel, n] for nsel sorts in one call ([n] beside [nsel, n] is shared by all of them).
    ``qa`` / ``qb``: the breakpoint levels (default k / na, k / nb); ``min_count`` (default na * nb):
    breakpoint rows a month needs; ``min_count_bin`` (default nb): those an a-bin needs, conditional
    only; ``max_seg_len``: the longest month if the caller knows it (else one host sync).  Plain
    device tensors in, ``DoubleSort`` out."""
    who = "double_sort"
    for t, what in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() not in (1, 2):
            raise ValueError(f"{who}: {what} must be a float64 [n] or [nsel, n] tensor")
    dev = a.device
    n = int(a.shape[-1])
    if int(b.shape[-1]) != n or b.device != dev:
        raise ValueError(f"{who}: a and b must have the same rows on one device, got {list(a.shape)} and {list(b.shape)}")
    batched = a.dim() == 2 or b.dim() == 2
    S = max(int(a.shape[0]) if a.dim() == 2 else 1, int(b.shape[0]) if b.dim() == 2 else 1)
    for t, what in ((a, "a"), (b, "b")):
        if t.dim() == 2 and int(t.shape[0]) != S:
            raise ValueError(f"{who}: {what} holds {int(t.shape[0])} sorts, the other signal {S}")
    seg_off, T = _months(who, seg_off, dev, "signals'")
    ret = _row_vector(who, ret, torch.float64, n, dev, "ret", required=True)
    weight = _row_vector(who, weight, torch.float64, n, dev, "weight")
    level = _row_vector(who, level, torch.uint8, n, dev, "level")
    nyse = _row_vector(who, nyse, torch.uint8, n, dev, "nyse")
    na, nb = int(na), int(nb)
    qa = _dsort_levels(who, "a", na, qa)
    qb = _dsort_levels(who, "b", nb, qb)
    min_count = na * nb if min_count is None else int(min_count)
    min_count_bin = nb if min_count_bin is None else int(min_count_bin)
    if min_count < 1 or min_count_bin < 1:
        raise ValueError(f"{who}: min_count and min_count_bin must be >= 1, got {min_count} and {min_count_bin}")
    if not 0 <= int(min_level) <= 255:
        raise ValueError(f"{who}: min_level must be 0..255, got {min_level}")
    if nyse_breakpoints and nyse is None:
        raise ValueError(f"{who}: nyse_breakpoints needs nyse")
    if S > 65535:
        raise ValueError(f"{who}: at most 65535 sorts per call, got {S}")
    a, b = a.contiguous(), b.contiguous()
    max_seg_len = _longest_month(seg_off, T, max_seg_len)

    empty, nan, f64, i32 = not (T and S), float("nan"), torch.float64, torch.int32
    out = DoubleSort(rec_b=_new_or_filled(empty, (S, na + 1, T, nb + 1, 4), f64, nan, dev),
                     rec_a=_new_or_filled(empty, (S, nb + 1, T, na + 1, 4), f64, nan, dev),
                     cnt=_new_or_filled(empty, (S, T, na, nb), i32, 0, dev),
                     cell=_new_or_filled(empty, (S, n), torch.uint8, 255, dev),
                     bpa=_new_or_filled(empty, (S, T, na - 1), f64, nan, dev),
                     bpb=_new_or_filled(empty, (S, T, na, nb - 1), f64, nan, dev),
                     status=_new_or_filled(empty, (S, T), i32, 0, dev), na=na, nb=nb, conditional=bool(conditional))
    args = L.DsortArgs(a=a.data_ptr(), b=b.data_ptr(), a_sort_stride=n if a.dim() == 2 else 0,
                       b_sort_stride=n if b.dim() == 2 else 0, ret=ret.data_ptr(), weight=_ptr(weight),
                       level=_ptr(level), nyse=_ptr(nyse), seg_off=seg_off.data_ptr(), nrows=n, nseg=T, nsel=S,
                       max_seg_len=max_seg_len, na=na, nb=nb, conditional=int(bool(conditional)),
                       min_level=int(min_level), nyse_breakpoints=int(bool(nyse_breakpoints)), min_count=min_count,
                       min_count_bin=min_count_bin, rec_b=out.rec_b.data_ptr(), rec_a=out.rec_a.data_ptr(),
                       cnt=out.cnt.data_ptr(), cell=out.cell.data_ptr(), bpa=out.bpa.data_ptr(),
                       bpb=out.bpb.data_ptr(), status=out.status.data_ptr())
    for j, v in enumerate(qa):
        args.qa[j] = v
    for j, v in enumerate(qb):
        args.qb[j] = v
    _kcall("fm_portfolio_double_sort", "fm_portfolio_double_sort", L.C.byref(args), _stream())
    _remember("fm_portfolio_double_sort", "fm_portfolio_double_sort", args, seg_off, a, b, ret, weight, level, nyse, out)
    return out


def double_sort_panel(panel: DevicePanel, a_col, b_cols, ret="retx", weight=None, level=None, nyse=None, **kw):
    """A21 on a panel: ``double_sort`` of the panel column ``a_col`` against every column of
    ``b_cols`` (a name or index, or a sequence of them: one sort each, in one launch, sharing a) with
    the panel column ``ret`` as the realised return.  ``weight``: a float64 [rows] vector, or "me" for
    the panel's market equity; ``nyse``: a uint8 [rows] vector, default the panel's own NYSE byte
    when ``nyse_breakpoints`` is asked for.  Further keywords are ``double_sort``'s."""
    single = isinstance(b_cols, (str, int))
    names = [b_cols] if single else list(b_cols)
    if not names:
        raise ValueError("double_sort_panel: b_cols is empty")
    if isinstance(weight, str):
        if weight != "me" or panel.me is None:
            raise ValueError("double_sort_panel: weight names the panel's 'me', which this panel must carry")
        weight = panel.me
    if nyse is None and kw.get("nyse_breakpoints"):
        nyse = panel.nyse
    a = column_vector(panel, a_col)
    if single:
        b = column_vector(panel, names[0])
    elif panel.cols is not None and all(isinstance(c, (str, int)) for c in names):
        idx = [panel.col(c) if isinstance(c, str) else int(c) for c in names]
        b = panel.cols[idx, :panel.nrows]
    else:
        b = torch.stack([column_vector(panel, c) for c in names])
    return double_sort(panel.seg_off, a, b, column_vector(panel, ret), weight=weight, level=level, nyse=nyse,
                       max_seg_len=kw.pop("max_seg_len", panel.max_seg_len), **kw)


def sort_factors(ds: DoubleSort, axis="b", weighted=True):
    """The neutral high-minus-low return series of every sort of ``ds`` as float64 [T, nsel], NaN in
    unsorted months: ``axis`` "b" the a-neutral spread of the b portfolios, "a" the b-neutral spread
    of the a portfolios; value- (``weighted``) or equal-weighted.  A view of the records (no kernel),
    in the shape ``portfolio_alphas`` takes as ``factors``."""
    if axis not in ("a", "b"):
        raise ValueError(f"sort_factors: axis must be 'a' or 'b', got {axis!r}")
    rec = ds.rec_b if axis == "b" else ds.rec_a
    return rec[:, -1, :, -1, 2 if weighted else 0].transpose(0, 1)


# ------------------------------------------------------------------------------------------
# Within-group (industry) adjustment of the characteristics (A20)
# ------------------------------------------------------------------------------------------
MAX_GROUPS = L.FM_MAX_GROUPS
GADJ_MODES = {"demean": L.FM_GADJ_DEMEAN, "mean": L.FM_GADJ_MEAN, "zscore": L.FM_GADJ_ZSCORE}


@dataclass
class GroupStats:
    mean: torch.Tensor             # [C, T, ngroups] float64: the group mean, NaN where n < max(1, min_count)
    sd: Optional[torch.Tensor]     # [C, T, ngroups] float64: the ddof-1 sd, NaN where n < 2 (mode "zscore" only)
    count: torch.Tensor            # [C, T, ngroups] int32: the group's eligible rows


def group_codes(labels):
    """Group labels (integers such as SIC codes, or strings) -> (codes int32, uniques): a sorted
    factorisation on the host, code k = the k-th smallest distinct label; a missing label (None,
    NaN, NaT) becomes -1, "no group"."""
    import pandas as pd
    codes, uniq = pd.factorize(np.asarray(labels) if not hasattr(labels, "dtype") else labels, sort=True)
    return np.asarray(codes).astype(np.int32), np.asarray(uniq)


def group_adjust_columns(seg_off, x, group, ngroups, mode="demean", min_count=1, level=None, min_level=0, out=None,
                         stats=False):
    """A20 on plain device tensors: every row of ``x`` (float64 [C, rows], rows sorted by month,
    months ``seg_off`` int64 [T+1]) adjusted within the groups ``group`` (int32 [rows], codes
    0..ngroups-1, any other value: no group) of each month -- ``mode`` "demean" x - group mean,
    "mean" the group mean, "zscore" (x - mean) / ddof-1 sd (fm_group_adjust; the definition is in
    fm_hip.h).  Groups with fewer than ``min_count`` rows, rows without a group and, with ``level``
    (uint8 [rows]), rows below ``min_level`` give NaN.  Returns (or fills ``out``) float64 [C, rows];
    with ``stats`` returns (out, GroupStats).  One launch, no host sync."""
    if mode not in GADJ_MODES:
        raise ValueError(f"group_adjust: mode must be one of {sorted(GADJ_MODES)}, got {mode!r}")
    ngroups = int(ngroups)
    if ngroups < 1 or ngroups > MAX_GROUPS:
        raise ValueError(f"group_adjust: ngroups must be 1..{MAX_GROUPS}, got {ngroups}")
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or min_count < 0:
        raise ValueError(f"group_adjust: min_count must be an integer >= 0, got {min_count!r}")
    if x.dtype != torch.float64 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("group_adjust: x must be a float64 [C, rows] tensor with contiguous rows")
    dev = x.device
    C, n = int(x.shape[0]), int(x.shape[1])
    seg_off, T = _months("group_adjust", seg_off, dev, "values'")
    group = _row_vector("group_adjust", group, torch.int32, n, dev, "group", required=True)
    level = _row_vector("group_adjust", level, torch.uint8, n, dev, "level")
    if out is None:
        out = torch.empty((C, n), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (C, n) or out.device != dev or \
            (n > 1 and out.stride(1) != 1):
        raise ValueError(f"group_adjust: out must be a float64 [{C}, {n}] tensor on {dev} with contiguous rows")
    if out.data_ptr() == x.data_ptr() and C * n:
        raise ValueError("group_adjust: out must not be the input's own memory")
    empty = not (C and n and T)
    st = None
    if stats:
        sh, nan = (C, T, ngroups), float("nan")
        st = GroupStats(mean=_new_or_filled(empty, sh, torch.float64, nan, dev),
                        sd=_new_or_filled(empty, sh, torch.float64, nan, dev) if mode == "zscore" else None,
                        count=_new_or_filled(empty, sh, torch.int32, 0, dev))
    a = L.GroupAdjArgs(src=x.data_ptr(), src_stride=x.stride(0) if C > 1 else max(n, 1), dst=out.data_ptr(),
                       dst_stride=out.stride(0) if C > 1 else max(n, 1), seg_off=seg_off.data_ptr(),
                       group=group.data_ptr(), level=_ptr(level), nrows=n, ncols=C, nseg=T, ngroups=ngroups,
                       mode=GADJ_MODES[mode], min_count=int(min_count), min_level=int(min_level),
                       gcount=None if st is None else st.count.data_ptr(),
                       gmean=None if st is None else st.mean.data_ptr(),
                       gsd=None if st is None or st.sd is None else st.sd.data_ptr())
    _kcall("fm_group_adjust", "fm_group_adjust", L.C.byref(a), _stream())
    _remember("fm_group_adjust", "fm_group_adjust", a, x, out, seg_off, group, level, st)
    return (out, st) if stats else out


def group_adjust(panel: DevicePanel, cols=None, mode="demean", min_count=1, level=None, min_level=0, out=None,
                 stats=False):
    """A20 on a panel: the chosen columns (names or indices; default all) adjusted within the panel's
    groups (``panel.group``, ``panel.ngroups``) of each month (``group_adjust_columns``), every other
    column copied unchanged.  Returns a new f64-layout ``DevicePanel`` that shares the input's
    segments, ``me``, ``nyse``, ``months``, ``order``, ``group``, ``ids``, ``month_index`` and links
    (``out``: its [C, n] float64 column block, not the input's), as ``rank_transform`` does; with
    ``stats`` the chosen columns' ``GroupStats`` ([len(cols), T, ngroups]) is its ``group_stats``
    attribute."""
    if mode not in GADJ_MODES:
        raise ValueError(f"group_adjust: mode must be one of {sorted(GADJ_MODES)}, got {mode!r}")
    if panel.group is None:
        raise ValueError("group_adjust: the panel carries no group codes (build it with group=...)")
    src = panel.values()
    C, n = panel.ncols, panel.nrows
    idx = list(range(C)) if cols is None else [panel.col(c) if isinstance(c, str) else int(c) for c in cols]
    if any(i < 0 or i >= C for i in idx) or len(set(idx)) != len(idx):
        raise ValueError("group_adjust: cols must be distinct columns of the panel")
    if out is None:
        out = torch.empty_like(src)
    elif out.dtype != torch.float64 or out.shape != src.shape or out.device != src.device or out.stride(1) != 1:
        raise ValueError("group_adjust: out must be a float64 tensor of the panel's [C, n] shape on its device")
    if out.data_ptr() == src.data_ptr():
        raise ValueError("group_adjust: out must not be the panel's own columns")
    for i in sorted(set(range(C)) - set(idx)):
        out[i].copy_(src[i])
    # consecutive columns go in one launch (all 14 predictors of the pipeline: one)
    runs, k = [], 0
    while k < len(idx):
        e = k + 1
        while e < len(idx) and idx[e] == idx[e - 1] + 1:
            e += 1
        runs.append((k, e))
        k = e
    parts = []
    for k, e in runs:
        r = group_adjust_columns(panel.seg_off, src[idx[k]:idx[k] + e - k, :n], panel.group, panel.ngroups, mode=mode,
                                 min_count=min_count, level=level, min_level=min_level,
                                 out=out[idx[k]:idx[k] + e - k, :n], stats=stats)
        if stats:
            parts.append(r[1])
    res = DevicePanel(cols=out, names=list(panel.names), seg_off=panel.seg_off, seg_off_h=panel.seg_off_h,
                      months=panel.months, me=panel.me, nyse=panel.nyse, order=panel.order,
                      chunk_rows=panel.chunk_rows, chunk_split=panel.chunk_split, chunk_policy=panel.chunk_policy,
                      row_origin=panel.row_origin, group=panel.group, ngroups=panel.ngroups, ids=panel.ids,
                      month_index=panel.month_index)
    _share_links(panel, res)
    if stats:
        cat = (lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)) if parts else None
        res.group_stats = None if not parts else GroupStats(
            mean=cat([p.mean for p in parts]), sd=None if parts[0].sd is None else cat([p.sd for p in parts]),
            count=cat([p.count for p in parts]))
    return res


def segment_moments(panel: DevicePanel, level=None, min_level=0, finite_only=True, cols=None):
    """Per (column, month) count, mean and ddof=1 std of the non-missing values."""
    src = panel.values() if cols is None else cols
    C, T = src.shape[0], panel.nseg
    cnt = torch.empty((C, T), dtype=torch.int32, device=src.device)
    mean = torch.empty((C, T), dtype=torch.float64, device=src.device)
    sd = torch.empty_like(mean)
    _kcall("fm_segment_moments", "fm_segment_moments", src.data_ptr(), src.stride(0), C,
           panel.seg_off.data_ptr(), T, _ptr(level), int(min_level), int(bool(finite_only)),
           cnt.data_ptr(), mean.data_ptr(), sd.data_ptr(), _stream())
    return cnt, mean, sd


def distinct_count(ids, cols, level=None, min_level=0, finite_only=True):
    """Number of distinct ids among rows where each column is present -> int32 [C]."""
    C, n = cols.shape
    dev = cols.device
    out = torch.empty(C, dtype=torch.int32, device=dev)
    if n == 0:
        out.zero_()
        return out
    lo = int(ids.min().item())
    rng = int(ids.max().item()) - lo + 1
    bitmap = torch.empty((C, (rng + 31) // 32), dtype=torch.int32, device=dev)
    _kcall("fm_distinct_count", "fm_distinct_count", ids.data_ptr(), n, cols.data_ptr(), cols.stride(0), C,
           _ptr(level), int(min_level), int(bool(finite_only)), lo, rng, bitmap.data_ptr(), out.data_ptr(),
           _stream())
    return out


# ------------------------------------------------------------------------------------------
# Firm-axis characteristics (src/calc_Lewellen_2014.py:137-466)
# ------------------------------------------------------------------------------------------
CHAR_FIELDS = ("me", "be", "retx", "accruals", "depreciation", "earnings", "assets", "dvc", "prc",
               "shrout", "total_debt", "sales")
CHAR_NAMES = ("log_size", "log_bm", "return_12_2", "accruals_final", "roa", "log_assets_growth",
              "dy", "log_return_13_36", "log_issues_12", "log_issues_36", "debt_price", "sales_price")


def _check_ids(ids):
    """Firm ids are read as raw int64 words: reject any other dtype / layout."""
    if ids.dtype != torch.int64 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError("firm ids must be a contiguous int64 [n] tensor")


def firm_chars(ids, fields, names=CHAR_NAMES, out=None):
    """Monthly characteristics for FIRM-major rows (each firm's rows contiguous, in frame
    order).  ``ids`` int64 [n]; ``fields`` maps CHAR_FIELDS names -> float64 [n] device
    tensors (only those the requested characteristics read); returns {name: float64 [n]}.
    ``out`` (optional) is a [len(names), n] float64 tensor to write into."""
    n = int(ids.shape[0])
    dev = ids.device
    _check_ids(ids)
    if out is None:
        out = torch.empty((len(names), n), dtype=torch.float64, device=dev)
    if out.dtype != torch.float64 or out.dim() != 2 or out.shape != (len(names), n) or out.stride(1) != 1:
        raise ValueError("firm_chars: out must be float64 [len(names), n] with contiguous rows")
    a = L.CharsArgs()
    a.ids = ids.data_ptr()
    a.n = n
    keep = [ids, out]
    for f, nm in enumerate(CHAR_FIELDS):
        t = fields.get(nm)
        if t is not None:
            if t.dtype != torch.float64 or t.dim() != 1 or t.shape[0] != n or t.device != dev:
                raise ValueError(f"firm_chars: field {nm!r} must be a float64 [{n}] tensor on {dev}")
            t = t.contiguous()
            keep.append(t)
            a.field[f] = t.data_ptr()
    for j, nm in enumerate(names):
        a.out[CHAR_NAMES.index(nm)] = out[j].data_ptr()
    _remember("fm_firm_chars", "fm_firm_chars", a, *keep)
    _kcall("fm_firm_chars", "fm_firm_chars", L.C.byref(a), _stream())
    return {nm: out[j] for j, nm in enumerate(names)}


def rolling_std(ids, x, window=252, min_periods=100, scale=252 ** 0.5, out=None):
    """Per-row rolling std (ddof=1) over the last ``window`` rows of each firm group."""
    n = int(x.shape[0])
    _check_ids(ids)
    if x.dtype != torch.float64 or x.dim() != 1 or ids.shape[0] != n or x.device != ids.device:
        raise ValueError("rolling_std: x must be a float64 [n] tensor beside int64 [n] ids")
    x = x.contiguous()
    # fm_rolling_std moves row pairs with 16-byte accesses: views at odd offsets are copied
    if x.data_ptr() % 16:
        x = x.clone()
    if ids.data_ptr() % 16 or not ids.is_contiguous():
        ids = ids.clone()
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=x.device)
    if out.dtype != torch.float64 or out.shape != (n,) or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError("rolling_std: out must be a contiguous, 16-byte aligned float64 [n] tensor")
    args = (ids.data_ptr(), x.data_ptr(), n, int(window), int(min_periods), float(scale), out.data_ptr())
    _kcall("fm_rolling_std", "fm_rolling_std", *args, _stream())
    LAST_LAUNCH["fm_rolling_std"] = ("fm_rolling_std", None, ((ids, x, out), args))
    return out


def rolling_beta(day, ri, rm, seg_off, q_seg, q_day0, q_day1, period_weeks=156):
    """fm_rolling_beta on device tensors: day int32 [n], ri / rm float64 [n] (firm-major,
    days ascending per firm), seg_off int64 [nseg+1]; queries int32 [nq]; -> float64 [nq]."""
    n = int(day.shape[0])
    for t, dt in ((day, torch.int32), (ri, torch.float64), (rm, torch.float64), (seg_off, torch.int64),
                  (q_seg, torch.int32), (q_day0, torch.int32), (q_day1, torch.int32)):
        if t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"rolling_beta: expected contiguous {dt} vectors")
    if ri.shape[0] != n or rm.shape[0] != n:
        raise ValueError("rolling_beta: day / ri / rm lengths differ")
    nq = int(q_seg.shape[0])
    out = torch.empty(nq, dtype=torch.float64, device=day.device)
    ws = torch.empty((5, max(n, 1)), dtype=torch.float64, device=day.device)
    _kcall("fm_rolling_beta", "fm_rolling_beta", day.data_ptr(), ri.data_ptr(), rm.data_ptr(), n,
           seg_off.data_ptr(), int(seg_off.shape[0]) - 1, int(period_weeks) * 7, q_seg.data_ptr(),
           q_day0.data_ptr(), q_day1.data_ptr(), nq, ws.data_ptr(), out.data_ptr(), _stream())
    return out


def stream_probe(t):
    """fm_stream_probe: the sum of a contiguous, 16-byte aligned float64 tensor read as a
    plain HBM stream (bench.py's measured read rate; re-issued by time_launch)."""
    if t.dtype != torch.float64 or not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError("stream_probe: a contiguous, 16-byte aligned float64 tensor")
    out = torch.zeros(1, dtype=torch.float64, device=t.device)
    args = (t.data_ptr(), t.numel(), out.data_ptr())
    _kcall("fm_stream_probe", "fm_stream_probe", *args, _stream())
    LAST_LAUNCH["fm_stream_probe"] = ("fm_stream_probe", None, ((t, out), args))
    return out


def stream_copy_probe(src, dst):
    """fm_stream_copy_probe: dst <- src (contiguous, 16-byte aligned float64 tensors of one
    size) as the probe's 16-byte stream (bench.py's measured copy rate; re-issued by
    time_launch)."""
    for t in (src, dst):
        if t.dtype != torch.float64 or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("stream_copy_probe: contiguous, 16-byte aligned float64 tensors")
    if src.numel() != dst.numel() or src.device != dst.device:
        raise ValueError("stream_copy_probe: src and dst must match in size and device")
    args = (src.data_ptr(), dst.data_ptr(), src.numel())
    _kcall("fm_stream_copy_probe", "fm_stream_copy_probe", *args, _stream())
    LAST_LAUNCH["fm_stream_copy_probe"] = ("fm_stream_copy_probe", None, ((src, dst), args))
    return dst
