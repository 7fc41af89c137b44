"""Timing of fm_portfolio_sort on the headline shape (600 months x 5,000 firms, nport = 10,
value weights, universe levels, NYSE breakpoints off), beside the two numbers it is read
against, all from one process: python tools/portbench.py [--months 600] [--firms 5000]
  * fm_stream_probe's read rate over a 1 GiB tensor (the measured HBM read peak);
  * fm_universe (universe_kernel<20>: universe_month<20>, the month routine that
    select_fixup_universe_kernel<20> runs), the existing one-workgroup-per-month kernel.
The forecasts are fm_forecast's over three synthetic characteristics.  Two timings of the
sort: re-issued back to back on one input set (81 MB: it stays in the Infinity Cache), and
rotating over input sets that together exceed the cache (every launch reads from HBM).
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fm-returnprediction_amd"))

from fmcore import engine as E  # noqa: E402
from fmcore import _lib as L  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=600)
    ap.add_argument("--firms", type=int, default=5000)
    ap.add_argument("--nport", type=int, default=10)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--sets", type=int, default=6)
    a = ap.parse_args()
    dev = E.require_device()
    panel = E.panel_synthetic(a.months, a.firms, 1234)
    T, n = panel.nseg, panel.nrows
    _, _, level = E.universe(panel)
    coef = torch.tensor([0.01, 0.002, 0.004, -0.003], dtype=torch.float64, device=dev).repeat(T, 1)
    x = panel.cols[1:4]
    F = E.forecast(panel, coef, cols=x)
    R, W = panel.cols[0], panel.me
    kw = dict(nport=a.nport, min_level=0, max_seg_len=panel.max_seg_len)
    p = E.portfolio_sort(panel.seg_off, F, R, weight=W, level=level, nyse=panel.nyse, **kw)
    torch.cuda.synchronize()
    sorted_months = int(p.status.sum().item())
    nbytes = n * (3 * 8 + 2 + 1)
    # warm: the same inputs re-issued (three windows for the spread)
    warm = [E.time_launch("fm_portfolio_sort", a.reps) * 1e3 for _ in range(3)]
    uni = [E.time_launch("fm_universe", a.reps) * 1e3 for _ in range(3)]
    # cold: rotate over input sets larger than the Infinity Cache together
    sets = [tuple(t.clone() for t in (F, R, W, level, panel.nyse)) for _ in range(a.sets)]
    args = []
    outs = []
    for f, r, w, lv, ny in sets:
        q = E.portfolio_sort(panel.seg_off, f, r, weight=w, level=lv, nyse=ny, **kw)
        outs.append(q)
        args.append(E.LAST_LAUNCH["fm_portfolio_sort"][1])
    st = E._stream()
    it = [0]

    def rot():
        L.call("fm_portfolio_sort", L.C.byref(args[it[0] % len(args)]), st)
        it[0] += 1

    cold = [timed(rot, a.reps) for _ in range(3)]
    me_sets = [(s[2], s[4], torch.empty(T, dtype=torch.float64, device=dev), torch.empty(T, dtype=torch.float64, device=dev),
                torch.empty(n, dtype=torch.uint8, device=dev)) for s in sets]

    def rot_u():
        me, ny, ca, cb, lv = me_sets[it[0] % len(me_sets)]
        L.call("fm_universe", me.data_ptr(), ny.data_ptr(), panel.seg_off.data_ptr(), T, panel.max_seg_len, 0.2, 0.5,
               ca.data_ptr(), cb.data_ptr(), lv.data_ptr(), st)
        it[0] += 1

    uni_cold = [timed(rot_u, a.reps) for _ in range(3)]
    big = torch.ones(1 << 27, dtype=torch.float64, device=dev)
    E.stream_probe(big)
    probe_ms = min(E.time_launch("fm_stream_probe", 50) for _ in range(3))
    peak = big.numel() * 8 / (probe_ms * 1e-3)
    floor_us = nbytes / peak * 1e6
    print(json.dumps({
        "shape": [a.months, a.firms, a.nport], "sorted_months": sorted_months, "algorithmic_bytes": nbytes,
        "port_us_warm": [round(v, 2) for v in warm], "port_us_hbm": [round(v, 2) for v in cold],
        "universe_us_warm": [round(v, 2) for v in uni], "universe_us_hbm": [round(v, 2) for v in uni_cold],
        "universe_bytes": n * (8 + 1 + 1),
        "stream_probe_read_TBps": round(peak / 1e12, 3), "port_floor_us": round(floor_us, 2),
        "port_fraction_of_read_peak_hbm": round(floor_us / float(np.median(cold)), 3),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
