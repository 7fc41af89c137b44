"""Timing of fm_forecast_portfolio_sort on the pipeline's Table-5 workload (600 months x 5,000
firms x 15 columns, the nine Table-2 sorts = Models 1/2/3 x three universes, nport = 10, value
weights), beside what it replaces, all from one process:
python tools/pipeportbench.py [--months 600] [--firms 5000]
  * the fused launch on an f64 panel and on a planes-only panel (engine.time_launch, three
    windows each);
  * the composition of the existing entry points on the same inputs: fm_clip of the panel, then
    per sort fm_forecast on its (already gathered) clipped columns and fm_portfolio_sort -- the
    kernels only, re-issued from prebuilt arguments, no gathers and no allocation in the window;
  * fm_stream_probe's read rate over a 1 GiB tensor (the measured HBM read peak).
Bytes (n rows, C columns, sort j with K_j predictors, S sorts):
  fused, as launched:  sum_j n (8 (K_j + 1) + 8 + 1 + 1 + 1)   predictors + return, weight, level,
                       NYSE byte, portfolio byte, once per sort;
  fused, unique:       n (8 C + 8 + 1 + 1) + S n               every input once + the portfolio bytes;
  composition:         2 * 8 C n (clip) + sum_j 8 n (K_j + 2) (forecast) + S n (3 * 8 + 2 + 1) (sort);
  extra HBM of the composition: the clipped panel 8 C n, S forecast vectors 8 n each, the
                       gathered columns 8 n sum_j K_j and, for a planes-only panel, its merged FP64
                       copy 8 C n.
The fused outputs are checked against the composition's bit for bit before anything is timed.
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
from fmcore import lewellen as LW  # noqa: E402
from fmcore import _lib as L  # noqa: E402

from portbench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=600)
    ap.add_argument("--firms", type=int, default=5000)
    ap.add_argument("--nport", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = E.require_device()
    panel = E.panel_synthetic(a.months, a.firms, 1234)
    planes = E.panel_synthetic(a.months, a.firms, 1234, layout="planes")
    T, n, C = panel.nseg, panel.nrows, panel.ncols
    cuts, (_, _, level) = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY, universe=(0.2, 0.5))
    sel = [([panel.col(c) for c in xs], u) for xs in LW.table2_models().values() for u in (0, 1, 2)]
    S, pmax = len(sel), 1 + max(len(xs) for xs, _ in sel)
    g = torch.Generator(device="cpu").manual_seed(5)
    coef = (torch.randn((S, T, pmax), generator=g, dtype=torch.float64) * 0.01).to(dev)
    ret = panel.col("retx")
    kw = dict(cuts=cuts, ret=ret, weight=panel.me, level=level, nyse=panel.nyse, nport=a.nport)

    # ---- the fused launch, both layouts
    fused = {}
    outs = {}
    for name, p in (("f64", panel), ("planes", planes)):
        outs[name] = E.forecast_portfolio_sort(p, coef, sel, **kw)
        fused[name] = [E.time_launch("fm_forecast_portfolio_sort", a.reps) * 1e3 for _ in range(3)]
    assert planes.cols is None and "_merged" not in planes.__dict__   # no FP64 copy was made

    # ---- the composition: clip, then per sort forecast + sort, from prebuilt arguments
    st = E._stream()
    clipped = torch.empty_like(panel.cols)
    E.clip(panel, cuts, out=clipped)
    gathered = [clipped[xs].contiguous() for xs, _ in sel]
    cj = [coef[j, :, :len(xs) + 1].contiguous() for j, (xs, _) in enumerate(sel)]
    Fs = [torch.empty(n, dtype=torch.float64, device=dev) for _ in sel]
    pargs, pouts = [], []
    for j, (xs, u) in enumerate(sel):
        L.call("fm_forecast", gathered[j].data_ptr(), gathered[j].stride(0), len(xs), panel.seg_off.data_ptr(), T, n,
               cj[j].data_ptr(), cj[j].stride(0), Fs[j].data_ptr(), st)
        pouts.append(E.portfolio_sort(panel.seg_off, Fs[j], panel.cols[ret], weight=panel.me, level=level,
                                      nyse=panel.nyse, nport=a.nport, min_level=u, max_seg_len=panel.max_seg_len))
        pargs.append(E.LAST_LAUNCH["fm_portfolio_sort"][1])
    torch.cuda.synchronize()
    for k in ("bp", "port", "rec", "cnt", "status"):
        comp = torch.stack([getattr(q, k) for q in pouts])
        for name in fused:
            assert torch.equal(comp.view(torch.uint8), getattr(outs[name], k).contiguous().view(torch.uint8)), (name, k)

    def composition():
        L.call("fm_clip", panel.cols.data_ptr(), clipped.data_ptr(), panel.cols.stride(0), C, panel.seg_off.data_ptr(),
               T, n, cuts.lo.data_ptr(), cuts.hi.data_ptr(), st)
        for j, (xs, _) in enumerate(sel):
            L.call("fm_forecast", gathered[j].data_ptr(), gathered[j].stride(0), len(xs), panel.seg_off.data_ptr(), T,
                   n, cj[j].data_ptr(), cj[j].stride(0), Fs[j].data_ptr(), st)
            L.call("fm_portfolio_sort", L.C.byref(pargs[j]), st)

    comp_us = [timed(composition, a.reps) for _ in range(3)]

    big = torch.ones(1 << 27, dtype=torch.float64, device=dev)
    E.stream_probe(big)
    probe_ms = min(E.time_launch("fm_stream_probe", 50) for _ in range(3))
    peak = big.numel() * 8 / (probe_ms * 1e-3)
    sumk = sum(len(xs) for xs, _ in sel)
    b_launched = n * (8 * (sumk + S) + S * (8 + 3))
    b_unique = n * (8 * C + 8 + 1 + 1) + S * n
    b_comp = 2 * 8 * C * n + 8 * n * (sumk + 2 * S) + S * n * (3 * 8 + 2 + 1)
    extra = 8 * C * n + 8 * n * S + 8 * n * sumk
    med = {k: float(np.median(v)) for k, v in fused.items()}
    print(json.dumps({
        "shape": [a.months, a.firms, C], "sorts": S, "nport": a.nport,
        "sorted_months": int(outs["f64"].status.sum().item()),
        "fused_us_f64": [round(v, 1) for v in fused["f64"]], "fused_us_planes": [round(v, 1) for v in fused["planes"]],
        "composition_us": [round(v, 1) for v in comp_us],
        "speedup_f64": round(float(np.median(comp_us)) / med["f64"], 2),
        "speedup_planes": round(float(np.median(comp_us)) / med["planes"], 2),
        "fused_bytes_as_launched": b_launched, "fused_bytes_unique": b_unique, "composition_bytes": b_comp,
        "composition_extra_hbm_bytes": extra, "composition_extra_hbm_bytes_planes_only": extra + 8 * C * n,
        "stream_probe_read_TBps": round(peak / 1e12, 3),
        "fused_f64_fraction_of_read_peak_as_launched": round(b_launched / peak * 1e6 / med["f64"], 3),
        "fused_f64_fraction_of_read_peak_unique": round(b_unique / peak * 1e6 / med["f64"], 3),
        "fused_planes_fraction_of_read_peak_as_launched": round(b_launched / peak * 1e6 / med["planes"], 3),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
