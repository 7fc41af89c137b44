"""Timing of fm_forecast_dist on the pipeline's Table-3 workload (600 months x 5,000 firms x 15
columns, the nine Table-2 sorts = Models 1/2/3 x three universes, q = (0.1, 0.9), the pipeline's
cuts and levels), beside what it replaces and beside the fused sort, all from one process:
python tools/fdistbench.py [--months 600] [--firms 5000]
  * the launch on an f64 panel and on a planes-only panel (engine.time_launch, three windows each);
  * the composition of the entry points that existed before it, on the same inputs: fm_clip of the
    panel, then per sort fm_forecast on its (already gathered) clipped columns, fm_segment_moments
    of the vector and fm_portfolio_sort(nport = 3, q = (0.1, 0.9)) for the two percentiles -- the
    kernels only, re-issued from prebuilt arguments, no gathers and no allocation in the window;
  * fm_forecast_portfolio_sort (nport = 10, value weights) for the same nine sorts;
  * fm_stream_probe's read rate over a 1 GiB tensor (the measured HBM read peak).
Bytes (n rows, C columns, sort j with K_j predictors, S sorts, U the columns some sort reads):
  dist, as launched:   sum_j n (8 K_j + 1)                 predictors and the level byte, once per sort;
  dist, unique:        n (8 U + 1)                         every input once;
  composition:         2 * 8 C n (clip) + sum_j 8 n (K_j + 1) (forecast) + S n (8 + 1) (moments)
                       + S n (8 + 8 + 1 + 1) (sort: forecast, return, level, portfolio byte);
  fused sort, as launched: pipeportbench's formula.
The launch's outputs are checked bit for bit against fm_clip -> fm_forecast -> the plain source
(and its percentiles against the composition's breakpoints) before anything is timed.
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

Q = (0.1, 0.9)


def spread(v):
    return round(float(max(v) - min(v)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=600)
    ap.add_argument("--firms", type=int, default=5000)
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

    # ---- the launch, both layouts
    dist, outs = {}, {}
    for name, p in (("f64", panel), ("planes", planes)):
        outs[name] = E.forecast_dist(p, coef, sel, cuts=cuts, level=level, q=Q)
        dist[name] = [E.time_launch("fm_forecast_dist", a.reps) * 1e3 for _ in range(3)]
    assert planes.cols is None and "_merged" not in planes.__dict__   # no FP64 copy was made

    # ---- the fused sort of the same nine sorts
    E.forecast_portfolio_sort(panel, coef, sel, cuts=cuts, ret=ret, weight=panel.me, level=level, nyse=panel.nyse, nport=10)
    fsort = [E.time_launch("fm_forecast_portfolio_sort", a.reps) * 1e3 for _ in range(3)]

    # ---- the composition: clip, then per sort forecast + moments + a three-portfolio sort
    st = E._stream()
    clipped = torch.empty_like(panel.cols)
    E.clip(panel, cuts, out=clipped)
    gathered = [clipped[xs].contiguous() for xs, _ in sel]
    cj = [coef[j, :, :len(xs) + 1].contiguous() for j, (xs, _) in enumerate(sel)]
    Fs = torch.empty((S, n), dtype=torch.float64, device=dev)
    mcnt = torch.empty((S, T), dtype=torch.int32, device=dev)
    mmean, msd = (torch.empty((S, T), dtype=torch.float64, device=dev) for _ in range(2))
    pargs, pouts = [], []

    def forecast_and_moments(j):
        xs, u = sel[j]
        L.call("fm_forecast", gathered[j].data_ptr(), gathered[j].stride(0), len(xs), panel.seg_off.data_ptr(), T, n,
               cj[j].data_ptr(), cj[j].stride(0), Fs[j].data_ptr(), st)
        L.call("fm_segment_moments", Fs[j].data_ptr(), n, 1, panel.seg_off.data_ptr(), T, level.data_ptr(), u, 1,
               mcnt[j].data_ptr(), mmean[j].data_ptr(), msd[j].data_ptr(), st)

    for j, (xs, u) in enumerate(sel):
        forecast_and_moments(j)
        pouts.append(E.portfolio_sort(panel.seg_off, Fs[j], panel.cols[ret], level=level, nport=3, q=Q, min_level=u,
                                      max_seg_len=panel.max_seg_len))
        pargs.append(E.LAST_LAUNCH["fm_portfolio_sort"][1])
    ref = E.forecast_dist_vector(panel.seg_off, Fs, level=level, min_level=[u for _, u in sel], q=Q,
                                 max_seg_len=panel.max_seg_len)
    torch.cuda.synchronize()
    for name in dist:
        for k in ("rec", "cnt", "status"):
            assert torch.equal(getattr(ref, k).view(torch.uint8), getattr(outs[name], k).view(torch.uint8)), (name, k)
    d = outs["f64"]
    assert bool(d.status.all()) and torch.equal(d.cnt, mcnt)
    assert torch.equal(torch.stack([p.bp for p in pouts]), d.rec[:, :, 2:])
    for got, exp in ((d.rec[:, :, 0], mmean), (d.rec[:, :, 1], msd)):
        assert bool(((got - exp).abs() <= 1e-9 * exp.abs().clamp_min(float(exp.square().mean().sqrt()))).all())

    def composition():
        L.call("fm_clip", panel.cols.data_ptr(), clipped.data_ptr(), panel.cols.stride(0), C, panel.seg_off.data_ptr(),
               T, n, cuts.lo.data_ptr(), cuts.hi.data_ptr(), st)
        for j in range(S):
            forecast_and_moments(j)
            L.call("fm_portfolio_sort", L.C.byref(pargs[j]), st)

    comp_us = [timed(composition, a.reps) for _ in range(3)]

    big = torch.ones(1 << 27, dtype=torch.float64, device=dev)
    E.stream_probe(big)
    probe_ms = min(E.time_launch("fm_stream_probe", 50) for _ in range(3))
    peak = big.numel() * 8 / (probe_ms * 1e-3)
    sumk = sum(len(xs) for xs, _ in sel)
    U = len({c for xs, _ in sel for c in xs})
    b_launched = n * (8 * sumk + S)
    b_unique = n * (8 * U + 1)
    b_comp = 2 * 8 * C * n + 8 * n * (sumk + S) + S * n * 9 + S * n * 18
    b_fsort = n * (8 * (sumk + S) + S * (8 + 3))
    med = {k: float(np.median(v)) for k, v in dist.items()}
    med_sort, med_comp = float(np.median(fsort)), float(np.median(comp_us))
    print(json.dumps({
        "shape": [a.months, a.firms, C], "sorts": S, "q": list(Q),
        "dist_us_f64": [round(v, 1) for v in dist["f64"]], "dist_us_planes": [round(v, 1) for v in dist["planes"]],
        "fused_sort_us_f64": [round(v, 1) for v in fsort], "composition_us": [round(v, 1) for v in comp_us],
        "spread_us": {"dist_f64": spread(dist["f64"]), "dist_planes": spread(dist["planes"]),
                      "fused_sort": spread(fsort), "composition": spread(comp_us)},
        "composition_over_dist_f64": round(med_comp / med["f64"], 2),
        "composition_over_dist_planes": round(med_comp / med["planes"], 2),
        "fused_sort_over_dist_f64": round(med_sort / med["f64"], 2),
        "dist_bytes_as_launched": b_launched, "dist_bytes_unique": b_unique, "composition_bytes": b_comp,
        "fused_sort_bytes_as_launched": b_fsort,
        "stream_probe_read_TBps": round(peak / 1e12, 3),
        "dist_f64_fraction_of_read_peak_as_launched": round(b_launched / peak * 1e6 / med["f64"], 3),
        "dist_f64_fraction_of_read_peak_unique": round(b_unique / peak * 1e6 / med["f64"], 3),
        "dist_planes_fraction_of_read_peak_as_launched": round(b_launched / peak * 1e6 / med["planes"], 3),
        "fused_sort_fraction_of_read_peak_as_launched": round(b_fsort / peak * 1e6 / med_sort, 3),
        "composition_fraction_of_read_peak": round(b_comp / peak * 1e6 / med_comp, 3),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
