"""Timing of fm_forecast_compare on the pipeline's Table-4 workload (600 months x 5,000 firms x 15
columns; the nine pairs = model j on model i for i < j of Models 1/2/3, in each of the three
universes; the pipeline's cuts and levels), beside fm_forecast_dist for the nine sorts the pairs
are made of, from one process with the two launches' windows alternating:
python tools/fcmpbench.py [--months 600] [--firms 5000]
  * both launches on an f64 panel and on a planes-only panel (engine.time_launch, three windows each);
  * fm_stream_probe's read rate over a 1 GiB tensor (the measured HBM read peak).
Bytes (n rows, pair p of forecasts with K_a and K_b predictors):
  compare, as launched: sum_p n (8 (K_a + K_b) + 8 + 1)    both forecasts' predictors, the return and
                                                           the level byte, once per pair;
  dist, as launched:    sum_j n (8 K_j + 1)                 (tools/fdistbench.py).
The launch's outputs are checked bit for bit against its own forecast vectors through the plain
source, and those vectors against fm_forecast_dist's, before anything is timed.
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
    models = list(LW.table2_models().values())
    sel = [([panel.col(c) for c in xs], u) for xs in models for u in (0, 1, 2)]
    M, S = len(models), len(sel)
    pairs = [(3 * i + u, 3 * j + u, u) for u in (0, 1, 2) for i in range(M) for j in range(i + 1, M)]
    pmax = 1 + max(len(xs) for xs, _ in sel)
    g = torch.Generator(device="cpu").manual_seed(5)
    coef = (torch.randn((S, T, pmax), generator=g, dtype=torch.float64) * 0.01).to(dev)
    ret = panel.col("retx")

    # ---- the bits first: fused == its own forecasts through the plain source, on both layouts
    outs = {}
    for name, p in (("f64", panel), ("planes", planes)):
        outs[name] = E.forecast_compare(p, coef, sel, pairs, cuts=cuts, ret=ret, level=level, forecast_out=True)
    dist = E.forecast_dist(panel, coef, sel, cuts=cuts, level=level, forecast_out=True)
    ref = E.forecast_compare_vector(panel.seg_off, outs["f64"].forecast, panel.cols[ret], pairs, level=level,
                                    max_seg_len=panel.max_seg_len)
    torch.cuda.synchronize()
    assert torch.equal(dist.forecast.view(torch.int64), outs["f64"].forecast.view(torch.int64))
    for name in outs:
        for k in ("rec", "cnt", "status"):
            assert torch.equal(getattr(ref, k).view(torch.uint8), getattr(outs[name], k).view(torch.uint8)), (name, k)
    assert bool(ref.status.all()) and bool(torch.isfinite(ref.rec).all())
    del outs, dist, ref

    # ---- the two launches as the pipeline issues them (no forecast vectors), windows alternating
    cmp_us = {"f64": [], "planes": []}
    dist_us = {"f64": [], "planes": []}
    for name, p in (("f64", panel), ("planes", planes)):
        E.forecast_compare(p, coef, sel, pairs, cuts=cuts, ret=ret, level=level)
        E.forecast_dist(p, coef, sel, cuts=cuts, level=level)
        for _ in range(3):
            cmp_us[name].append(E.time_launch("fm_forecast_compare", a.reps) * 1e3)
            dist_us[name].append(E.time_launch("fm_forecast_dist", a.reps) * 1e3)
    assert planes.cols is None and "_merged" not in planes.__dict__   # no FP64 copy was made

    big = torch.ones(1 << 27, dtype=torch.float64, device=dev)
    E.stream_probe(big)
    probe_ms = min(E.time_launch("fm_stream_probe", 50) for _ in range(3))
    peak = big.numel() * 8 / (probe_ms * 1e-3)
    b_cmp = sum(n * (8 * (len(sel[pa][0]) + len(sel[pb][0])) + 9) for pa, pb, _ in pairs)
    b_dist = n * (8 * sum(len(xs) for xs, _ in sel) + S)
    med = lambda v: float(np.median(v))
    rnd = lambda v: [round(x, 1) for x in v]
    print(json.dumps({
        "shape": [a.months, a.firms, C], "pairs": len(pairs), "sorts": S, "reps": a.reps,
        "compare_us_f64": rnd(cmp_us["f64"]), "compare_us_planes": rnd(cmp_us["planes"]),
        "dist_us_f64": rnd(dist_us["f64"]), "dist_us_planes": rnd(dist_us["planes"]),
        "compare_over_dist_f64": round(med(cmp_us["f64"]) / med(dist_us["f64"]), 2),
        "compare_bytes_as_launched": b_cmp, "dist_bytes_as_launched": b_dist,
        "stream_probe_read_TBps": round(peak / 1e12, 3),
        "compare_f64_fraction_of_read_peak_as_launched": round(b_cmp / peak * 1e6 / med(cmp_us["f64"]), 3),
        "compare_planes_fraction_of_read_peak_as_launched": round(b_cmp / peak * 1e6 / med(cmp_us["planes"]), 3),
        "dist_f64_fraction_of_read_peak_as_launched": round(b_dist / peak * 1e6 / med(dist_us["f64"]), 3),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
