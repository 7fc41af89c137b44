"""Timing of fm_forecast_horizon beside fm_forecast_dist on the same panel (600 months x 5,000
firms x 15 columns, the nine Table-2 sorts = Models 1/2/3 x three universes, q = (0.1, 0.9), the
pipeline's cuts and levels, k = 12 and decay 0.9), from one process:
python tools/fhorbench.py [--months 600] [--firms 5000] [--horizon 12]
Each launch is re-issued back to back between two HIP events (engine.time_launch, one warm-up launch
before the window); the two kernels alternate over five windows each, on an f64 panel and on a
planes-only panel, and fm_horizon_return (the k-month return the new launch reads) is timed once
beside them.  Bytes (n rows, sort j with K_j predictors, S sorts):
  dist, as launched:     sum_j n (8 K_j + 1)        predictors and the level byte, once per sort;
  horizon, as launched:  that + S * 8 n             the return vector, once per sort.
Before anything is timed the new launch's m and count are checked byte for byte against
fm_forecast_dist's mean and count, and the f64 and planes outputs against each other.
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

Q = (0.1, 0.9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=600)
    ap.add_argument("--firms", type=int, default=5000)
    ap.add_argument("--horizon", type=int, default=12)
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
    k = a.horizon
    ret_k = E.horizon_return(panel.seg_off, E.column_vector(panel, "retx"), E.month_links(panel, 1), k)
    ret_us = E.time_launch("fm_horizon_return", a.reps) * 1e3
    gain = E.extrapolation_gain(k, 0.9)

    times = {"dist_f64": [], "horizon_f64": [], "dist_planes": [], "horizon_planes": []}
    outs = {}
    for w in range(5):
        for name, p in (("f64", panel), ("planes", planes)):
            d = E.forecast_dist(p, coef, sel, cuts=cuts, level=level, q=Q)
            times["dist_" + name].append(E.time_launch("fm_forecast_dist", a.reps) * 1e3)
            h = E.forecast_horizon(p, coef, sel, ret_k, float(k), gain, cuts=cuts, level=level, q=Q)
            times["horizon_" + name].append(E.time_launch("fm_forecast_horizon", a.reps) * 1e3)
            if w == 0:
                torch.cuda.synchronize()
                assert torch.equal(h.rec[..., 5].contiguous().view(torch.int64), d.rec[..., 0].contiguous().view(torch.int64))
                assert torch.equal(h.cnt[..., 0], d.cnt) and bool(h.status.all())
                outs[name] = h
    for key in ("rec", "cnt", "status"):
        assert torch.equal(getattr(outs["f64"], key).view(torch.uint8), getattr(outs["planes"], key).view(torch.uint8)), key
    assert planes.cols is None and "_merged" not in planes.__dict__   # no FP64 copy was made

    sumk = sum(len(xs) for xs, _ in sel)
    b_dist = n * (8 * sumk + S)
    b_hor = b_dist + S * 8 * n
    med = {key: float(np.median(v)) for key, v in times.items()}
    print(json.dumps({
        "shape": [a.months, a.firms, C], "sorts": S, "q": list(Q), "horizon": k, "reps": a.reps,
        **{key + "_us": [round(x, 1) for x in v] for key, v in times.items()},
        "median_us": {key: round(v, 1) for key, v in med.items()},
        "spread_us": {key: round(float(max(v) - min(v)), 1) for key, v in times.items()},
        "horizon_over_dist_f64": round(med["horizon_f64"] / med["dist_f64"], 3),
        "horizon_over_dist_planes": round(med["horizon_planes"] / med["dist_planes"], 3),
        "horizon_return_us": round(ret_us, 1),
        "dist_bytes_as_launched": b_dist, "horizon_bytes_as_launched": b_hor,
        "horizon_f64_TBps_as_launched": round(b_hor / med["horizon_f64"] * 1e6 / 1e12, 3),
        "dist_f64_TBps_as_launched": round(b_dist / med["dist_f64"] * 1e6 / 1e12, 3),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
