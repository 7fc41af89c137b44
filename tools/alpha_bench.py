"""Timing of fm_portfolio_alpha on the pipeline's workload (600 months x 5,000 firms, the nine
Table-2 sorts x 11 rows x 2 weightings x 2 factor models = 396 workgroups over 600 months), from
one process:
python tools/alpha_bench.py [--months 600] [--firms 5000] [--lags 4]
  * the launch alone (engine.time_launch: re-issued back to back, five windows), at ``--lags``
    Newey-West lags and at 12;
  * what it adds to run_pipeline(portfolios=10): the whole pass with and without alpha_factors,
    alternating, a host clock around each pass and its device synchronise.
The factor table is seeded noise of market-like size; the kernel's time does not depend on the
values.  The launch's outputs are held to a float64 numpy regression of three series before
anything is timed.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fm-returnprediction_amd"))

from fmcore import engine as E  # noqa: E402
from fmcore import lewellen as LW  # noqa: E402


def check(ports, alphas, F, lags):
    """alpha and its classical t of (sort 0, rows 0 / 5 / spread, ew, all factors) by numpy."""
    rec, st = ports.rec.cpu().numpy(), ports.status.cpu().numpy()
    coef, se = alphas.coef.cpu().numpy(), alphas.se.cpu().numpy()
    for p in (0, 5, rec.shape[2] - 1):
        d = rec[0, :, p, 0]
        use = (st[0] == 1) & np.isfinite(d)
        X = np.column_stack([np.ones(int(use.sum())), F[use]])
        th = np.linalg.lstsq(X, d[use], rcond=None)[0]
        e = d[use] - X @ th
        s = np.sqrt(e @ e / (len(e) - X.shape[1]) * np.linalg.inv(X.T @ X)[0, 0])
        assert abs(coef[0, p, 0, 1, 0] - th[0]) <= 1e-9 * np.abs(d[use]).mean(), (p, coef[0, p, 0, 1, 0], th[0])
        assert abs(se[0, p, 0, 1, 0] - s) <= 1e-9 * s, (p, se[0, p, 0, 1, 0], s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=600)
    ap.add_argument("--firms", type=int, default=5000)
    ap.add_argument("--lags", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=12)
    a = ap.parse_args()
    dev = E.require_device()
    panel = E.panel_synthetic(a.months, a.firms, 1234)
    F = np.random.default_rng(18).normal(0.005, 0.04, (panel.nseg, 3))
    Fd = torch.from_numpy(F).to(dev)
    base = dict(portfolios=10)
    cfg_off = LW.PipelineConfig(**base)
    cfg_on = LW.PipelineConfig(**base, alpha_factors=Fd, alpha_nw_lags=a.lags)
    out = LW.run_pipeline(panel, cfg_on)
    torch.cuda.synchronize()
    check(out.portfolios, out.portfolio_alphas, F, a.lags)
    S, nrow, _, M = out.portfolio_alphas.nobs.shape
    nobs = out.portfolio_alphas.nobs.cpu().numpy()

    launch = {}
    for lags in sorted({a.lags, 12}):
        E.portfolio_alphas(out.portfolios, Fd, nw_lags=lags)
        launch[lags] = [E.time_launch("fm_portfolio_alpha", a.reps) * 1e3 for _ in range(5)]

    def one(cfg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        LW.run_pipeline(panel, cfg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for cfg in (cfg_off, cfg_on):
        one(cfg)
    on, off = [], []
    for _ in range(a.passes):
        off.append(one(cfg_off))
        on.append(one(cfg_on))
    print(json.dumps({
        "shape": [a.months, a.firms], "sorts": S, "rows": nrow, "models": M, "workgroups": S * nrow * 2 * M,
        "months_used": [int(nobs.min()), int(nobs.max())],
        "launch_us": {str(k): [round(v, 1) for v in vs] for k, vs in launch.items()},
        "launch_us_median": {str(k): round(float(np.median(vs)), 1) for k, vs in launch.items()},
        "pipeline_ms_off": [round(v, 3) for v in off], "pipeline_ms_on": [round(v, 3) for v in on],
        "pipeline_ms_off_median": round(float(np.median(off)), 3), "pipeline_ms_on_median": round(float(np.median(on)), 3),
        "pipeline_ms_added_median": round(float(np.median(on) - np.median(off)), 3),
        "pipeline_ms_spread": {"off": round(max(off) - min(off), 3), "on": round(max(on) - min(on), 3)},
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
