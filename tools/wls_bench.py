"""Timing of fm_wls on the pipeline's workload (600 months x 5,000 firms, the 15 columns, the
Table-2 and Figure-1 problems over the three universes, winsorize cuts, weights = market equity),
from one process:
python tools/wls_bench.py [--months 600] [--firms 5000]
  * the fm_wls launch alone (engine.time_launch: re-issued back to back, five windows);
  * beside it the OLS pair on the same panel, fm_gram and fm_solve, timed the same way;
  * and a torch restatement on the same device -- per problem a batched torch.linalg.lstsq on
    sqrt(w)-scaled rows, what a user would otherwise write -- timed with events around ``reps``
    calls (each call timed on its own: it is by far the slowest part).
The launch is held to the restatement at 1e-9 of each slope series' RMS.  Progress goes to stderr
stage by stage; one JSON line to stdout at the end."""
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


def torch_wls(x, w, level, models, problems, T, N):
    """x [C, T*N] clipped, balanced months: per problem the rows that do not take part get weight 0
    (and zeroed values), then one batched least-squares solve of [T, N, K+1] on sqrt(w)-scaled rows."""
    out = []
    wok = torch.isfinite(w) & (w > 0)
    for p in problems:
        m = models[p.model]
        cols = x[m.xs + [m.y]]
        use = wok & ~torch.isnan(cols).any(dim=0) & (level >= p.level)
        r = torch.where(use, torch.sqrt(torch.where(wok, w, 1.0)), 0.0)
        z = torch.where(use[None], cols, 0.0) * r[None]
        A = torch.cat([r[None], z[:-1]], dim=0).reshape(p.K + 1, T, N).permute(1, 2, 0)
        b = z[-1].reshape(T, N, 1)
        out.append(torch.linalg.lstsq(A, b).solution[:, :, 0])
    return out


def time_torch(fn, reps, warm=True):
    if warm:
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=600)
    ap.add_argument("--firms", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=2)
    a = ap.parse_args()
    E.require_device()
    panel = E.panel_synthetic(a.months, a.firms, 1234)
    T, N = panel.nseg, a.firms
    assert panel.nrows == T * N and panel.ncols == 15
    models, _ = LW.build_models(panel, LW.table2_models())
    cuts, (_, _, level) = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY, center=True, universe=(0.2, 0.5))
    out = {"shape": [a.months, a.firms, panel.ncols]}

    def note(key, value):   # progress on stderr: a slow stage shows in the log while it runs
        out[key] = value
        print(f"{key}: {value}", file=sys.stderr, flush=True)

    res = E.fm_pass_wls(panel, models, weight="me", level=level, nlevels=3, cuts=cuts, shift=cuts.center, moments=True)
    torch.cuda.synchronize()
    fitted = (res.status & E.L.FM_ST_FITTED) != 0
    assert bool(fitted.all())
    note("problems", len(res.problems))
    note("fm_wls_us", [round(E.time_launch("fm_wls", a.reps) * 1e3, 1) for _ in range(5)])
    E.fm_pass(panel, models, level=level, nlevels=3, cuts=cuts, shift=cuts.center, moments=True)
    note("fm_gram_us", [round(E.time_launch("fm_gram", a.reps) * 1e3, 1) for _ in range(5)])
    note("fm_solve_us", [round(E.time_launch("fm_solve", a.reps) * 1e3, 1) for _ in range(5)])
    x = E.clip(panel, cuts)
    ref = None

    def run_torch():
        nonlocal ref
        ref = torch_wls(x, panel.me, level, models, res.problems, T, N)

    # every call of the restatement is timed, the first included (it also gives the values to compare)
    times = []
    for i in range(a.torch_reps):
        times.append(round(time_torch(run_torch, 1, warm=False) * 1e3, 1))
        print(f"torch call {i + 1} of {a.torch_reps} done", file=sys.stderr, flush=True)
    note("torch_lstsq_us", times)
    worst = 0.0
    for k, p in enumerate(res.problems):
        got, exp = res.rec[:, k, :p.K + 1], ref[k]
        rms = exp.pow(2).mean(dim=0).sqrt()
        worst = max(worst, float(((got - exp).abs() / torch.maximum(exp.abs(), rms[None])).max()))
    note("max_rel_diff_vs_torch", worst)
    assert worst <= 1e-9, worst
    for k in ("fm_wls_us", "fm_gram_us", "fm_solve_us", "torch_lstsq_us"):
        out[k + "_median"] = float(np.median(out[k]))
    out["bytes_read_once"] = int(panel.nrows * 8 * (panel.ncols + 1) + panel.nrows)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
