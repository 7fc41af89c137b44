"""Timing of fm_pool on the pipeline's workload (600 months x 5,000 firms, the 15 columns, the nine
Table-2 problems over the three universes, winsorize cuts), with and without month fixed effects,
from one process:
python tools/pool_bench.py [--months 600] [--firms 5000]
  * the whole fm_pool call (engine.time_launch: re-issued back to back, five windows);
  * each of its eight launches alone (fm_pool_args.stage), timed the same way on the workspace the
    full call left: check, sums, means, moments, fit, scores, firm, cov;
  * beside them the monthly OLS pair on the same panel in the same run, fm_gram and fm_solve.
The pooled slopes are held to a torch restatement (centred normal equations in FP64 on the device)
at 1e-9 of the slope vector's RMS.  Progress goes to stderr; one JSON line to stdout at the end."""
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

STAGES = ("check", "sums", "means", "moments", "fit", "scores", "firm", "cov")


def torch_slopes(x, level, models, problems, month, T, month_fe):
    out = []
    for p in problems:
        m = models[p.model]
        z = x[m.xs + [m.y]]
        use = ~torch.isnan(z).any(dim=0) & (level >= p.level)
        z, mo = z[:, use], month[use]
        if month_fe:
            n = torch.zeros(T, dtype=torch.float64, device=z.device).index_add_(0, mo, torch.ones_like(z[0]))
            s = torch.zeros((z.shape[0], T), dtype=torch.float64, device=z.device).index_add_(1, mo, z)
            z = z - (s / n.clamp(min=1))[:, mo]
        else:
            z = z - z.mean(dim=1, keepdim=True)
        S = z @ z.t()
        out.append(torch.linalg.solve(S[:-1, :-1], S[:-1, -1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--months", type=int, default=600)
    ap.add_argument("--firms", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = E.require_device()
    panel = E.panel_synthetic(a.months, a.firms, 1234)
    T, N = panel.nseg, a.firms
    assert panel.nrows == T * N
    models, _ = LW.build_models(panel, LW.table2_models(), fig1=False)
    cuts, (_, _, level) = E.select_cuts(panel, 0.01, 0.99, 5, E.LERP_NUMPY, center=True, universe=(0.2, 0.5))
    firm = (torch.arange(N, dtype=torch.int32, device=dev).repeat(T), N)     # a balanced panel: firm = row within month
    month = torch.arange(T, device=dev).repeat_interleave(N)
    x = E.clip(panel, cuts)
    out = {"shape": [a.months, a.firms, panel.ncols], "firm_block": E.L.FM_POOL_FIRM_BLOCK}

    def note(key, value):
        out[key] = value
        print(f"{key}: {value}", file=sys.stderr, flush=True)

    def windows(tag):
        return [round(E.time_launch(tag, a.reps) * 1e3, 1) for _ in range(5)]

    for fe in (False, True):
        key = "fe" if fe else "pooled"
        res = E.pooled_regressions(panel, models, level=level, nlevels=3, cuts=cuts, shift=cuts.center, month_fe=fe,
                                   firm=firm)
        torch.cuda.synchronize()
        assert bool(((res.status & E.L.FM_ST_FITTED) != 0).all())
        note("problems", len(res.problems))
        note(f"{key}_fm_pool_us", windows("fm_pool"))
        struct = E.LAST_LAUNCH["fm_pool"][1]
        for k, name in enumerate(STAGES, start=1):
            struct.stage = k
            note(f"{key}_{name}_us", windows("fm_pool"))
        struct.stage = 0
        worst = 0.0
        for k, b in enumerate(torch_slopes(x, level, models, res.problems, month, T, fe)):
            got = res.coef[k, 1:1 + b.numel()]
            rms = b.pow(2).mean().sqrt()
            worst = max(worst, float(((got - b).abs() / torch.maximum(b.abs(), rms)).max()))
        note(f"{key}_max_rel_diff_vs_torch", worst)
        assert worst <= 1e-9, worst
    E.fm_pass(panel, models, level=level, nlevels=3, cuts=cuts, shift=cuts.center, moments=True)
    note("fm_gram_us", windows("fm_gram"))
    note("fm_solve_us", windows("fm_solve"))
    for k in [k for k in out if k.endswith("_us")]:
        out[k + "_median"] = float(np.median(out[k]))
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
