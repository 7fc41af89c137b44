"""Timing of fm_group_adjust on the pipeline's workload (600 months x 5,000 firms, the 14 predictor
columns, 49 random groups), from one process:
python tools/gadj_bench.py [--months 600] [--firms 5000] [--groups 49]
  * the launch alone in every mode (engine.time_launch: re-issued back to back, five windows);
  * beside it a torch restatement on the same device -- index_add_ on month * G + code keys, what a
    user would otherwise write -- timed the same way (events around ``reps`` back-to-back calls).
Before anything is timed the launch is held to the restatement at 1e-9.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fm-returnprediction_amd"))

from fmcore import engine as E  # noqa: E402


def torch_adjust(x, key, valid, nkeys, mode):
    """x [C, n] adjusted within the keys (month * G + code) of the valid rows, with scatter adds."""
    nan = torch.full_like(x, float("nan"))
    ok = valid[None] & ~torch.isnan(x)
    z = torch.zeros((x.shape[0], nkeys), dtype=torch.float64, device=x.device)
    S = z.clone().index_add_(1, key, torch.where(ok, x, 0.0))
    N = z.clone().index_add_(1, key, ok.to(torch.float64))
    m = (S / N)[:, key]
    if mode == "mean":
        return torch.where(ok, m, nan)
    d = x - m
    if mode == "demean":
        return torch.where(ok, d, nan)
    ss = z.clone().index_add_(1, key, torch.where(ok, d * d, 0.0))
    sd = torch.sqrt(ss / (N - 1.0))[:, key]
    return torch.where(ok & (sd > 0) & torch.isfinite(sd), d / sd, nan)


def time_torch(fn, reps):
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
    ap.add_argument("--groups", type=int, default=49)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = E.require_device()
    panel = E.panel_synthetic(a.months, a.firms, 1234)
    idx = [i for i, c in enumerate(panel.names) if c != "retx"]
    x = panel.values()[idx[0]:idx[-1] + 1]
    assert idx == list(range(idx[0], idx[-1] + 1)) and x.shape[0] == 14
    n, T, G = panel.nrows, panel.nseg, a.groups
    code = torch.from_numpy(np.random.default_rng(5).integers(0, G, n).astype(np.int32)).to(dev)
    month = torch.repeat_interleave(torch.arange(T, device=dev), panel.seg_off[1:] - panel.seg_off[:-1])
    key = month * G + code.to(torch.int64)
    valid = torch.ones(n, dtype=torch.bool, device=dev)
    out = torch.empty_like(x)
    res = {"shape": [a.months, a.firms, int(x.shape[0])], "groups": G,
           "batch": int(E.L.load().fm_group_adjust_batch(G)), "kernel_us": {}, "torch_us": {}}
    for mode in E.GADJ_MODES:
        E.group_adjust_columns(panel.seg_off, x, code, G, mode=mode, out=out)
        ref = torch_adjust(x, key, valid, T * G, mode)
        torch.cuda.synchronize()
        assert torch.equal(torch.isnan(out), torch.isnan(ref)), mode
        err = torch.nan_to_num((out - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
        assert err <= 1e-9, (mode, err)
        res["kernel_us"][mode] = [round(E.time_launch("fm_group_adjust", a.reps) * 1e3, 1) for _ in range(5)]
        res["torch_us"][mode] = [round(time_torch(lambda: torch_adjust(x, key, valid, T * G, mode), a.reps) * 1e3, 1)
                                 for _ in range(5)]
        del ref
    res["kernel_us_median"] = {k: float(np.median(v)) for k, v in res["kernel_us"].items()}
    res["torch_us_median"] = {k: float(np.median(v)) for k, v in res["torch_us"].items()}
    res["bytes_moved"] = int(x.numel() * 8 * 3)   # two reads (the second from L2 at best) and one write per value
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
