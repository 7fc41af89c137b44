"""Timing of fm_rank_transform on the bench panel (600 months x 5,000 firms, the 14 predictor
columns, average ties, uniform scale), beside the numbers it is read against, all from one
process: python tools/rankbench.py [--months 600] [--firms 5000]
  * the algorithmic traffic, rows x 14 x 16 B (every value read once, every rank written once);
  * fm_stream_copy_probe's copy rate over a 1 GiB tensor in the same run, that traffic's time
    at this rate, and the fraction of it the kernel reaches;
  * the host time of the equivalent pandas groupby.rank on this machine (the CPU baseline).
Two timings of the kernel: one input set re-issued back to back, and rotating over input sets
(one call already moves more than the Infinity Cache holds, so both read from HBM).
Prints one JSON line."""
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--no-pandas", action="store_true", help="skip the CPU baseline")
    a = ap.parse_args()
    dev = E.require_device()
    panel = E.panel_synthetic(a.months, a.firms, 1234)
    n, C = panel.nrows, panel.ncols
    cols = list(range(1, C))   # the 14 predictors; column 0 is the return
    out = torch.empty_like(panel.cols)
    kw = dict(cols=cols, method="average", scale="uniform", out=out)
    res = E.rank_transform(panel, **kw)
    torch.cuda.synchronize()
    nbytes = n * len(cols) * 16
    warm = [E.time_launch("fm_rank_transform", a.reps) * 1e3 for _ in range(3)]
    # rotating input sets, one output block
    args, keep = [], []
    for _ in range(a.sets):
        p = E.DevicePanel(cols=panel.cols.clone(), names=panel.names, seg_off=panel.seg_off, seg_off_h=panel.seg_off_h)
        E.rank_transform(p, **kw)
        keep.append(p)
        args.append(E.LAST_LAUNCH["fm_rank_transform"][1])
    st = E._stream()
    it = [0]

    def rot():
        L.call("fm_rank_transform", L.C.byref(args[it[0] % len(args)]), st)
        it[0] += 1

    cold = [timed(rot, a.reps) for _ in range(3)]
    del keep, args
    src = torch.ones(1 << 27, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    E.stream_copy_probe(src, dst)
    copy_ms = min(E.time_launch("fm_stream_copy_probe", 20) for _ in range(3))
    rate = 2 * src.numel() * 8 / (copy_ms * 1e-3)   # bytes moved (read + written) per second
    floor_us = nbytes / rate * 1e6
    r = {"shape": [a.months, a.firms, len(cols)], "method": "average", "scale": "uniform",
         "algorithmic_bytes": nbytes, "rank_us_reissued": [round(v, 1) for v in warm],
         "rank_us_rotating": [round(v, 1) for v in cold],
         "stream_copy_TBps": round(rate / 1e12, 3), "rank_floor_us_at_copy_rate": round(floor_us, 1),
         "rank_fraction_of_copy_rate": round(floor_us / float(np.median(cold)), 3),
         "nvalid_total": int(res.rank_nvalid.sum().item()), "device": torch.cuda.get_device_name(0)}
    if not a.no_pandas:
        import pandas as pd
        host = panel.cols[1:].cpu().numpy()
        codes = np.repeat(np.arange(a.months), a.firms)
        df = pd.DataFrame(host.T)
        t0 = time.perf_counter()
        g = df.groupby(codes)
        ranks = g.rank() / (g.transform("count") + 1) - 0.5
        r["cpu_baseline_pandas_groupby_rank_s"] = round(time.perf_counter() - t0, 3)
        got = out[1:].cpu().numpy()
        exp = ranks.to_numpy().T
        r["equals_pandas_bits"] = bool(np.array_equal(np.isnan(got), np.isnan(exp)) and
                                       np.array_equal(got[~np.isnan(got)].view(np.int64), exp[~np.isnan(exp)].view(np.int64)))
    print(json.dumps(r))


if __name__ == "__main__":
    main()
