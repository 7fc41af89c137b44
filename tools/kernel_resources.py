"""Register / LDS / scratch report of the hot kernels (gfx950), from the compiler's own
metadata: python tools/kernel_resources.py [source.hip ...]
Compiles each source device-only to assembly (hipcc -S, the library's flags) and prints, per
kernel matching the hot-path names, VGPRs, spilled VGPRs, static LDS, the private
(scratch) segment, the buffer loads that sit inside an exec-masked retry loop (a descriptor
the compiler could not prove wave-uniform) and, for the Gram, the LDS waits (s_waitcnt
lgkmcnt) inside the tile loop.  A spill or a scratch segment in a hot kernel is a regression
to catch before a GPU run (scratch can also throttle how many waves a launch gets)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "fm-returnprediction_amd", "csrc")
HOT = ("select_pair_hk_kernelILi", "select_pair_kernelILi40", "select_fixup_universe_kernelILi20",
       "select_fixup_kernelILi20", "select_long_hk_kernelILi40", "universe_kernelILi20",
       "gram_kernelILi1ELi15ELi3ELb1", "gram_kernelILi1ELi15ELi3ELb0", "solve16_kernel", "ts_fused_kernel",
       "rolling_std_kernel", "firm_chars_kernel", "split_planes_kernel", "port_kernelILi", "fdist_kernelILi", "fcmp_kernelILi", "fhor_kernelILi", "rank_kernelILi",
       "rank_long_kernel", "wls_kernel", "pool_pass_kernelILi", "pool_firm_kernel")


def bodies(s):
    """{kernel name: list of instruction / label lines} of an assembly file."""
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.S | re.M):
        lines = [ln.split(";")[0].strip() for ln in m.group(2).split("\n")]
        out[m.group(1)] = [ln for ln in lines if ln]
    return out


def retry_loads(lines):
    """Buffer loads inside an exec-masked retry loop: the loop the compiler wraps round a
    buffer instruction whose descriptor it holds in VGPRs (readfirstlane, compare, saveexec,
    the load, s_cbranch_execnz back to the loop's own label)."""
    n, label, loads, masked = 0, None, 0, False
    for ln in lines:
        if ln.endswith(":"):
            label, loads, masked = ln[:-1], 0, False
        elif ln.startswith("s_and_saveexec"):
            masked = True
        elif ln.startswith("buffer_load"):
            loads += 1
        elif ln.startswith("s_cbranch_execnz") and masked and ln.split()[-1] == label:
            n += loads
    return n


def tile_loop_waits(lines):
    """(LDS waits in the Gram's tile loop, those of them before its first MFMA: the sort and
    the clip, scaled and unscaled, and the LDS round trips among those).  The tile loop is the
    widest loop with an MFMA and no workgroup barrier in it."""
    pos = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    best = None
    for i, ln in enumerate(lines):
        if not ln.startswith("s_cbranch") and not ln.startswith("s_branch"):
            continue
        j = pos.get(ln.split()[-1], i)
        if j >= i:
            continue
        body = lines[j:i]
        if any(b.startswith("s_barrier") for b in body) or not any(b.startswith("v_mfma") for b in body):
            continue
        if best is None or i - j > best[1] - best[0]:
            best = (j, i)
    if best is None:
        return -1, -1, -1
    body = lines[best[0]:best[1]]
    first = next(k for k, b in enumerate(body) if b.startswith("v_mfma"))
    waits = [k for k, b in enumerate(body) if b.startswith("s_waitcnt") and "lgkmcnt" in b]
    # round trips: waits with an LDS read issued since the wait before (the counted waits
    # lgkmcnt(3), (2), (1), (0) behind one batch of reads are one round trip)
    trips, fresh = 0, False
    for b in body[:first]:
        if b.startswith("ds_read"):
            fresh = True
        elif b.startswith("s_waitcnt") and "lgkmcnt" in b and fresh:
            trips, fresh = trips + 1, False
    return len(waits), sum(1 for k in waits if k < first), trips


def report(src):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + CS, "--offload-device-only", "-S", "-o", out, src]
        cmd += os.environ.get("EXTRA", "").split()   # as the Makefile's EXTRA: -D switches
        subprocess.run(cmd, check=True, capture_output=True)
        s = open(out).read()
    code = bodies(s)
    rows = []
    for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\S+).*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)",
                         s, re.S):
        blk = m.group(0)
        name = m.group(1)
        if not any(h in name for h in HOT):
            continue
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk)
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        body = code.get(name, [])
        rows.append((name, int(m.group(2)), int(m.group(3)), int(lds.group(1)) if lds else -1,
                     int(priv.group(1)) if priv else -1, retry_loads(body),
                     tile_loop_waits(body) if "gram_kernel" in name else None))
    return rows


def main():
    srcs = sys.argv[1:] or [os.path.join(CS, f) for f in ("fm_select.hip", "fm_gram.hip", "fm_solve.hip",
                                                           "fm_ts.hip", "fm_chars.hip", "fm_elem.hip", "fm_port.hip",
                                                           "fm_rank.hip")]
    bad = 0
    for src in srcs:
        for name, vgpr, spill, lds, priv, retry, waits in report(src):
            flag = "  <-- spills / scratch" if spill or priv > 0 else ""
            bad += bool(flag)
            lgkm = f" lgkm-waits tile {waits[0]:3d} pre-mfma {waits[1]:3d} trips {waits[2]:3d}" if waits else ""
            print(f"{os.path.basename(src):14s} {name[:64]:64s} vgpr {vgpr:3d} spill {spill:3d} lds {lds:6d} "
                  f"scratch {priv:4d} retry-loads {retry:3d}{lgkm}{flag}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
