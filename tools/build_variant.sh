#!/bin/bash
# Probe and tuning variants of libfm_hip.so (never shipped):
#   tools/build_variant.sh <name> "<extra hipcc flags>" source.hip [source.hip ...]
# The flags the sources still take: -DFM_PROBE=1 (tools/tail_probe.py), -DFM_GRAM_WGTIME=1
# (tools/gram_wgtime.py) and the numeric parameters (FM_GRAM_MINW, FM_STD_T / _R / _LP,
# FM_TS_RROWS, FM_SELECT_STREAM_VPT / _SB, FM_UNI_HB / _CAP, FM_PAIR_HK_WGS, FM_NP_MOM_DEPTH) for
# tools/kbench.py A/B runs.  The sources hold no ablation or strategy switches any more.
# Reuses the in-tree objects and recompiles only the listed sources with the extra flags
# into build_variants/<name>/libfm_hip.so.
set -e
name=$1; flags=$2; shift 2
# the flags only reach the sources named here: with none the "variant" would be a copy
[ $# -ge 1 ] || { echo "build_variant: name the source(s) to rebuild with \"$flags\"" >&2; exit 2; }
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CS=$ROOT/fm-returnprediction_amd/csrc
VD=$ROOT/build_variants/$name
mkdir -p "$VD/obj"
cp -p "$CS"/build/*.o "$VD/obj/"
pids=()
for src in "$@"; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I"$ROOT/include" \
    -Wall -Wno-unused-function $flags -c "$CS/$src" -o "$VD/obj/${src%.hip}.o" &
  pids+=($!)
done
for p in "${pids[@]}"; do
  wait "$p" || { echo "build_variant: a compile failed" >&2; rm -rf "$VD"; exit 1; }
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC "$VD"/obj/*.o -o "$VD/libfm_hip.so"
rm -rf "$VD/obj"
echo "$VD/libfm_hip.so"
