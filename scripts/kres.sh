#!/bin/bash
# Register/scratch usage of every kernel of one translation unit for a set of -D flags
# (device-only compile, no GPU):  scripts/kres.sh [capi|queries|park] [-DNAME=V ...]
R=$(cd "$(dirname "$0")/.." && pwd)/3360-ray-tracer_amd
TU=${1:-capi}; shift
case "$TU" in
  park) F="" ;;
  capi|queries) F="-mllvm -amdgpu-disable-clustered-low-occupancy-reschedule" ;;
  *) echo "unit must be capi, queries or park" >&2; exit 2 ;;
esac
SRC=csrc/rtx_$TU.hip
OUT=$(mktemp /tmp/kres.XXXXXX.s)
cd $R && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I$R/../include \
  -Icsrc -Ihost/include $F "$@" --cuda-device-only -S $SRC -o $OUT 2>/dev/null || exit 1
echo "kernel (k_persistent<STACK,FAST,COUNT,SCATTER,PARK,TK,LAMB,NOTEX,NODOF,MAP>)  scratch_B sgpr vgpr vgpr_spill"
grep -A12 "\.name: " $OUT | grep -E "\.name|private_segment|sgpr_count|vgpr_count|vgpr_spill" |
  paste - - - - - | awk '{print $2, $4, $6, $8, $10}' | sed 's/_ZN4rtxd12k_persistentI//; s/EEEvNS_10RenderArgsEPy//'
echo "asm: $OUT"
