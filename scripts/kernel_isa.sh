#!/bin/bash
# Disassembles the gfx950 code objects inside a built library (one per unit: build.code_objects) and prints one kernel's ISA
# (or the list of kernels).
#   scripts/kernel_isa.sh                      -> kernel names with their register / LDS use
#   scripts/kernel_isa.sh k_p3_dedupILb1       -> the instructions of the first kernel whose mangled name contains that
#   MC_LIB=metacherchant_amd/lib/libmcgpu_x.so scripts/kernel_isa.sh ...   -> another build
set -e
LLVM=/opt/rocm/lib/llvm/bin
ROOT=$(cd "$(dirname "$0")/.." && pwd)
LIB=${MC_LIB:-$ROOT/metacherchant_amd/lib/libmcgpu.so}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
CO=$(PYTHONPATH=$ROOT python3 -c 'import sys; from metacherchant_amd import build; print(" ".join(build.code_objects(sys.argv[1], sys.argv[2])))' "$LIB" "$T")
if [ -z "$1" ]; then
    for co in $CO; do $LLVM/llvm-readelf --notes $co; done | grep -E "^\s+\.(name|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):" | paste - - - - - | sed 's/  */ /g'
    exit 0
fi
for co in $CO; do $LLVM/llvm-objdump -d --no-show-raw-insn $co; done > $T/all.s
awk -v pat="$1" '
    /^[0-9a-f]+ <.*>:$/ { on = index($0, pat) > 0 ? (seen ? 0 : 1) : 0; if (on) seen = 1 }
    on { print }' $T/all.s
