#!/bin/bash
# Variant builds for probes: tools/build_var.sh NAME "-DFOO ..." unit1 [unit2 ...]  ->  abtest/libhvr_NAME.so (abtest/ travels to the GPU box, dbg/ does not)
# The listed units of hvrnet_amd/csrc/units.txt (names without .hip) are recompiled with their flags there plus the extra defines; every
# other object is the product build's (hvrnet_amd/csrc/build/*.o).  Results of ablation builds (-DHVR_DBG_X_*) are timings only, never
# valid outputs.  The tuning knobs of the C API are a define of its own unit: "-DHVR_DEBUG_KNOBS" with that unit among the listed ones.
set -euo pipefail
cd "$(dirname "$0")/.."
name=$1; defs=$2; shift 2
C=hvrnet_amd/csrc
mkdir -p dbg/$name abtest
objs=()
while read -r f opts <&3; do
  [ -n "$f" ] || continue
  o=$C/build/$f.o
  if [[ " $* " == *" $f "* ]]; then
    nofma=""; [[ " $opts " != *" nofma "* ]] || nofma=-ffp-contract=off
    o=dbg/$name/$f.o
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value $nofma $defs -c $C/$f.hip -o $o &
  fi
  objs+=($o)
done 3< <(sed 's/#.*//' $C/units.txt)
wait
hipcc --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o abtest/libhvr_$name.so
rm -rf dbg/$name
echo built abtest/libhvr_$name.so
