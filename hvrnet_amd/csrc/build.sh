#!/bin/bash
# Builds libhvr_hip.so (gfx950 only) in-tree next to the sources.  units.txt lists the translation units in link order and says how
# each is compiled; this script names none of them.
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libhvr_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value"
mkdir -p build
objs=(); remarks=(); asm=()
while read -r f opts <&3; do
  [ -n "$f" ] || continue
  o=build/$f.o; objs+=($o)
  nofma=""; keep=0; stale=0
  for w in $opts; do case $w in nofma) nofma=-ffp-contract=off;; remarks) keep=1;; *) echo "units.txt: $f: unknown word '$w'" >&2; exit 1;; esac; done
  if [ $keep = 1 ]; then
    remarks+=(build/$f.remarks); asm+=(build/$f-hip-amdgcn-amd-amdhsa-gfx950.s)   # (the device assembly that -save-temps=obj leaves)
    [ -f build/$f.remarks ] || stale=1
  fi
  for d in $f.hip *.h ../../include/hvr_hip.h units.txt; do [ ! $d -nt $o ] || stale=1; done   # (-nt: also true when $o is missing)
  [ $stale = 1 ] || continue
  rm -f $o
  while [ "$(jobs -rp | wc -l)" -ge "${MAX_JOBS:-16}" ]; do wait -n || true; done
  if [ $keep = 1 ]; then
    ( hipcc $FLAGS $nofma -save-temps=obj -Rpass-analysis=kernel-resource-usage -c $f.hip -o $o 2> build/$f.remarks; rm -f build/$f-h*.hipi build/$f-h*.bc build/$f-host-*.s build/$f-hip-*.out* ) &
  else
    hipcc $FLAGS $nofma -c $f.hip -o $o &
  fi
done 3< <(sed 's/#.*//' units.txt)
wait
for r in "${remarks[@]}"; do
  if grep -q "error:" $r; then grep -A3 "error:" $r; exit 1; fi
done
for o in "${objs[@]}"; do [ -f $o ] || { echo "build.sh: $o was not compiled" >&2; exit 1; }; done
python3 check_asm_waits.py "${asm[@]}"
python3 check_regs.py "${remarks[@]}"
hipcc --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o $OUT
echo "built $(realpath $OUT)"
