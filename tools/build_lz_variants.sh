#!/bin/bash
# Build A/B variants of one kernel unit (UNIT, default nus_k_lanczos_x2) into tools/_ablate/lib_<name>.so (timing only; dev tool).
#   [UNIT=nus_k_flow] tools/build_lz_variants.sh name1="-DFLAG=1 -DX=2" name2="" old=@<git-rev> exp="@<git-rev> -DFLAG=1"
# "@rev [flags]": the unit as of that commit, built with the flags -- against that commit's headers and linked with that commit's
# other objects (exported to tools/_ablate/tree_<name>), so a variant survives later changes to the launch structs.
set -e
cd "$(dirname "$0")/.."
CS=nu_scaler_amd/csrc
make -s -j8 -C $CS >/dev/null
mkdir -p tools/_ablate
UNIT=${UNIT:-nus_k_lanczos_x2}
declare -A DIR
for spec in "$@"; do
  name="${spec%%=*}"; flags="${spec#*=}"
  root=.
  if [[ "$flags" == @* ]]; then
    rev="${flags%% *}"; rev="${rev#@}"
    if [[ "$flags" == *" "* ]]; then flags="${flags#* }"; else flags=""; fi
    root=tools/_ablate/tree_$name
    mkdir -p $root
    git archive "$rev" $CS include | tar -xm -C $root  # (-m: extracted now, so make rebuilds what an earlier revision left there)
    make -s -j8 -C $root/$CS ../lib/libnuscaler_hip.so >/dev/null
  fi
  DIR[$name]=$root/$CS
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function -x hip -I$root/$CS -I$root/include \
      -DNUS_DEV_BUILD $flags -c -o tools/_ablate/lz_$name.o $root/$CS/$UNIT.hip &
done
wait
for spec in "$@"; do
  name="${spec%%=*}"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/_ablate/lib_$name.so tools/_ablate/lz_$name.o \
      $(ls ${DIR[$name]}/build/*.o | grep -v $UNIT.o)
  echo "built tools/_ablate/lib_$name.so"
done
