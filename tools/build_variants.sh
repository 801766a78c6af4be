#!/bin/bash
# A/B builds of librepairgbm.so for timing experiments (RGBM_LIB_PATH=<file> selects one): tools/build_variants.sh name "-DFLAG ..." [name flags ...]
# (one compile line over every .hip of csrc/ -- the directory this script changes into, so keep no stray .hip there -- like the library before it
# was built from objects: a variant shares no object with another.)
# Knobs that exist: -DMT_DBL_ATOM=1, -DMT_CONSUMERS_N=n, -DMT_SPARSE_DIV_N=n, -DSM_THREADS_N=n, -DSM_PROF=1.  The rotate-everything and ring-size knobs of the
# level pass were removed with the other rejected experiments ("Retired experiments": the last commit that builds them is named there).
cd "$(dirname "$0")/../spark-data-repair-plugin_amd/csrc" || exit 1
mkdir -p ../lib/variants
while [ $# -ge 2 ]; do
  n=$1; f=$2; shift 2
  /opt/rocm/bin/hipcc $f -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden --offload-arch=gfx950 -Wall -Wno-unused-result -shared \
     -o ../lib/variants/librepairgbm_$n.so *.hip -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib 2>&1 | grep -E "error" &
done
wait
ls -la ../lib/variants
