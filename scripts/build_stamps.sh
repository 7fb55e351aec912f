#!/bin/bash
# Stamps build of the library (device-side s_memtime / s_memrealtime stamps read by scripts/*stamps*.py,
# link_phases.py, link_timeline.py, ring_gaps.py): scripts/var_stamps.so, selected with YSMR_HIP_LIB.  Run in the
# build container (hipcc cross-compiles).
R=${GRAFT_REPO_ROOT:-/root/repo}; C=$R/ysmr_amd/csrc; T=/tmp/stampbuild; mkdir -p $T
for f in common detect thr_mfma meangray track rows select evaluate ingest luminosity annotate plots mjpeg violin mjpeg_decode png view; do   # (the Makefile's SRCS: the host code binds every export)
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -I$R/include -Wall -Wno-unused-function -DYSMR_STAMPS $EXTRA -c $C/$f.hip -o $T/$f.o || exit 1
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $R/scripts/var_stamps.so $T/*.o && echo built scripts/var_stamps.so
# k_batch's written-out scalar loads and 16-byte ring loads (batch_link.h): nothing may touch their registers before their
# wait, in THIS build too
python3 $R/scripts/k_batch_census.py $R/scripts/var_stamps.so > $T/census.log; rc=$?; tail -1 $T/census.log
[ $rc -eq 0 ] || { echo "scripts/var_stamps.so: a pending load's registers are touched -- do not run it"; exit 1; }
