#!/bin/bash
# Ablation builds of csrc/dense_dx_split_bf16.hip (probe macros DX_PROBE_*): what each stream of the wide input-gradient launch
# costs -- the output stores, the A-fragment reads from LDS, the refill of the B registers from L2, the prologue that splits G.
# Each variant is linked with the product's other objects and loaded through GEOM_LIB_OVERRIDE by tools/time_wide_dx.py.
# usage: dx_variants.sh build | run
set -e
cd "$(dirname "$0")/../.."
VARIANTS=("base:" "nostore:-DDX_PROBE_NO_STORE" "nolds:-DDX_PROBE_NO_LDS" "norefill:-DDX_PROBE_NO_REFILL" "noprologue:-DDX_PROBE_NO_PROLOGUE"
          "mfmaonly:-DDX_PROBE_NO_STORE -DDX_PROBE_NO_LDS -DDX_PROBE_NO_REFILL -DDX_PROBE_NO_PROLOGUE")
if [ "$1" = build ]; then
  mkdir -p tools/probe/bin
  for v in "${VARIANTS[@]}"; do
    name=${v%%:*}; flags=${v#*:}
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -fno-gpu-rdc -fno-slp-vectorize \
      -mllvm -amdgpu-mfma-vgpr-form=1 $flags -I include -I geometrics_amd/csrc -c geometrics_amd/csrc/dense_dx_split_bf16.hip -o /tmp/dx_$name.o &
  done
  wait
  for v in "${VARIANTS[@]}"; do
    name=${v%%:*}
    objs=$(ls geometrics_amd/lib/*.o | grep -v dense_dx_split_bf16.o)
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -fno-gpu-rdc $objs /tmp/dx_$name.o -o tools/probe/bin/libgeom_dx_$name.so
    # (the MFMAs must survive an ablation: 72 per row-block and B register set, 3024 in all)
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-gpu-rdc -fno-slp-vectorize -mllvm -amdgpu-mfma-vgpr-form=1 \
      ${v#*:} -I include -I geometrics_amd/csrc -S --cuda-device-only geometrics_amd/csrc/dense_dx_split_bf16.hip -o /tmp/dx_$name.s 2>/dev/null
    echo "$name: $(grep -c v_mfma /tmp/dx_$name.s) MFMAs in the ISA"
  done
else
  for v in "${VARIANTS[@]}"; do
    name=${v%%:*}
    echo "== $name"
    GEOM_ALLOW_STALE_LIB=1 GEOM_LIB_OVERRIDE=$PWD/tools/probe/bin/libgeom_dx_$name.so timeout -k 10 120 python tools/time_wide_dx.py 2>&1 | grep "split bf16\|^rows" || exit $?
  done
fi
