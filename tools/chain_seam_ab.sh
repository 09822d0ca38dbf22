# Per-item A/B of the chain kernel's seam work (chain_v4.hip, REDIO_EXP_SEAM: bit 0 hoisted LDS slots, 1 buffer descriptors on a scalar
# base, 2 early halo read, 3 one-latency prologue): one library per mask under tools/exp/, timed in alternating processes on one box.
#   build here:   bash tools/chain_seam_ab.sh build [masks]   (default masks: 0 1 2 4 8 15; 0 is the parent's code, 15 the product's)
#   on the box:   bash tools/chain_seam_ab.sh run [rounds] [masks]
# Only chain_v4.o differs between the libraries: the other objects are copied from the measurement build, which is made first.
set -eo pipefail # a process that fails ends the run: nothing more is started on that card
R=$(cd "$(dirname "$0")/.." && pwd)
MODE=$1; shift || true
if [ "$MODE" = "build" ]; then
  MASKS=${*:-0 1 2 4 8 15}
  make -C $R/libredio_amd/csrc -s -j16 measure
  for m in $MASKS; do
    O=$R/tools/exp/_build_seam$m
    mkdir -p $O
    cp -p $R/libredio_amd/_build_measure/*.o $O/
    rm -f $O/chain_v4.o
    make -C $R/libredio_amd/csrc -s -j16 OUT=$O EXTRA="-DREDIO_MEASURE -DREDIO_EXP_SEAM=$m" all
  done
else
  ROUNDS=${1:-2}; shift || true
  MASKS=${*:-0 1 2 4 8 15}
  cd $R
  for r in $(seq 1 $ROUNDS); do
    for m in $MASKS; do
      REDIO_BUILD_DIR=$R/tools/exp/_build_seam$m timeout -k 10 240 python3 tools/chain_seam_time.py "mask $m" 2>&1 | grep -v amdgpu.ids
    done
  done
fi
