#!/bin/bash
# Session of the weight-chunks-by-LDS-DMA change of fused_layer_ws.hip: the product build (W by global_load_lds) against
# the PARENT commit's build and against the -DPDR_LAB_W_REGS build of the same source (W through registers).
#   bash tools/lab/ws_weight_dma_session.sh PARENT.so WREGS.so STAGE...
#     PARENT.so  libpdr_hip.so of the parent commit (`make -C point_diffusion_refinement_amd/csrc` in a checkout of it)
#     WREGS.so   this commit built with FLAGS += -DPDR_LAB_W_REGS
#     STAGE      identity | kernels | trace | step | forms     (any number, in this order; STEP_REPS / FORM_REPS:
#                alternating repetitions of the last two, default 3)
# A process loads the in-tree libpdr_hip.so and nothing else, so the script copies the build under test there and
# puts the product back at the end (also when a step fails).  Every GPU step has its own time limit; the first
# failure, time limit or signal ends the script.  Results: $WDMA_OUT/wdma_*.txt
# (default: $TMPDIR/wdma) -> profiles/ws_weight_dma_ab.txt.
set -euo pipefail
PARENT=$1; WREGS=$2; shift 2
L=point_diffusion_refinement_amd/libpdr_hip.so
export TMPDIR=${TMPDIR:-/tmp}
O=${WDMA_OUT:-$TMPDIR/wdma}
mkdir -p $O
CHILD=$(mktemp $TMPDIR/wdma_child.XXXXXX)
cp $L $CHILD
trap 'cp $CHILD $L; rm -f $CHILD' EXIT
use() { case $1 in parent) cp "$PARENT" $L;; wregs) cp "$WREGS" $L;; child) cp $CHILD $L;; esac; }
ms() { python -c "import sys,json; print(json.loads(sys.stdin.read().strip().splitlines()[-1])['ms_per_step'])"; }

for stage in "$@"; do
case $stage in
identity)
  # outputs and statistics rows byte for byte: product vs register staging vs parent; four reverse steps at B = 8
  {
  for b in wregs parent child; do
    use $b
    echo "== $b"
    timeout -k 10 300 python -m tools.lab.ws_weight_dma_identity $O/wdma_id_$b.json $([ $b = wregs ] || echo $O/wdma_id_wregs.json)
    ORDER_CHECK_B=8 timeout -k 10 300 python -m tools.lab.order_check $O/wdma_steps_$b.pt $([ $b = wregs ] || echo $O/wdma_steps_wregs.pt) > $O/wdma_steps_$b.log 2>&1
    grep identical $O/wdma_steps_$b.log || echo "four reverse steps at B = 8 written"
  done
  } 2>&1 | tee $O/wdma_identity.txt
  rm -f $O/wdma_steps_*.pt $O/wdma_steps_*.log
  if grep -q " [1-9][0-9]* differ\|identical to .*: False" $O/wdma_identity.txt; then echo "NOT IDENTICAL"; exit 1; fi
  ;;
kernels)
  # kernels alone on the chip: the shapes of profiles/r5_lds_counter_handover_ab.txt + a residual-gathered
  # 16384 x 171 -> 128 (ball and kNN form), narrow and 64-column outputs, split-f16; two alternating repetitions per build
  FB="timeout -k 10 200 python -m tools.fused_layer_bench --reps 50"
  {
  for rep in 1 2; do
    for b in parent child; do
      use $b
      echo "== rep $rep $b"
      echo -n "knn8    "; $FB --only 0 --gath 8 --knn | grep rpb
      echo -n "knn8b   "; $FB --only 2 --gath 8 --knn | grep rpb
      echo -n "ball32  "; $FB --only 0 --gath 32 | grep rpb
      echo -n "plain   "; $FB --only 0 | grep rpb
      echo -n "rg171   "; $FB --only 1 --gath 8 --rg | grep rpb
      echo -n "rg171k  "; $FB --only 1 --gath 8 --knn --rg | grep rpb
      echo -n "p256    "; $FB --only 14 | grep rpb
      echo -n "p512    "; $FB --only 13 | grep rpb
      echo -n "d512    "; $FB --only 6 | grep rpb
      echo -n "n32     "; $FB --only 8 | grep rpb
      echo -n "n41     "; $FB --only 10 | grep rpb
      echo -n "m64     "; $FB --only 9 | grep rpb
      echo -n "split   "; $FB --only 0 --split | grep rpb
    done
  done
  } 2>&1 | tee $O/wdma_kernels.txt
  ;;
trace)
  # kernel trace of the benchmark, a run of its own without counters: per-instantiation averages of the layer kernel
  for b in parent child; do
    use $b
    rm -rf $O/wdma_trace_$b
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/wdma_trace_$b -o t --output-format csv -- \
      python bench.py --gpus 1 --steps 20 --warmup 5 > $O/wdma_trace_$b.log 2>&1
    python tools/lab/ws_weight_dma_trace.py $O/wdma_trace_$b > $O/wdma_trace_$b.txt
    rm -rf $O/wdma_trace_$b
  done
  paste -d'|' $O/wdma_trace_parent.txt $O/wdma_trace_child.txt | tee $O/wdma_trace.txt
  ;;
step)
  # the step: alternating parent / child processes, every value
  {
  for i in $(seq ${STEP_REPS:-3}); do
    for b in parent child; do
      use $b
      echo -n "$b adaptive "; timeout -k 10 400 python bench.py --gpus 1 --steps 100 --warmup 5 2>/dev/null | ms
    done
  done
  } 2>&1 | tee $O/wdma_step.txt
  ;;
forms)
  {
  for i in $(seq ${FORM_REPS:-3}); do
    for b in parent child; do
      use $b
      echo -n "$b whole "; timeout -k 10 400 python bench.py --gpus 1 --steps 100 --warmup 5 --neighbourhoods whole 2>/dev/null | ms
      echo -n "$b split_f16 "; timeout -k 10 400 python bench.py --gpus 1 --steps 100 --warmup 5 --precision split_f16 2>/dev/null | ms
    done
  done
  } 2>&1 | tee $O/wdma_forms.txt
  ;;
*) echo "unknown stage $stage"; exit 2;;
esac
done
