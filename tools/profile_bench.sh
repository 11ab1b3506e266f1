#!/bin/bash
# Collects the rocprofv3 evidence for bench.py on the GPU box: kernel-trace stats, then separate PMC passes
# (counters are never combined with tracing domains other than --kernel-trace).
# usage (on the GPU box): bash tools/profile_bench.sh <tag>[:<set>] [bench args...]
#   <set>  all (default): every pass below
#          solver: what a change of the solver kernel needs and tools/summarize_profile.py reads for <tag>_pmc_traffic.json --
#                  the kernel trace with --stats, the SQ_INSTS_VALU group (pmc1), FETCH_SIZE (pmc3), WRITE_SIZE (pmc4)
#          trace / valu / traffic / fast: one part of it (the trace alone, pmc1 alone, pmc3 + pmc4, the three fast-build passes)
# Every pass is a GPU step of its own: it runs under a time limit sized to a 4-step bench.py run (PROFILE_PASS_TIMEOUT seconds,
# default 240), and the first pass that fails, faults or runs into its limit ends the script -- nothing more is started on the card.
set -u -o pipefail
SPEC=${1:-r01}; shift || true
TAG=${SPEC%%:*}
SET=all; [ "$SPEC" != "$TAG" ] && SET=${SPEC#*:}
case "$SET" in
  all)     PASSES="trace pmc1 pmc2 pmc5 pmc6 pmc7 pmc3 pmc4 fast_trace fast_pmc1 fast_pmc5" ;;
  solver)  PASSES="trace pmc1 pmc3 pmc4" ;;
  trace)   PASSES="trace" ;;
  valu)    PASSES="pmc1" ;;
  traffic) PASSES="pmc3 pmc4" ;;
  fast)    PASSES="fast_trace fast_pmc1 fast_pmc5" ;;
  *) echo "profile_bench.sh: unknown set '$SET' (all, solver, trace, valu, traffic, fast)" >&2; exit 2 ;;
esac
LIMIT=${PROFILE_PASS_TIMEOUT:-240}
cd "$(dirname "$0")/.."
ROOT=$PWD
export TMPDIR=/tmp
OUT=$ROOT/gpurun_out/prof_$TAG; rm -rf "$OUT"
mkdir -p "$OUT"
ARGS="--steps 3 --warmup 1 --no-cpu-baseline --no-secondary --no-fast-build $*"

counters_of() {
  case "${1#fast_}" in
    pmc1) echo "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_ANY" ;;
    pmc2) echo "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_ANY" ;;
    pmc5) echo "SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_INT32 SQ_INSTS_VALU_CVT SQ_INSTS_BRANCH SQ_INSTS_SMEM" ;;
    pmc6) echo "SQ_ACTIVE_INST_VALU2 SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_SCA SQ_INST_CYCLES_SALU SQ_BUSY_CU_CYCLES SQ_INST_LEVEL_LDS SQ_LDS_ADDR_CONFLICT SQ_LDS_UNALIGNED_STALL" ;;
    pmc7) echo "GRBM_GUI_ACTIVE SQ_CYCLES SQ_LDS_DATA_FIFO_FULL SQ_LDS_CMD_FIFO_FULL SQ_IFETCH SQ_INSTS_LDS_LOAD SQ_INSTS_LDS_STORE SQ_INSTS_LDS_ATOMIC" ;;
    pmc3) echo "FETCH_SIZE" ;;
    pmc4) echo "WRITE_SIZE" ;;
  esac
}

# one pass = one rocprofv3 run of bench.py under its own time limit; a non-zero status is handed to the caller, which stops
run_pass() {
  local name=$1 build=parity
  case "$name" in fast_*) build=fast ;; esac   # the opt-in fast build of the same kernel: stats + the two groups that carry its instruction count and mix
  local -a mode
  if [ "${name#fast_}" = trace ]; then mode=(--kernel-trace --stats -d "$OUT/$name" -o trace)
  else mode=(--kernel-trace --pmc $(counters_of "$name") -d "$OUT/$name" -o pmc); fi
  echo "[profile_bench] pass $name (limit ${LIMIT}s)"
  ( cd /tmp && PDP_BUILD=$build timeout -k 10 "$LIMIT" rocprofv3 --output-format csv "${mode[@]}" -- python3 "$ROOT/bench.py" $ARGS ) > "$OUT/bench_$name.log" 2>&1
}

for pass in $PASSES; do
  run_pass "$pass"; rc=$?
  if [ $rc -ne 0 ]; then
    echo "[profile_bench] pass $pass ended with status $rc: stopping here, the passes behind it were not started" >&2
    tail -5 "$OUT/bench_$pass.log" >&2
    exit $rc
  fi
done
cd "$ROOT"
python3 tools/summarize_profile.py "$OUT" > "$OUT/summary.txt" 2>&1 || exit $?
case " $PASSES " in *" fast_trace "*) python3 tools/summarize_profile.py "$OUT" fast_ > "$OUT/summary_fast.txt" 2>&1 || true ;; esac
cat "$OUT/summary.txt"
case " $PASSES " in *" trace "*) tail -2 "$OUT/bench_trace.log" ;; esac
