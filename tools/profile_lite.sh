#!/bin/bash
# The rocprofv3 evidence of a round: kernel stats (one frame at a time, and three in flight) and the PMC counters
# (SQ_*, FETCH_SIZE, WRITE_SIZE: three separate passes; counters never share a run with a trace domain other than the
# kernel trace) for each of the benched workloads.  The profiled process is tools/tune_sweep.py -- the same C-ABI calls as
# bench.py's timed region, without the torch import.
#   gpurun --timeout 900 -- 'bash tools/profile_lite.sh r04 B C T E'   then here:   python tools/profile_summary.py r04
set -u
exec < /dev/null
TAG=${1:-r04}
shift
WL=${@:-B}
R=$(pwd)
OUT=$R/gpurun_out/prof_$TAG
mkdir -p "$OUT"
python -c "import __graft_entry__ as e; print(e.load_package().binding.library_source_hash())" > "$OUT/source_hash.txt"
cd /tmp && export TMPDIR=/tmp
# counter passes: enough untimed frames ahead of the three counted ones that the renderer has settled -- the depth-order level (config C
# refines its bins and steps down to k_bin_fast<12> on the first clean frame), and the blend's lockstep, which it measures over 55 to 125 frames
PW=${GS_PROFILE_WARM:-200}
# a step that fails -- a fault, a hang cut off by its time limit -- ends the collection: nothing more is started on that GPU
step() { timeout -k 10 120 "$@" > /dev/null 2>&1; local rc=$?; [ $rc -eq 0 ] || { echo "step failed (exit $rc): $*"; exit $rc; }; }
PMC="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_ANY"
for W in $WL; do
  case $W in
    B) ARGS="--gaussians 1000000 --width 1920 --height 1080 --scene S"; FR=300;;
    C) ARGS="--gaussians 6000000 --width 1920 --height 1080 --scene S"; FR=100;;
    T) ARGS="--gaussians 6000000 --width 1920 --height 1080 --scene T"; FR=100;;
    E) ARGS="--gaussians 6000000 --width 3840 --height 2160 --scene S"; FR=60;;
    *) echo "unknown workload $W"; continue;;
  esac
  D="python $R/tools/tune_sweep.py --no-prime --batches 1 $ARGS"
  O=$OUT/$W
  mkdir -p "$O"/{default,serial,pmc,fetch,write}
  # The blend's lockstep is the renderer's own choice, measured over its first 60-130 frames -- frames a profiler would average into every
  # kernel's row.  One unprofiled run reads the choice (three in flight, as shipped); the profiled runs below are PINNED to it.
  unset GS_BLEND_LOCKSTEP
  timeout -k 10 120 $D --fif 3 --frames 200 > "$O/unprofiled.txt" 2> /dev/null || { echo "step failed (exit $?): the unprofiled run of $W"; exit 1; }
  LS=$(grep "^fif" "$O/unprofiled.txt" | tail -1 | grep -o "lockstep [A-Za-z]*" | cut -d" " -f2)
  case "$LS" in True) export GS_BLEND_LOCKSTEP=1;; False) export GS_BLEND_LOCKSTEP=0;; *) unset GS_BLEND_LOCKSTEP;; esac
  echo "${LS:-unknown}" > "$O/lockstep.txt"
  step rocprofv3 --kernel-trace --stats --output-format csv -d "$O/serial" -o s -- $D --fif 1 --frames $FR --warm $PW --json-out "$O/serial/bench.json"
  step rocprofv3 --kernel-trace --stats --output-format csv -d "$O/default" -o d -- $D --fif 3 --frames $FR --warm $PW --json-out "$O/default/bench.json"
  step rocprofv3 --kernel-trace --pmc $PMC --output-format csv -d "$O/pmc" -o p -- $D --fif 1 --frames 3 --warm $PW
  step rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$O/fetch" -o f -- $D --fif 1 --frames 3 --warm $PW
  step rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$O/write" -o w -- $D --fif 1 --frames 3 --warm $PW
  if [ "$W" = "B" ]; then  # the other blend modes' counters as well: exact (exp mode 2), unguarded v_exp_f32, and the opt-in fast blend
    mkdir -p "$O"/pmc_exact "$O"/pmc_hw "$O"/pmc_fast "$O"/serial_exact
    step rocprofv3 --kernel-trace --pmc $PMC --output-format csv -d "$O/pmc_exact" -o p -- $D --fif 1 --frames 3 --warm $PW --exp-mode 2
    step rocprofv3 --kernel-trace --pmc $PMC --output-format csv -d "$O/pmc_hw" -o p -- $D --fif 1 --frames 3 --warm $PW --exp-mode 1
    step rocprofv3 --kernel-trace --pmc $PMC --output-format csv -d "$O/pmc_fast" -o p -- $D --fif 1 --frames 3 --warm $PW --exp-mode 0 --contract 1
    step rocprofv3 --kernel-trace --stats --output-format csv -d "$O/serial_exact" -o s -- $D --fif 1 --frames $FR --warm $PW --exp-mode 2 --json-out "$O/serial_exact/bench.json"
  fi
done
# per-dispatch traces are large; the stats and counter CSVs are what is summarised
unset GS_BLEND_LOCKSTEP
find "$R/gpurun_out/prof_$TAG" -name '*_kernel_trace.csv' -delete
cd "$R"
ls -R "$OUT" | head -60
