#!/bin/bash
# Run where the GPU is: k_floor phase by phase (profiles/r12_floor_phases.txt).  The stage carries a phase stopwatch whose
# marks (5 tone paint, 6 group minima, 0 fold + mix, 1 accumulate + terms, 2 greedy split, 7 post settling + quantise /
# predict, 3 curve rows, 4 curve) double as exits: a scratch build with -DVAMD_STOP_AFTER=k ends every wave at mark k, so
# the builds' counters are cumulative and a phase's share is the difference of two neighbours.  (What the later stages
# make of a cut-off floor is garbage; only the floor's counters and its time are read.)  Build first, where the compiler is:
#   for k in 5 6 0 1 2 7 3; do tools/build_variant.sh fl_stop$k [-D...] -DVAMD_STOP_AFTER=$k; done
#   tools/build_variant.sh fl_full [-D...]; tools/build_variant.sh fl_count [-D...] -DVAMD_COUNT_CALLS
# Per build: one rocprofv3 --pmc pass of its own (counters per wave = per channel-block) over 32 768 stereo blocks, and the
# stage's HIP-event time from bench.py (131 072 stereo blocks).  Then the split loop's calls per channel-block (fl_count).
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
OUT=${1:-/tmp/fl_phases.txt}
cp vorbis_amd/libvorbis_amd.so /tmp/fl_keep.so
trap 'cp /tmp/fl_keep.so $R/vorbis_amd/libvorbis_amd.so' EXIT
for v in ${FL_VARIANTS:-stop5 stop6 stop0 stop1 stop2 stop7 stop3 full}; do
  [ -f ab/libfl_$v.so ] || continue
  cp ab/libfl_$v.so vorbis_amd/libvorbis_amd.so
  rm -rf /tmp/flp
  timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_THREAD_CYCLES_VALU SQ_WAVE_CYCLES -d /tmp/flp -o x -- python tools/prof_run.py 32768 1 > /dev/null 2> /tmp/flp.log || { echo "$v: counter run failed ($?)" | tee -a $OUT; tail -5 /tmp/flp.log; exit 1; }
  c=$(python tools/pmc_summary.py /tmp/flp/x_results.db | grep "^k_floor ")
  t=$(timeout -k 10 240 python bench.py --gpus 1 --steps 10 --warmup 2 --no-cpu-baseline --no-parity-sample --no-neighbours --no-workloads --no-host-fed 2>/dev/null |
      python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('floor %.4f ms  step %.4f ms' % (d['roofline']['kernels_ms_per_step']['floor'], d['ms_per_step']))") || { echo "$v: bench run failed" | tee -a $OUT; exit 1; }
  echo "$v  $t  $c" | tee -a $OUT
done
if [ -f ab/libfl_count.so ]; then
  cp ab/libfl_count.so vorbis_amd/libvorbis_amd.so
  timeout -k 10 120 python tools/fl_calls.py | tee -a $OUT
fi
