#!/bin/bash
# Training-side profiles of a round (GPU box): rocprofv3 kernel stats of bench.py --mode train, the torch-profiler kernel split of one step,
# the --full bench line and the batch sweep.  Usage: scripts/prof_round_train.sh <output folder>, a folder beside the prof_train/ that
# scripts/prof_stats.sh writes; scripts/collect_profiles.py does not touch these - copy them by hand.
set -u
cd ${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${1:?usage: scripts/prof_round_train.sh <output folder>}; PROF=$(dirname "$OUT")/prof_train
mkdir -p "$OUT"
timeout 300 scripts/prof_stats.sh train --full --mode train --steps 100 --warmup 10 > /dev/null 2>&1
python scripts/summarize_stats.py "$PROF/kernel_stats.csv" "$OUT/train_kernel_stats.txt" "r06: bench.py --full --mode train --steps 100 --warmup 10 (captured step replayed 110 times + 3 eager warm-up + 3 eager split steps: 116 steps; divide calls by 116)"
cp "$PROF/bench.json" "$OUT/bench_train.json"
{ echo "# scripts/prof_train_steady.py 32 90 (torch.profiler, device activities, 5 eager steps after warm-up; round 6 HEAD): device time per kernel of one training step at 32 clips"; python scripts/prof_train_steady.py 32 90 2>&1 | grep -v -i "warn\|amdgpu"; } > "$OUT/train_step_split.txt"
python bench.py --full --steps 20 --warmup 5 > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"
{ echo "# scripts/diag_batch_sweep.py, round 6 (one MI355X box): steady-state DDPM step, library's kernel choice and slicing"; python scripts/diag_batch_sweep.py 2>&1 | grep -v amdgpu; } > "$OUT/diag_batch_sweep.txt"
python scripts/diag_stack_train.py 32 2>&1 | grep -v amdgpu > "$OUT/diag_stack_train.txt"
tail -3 "$OUT/train_step_split.txt"; head -c 300 "$OUT/bench_default.json"; echo; tail -5 "$OUT/diag_batch_sweep.txt"
