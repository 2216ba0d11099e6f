#!/bin/bash
# Round-3 measurements of HEAD: config-1 drop-in lines (trot and STANDING, with the CPU
# port beside them), config-2 phase stamps (stamps build) and SQ counter passes.
#   gpurun -- 'TAG=r3_prof bash tools/gpu_r3_prof.sh'
set -o pipefail
cd $GRAFT_REPO_ROOT
export RUN_OUT=${RUN_OUT:-run_out}   # where this script writes
mkdir -p $RUN_OUT
T=${TAG:-r3_prof}
timeout -k 10 240 python bench.py --full --config config1 > $RUN_OUT/${T}_c1_trot.json || exit 1
tail -1 $RUN_OUT/${T}_c1_trot.json | cut -c1-400
timeout -k 10 300 python bench.py --full --config config1 --gait standing --steps 100 --warmup 10 > $RUN_OUT/${T}_c1_standing.json || exit 1
tail -1 $RUN_OUT/${T}_c1_standing.json | cut -c1-400
timeout -k 10 120 python tools/phase_stamps.py 1024 10 trot10 > $RUN_OUT/${T}_stamps_c2.txt 2>&1 || { cat $RUN_OUT/${T}_stamps_c2.txt; exit 1; }
head -20 $RUN_OUT/${T}_stamps_c2.txt
bash tools/pmc_sq.sh ${T}_c2 --config config2 > $RUN_OUT/${T}_sq_c2.txt 2>&1 || { tail -20 $RUN_OUT/${T}_sq_c2.txt; exit 1; }
cat $RUN_OUT/${T}_sq_c2.txt
