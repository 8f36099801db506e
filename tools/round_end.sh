#!/bin/bash
# Round-end measurement with the final binary: the full bench line (bench.py --full), the 1-rank RCCL smoke of the multi-GPU path, the strong-scaling preview.
# (tools/profile_round.sh: the rocprofv3 passes over the same bench command; tools/gpu_suite.sh: the whole GPU test suite.)
OUT=${OUT:-bench_logs}     # log directory
mkdir -p $OUT
python bench.py --full > $OUT/bench_final.log 2>&1; tail -c 600 $OUT/bench_final.log; echo
MVE_BENCH_FORCE_DIST=1 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 1 --steps 2 --warmup 1 --no-extra --no-secondary --no-cpu-baseline > $OUT/bench_dist_smoke.log 2>&1; tail -c 400 $OUT/bench_dist_smoke.log; echo
python tools/scale_preview.py > $OUT/scale_preview.log 2>&1; grep -v amdgpu $OUT/scale_preview.log
# (round 5) everything of a round's end in one gpurun call: PROF_TAG=rNN bash tools/profile_round.sh; python __graft_entry__.py smoke; bash tools/gpu_suite.sh; bash tools/round_end.sh
