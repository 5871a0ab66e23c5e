#!/bin/bash
# Multi-rank logic of bench.py on a 1-GPU box: N ranks share GPU 0 and exchange through gloo (host copies).
# With --full, so that the N-rank file leg (end_to_end.genome_frag_delfi_api_ranks) runs too.
# usage: tools/bench_2rank_1gpu.sh [N=2] [extra bench.py args]   (rank r's stderr: $LOG_DIR/rank<r>.err, default .)
N=${1:-2}; shift
export MASTER_ADDR=127.0.0.1 MASTER_PORT=29571 WORLD_SIZE=$N LOCAL_RANK=0 FTK_BENCH_DIST_BACKEND=gloo
pids=()
for r in $(seq 1 $((N-1))); do RANK=$r python bench.py --gpus $N --full --no-cpu-baseline "$@" > /dev/null 2> "${LOG_DIR:-.}/rank$r.err" & pids+=($!); done
RANK=0 timeout 600 python bench.py --gpus $N --full --no-cpu-baseline "$@"
rc=$?
for p in "${pids[@]}"; do wait $p || rc=$?; done
exit $rc
