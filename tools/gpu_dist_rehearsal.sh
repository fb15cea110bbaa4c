#!/bin/bash
# N=2 rehearsal of the whole bench on one GPU (two ranks share the device; gloo instead of
# RCCL, which cannot put two ranks on one GPU): every phase's distributed path runs.
#   tools/gpu_dist_rehearsal.sh OUT_DIR
O=${1:?usage: tools/gpu_dist_rehearsal.sh OUT_DIR}; mkdir -p "$O"; export TMPDIR=/tmp
BPK_DIST_BACKEND=gloo timeout -k 10 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 4 --warmup 1 --train-steps 2 --cifar-steps 2 --pinn-steps 2 --dps-steps 1 > "$O/bench_n2.log" 2> "$O/bench_n2.err" || { tail -30 "$O/bench_n2.err"; exit 1; }
cat "$O/bench_n2.log"
python tools/show_line.py "$O/bench_n2.log"; grep -o "\"pinn_losses\": \[[^]]*\]" "$O/bench_n2.log"
