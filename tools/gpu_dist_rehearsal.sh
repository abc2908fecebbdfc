# Multi-rank bench rehearsal on a one-GPU box: two ranks share the card over gloo (the driver's N-GPU runs use RCCL,
# one rank per GPU); exercises bench.py's distributed path end to end (ring cameras, bucketed exchange, barriers,
# max-over-ranks timing, rank-0 line).  The log goes to $HLGS_OUT (default out/).
set -u
cd "$(dirname "$0")/.."
O=${HLGS_OUT:-out}
mkdir -p $O
HLGS_DIST_BACKEND=gloo timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 \
  --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 2 --steps 5 --warmup 2 > $O/dist2.log 2>&1
rc=$?; echo "dist rc=$rc"; tail -4 $O/dist2.log; exit $rc
