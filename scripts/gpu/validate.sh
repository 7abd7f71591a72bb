#!/bin/bash
# Validation of the current tree: GPU suite, smoke, 2-rank shared-GPU run,
# configs 2 and 3 (bench.py --full: each run checks its residual)
set -o pipefail
OUT=${VALIDATE_OUT:-validate_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export PYTHONUNBUFFERED=1
timeout -k 10 900 python3 -u -m pytest --maxfail=6 -v --timeout 150 --timeout-method thread -m gpu tests/ > $OUT/suite.log 2>&1
rc0=$?
tail -3 $OUT/suite.log; grep -E "FAILED|ERROR" $OUT/suite.log | head -10
[ $rc0 -le 1 ] &&
timeout -k 10 200 python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 &&
timeout -k 10 240 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29581 \
   bench.py --gpus 2 --size 16384 --nb 512 --steps 3 --warmup 1 --share-gpu --cores 3 --full > $OUT/m2.log 2>&1 &&
timeout -k 10 200 python3 bench.py --size 16384 --nb 512 --steps 5 --warmup 1 --full > $OUT/b16.log 2>&1 &&
timeout -k 10 240 python3 bench.py --steps 5 --warmup 1 --full > $OUT/b64.log 2>&1
rc=$?
tail -1 $OUT/smoke.log; grep -h '^{' $OUT/m2.log $OUT/b16.log $OUT/b64.log | cut -c1-220
exit $((rc0 + rc))
