#!/bin/bash
# rocprofv3 --pmc passes of the training step (counters only: no trace domains, as the pool requires; program directly after `--`).
# usage: bash profiles/run_pmc_train.sh <tag> "<COUNTER ...>" [bench args...]  -> $OUT/pmc_<tag>/pmc_counter_collection.csv (OUT: profiles/out)
# PS_BENCH_NO_PREHEAT: the run is 1 (first) + W + K steps, nothing else (--no-stage-timing: no profiled extra steps)
tag=$1; shift
ctrs=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profiles/out}
mkdir -p "$OUT"
export PS_BENCH_NO_PREHEAT=1
rocprofv3 --pmc $ctrs --output-format csv -d $OUT/pmc_$tag -o pmc -- python3 bench.py --mode train --no-cpu-baseline --no-stage-timing --steps 2 --warmup 1 "$@" > $OUT/pmc_$tag.log 2>&1
ls $OUT/pmc_$tag | head
