#!/bin/bash
# rocprofv3 --pmc passes of one serial bench.py run on the GPU box (counters only: no trace domains, as the pool requires).
# usage: bash profiles/run_pmc.sh <tag> "<COUNTER ...>" [bench args...]  -> $OUT/pmc_<tag>/pmc_counter_collection.csv (OUT: profiles/out)
tag=$1; shift
ctrs=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profiles/out}
mkdir -p "$OUT"
rocprofv3 --pmc $ctrs --output-format csv -d $OUT/pmc_$tag -o pmc -- python3 bench.py --no-pipeline --no-cpu-baseline --no-stage-timing "$@" > $OUT/pmc_$tag.log 2>&1
ls $OUT/pmc_$tag | head
