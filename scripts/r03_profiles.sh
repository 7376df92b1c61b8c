#!/bin/bash
# Round-3 evidence, one GPU box call: HBM traffic of the merge and of the intersection (FETCH_SIZE / WRITE_SIZE passes), the SQ
# counters of the merge kernels (where scripts/pmc_run.sh and pmc_merge_sq.sh put them), kernel-trace stats of the whole bench
# (under $PROF_OUT/r03/bench).
cd $GRAFT_REPO_ROOT
scripts/pmc_run.sh r03/pmc_merge ii2::k_mp_terms 3 scripts/merge_loop.py steps=3 || echo "pmc merge failed"
scripts/pmc_run.sh r03/pmc_isect ii2::k_dense_tiles 20 scripts/c2_loop.py steps=20 || echo "pmc isect failed"
scripts/pmc_merge_sq.sh r03/sq_merge terms=1000000 > gpurun_out/prof/r03/sq_merge.log 2>&1 || echo "sq merge failed"
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${PROF_OUT:?set PROF_OUT to the directory the bench profile goes to}/r03
mkdir -p $out/bench
timeout -k 5 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/bench -o bench -- python3 bench.py --full --steps 20 --warmup 5 > $out/bench.json 2> $out/bench.err || echo "bench profile failed"
ls $out $out/*
