cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${PROF_OUT:?set PROF_OUT to the directory the trace goes to}
mkdir -p $out/prof_pre
BENCH_PRETEND=${1:-3}/8 rocprofv3 --kernel-trace --output-format csv -d $out/prof_pre -o pre -- python3 bench.py --full --workload strong --steps 6 --warmup 2 > $out/pre.json 2> $out/pre.err
