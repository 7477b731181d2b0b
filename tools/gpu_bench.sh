#!/bin/bash
# bench + rocprofv3 kernel-trace stats of the same command (summaries are copied to profiles/ by hand afterwards).
# Both runs load the committed igemm tile choices (profiles/tune_cache.json), so the profiled run launches the same kernels.
R=${GRAFT_REPO_ROOT:-$(pwd)}
export OUT=$(cd "$R" && mkdir -p "${OUT:-results}" && cd "${OUT:-results}" && pwd)      # results folder: $OUT, default results/ in the repository
timeout 900 python bench.py --full "$@" > $OUT/bench.json 2> $OUT/bench.err
tail -c 6000 $OUT/bench.json; tail -5 $OUT/bench.err
cd /tmp && export TMPDIR=/tmp
RAW=/tmp/icaf_raw; mkdir -p $RAW; rm -rf $RAW/prof
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $RAW/prof -o bench -- python $R/bench.py --full "$@" --no-cpu-baseline --no-latency --no-h2d > $OUT/prof_bench.json 2> $OUT/prof.err
tail -3 $OUT/prof.err
f=$(find $RAW/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $OUT/prof_kernel_stats.csv && cut -c1-160 "$f" | head -25
