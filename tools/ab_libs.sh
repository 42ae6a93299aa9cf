#!/bin/bash
# A/B alternative builds of libdpt.so on the bench workload (DPT_LIB=path), one process each.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
out=${DPT_OUT:-bench_out}; mkdir -p $out
for lib in "$@"; do
  tag=$(basename $(dirname $lib))_$(basename $lib .so)
  DPT_LIB=$PWD/$lib timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --exact-sample 65536 > $out/bench_$tag.log 2>&1 || { tail -5 $out/bench_$tag.log; exit 1; }
  tail -1 $out/bench_$tag.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$tag', 'GB/s %.2f' % (d['value']/1e9), 'exact', d['exact_match']['rate'], 'stages', {k: round(v,3) for k,v in d['stage_ms_per_step'].items()})"
done
