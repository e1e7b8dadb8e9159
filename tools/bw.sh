#!/bin/bash
# Development: one short bench line per workload given (default cfg2..cfg5), no CPU / e2e legs.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(pwd)}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for w in ${@:-cfg2 cfg3 cfg4 cfg5}; do
  timeout -k 10 200 python bench.py --full --workload $w --no-cpu-baseline --no-e2e > $OUT/b.json 2> $OUT/b.err || { tail $OUT/b.err; exit 1; }
  python -c "import json;d=json.load(open('$OUT/b.json'));print('$w', round(d['value']/1e9,2), 'G ev/s', round(d['ms_per_step'],4), {k: round(v*1e3,1) for k,v in d['device_ms_per_step'].items()}, 'host', round(d['host_issue_ms_per_step']*1e3,1), 'sb', d['config']['superbuckets'], 'frac', round(d['roofline']['frac'],3), round(d['roofline_merge']['frac'],3))"
done
