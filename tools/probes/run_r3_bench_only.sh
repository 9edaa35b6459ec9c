#!/bin/bash
# the default bench line with every leg (--full; no profiler), into $O/r03_bench_default_line.json
set -o pipefail
export O=${NVH_PROBE_OUT:-probe_out}
mkdir -p $O
timeout -k 10 600 python3 bench.py --full > $O/bench_default.log 2>$O/bench_default.err || { tail -5 $O/bench_default.err; exit 1; }
tail -1 $O/bench_default.log > $O/r03_bench_default_line.json
python3 - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['O'], 'r03_bench_default_line.json')).read())
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['us_per_launch'])
for k,v in d['prefill'].items(): print(k, {kk:v[kk] for kk in ('us_per_launch','us_per_launch_inputs_in_infinity_cache','achieved_TFLOPs','achieved_GBps','frac')})
PY
