#!/bin/bash
# Health round: smoke, then the C3 (default, with its roofline), C4 and C1 bench lines.
# Logs and lines go to $LLM_RECORD_DIR (default build/records).
set -o pipefail
O=${LLM_RECORD_DIR:-build/records}
mkdir -p $O
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { cat $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
timeout -k 10 400 python bench.py --full > $O/bench_c3.json 2> $O/bench_c3.err || { tail -5 $O/bench_c3.err; exit 1; }
python -c "import json;d=json.load(open('$O/bench_c3.json'));print('c3',d['value'],d['ms_per_step'],d['roofline']['frac'])"
timeout -k 10 400 python bench.py --config c4 > $O/bench_c4.json 2> $O/bench_c4.err || { tail -5 $O/bench_c4.err; exit 1; }
python -c "import json;d=json.load(open('$O/bench_c4.json'));print('c4',d['value'],d['ms_per_step'])"
timeout -k 10 300 python bench.py --config c1 > $O/bench_c1.json 2> $O/bench_c1.err || { tail -5 $O/bench_c1.err; exit 1; }
python -c "import json;d=json.load(open('$O/bench_c1.json'));print('c1',d['value'],d['ms_per_step'])"
