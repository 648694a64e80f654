#!/bin/bash
# streaming extra of bench.py with and without the per-call flow cache; the lines go to the directory given (default bench_out/)
cd "$(dirname "$0")/.."
OUT=${1:-bench_out}
mkdir -p "$OUT"
python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/stream_cache_on.json" 2> "$OUT/stream_cache_on.err"
CV2_FLOW_CACHE=0 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > "$OUT/stream_cache_off.json" 2> "$OUT/stream_cache_off.err"
OUT="$OUT" python - <<'P'
import json, os
out = os.environ['OUT']
for f in ('on','off'):
    try:
        d=json.loads(open(f'{out}/stream_cache_{f}.json').read().strip().splitlines()[-1])
        print(f, json.dumps(d['extra']['streaming'], indent=None)[:1500])
    except Exception as e:
        print(f, 'ERR', e); print(open(f'{out}/stream_cache_{f}.err').read()[-3000:])
P
