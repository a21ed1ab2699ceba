#!/bin/bash
# full round evidence: GPU tests (parity records), smoke, the plain bench line and the --full one
set -u
cd "$(dirname "$0")/.."
mkdir -p gpurun_out
export TMPDIR=/tmp
rm -f gpurun_out/parity.jsonl
echo "== tests"; date
timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider > gpurun_out/tests_full.log 2>&1; echo "tests rc=$?"
grep -E "passed|failed|FAILED|Error" gpurun_out/tests_full.log | tail -8
echo "== smoke"; date
timeout 600 python __graft_entry__.py smoke 2>&1 | tail -2
echo "== bench"; date
export OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout 300 python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/bench_line.json 2> $OUT/bench_line.err; echo "bench rc=$?"
timeout 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_full_line.json 2> $OUT/bench_full.err; echo "bench --full rc=$?"
tail -c 600 $OUT/bench_full.err
python - <<'PY'
import json, os
out = os.environ['OUT']
p=json.loads(open(os.path.join(out, 'bench_line.json')).read().strip().splitlines()[-1])
print('plain: encode', round(p['value']), 'frames/s', round(p['ms_per_step'],4), 'ms')
line=open(os.path.join(out, 'bench_full_line.json')).read().strip().splitlines()[-1]
c=json.loads(line)
print('full: encode', round(c['value']), 'frames/s', round(c['ms_per_step'],4), 'ms; roofline', c['roofline']['kernel'], round(c['roofline']['frac'],3), 'traffic', c['roofline']['traffic'])
print('compact line bytes', len(line), 'sample', c['sample']['value'], 'parity', c['parity'], 'legs', c['legs'])
print('cpu', c['cpu_baseline'])
PY
echo "== done"; date
