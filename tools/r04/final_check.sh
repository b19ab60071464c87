# end-of-round check on the GPU box: the whole -m gpu suite, smoke(), the full bench line
timeout 700 python -m pytest tests -m gpu -x -q 2>&1 | tail -1
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
B=$(mktemp)
python bench.py --full --steps 20 --warmup 5 2>/dev/null | tail -1 > $B
python - "$B" <<'P'
import json, sys
d = json.loads(open(sys.argv[1]).read())
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['config3_step'].get('ms_per_step'), d['config4_step'].get('ms_per_step'))
P
