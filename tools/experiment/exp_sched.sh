export O=$(realpath -m "${1:?usage: exp_sched.sh OUTDIR}"); mkdir -p "$O"; cd "$(dirname "$0")/../.."
for sched in 0 1; do for seeds in 196608 786432 3145728; do for st in 1 2; do
MADSIM_BENCH_SCHED=$sched timeout 300 python bench.py --full --seeds $seeds --streams $st --steps 6 --warmup 2 --no-cpu-baseline --no-measure-traffic --no-first-fail --no-extras > "$O"/s.json 2> "$O"/s.err
python - $sched $seeds $st <<'PY'
import json,os,sys
try:
    d=json.loads(open(os.environ['O']+'/s.json').read().strip().splitlines()[-1]); e=d['extra']
    print('sched',sys.argv[1],'seeds',sys.argv[2],'streams',sys.argv[3],'ms/step',round(d['ms_per_step'],3),'Mseeds/s',round(e['seeds_per_sec']/1e6,2),'verified',d['verified_seeds'])
except Exception as ex: print('fail',sys.argv[1:],ex, open(os.environ['O']+'/s.err').read()[-300:])
PY
done; done; done | tee "$O"/sched.txt
