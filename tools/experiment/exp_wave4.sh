# Does a 4th wave per SIMD pay?  The 2-node ping-pong needs 136 B of LDS per seed (4-node: 200 B), so four batches fit a CU.
export O=$(realpath -m "${1:?usage: exp_wave4.sh OUTDIR}"); mkdir -p "$O"; cd "$(dirname "$0")/../.."
for rep in 1 2; do for st in 2 3 4 5; do
timeout 300 python bench.py --full --nodes 2 --streams $st --steps 60 --warmup 8 --no-cpu-baseline --no-measure-traffic --no-first-fail --no-extras > "$O"/s.json 2> "$O"/s.err
python - $st <<'PY'
import json,os,sys
try:
    d=json.loads(open(os.environ['O']+'/s.json').read().strip().splitlines()[-1]); e=d['extra']
    print('nodes 2 streams',sys.argv[1],'ms/step',round(d['ms_per_step'],4),'Mseeds/s',round(e['seeds_per_sec']/1e6,2),'Gsteps/s',round(e['executor_steps_per_sec']/1e9,2),'lds',e['lds_bytes_per_seed'],'waves/cu',e['waves_per_cu'],'verified',d['verified_seeds'])
except Exception as ex: print('fail',sys.argv[1:],ex, open(os.environ['O']+'/s.err').read()[-400:])
PY
done; done | tee "$O"/wave4.txt
