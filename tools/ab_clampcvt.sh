#!/bin/bash
# interleaved A/B on one box: shipping library vs the DFN_EXP_CLAMPCVT build, head activations scaled by 1/16 in both
OUT="${AB_OUT:-/tmp/ab_clampcvt}"
mkdir -p "$OUT"
export DFN_BENCH_ACT_SCALE=0.0625
ARGS="--workload c2 --steps 60 --warmup 10 --sustain-seconds 0 --no-cpu-baseline --no-extra --full"
for r in 1 2 3; do
  python bench.py $ARGS 2>/dev/null | grep "^{" > "$OUT/ship_$r.json"
  DFN_LIB=$PWD/exp_libs/libdfanerf_clampcvt.so python bench.py $ARGS 2>/dev/null | grep "^{" > "$OUT/exp_$r.json"
done
ARGS_C1="--workload c1 --steps 100 --warmup 10 --sustain-seconds 0 --no-cpu-baseline --no-extra --full"
DFN_LIB=$PWD/exp_libs/libdfanerf_clampcvt.so python bench.py $ARGS_C1 2>/dev/null | grep "^{" > "$OUT/exp_c1.json"
python bench.py $ARGS_C1 2>/dev/null | grep "^{" > "$OUT/ship_c1.json"
AB_OUT="$OUT" python - <<'P'
import json,glob,os
for f in sorted(glob.glob(os.path.join(os.environ['AB_OUT'], '*.json'))):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1]); pc=d.get('parity_check',{})
        print(f.split('/')[-1], round(d['ms_per_step'],3), round(d['roofline']['frac'],4), round(d['roofline']['clock_ghz'],3), pc.get('psnr_db'), pc.get('max_abs_rgb'), (pc.get('vs_oracle_pipeline') or {}).get('psnr_db'))
    except Exception as e: print(f, 'ERR', e)
P
