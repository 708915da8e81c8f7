# Round 6: the wave-specialised kernel's tap-table consumers (GV_WS_DIET=1) against the arithmetic form: parity tests, whole plans
# c3 / c5 alternating twice on one box, and every tile per layer shape with the table form on (profiles/r6_ws_diet_ab.txt).
#   OUT=DIR bash tools/r6_diet.sh        (on the GPU box; bench lines and tables under DIR)
OUT=${OUT:?set OUT to the output directory}
mkdir -p $OUT
timeout 900 python -m pytest tests/test_gpu_lowp.py -x -q -m gpu -k "ws" > $OUT/t_ws.txt 2>&1; echo "ws rc $?"; tail -n 6 $OUT/t_ws.txt
for p in c3 c5; do
for mode in nodiet diet nodiet diet; do
  if [ $mode = nodiet ]; then unset GV_WS_DIET; else export GV_WS_DIET=1; fi
  python bench.py --full --preset $p --no-cpu-baseline --no-traffic --no-exact > $OUT/diet_${p}_${mode}.json 2> $OUT/diet_${p}_${mode}.err
  python - <<PY
import json
d=json.loads(open("$OUT/diet_${p}_${mode}.json").read().strip().splitlines()[-1])
r=d.get("roofline",{})
print("${p} ${mode}: %.0f views/s, %.3f ms/step, conv %.3f ms, %.0f TF/s, frac %.4f | stages %s" % (d["value"], d["ms_per_step"], r.get("conv_ms_per_step",0), r.get("achieved",0), r.get("frac",0), {k: round(v["frac"],3) for k,v in r.get("stages",{}).items()}))
PY
done
done 2>&1 | tee $OUT/ws_diet_plan_ab.txt

export GV_WS_DIET=1
python tools/ws_probe.py bf16 both > $OUT/ws_probe_diet.txt 2>&1; tail -30 $OUT/ws_probe_diet.txt
