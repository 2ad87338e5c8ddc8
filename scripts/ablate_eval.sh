# diagnostic (wrong results for ablate != 0): 1 = no collision work, 2 = no scalar warm-up loads
for a in 0 1 2; do
  echo -n "ablate=$a "; FOT_EVAL_ABLATE=$a timeout -k 10 120 python bench.py --full --steps 50 --warmup 5 --overlap 1 --no-cpu-baseline --no-latency --no-parity 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().split('\n')[-1]); print(d['kernel_ms']['k_evaluate'], d['ms_per_step'])" || echo failed
done
