#!/bin/bash
# Run ON the GPU box: bench.py against the default library and each A/B variant (tools/variant_build.sh), one line per variant:
#   bash tools/ab_bench.sh [steps=20] name1 name2 ...        (name "default" = nerf-ca_amd/lib/libnerfca_hip.so)
STEPS=${1:-20}; shift
OUT=${OUT:-bench_out}; mkdir -p $OUT
for N in "$@"; do
  LIB=nerf-ca_amd/lib/libnerfca_hip_$N.so; [ "$N" = default ] && LIB=nerf-ca_amd/lib/libnerfca_hip.so
  NERFCA_LIB=$PWD/$LIB timeout -k 10 240 python3 bench.py --full --steps $STEPS --warmup 3 --no-extras --no-cpu-baseline --full-record $OUT/ab_${N}_full.json > $OUT/ab_$N.json 2> $OUT/ab_$N.err
  rc=$?
  [ $rc -ge 124 ] && { echo "$N: killed ($rc)"; exit $rc; }
  python3 - "$N" "$OUT" <<'PY'
import json, sys
n, o = sys.argv[1], sys.argv[2]
try:
    b = json.load(open(f"{o}/ab_{n}_full.json"))
    k = b["roofline"]["all_kernels"]
    print(f"{n:14s} graph {b['ms_per_step']:.3f} ms  eager {b['eager_ms_per_step']:.3f}  " + "  ".join(f"{x} {k[x]['ms_per_step']:.3f}" for x in ("fwd", "bwd_dgrad", "bwd_wgrad", "loss", "bwd_reduce")) + f"  loss {b['final_loss']:.6e}", flush=True)
except Exception as e:
    print(n, "failed:", e, open(f"{o}/ab_{n}.err").read()[-400:])
PY
done
