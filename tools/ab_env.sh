#!/bin/bash
# Generic A/B over environment settings on the whole forward (B = 32): bash tools/ab_env.sh "VAR=1 VAR2=0" "VAR=0" ...
# Each arm's throughput and per-kernel lines go to $AB_ENV_LOG (default build/ab_env.log, relative to the repository root).
cd "$(dirname "$0")/.." || exit 1
log="${AB_ENV_LOG:-build/ab_env.log}"; mkdir -p "$(dirname "$log")"
: > "$log"
for arm in "$@"; do
  echo "== $arm" >> "$log"
  env $arm timeout 300 python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-fast --no-aligner 2>&1 >/dev/null | grep -E "pairs/s|per-kernel|linear cfg|conv cfg|attention|other" | head -18 >> "$log"
done
grep -E "==|pairs/s" "$log"
