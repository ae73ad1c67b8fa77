#!/bin/bash
# bench.py's fixed priming (PRIME_STEPS untimed env steps before the warm-up) against a single priming step, on the
# headline as the driver runs it (--steps 20 --warmup 5, cpu_baseline first), alternating; and the headline over a 1 s
# window (--steps 2500) with a single priming step, the steady-state rate.  tools/priming_ab.sh [rounds]
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"
run() {   # run <priming steps> <bench args...>
  local p=$1; shift
  python3 -c "import sys, bench; bench.PRIME_STEPS = int(sys.argv[1]); sys.argv = ['bench.py'] + sys.argv[2:]; bench.main()" \
    "$p" --gpus 1 --also-seconds 0 "$@" 2>/dev/null | python3 -c "import json,sys; d=json.loads(sys.stdin.read());
print('priming %4d  steps %5d  %.1f M sims/s  %.4f ms/step' % ($p, d['steps'], d['value'] / 1e6, d['ms_per_step']))"
}
for rep in $(seq "${1:-3}"); do
  run 1 --steps 20 --warmup 5
  run 256 --steps 20 --warmup 5
  run 1 --steps 2500 --warmup 5 --no-cpu-baseline
done
