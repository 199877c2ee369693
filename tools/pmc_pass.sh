# one PMC pass over the bench (counters + kernel trace only; no other trace domains)
export TMPDIR=/tmp; R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT_DIR:-$R/prof_out}; mkdir -p $O; cd /tmp
rocprofv3 --kernel-trace --pmc $1 -d $O/$2 -o pmc -- python3 $R/bench.py --streams 1 --steps 2 --warmup 1 --no-cpu-baseline --no-in-run-ab --no-full-swap --no-pti --clip 0 --no-mask-sensitivity --soak-seconds 0 > $O/$2.log 2>&1
tail -2 $O/$2.log | cut -c1-300
