# one-stream kernel table of the headline step (what each launch costs with the chip to itself) -> $OUT_DIR/${1}_one_stream_kernel_stats.txt (default prof_out/), then the default bench line
export TMPDIR=/tmp; R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT_DIR:-$R/prof_out}; mkdir -p $O; cd /tmp
T=${1:-r04_mid}
rocprofv3 --kernel-trace --stats -d $O/prof_bench1 -o bench -- python3 $R/bench.py --streams 1 --steps 10 --warmup 3 --no-cpu-baseline --no-in-run-ab --no-full-swap --no-pti --clip 0 --no-mask-sensitivity --soak-seconds 0 > $O/prof_bench1.log 2>&1
cd $R
python tools/rocpd_summary.py $O/prof_bench1/bench_results.db | cut -c1-200 > $O/${T}_one_stream_kernel_stats.txt
rm -rf $O/prof_bench1
python bench.py --full --no-cpu-baseline --no-full-swap --no-pti --clip 0 --no-mask-sensitivity > $O/${T}_bench_quick.json 2> $O/${T}_bench_quick.err
head -c 400 $O/${T}_bench_quick.json
