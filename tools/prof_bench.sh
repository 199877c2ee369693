# kernel-trace profile of the headline bench (short), per-kernel and per-(kernel, grid) summaries under $OUT_DIR (default prof_out/)
export TMPDIR=/tmp; R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT_DIR:-$R/prof_out}; mkdir -p $O; cd /tmp
rocprofv3 --kernel-trace --stats -d $O/prof_bench -o bench -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-in-run-ab --no-full-swap --no-pti --clip 0 > $O/prof_bench.log 2>&1
cd $R
python tools/rocpd_summary.py $O/prof_bench/bench_results.db | cut -c1-230 > $O/${1:-r02}_bench_kernel_stats.txt
python tools/rocpd_by_grid.py $O/prof_bench/bench_results.db 0.05 | cut -c1-230 > $O/${1:-r02}_bench_by_layer.txt
grep '^{' $O/prof_bench.log | cut -c1-300
rm -rf $O/prof_bench
head -30 $O/${1:-r02}_bench_by_layer.txt
