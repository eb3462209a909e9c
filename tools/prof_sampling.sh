# usage: bash tools/prof_sampling.sh OUT_DIR - kernel trace of a short bench run -> OUT_DIR/kernel_stats.txt
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "${1:?usage: prof_sampling.sh OUT_DIR}" && cd "$1" && pwd); cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/kt -o bench -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --train-steps 0 > $O/bench_prof.json 2> $O/kt.err
python $R/tools/rocpd_stats.py $(find $O/kt -name '*.db' | head -1) > $O/kernel_stats.txt 2>&1
rm -rf $O/kt
head -24 $O/kernel_stats.txt
