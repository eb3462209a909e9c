# usage: bash tools/prof_round.sh OUT_DIR - the bench with every leg, throughput mode, a kernel trace and the --pmc passes -> OUT_DIR
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "${1:?usage: prof_round.sh OUT_DIR}" && cd "$1" && pwd); cd /tmp; export TMPDIR=/tmp
python $R/bench.py --full --steps 3 --warmup 1 > $O/bench.json 2> $O/bench.err
python $R/bench.py --full --steps 2 --warmup 1 --batch 8 --no-cpu-baseline --no-roofline --train-steps 0 > $O/bench_b8.json 2>> $O/bench.err
rocprofv3 --kernel-trace --stats -d $O/kt -o bench -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --train-steps 0 > $O/bench_prof.json 2> $O/kt.err
python $R/tools/rocpd_stats.py $(find $O/kt -name '*.db' | head -1) > $O/kernel_stats.txt 2>&1
rocprofv3 --pmc FETCH_SIZE -d $O/pf -o f -- python $R/tools/unet_step.py 3 > /dev/null 2> $O/pf.err
rocprofv3 --pmc WRITE_SIZE -d $O/pw -o w -- python $R/tools/unet_step.py 3 > /dev/null 2> $O/pw.err
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY -d $O/ps -o s -- python $R/tools/unet_step.py 3 > /dev/null 2> $O/ps.err
for k in conv_ksw conv_igemm conv_splitk temporal_attn_fused attention_kernel linattn_fused gn_apply; do for d in pf pw ps; do echo "== $d $k"; python $R/tools/rocpd_pmc.py $(find $O/$d -name '*.db' | head -1) $k; done; done > $O/pmc.txt 2>&1
rm -rf $O/kt $O/pf $O/pw $O/ps
tail -2 $O/bench.err; cat $O/bench_b8.json | cut -c1-200
