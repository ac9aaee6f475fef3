#!/bin/bash
# Round-5 evidence on an MI355X (from the repo root): bash tools/r05_evidence.sh r05a
# Outputs land in $EVIDENCE_DIR (default build/evidence/, as tools/collect_evidence.sh) and in profiles/.
TAG=${1:-r05a}
R=$(pwd)
O=${EVIDENCE_DIR:-$R/build/evidence}
export EVIDENCE_DIR=$O
mkdir -p $O profiles
bash tools/collect_evidence.sh $TAG cfg2 cfg4 cfg5 cfg1 2>&1 | grep -E "^configs|^dominant"
# the fp16 x3 mode's own line (with its roofline and CPU baseline: --full) + the kernel trace of the same command
python bench.py --gemm f16x3 --full > $O/${TAG}_bench_f16x3.json 2> $O/${TAG}_bench_f16x3.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_${TAG}_f16x3 -o ${TAG}_f16x3 -- python $R/bench.py --gemm f16x3 --full --no-cpu-baseline > $O/prof_${TAG}_f16x3.log 2>&1
cd $R
db=$(find $O/prof_${TAG}_f16x3 -name '*_results.db' 2>/dev/null | head -1)
[ -n "$db" ] && python tools/rocpd_summary.py $db > $O/${TAG}_f16x3_kernel_trace.txt
rm -rf $O/prof_${TAG}_f16x3
cp $O/${TAG}_bench_f16x3.json $O/${TAG}_f16x3_kernel_trace.txt profiles/ 2>/dev/null
python tools/bench_ds2.py > $O/${TAG}_ds2_shapes.txt 2> $O/${TAG}_ds2_shapes.err
python tools/bench_beam.py > $O/${TAG}_beam.txt 2> $O/${TAG}_beam.err
python tools/bench_streams.py > $O/${TAG}_streams.txt 2> $O/${TAG}_streams.err
python tools/phase_ts.py --h3 > $O/${TAG}_phase_ts_h3.txt 2>&1
cp $O/${TAG}_ds2_shapes.txt $O/${TAG}_beam.txt $O/${TAG}_streams.txt $O/${TAG}_phase_ts_h3.txt profiles/ 2>/dev/null
cp profiles/${TAG}* profiles/hbm_traffic*.json $O/ 2>/dev/null
python tools/show_bench.py $O/${TAG}_bench_f16x3.json 2>/dev/null | head -12
true
