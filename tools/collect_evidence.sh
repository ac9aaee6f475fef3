#!/bin/bash
# Round evidence for every BASELINE config, on the sources as they are: bench line + rocprofv3 kernel-trace summary of the
# same command + PMC passes (each --pmc set in its own run, with --kernel-trace only) + (cfg2) a sustained-load record.
# Every bench command runs with --full (roofline, serial and fp16 x3 legs, CPU baseline), as the committed lines carry them.
# Summaries land in $EVIDENCE_DIR (default build/evidence/) AND in profiles/ (profiles/hbm_traffic[_cfgN].json
# regenerated, stamped with the digest of the kernel sources).
#   usage (on an MI355X, from the repo root): bash tools/collect_evidence.sh r03a [cfg2 cfg4 cfg5 cfg1]
tag=${1:-r03x}
shift
cfgs=${@:-cfg2 cfg4 cfg5 cfg1}
R=$(pwd)
O=${EVIDENCE_DIR:-$R/build/evidence}
mkdir -p $O $R/profiles
for cfg in $cfgs; do
  if [ $cfg = cfg2 ]; then sfx=""; else sfx="_$cfg"; fi
  pre=${tag}${sfx}
  python bench.py --config $cfg --full > $O/bench_$pre.json 2> $O/bench_$pre.err
  if [ $cfg = cfg2 ]; then
    python bench.py --steps 1500 --warmup 20 --full --no-cpu-baseline > $O/bench_sustained_$tag.json 2>> $O/bench_$pre.err
  fi
  cd /tmp && export TMPDIR=/tmp
  rocprofv3 --kernel-trace --stats -d $O/prof_$pre -o $pre -- python $R/bench.py --config $cfg --full --no-cpu-baseline > $O/prof_$pre.log 2>&1
  if [ $cfg = cfg2 ]; then
    rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F32 GRBM_GUI_ACTIVE -d $O/pmc_mfma_$pre -o $pre -- python $R/bench.py --config $cfg --full --no-cpu-baseline --steps 2 --warmup 1 > $O/pmc_mfma_$pre.log 2>&1
  fi
  rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/pmc_fetch_$pre -o $pre -- python $R/bench.py --config $cfg --full --no-cpu-baseline --steps 2 --warmup 1 > $O/pmc_fetch_$pre.log 2>&1
  rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/pmc_write_$pre -o $pre -- python $R/bench.py --config $cfg --full --no-cpu-baseline --steps 2 --warmup 1 > $O/pmc_write_$pre.log 2>&1
  cd $R
  for d in prof pmc_mfma pmc_fetch pmc_write; do
    db=$(find $O/${d}_$pre -name '*_results.db' 2>/dev/null | head -1)
    [ -n "$db" ] && python tools/rocpd_summary.py $db > $O/${d}_$pre.txt
    rm -rf $O/${d}_$pre
  done
  cp $O/prof_$pre.txt profiles/${pre}_kernel_trace_bench.txt
  [ -f $O/pmc_mfma_$pre.txt ] && cp $O/pmc_mfma_$pre.txt profiles/${pre}_pmc_mfma_busy.txt
  { echo "# FETCH_SIZE and WRITE_SIZE collected in two separate rocprofv3 --pmc passes (tools/collect_evidence.sh $tag $cfg); unit KiB per dispatch.";
    echo "# gfx950 correction (MI355X_MICROARCH.md, HBM section): FETCH_SIZE reports 1/2 of wide coalesced reads -> HBM read bytes = 2 x FETCH_SIZE.";
    grep "| FETCH_SIZE |" $O/pmc_fetch_$pre.txt; grep "| WRITE_SIZE |" $O/pmc_write_$pre.txt; } > profiles/${pre}_pmc_hbm_traffic.txt
  python tools/make_hbm_traffic.py $O/pmc_fetch_$pre.txt $O/pmc_write_$pre.txt $tag $cfg $O/prof_$pre.txt > $O/hbm_traffic_$pre.json
  # the bench line again, now that the traffic evidence belongs to this build
  python bench.py --config $cfg --full > $O/bench_$pre.json 2>> $O/bench_$pre.err
  cp $O/bench_$pre.json profiles/${pre}_bench.json
  [ $cfg = cfg2 ] && cp $O/bench_sustained_$tag.json profiles/${tag}_bench_sustained.json
  python tools/show_bench.py $O/bench_$pre.json 2>/dev/null | head -40
done
cp profiles/${tag}*.txt profiles/${tag}*.json profiles/hbm_traffic*.json $O/ 2>/dev/null
true
