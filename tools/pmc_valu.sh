#!/bin/bash
# VALU / SALU instruction counters of the frame's two kernels per dispatch at the driver's command (bench.py --pmc-inner --steps 20
# --warmup 5), one rocprofv3 --pmc pass of its own per library build, nothing traced beside it.  The counts are deterministic: this is
# the check of every change to k_back's instruction stream (profiles/r07/README.md).
#   usage: tools/pmc_valu.sh name1 [name2 ...]   (mrhash_amd/csrc/libmrhash_<name>.so; "hip" is the product build, others come from
#   python -m mrhash_amd.build variant <name>)
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
for n in "$@"; do
  OUT=$(mktemp -d)
  timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_SALU SQ_WAVES --output-format csv -d $OUT/pmc_sq -o p -- \
    python tools/bench_with_lib.py mrhash_amd/csrc/libmrhash_$n.so --pmc-inner --steps 20 --warmup 5 > $OUT/log.txt 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "## $n: rocprofv3 exit $rc"; tail -20 $OUT/log.txt; exit $rc; fi  # nothing more runs on the device after a failure
  echo "## $n"
  python tools/summarize_pmc.py $OUT | grep -A1 -E "k_back<|k_front<"
  rm -rf $OUT
done
