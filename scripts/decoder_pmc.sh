#!/bin/bash
# counter summaries for the present ctc.hip / tdt.hip: counter passes only, each its own run under its own time limit, chained
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
ROOT=$PWD
export TMPDIR=${TMPDIR:-/tmp}
OUT=${1:-build/decoder_pmc}   # where the passes and the two summaries go (build/ is not tracked)
mkdir -p $OUT/summary
pass() {  # pass <name> <pass-name> <probe command...> -- counters...
  name=$1; n=$2; shift 2; cmd=(); while [ "$1" != "--" ]; do cmd+=("$1"); shift; done; shift
  mkdir -p $ROOT/$OUT/pmc_$name
  echo "== $name/$n"
  ( cd $TMPDIR && timeout -k 10 400 rocprofv3 --pmc "$@" -d "$ROOT/$OUT/pmc_$name/$n" -o $n -- "${cmd[@]}" ) > $ROOT/$OUT/pmc_$name/$n.log 2>&1
  rc=$?; tail -n 2 $ROOT/$OUT/pmc_$name/$n.log | cut -c1-300; echo "== $name/$n rc=$rc"; return $rc
}
summ() {  # summ <name> <kernel-substring> <source>
  python scripts/pmc_summary.py "$2" $(find $OUT/pmc_$1 -name "*.db") > $OUT/summary/$1_pmc.json &&
  python - "$1" "$3" "$OUT" <<'PY'
import json, sys
sys.path.insert(0, '.')
import bench
name, srcs = sys.argv[1], tuple(sys.argv[2].split())
p = f'{sys.argv[3]}/summary/{name}_pmc.json'
j = json.load(open(p))
j['kernel_sources_sha256'] = bench.sources_sha256(srcs)
j['kernel_sources'] = list(srcs)
json.dump(j, open(p, 'w'), indent=1)
print({k: v for k, v in j.items() if k != 'counters'})
PY
}
SQ="SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR"
export FA_PROBE=tdt
pass tdt tcc1 python $ROOT/scripts/r4_kernels_probe.py -- FETCH_SIZE GRBM_GUI_ACTIVE &&
pass tdt tcc2 python $ROOT/scripts/r4_kernels_probe.py -- WRITE_SIZE GRBM_GUI_ACTIVE &&
pass tdt sq1 python $ROOT/scripts/r4_kernels_probe.py -- $SQ &&
summ tdt tdt_logits_fits_kernel tdt.hip &&
pass ctc tcc1 python $ROOT/scripts/ctc_probe.py -- FETCH_SIZE GRBM_GUI_ACTIVE &&
pass ctc tcc2 python $ROOT/scripts/ctc_probe.py -- WRITE_SIZE GRBM_GUI_ACTIVE &&
pass ctc sq1 python $ROOT/scripts/ctc_probe.py -- $SQ &&
summ ctc ctc_greedy ctc.hip
rc=$?
find $OUT -name "*.db" -delete
echo "decoder_pmc rc=$rc"
