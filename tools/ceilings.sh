#!/bin/bash
# The slices of the headline, measured at the current code (DESIGN.md sections 4 and 8): the device side alone (bins
# produced, neither copied nor coded), bins packed and handed over but not copied, everything but the coding (bins reach
# the host), and the plain line.  The legs run back to back, each under its own time limit; the script stops at the
# first one that fails.  usage: tools/ceilings.sh OUTDIR
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/$1
mkdir -p $OUT
COMMON="--steps 8 --warmup 2 --full --no-extra-legs --no-cpu-baseline"
leg() {   # leg NAME [NBLIC_AMD_DBG].  A debug leg writes no valid streams, so bench.py ends it with status 3 ("not bit-exact"): no failure here
    if [ -n "$2" ]; then export NBLIC_AMD_DBG=$2; else unset NBLIC_AMD_DBG; fi
    timeout -k 10 300 python3 $R/bench.py $COMMON > $OUT/$1.json 2> $OUT/$1.err
    local rc=$?
    if { [ $rc -ne 0 ] && [ $rc -ne 3 ]; } || { [ -z "$2" ] && [ $rc -ne 0 ]; } || grep -qi "illegal memory access" $OUT/$1.err; then echo "$1: exit status $rc"; return 1; fi
}
leg device_side_only 16 && leg no_copy 1152 && leg no_coding 128 && leg plain8
rc=$?
python3 - <<PY
import json
for n in ("device_side_only", "no_copy", "no_coding", "plain8"):
    try:
        d = json.load(open("$OUT/" + n + ".json"))
        print(n, d["value"], "Mpixel/s", "bit_exact", d.get("bit_exact"))
    except Exception as e:
        print(n, "failed:", e)
PY
exit $rc
