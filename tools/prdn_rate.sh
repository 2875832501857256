#!/bin/sh
# Time the PRDN stage (tools/prdn_rate.py): the fast path, the sequential path and the CPU restatement on the same batch, each
# step under its own time limit, the next one only if the one before ended well.  Writes OUT (default profiles/prdn_bench.json).
set -e
cd "$(dirname "$0")/.."
OUT=${1:-profiles/prdn_bench.json}
T=$(mktemp -d)
timeout -k 10 240 python tools/prdn_rate.py --mode fast --out "$T/fast.json" &&
timeout -k 10 300 python tools/prdn_rate.py --mode seq --out "$T/seq.json" &&
timeout -k 10 240 python tools/prdn_rate.py --mode orc --out "$T/orc.json" &&
python - "$T" "$OUT" <<'PY'
import json, sys
t, out = sys.argv[1:3]
runs = {m: json.load(open("%s/%s.json" % (t, m))) for m in ("fast", "seq", "orc")}
with open(out, "w") as f:
    f.write(json.dumps(dict(tool="prdn_rate", runs=runs)) + "\n")
PY
rm -rf "$T"
