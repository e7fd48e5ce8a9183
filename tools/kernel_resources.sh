#!/bin/bash
# Registers / LDS / scratch of every kernel of the library (no GPU needed): compiles every unit of saro-gs_amd/build.py (its sources, its
# flags) with -save-temps into a temporary directory and prints the resource lines of the kernels whose name matches $1 (default: all).
# usage: [EXTRA="-DFOO=1"] tools/kernel_resources.sh [pattern]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
D=$(mktemp -d /tmp/gsres.XXXXXX)
S=$(python3 "$ROOT/saro-gs_amd/build.py" --save-temps "$D" $EXTRA 2>/dev/null)
python3 - "${1:-.}" $S <<'PY'
import re, sys
pat = re.compile(sys.argv[1])
for path in sys.argv[2:]:
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(path).read(), re.S):
        name, body = m.group(1), m.group(2)
        if not pat.search(name):
            continue
        g = lambda k: (re.search(r"\.amdhsa_" + k + r" (\S+)", body) or [None, "?"])[1]
        print(f"{name[:90]:90s} vgpr {g('next_free_vgpr'):>4s} sgpr {g('next_free_sgpr'):>4s} lds {g('group_segment_fixed_size'):>6s} scratch {g('private_segment_fixed_size'):>5s}")
PY
echo "(assembly: $S)"
