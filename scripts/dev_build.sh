#!/bin/bash
# A copy of the HIP library built from the working tree with extra defines (e.g. -DCRENDER_STAMPS)
# -> /tmp/libcrender_hip_dev.so.  Use with CRENDER_LIB=/tmp/libcrender_hip_dev.so.
#   scripts/dev_build.sh [-DNAME=VALUE ...] [--out PATH]
cd ${GRAFT_REPO_ROOT:-$(dirname $0)/..}
python - "$@" <<'PY'
import sys
from cython3dmodelrenderer_amd import _build
args = sys.argv[1:]
out = "/tmp/libcrender_hip_dev.so"
if "--out" in args:
    i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
_build.compile_library(out, args, quiet=True)
print(out)
PY
