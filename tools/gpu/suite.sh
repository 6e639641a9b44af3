#!/bin/bash
# the full -m gpu suite, smoke(), then the default C2 bench (1024 s) with its bit-exactness check, without
# the CPU leg; logs in $OUT_DIR (default: out)
cd "${GRAFT_REPO_ROOT:-/root/repo}"
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 1100 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/suite.log 2>&1
rc=$?; tail -3 $O/suite.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || exit 3
tail -1 $O/smoke.log
[ -n "$NOBENCH" ] && exit 0
GSC_HOST_TIMING=1 timeout -k 10 300 python -u bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > $O/c2.log 2>&1 || exit 4
tail -1 $O/c2.log | cut -c1-400
