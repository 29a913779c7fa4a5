#!/bin/bash
# kernel trace of the prefill chunk (8192 tokens through the 28 layers): bench.py with ONE decode step so that the chunk's four runs dominate the trace
R="${GRAFT_REPO_ROOT:-/root/repo}"
O="${1:-${TMPDIR:-/tmp}/prefill_trace}"    # output directory (first argument)
mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_pf -- python $R/bench.py --full --no-cpu-baseline --no-gemm --no-engine --no-pmc --no-per-rank --no-allocator-pages --steps 1 --warmup 1 > $O/prefill_trace.log 2>&1
python $R/tools/rocpd_summary.py $(find $O/prof_pf -name "*.db" | head -1) > $O/r06_prefill_kernel_stats.txt 2>&1
rm -rf $O/prof_pf
grep '^{' $O/prefill_trace.log | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('# prefill', d['prefill'])"
head -30 $O/r06_prefill_kernel_stats.txt | cut -c1-175
