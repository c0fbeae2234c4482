#!/bin/bash
# usage (from the repo root, on a GPU box): tools/evidence.sh <dir>   -- then, back home: tools/collect_evidence.sh r06 <dir>
# the round's evidence on ONE box: GPU test suite + smoke, profiles (kernel trace + PMC passes), then the bench lines quoting the traffic just measured, then the fuzz runs
OUT=$(realpath -m "${1:?usage: tools/evidence.sh <output directory>}")
cd ${GRAFT_REPO_ROOT:-.}
mkdir -p "$OUT"
export TMPDIR=/tmp
rocm-smi --showmemorypartition --showcomputepartition 2>/dev/null | grep -E "Partition" > "$OUT"/r06_box.txt
timeout 1500 python -m pytest tests -x -q -m gpu > "$OUT"/r06_pytest_gpu.txt 2>&1; echo "pytest rc=$?" >> "$OUT"/r06_pytest_gpu.txt
python -c "import __graft_entry__ as g; g.smoke()" >> "$OUT"/r06_pytest_gpu.txt 2>&1
tools/prof.sh r06 "$OUT" > "$OUT"/r06_prof.log 2>&1
cp "$OUT"/prof_r06/hbm_traffic.json profiles/hbm_traffic.json
tools/bench_lines.sh r06 "$OUT" > "$OUT"/r06_bench_lines.log 2>&1
timeout 900 python tools/fuzz_gpu.py 500 606 > "$OUT"/r06_fuzz_a.txt 2>&1
FUZZ_LARGE=1 timeout 900 python tools/fuzz_gpu.py 120 607 > "$OUT"/r06_fuzz_b.txt 2>&1
timeout 600 python tools/fuzz_backward_gpu.py 600 608 > "$OUT"/r06_fuzz_bwd.txt 2>&1
FUZZ_BWD=gather timeout 600 python tools/fuzz_backward_gpu.py 600 609 > "$OUT"/r06_fuzz_bwd_gather.txt 2>&1
tail -n 4 "$OUT"/r06_pytest_gpu.txt; for f in a b bwd bwd_gather; do tail -n 1 "$OUT"/r06_fuzz_$f.txt; done; tail -15 "$OUT"/r06_bench_lines.log | cut -c1-420
