#!/bin/bash
# SpGEMM (A @ B_sparse) against SpMM (A @ B_dense): the grids of others/spmm/spMM.py
# (n {128..1024} x density {0.01,0.1,0.5}) and others/spmm/diff_matrix_size.py
# (n {2^11..2^14} at density 0.001).  RUNS timed products per cell (median), WARMUP untimed.
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUTFILE="${OUTFILE:-benchmark_results.txt}"
export RUNS="${RUNS:-5}"
export WARMUP="${WARMUP:-2}"
echo "Benchmark results - $(date)" > "$OUTFILE"
echo -e "==========================================\n" >> "$OUTFILE"
python3 "$HERE/profiler.py" --grid "${GRID:-both}" 2>&1 | tee -a "$OUTFILE"
rc=${PIPESTATUS[0]}
echo -e "\nAll runs completed. Results saved to $OUTFILE\n"
exit $rc
