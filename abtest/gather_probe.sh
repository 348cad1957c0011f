#!/usr/bin/env bash
# Runs abtest/gather_probe over the slice sizes / segment lengths of the tile path (tile width TW
# at config 4: slice = TW x 3.94 KB, L = TW x 0.005) and collects, per run, the TCC request mix
# (32/64/128-B fabric read requests), FETCH_SIZE + TCC_HIT, and TCC_MISS + WRITE_SIZE, each pass
# its own rocprofv3 run.  Output: gpurun_out/probe/*; abtest/probe_report.py folds it.
#
#   gather_probe.sh        the sweep above
#   gather_probe.sh segs   only the packed-segment question: 10-byte records behind a segment table,
#                          segments back to back against segments placed so that none straddles a
#                          128-byte line it need not (timed alternately, then the vector L1's read
#                          requests and the L2 hit rate, each in a counter pass of its own)
set -euo pipefail
cd "$(dirname "$0")/.."
B=$PWD/abtest/gather_probe
OUT=$PWD/gpurun_out/probe
mkdir -p "$OUT"
export TMPDIR=/tmp
run() {
  local tag=$1; shift
  timeout -k 10 60 "$B" "$@" > "$OUT/$tag.json"
  timeout -s KILL 60 rocprofv3 --pmc TCC_EA0_RDREQ_32B_sum TCC_EA0_RDREQ_64B_sum TCC_EA0_RDREQ_128B_sum TCC_EA0_RDREQ_sum \
      --output-format csv -d "$OUT/p_$tag" -o req -- "$B" "$@" > "$OUT/p_$tag.req.log" 2>&1
  timeout -s KILL 60 rocprofv3 --pmc FETCH_SIZE TCC_HIT_sum --output-format csv -d "$OUT/p_$tag" -o fh \
      -- "$B" "$@" > "$OUT/p_$tag.fh.log" 2>&1
  timeout -s KILL 60 rocprofv3 --pmc TCC_MISS_sum WRITE_SIZE --output-format csv -d "$OUT/p_$tag" -o mw \
      -- "$B" "$@" > "$OUT/p_$tag.mw.log" 2>&1
  echo "$tag $(cat "$OUT/$tag.json")"
}
if [ "${1:-}" = segs ]; then
  for rep in 1 2 3; do   # timing first, the two layouts alternated
    for p in 0 1; do
      timeout -k 10 60 "$B" segs $p > "$OUT/segs_p${p}_t$rep.txt"
      echo "timing $rep place=$p $(cat "$OUT/segs_p${p}_t$rep.txt")"
    done
  done
  for p in 0 1; do
    cp "$OUT/segs_p${p}_t3.txt" "$OUT/segs_p$p.json"
    timeout -s KILL 90 rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCP_TCC_READ_REQ_LATENCY_sum --output-format csv \
        -d "$OUT/p_segs_p$p" -o tcp -- "$B" segs $p > "$OUT/p_segs_p$p.tcp.log" 2>&1
    timeout -s KILL 90 rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv \
        -d "$OUT/p_segs_p$p" -o hm -- "$B" segs $p > "$OUT/p_segs_p$p.hm.log" 2>&1
    timeout -s KILL 90 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_128B_sum --output-format csv \
        -d "$OUT/p_segs_p$p" -o ea -- "$B" segs $p > "$OUT/p_segs_p$p.ea.log" 2>&1
  done
  python3 abtest/probe_report.py "$OUT" | grep '"segs_' > "$OUT/segs_report.txt"
  cat "$OUT/segs_report.txt"
  exit 0
fi
run stream1g stream 1024
for s in ${SLICES:-1 2 4 8 16 64}; do run g_s${s}_l10 gather $s 10; done
run g_s2_l3 gather 2 3
run g_s8_l3 gather 8 3
run g_s8_l40 gather 8 40
run gs_s2_l3 gather 2 3 1
run gs_s4_l5 gather 4 5 1
run gs_s8_l10 gather 8 10 1
python3 abtest/probe_report.py "$OUT" > "$OUT/report.txt"
cat "$OUT/report.txt"
