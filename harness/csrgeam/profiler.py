#!/usr/bin/env python3
"""Sparse addition on the GPU: spg_csrgeam against the torch formulation of the same addition.

Ports nothing the reference times: the reference adds with cupyx.cusparse.csrgeam2
(modify_src/cupy-src/cupyx/cusparse.py:525-591) inside ``A + B`` / ``A - B`` and never measures
it on its own.  This profiler records what ``A + B`` costs on the matrices of the benchmark
configurations (harness/configs.py): config 4's A and B (N = 65536, density 5e-3, fp64, about 328
entries per row) and config 2's (N = 16384, density 1e-3, fp64, about 16 per row).

Per case, in fresh child processes (ROUNDS of them, default 3):
  (a) ``cusparse.csrgeam2(A, B)``: wall ms per call (device events around the call, the
      workspace and result allocations and the one host wait for nnz(C) included) and the device
      ms of its kernels from spg_get_timing, with the launches per phase;
  (b) as the outside figure, ``sparse._geam_torch(A, B, 1, 1)`` on the same device tensors: the
      same rule as torch ops (int64 keys, unique, searchsorted, index_put);
  the bytes/s of (a)'s device time over the least traffic an addition can do,
  (nnzA + nnzB + nnzC) * (4 + sizeof T) plus the three row pointers.
Every figure is the median of RUNS (environment, default 20) calls after WARMUP (default 5); min
and max are printed beside it.  The two results are compared array for array.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"config4": (65536, 5e-3), "config2": (16384, 1e-3)}


def stats(times):
    times = sorted(times)
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1]}


def worker(root, case, runs, warmup):
    """One case's figures as a JSON line."""
    sys.path.insert(0, root)
    import torch
    from spmm_amd import _lib, cusparse, gen, sparse
    from spmm_amd.sparse import csr_matrix
    n, density = CASES[case]
    dev = torch.device("cuda", 0)
    if n <= 16384:
        A, B = (csr_matrix(S, device=dev) for S in gen.scipy_pair(n, density, seed=42, normal=True))
    else:
        A = gen.random_csr(n, n, density, seed=42, device=dev)
        B = gen.random_csr(n, n, density, seed=43, device=dev)
    assert A.has_canonical_format and B.has_canonical_format
    if not cusparse.has_csrgeam():
        sys.exit("this tree's library does not export spg_csrgeam")

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
            del r
        return stats(out)

    def engine():
        return cusparse.csrgeam2(A, B)

    def torch_form():
        return sparse._geam_torch(A, B, 1, 1)

    res = {"case": case, "N": n, "nnzA": A.nnz, "nnzB": B.nnz, "device": torch.cuda.get_device_name(0),
           "torch_version": torch.__version__, "source_id": _lib.source_id()}
    res["wall_ms"] = timed(engine)
    res["torch_ms"] = timed(torch_form)
    C, T = engine(), torch_form()
    torch.cuda.synchronize()
    res["nnzC"] = C.nnz
    res["identical"] = bool(torch.equal(C.indptr.to(torch.int64), T.indptr.to(torch.int64)) and
                            torch.equal(C.indices, T.indices) and
                            torch.equal(C.data.view(torch.int64), T.data.view(torch.int64)))
    hd = _lib.get_handle(0)
    hd.set_stream(torch.cuda.current_stream().cuda_stream)
    dev_ms = []
    for _ in range(runs):
        hd.set_timing(True)
        engine()
        t = hd.get_timing()
        dev_ms.append(sum(ms for ms, launches in t.values() if launches))
        res["launches"] = {k: v[1] for k, v in t.items() if v[1]}
        res["phase_ms"] = {k: round(v[0], 4) for k, v in t.items() if v[1]}
    hd.set_timing(False)
    res["device_ms"] = stats(dev_ms)
    esz = A.data.element_size()
    res["min_traffic_bytes"] = (A.nnz + B.nnz + C.nnz) * (4 + esz) + \
        (A.indptr.element_size() + B.indptr.element_size() + C.indptr.element_size()) * (n + 1)
    print("RESULT " + json.dumps(res), flush=True)


def child(root, case, runs, warmup):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--case", case]
    env = dict(os.environ, RUNS=str(runs), WARMUP=str(warmup))
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    if out.returncode != 0:
        sys.exit(f"worker failed ({root}, {case}):\n{out.stdout}\n{out.stderr}")
    line = [x for x in out.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def fmt(s):
    return f"{s['median']:.3f} ms (min {s['min']:.3f}, max {s['max']:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.abspath(os.path.join(HERE, "..", "..")))
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--rounds", type=int, default=int(os.environ.get("ROUNDS", "3")))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--case")
    args = ap.parse_args()
    runs, warmup = int(os.environ.get("RUNS", "20")), int(os.environ.get("WARMUP", "5"))
    if args.worker:
        return worker(args.root, args.case, runs, warmup)
    print(f"RUNS={runs} WARMUP={warmup} ROUNDS={args.rounds}")
    for case in args.cases:
        rounds = [child(args.root, case, runs, warmup) for _ in range(args.rounds)]   # each a fresh process
        a = rounds[0]
        print(f"== {case}: N={a['N']} nnzA={a['nnzA']} nnzB={a['nnzB']} nnzC={a['nnzC']} fp64 on {a['device']} "
              f"(source_id {a['source_id']})")
        for r, x in enumerate(rounds):
            print(f"(a) spg_csrgeam  round {r}: wall {fmt(x['wall_ms'])}; device {fmt(x['device_ms'])}")
        for r, x in enumerate(rounds):
            print(f"(b) torch ops    round {r}: wall {fmt(x['torch_ms'])}   (torch {x['torch_version']})")
        print(f"    launches per call: {a['launches']}; device ms per phase (last run): {a['phase_ms']}")
        am = sorted(x["wall_ms"]["median"] for x in rounds)
        bm = sorted(x["torch_ms"]["median"] for x in rounds)
        print(f"    (b)/(a) median/median: {bm[len(bm) // 2] / am[len(am) // 2]:.2f}x; "
              f"worst case for (a) [min (b) / max (a)]: {bm[0] / am[-1]:.2f}x")
        print(f"    results identical (indptr, indices, value bits): {all(x['identical'] for x in rounds)}")
        dm = sorted(x["device_ms"]["median"] for x in rounds)[len(rounds) // 2]
        print(f"    minimum traffic {a['min_traffic_bytes']} bytes; over device time {dm:.3f} ms = "
              f"{a['min_traffic_bytes'] / dm / 1e6:.1f} GB/s")


if __name__ == "__main__":
    main()
