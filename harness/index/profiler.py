#!/usr/bin/env python3
"""Submatrix extraction on the GPU: spg_csr_extract against the torch formulation of the same rule.

Ports nothing the reference times: the reference's users index with cupyx's ``__getitem__``
(modify_src/cupy-src/cupyx/scipy/sparse/_index.py:348, kernels of its own) and never measure it.
This profiler records what ``A[rows, cols]`` costs on config 4's A (harness/configs.py: N = 65536,
density 5e-3, fp64, about 328 entries per row):

  a  2048 stratified rows (one from every 32), all columns;
  b  all rows, columns [N/4, N/2);
  c  a random permutation P on both axes, A[P][:, P] in one call;
  d  rows [N/4, N/2), all columns (one contiguous span of A).

Per case, in fresh child processes (ROUNDS of them, default 3):
  (1) ``cusparse.extract(A, rows, cols)``: wall ms per call (device events around the call, the
      workspace and result allocations and the one host wait for nnz(C) included) and the device
      ms of its kernels from spg_get_timing, with the launches and the device ms per phase;
  (2) as the outside figure, ``sparse._extract_torch`` on the same device tensors: the same rule as
      torch ops (repeat_interleave, a stable sort of the column list, index_select);
  nnz(C), and the bytes/s of (1)'s device time over the compulsory traffic: the indices of the
  selected source rows (all of them must be read to test their column; K = all: only those kept),
  the kept values, C's three arrays, the selected rows' row pointers and the index lists.
Every figure is the median of RUNS (environment, default 20) calls after WARMUP (default 5); min
and max are printed beside it.  The two results are compared array for array.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
N, DENSITY = 65536, 5e-3
CASES = ("a", "b", "c", "d")


def stats(times):
    times = sorted(times)
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1]}


def selections(case, torch, dev):
    """(rows key, cols key) of a case, as cusparse.extract takes them."""
    g = torch.Generator().manual_seed(7)
    if case == "a":
        rows = torch.arange(0, N, 32) + torch.randint(0, 32, (N // 32,), generator=g)
        return rows.to(dev), None
    if case == "b":
        return None, slice(N // 4, N // 2)
    if case == "c":
        p = torch.randperm(N, generator=g).to(dev)
        return p, p
    return slice(N // 4, N // 2), None


def worker(root, case, runs, warmup):
    """One case's figures as a JSON line."""
    sys.path.insert(0, root)
    import torch
    from spmm_amd import _lib, cusparse, gen, sparse
    dev = torch.device("cuda", 0)
    A = gen.random_csr(N, N, DENSITY, seed=42, device=dev)
    assert A.has_canonical_format
    if not cusparse.has_extract():
        sys.exit("this tree's library does not export spg_csr_extract")
    rk, ck = selections(case, torch, dev)
    rsel, csel = sparse._axis_selector(rk, N, dev), sparse._axis_selector(ck, N, dev)

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
        return cusparse._extract_arrays(A.data, A.indices, A.indptr, (N, N), rsel, csel)

    def torch_form():
        return sparse._extract_torch(A.data, A.indices, A.indptr, N, N, rsel, csel)

    res = {"case": case, "N": N, "nnzA": A.nnz, "device": torch.cuda.get_device_name(0),
           "torch_version": torch.__version__, "source_id": _lib.source_id()}
    res["wall_ms"] = timed(engine)
    res["torch_ms"] = timed(torch_form)
    (cx, cj, cp), (tx, tj, tp) = engine(), torch_form()
    torch.cuda.synchronize()
    res["nnzC"] = int(cx.numel())
    res["identical"] = bool(torch.equal(cp.to(torch.int64), tp.to(torch.int64)) and torch.equal(cj, tj) and
                            torch.equal(cx.view(torch.int64), tx.view(torch.int64)))
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
    esz, ip = A.data.element_size(), A.indptr.element_size()
    r = torch.arange(N, device=dev) if rsel is None else (
        rsel[0] + rsel[1] * torch.arange(rsel[2], device=dev) if isinstance(rsel, tuple) else rsel.to(torch.int64))
    src = int((A.indptr[r + 1] - A.indptr[r]).sum())          # entries of the selected source rows
    nr = int(r.numel())
    lists = sum(4 * int(s.numel()) for s in (rsel, csel) if isinstance(s, torch.Tensor))
    res["src_entries"] = src
    res["min_traffic_bytes"] = (res["nnzC"] if csel is None else src) * 4 + res["nnzC"] * esz + \
        res["nnzC"] * (4 + esz) + 2 * nr * ip + (nr + 1) * cp.element_size() + lists
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
        print(f"== case {case}: N={a['N']} nnzA={a['nnzA']} source entries={a['src_entries']} nnzC={a['nnzC']} "
              f"fp64 on {a['device']} (source_id {a['source_id']})")
        for r, x in enumerate(rounds):
            print(f"(1) spg_csr_extract round {r}: wall {fmt(x['wall_ms'])}; device {fmt(x['device_ms'])}")
        for r, x in enumerate(rounds):
            print(f"(2) torch ops       round {r}: wall {fmt(x['torch_ms'])}   (torch {x['torch_version']})")
        print(f"    launches per call: {a['launches']}; device ms per phase (last run): {a['phase_ms']}")
        am = sorted(x["wall_ms"]["median"] for x in rounds)
        bm = sorted(x["torch_ms"]["median"] for x in rounds)
        print(f"    (2)/(1) median/median: {bm[len(bm) // 2] / am[len(am) // 2]:.2f}x; "
              f"worst case for (1) [min (2) / max (1)]: {bm[0] / am[-1]:.2f}x")
        print(f"    results identical (indptr, indices, value bits): {all(x['identical'] for x in rounds)}")
        dm = sorted(x["device_ms"]["median"] for x in rounds)[len(rounds) // 2]
        print(f"    compulsory traffic {a['min_traffic_bytes']} bytes; over device time {dm:.3f} ms = "
              f"{a['min_traffic_bytes'] / dm / 1e6:.1f} GB/s")


if __name__ == "__main__":
    main()
