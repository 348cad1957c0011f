#!/usr/bin/env python3
"""Canonicalisation on the GPU: spg_canonicalize against the torch formulation it replaces.

Ports nothing the reference times: the reference canonicalises with cupyx's ``sum_duplicates()`` /
``eliminate_zeros()`` / ``tocsr()`` while it builds its matrices (others/profiler.py:66-69) and in
front of every ``A @ B`` and ``A + B`` (modify_src/cupy-src/cupyx/scipy/sparse/_csr.py:151-166,
_compressed.py:971-991), and never measures it on its own.  This profiler records what the
containers' calls cost on the matrices of the benchmark configurations (harness/configs.py):
config 4's A (N = 65536, density 5e-3, fp64, about 328 entries per row) and config 2's (N = 16384,
density 1e-3, fp64, about 16 per row).

Cases:
  c4_reversed     ``sum_duplicates()`` of config 4's A with every row reversed (unsorted, no duplicates);
  c4_dup5         the same with every fifth entry stored a second time (another value) at its row's end;
  c2_dup5         config 2's A built likewise;
  c4_coo          ``coo_matrix.tocsr()`` of config 4's A as triplets in shuffled order;
  c4_zeros        ``eliminate_zeros()`` of config 4's A with a tenth of its values set to 0.

Per case, in fresh child processes (ROUNDS of them, default 3):
  (a) the call on the engine: wall ms per call (device events around the call, the workspace and
      result allocations and the one host wait for nnz(C) included) and the device ms of its
      kernels from spg_get_timing, with the launches per phase;
  (b) the same call with the engine routing switched off, i.e. the torch ops it replaces (int64
      keys, a stable sort, unique_consecutive, the segmented sequential sum, bincount and cumsum)
      on the same device tensors.
Every figure is the median of RUNS (environment, default 20) calls after WARMUP (default 5); min
and max are printed beside it.  The two results are compared array for array, values by their bits.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"c4_reversed": (65536, 5e-3), "c4_dup5": (65536, 5e-3), "c2_dup5": (16384, 1e-3),
         "c4_coo": (65536, 5e-3), "c4_zeros": (65536, 5e-3)}


def stats(times):
    times = sorted(times)
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1]}


def worker(root, case, runs, warmup):
    """One case's figures as a JSON line."""
    sys.path.insert(0, root)
    import torch
    from spmm_amd import _lib, cusparse, gen, sparse
    from spmm_amd.sparse import coo_matrix, csr_matrix
    n, density = CASES[case]
    dev = torch.device("cuda", 0)
    if n <= 16384:
        A = csr_matrix(gen.scipy_pair(n, density, seed=42, normal=True)[0], device=dev)
    else:
        A = gen.random_csr(n, n, density, seed=42, device=dev)
    assert A.has_canonical_format
    if not cusparse.has_canonicalize():
        sys.exit("this tree's library does not export spg_canonicalize")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    rows = A._row_ids()
    e = torch.arange(A.nnz, device=dev)
    ip = A.indptr.to(torch.int64)
    src = ip[rows] + ip[rows + 1] - 1 - e                 # every row reversed
    cols, vals = A.indices[src], A.data[src]
    if case.endswith("dup5"):                             # every fifth entry once more, at its row's end
        extra = torch.randn(rows[::5].numel(), dtype=vals.dtype, device=dev, generator=g)
        rows, cols, vals = torch.cat((rows, rows[::5])), torch.cat((cols, cols[::5])), torch.cat((vals, extra))
        rows, order = torch.sort(rows, stable=True)
        cols, vals = cols[order].contiguous(), vals[order].contiguous()
    if case == "c4_zeros":
        cols, vals = A.indices, A.data.clone()
        vals[torch.rand(A.nnz, device=dev, generator=g) < 0.1] = 0
    if case == "c4_coo":
        perm = torch.randperm(A.nnz, device=dev, generator=g)
        rows, cols, vals = A._row_ids()[perm].contiguous(), A.indices[perm].to(torch.int64), A.data[perm].contiguous()
    indptr = sparse._indptr_from_rows(rows, n, torch.int32)
    nnz = int(vals.numel())

    def call():
        if case == "c4_coo":
            return coo_matrix((vals, (rows, cols)), shape=(n, n), device=dev).tocsr()
        M = csr_matrix._from_parts(vals, cols, indptr, (n, n), canonical=False)
        M.eliminate_zeros() if case == "c4_zeros" else M.sum_duplicates()
        return M

    routed = sparse._engine_has

    def torch_form():
        sparse._engine_has = lambda t, symbols, *a: symbols is not _lib.CANONICALIZE and routed(t, symbols, *a)
        try:
            return call()
        finally:
            sparse._engine_has = routed

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

    res = {"case": case, "N": n, "nnz": nnz, "device": torch.cuda.get_device_name(0),
           "torch_version": torch.__version__, "source_id": _lib.source_id()}
    res["wall_ms"] = timed(call)
    res["torch_ms"] = timed(torch_form)
    C, T = call(), torch_form()
    torch.cuda.synchronize()
    res["nnzC"] = C.nnz
    res["identical"] = bool(C.indptr.dtype == T.indptr.dtype and torch.equal(C.indptr, T.indptr) and
                            torch.equal(C.indices, T.indices) and
                            torch.equal(C.data.view(torch.int64), T.data.view(torch.int64)))
    hd = _lib.get_handle(0)
    hd.set_stream(torch.cuda.current_stream().cuda_stream)
    dev_ms = []
    for _ in range(runs):
        hd.set_timing(True)
        call()
        t = hd.get_timing()
        dev_ms.append(sum(ms for ms, launches in t.values() if launches))
        res["launches"] = {k: v[1] for k, v in t.items() if v[1]}
        res["phase_ms"] = {k: round(v[0], 4) for k, v in t.items() if v[1]}
    hd.set_timing(False)
    res["device_ms"] = stats(dev_ms)
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
    print(f"RUNS={runs} WARMUP={warmup} ROUNDS={args.rounds}", flush=True)
    for case in args.cases:
        rounds = [child(args.root, case, runs, warmup) for _ in range(args.rounds)]   # each a fresh process
        a = rounds[0]
        print(f"== {case}: N={a['N']} nnz={a['nnz']} nnzC={a['nnzC']} fp64 on {a['device']} "
              f"(source_id {a['source_id']})")
        for r, x in enumerate(rounds):
            print(f"(a) spg_canonicalize round {r}: wall {fmt(x['wall_ms'])}; device {fmt(x['device_ms'])}")
        for r, x in enumerate(rounds):
            print(f"(b) torch ops        round {r}: wall {fmt(x['torch_ms'])}   (torch {x['torch_version']})")
        print(f"    launches per call: {a['launches']}; device ms per phase (last run): {a['phase_ms']}")
        am = sorted(x["wall_ms"]["median"] for x in rounds)
        bm = sorted(x["torch_ms"]["median"] for x in rounds)
        print(f"    (b)/(a) median/median: {bm[len(bm) // 2] / am[len(am) // 2]:.2f}x; "
              f"worst case for (a) [min (b) / max (a)]: {bm[0] / am[-1]:.2f}x")
        print(f"    results identical (indptr, indices, value bits): {all(x['identical'] for x in rounds)}", flush=True)


if __name__ == "__main__":
    main()
