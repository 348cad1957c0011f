#!/usr/bin/env python3
"""CSR transpose on the GPU: spg_csr2csc against the torch conversion it replaces.

Ports nothing the reference times: the reference converts with cupyx.cusparse.csr2csc
(modify_src/cupy-src/cupyx/cusparse.py:1014-1035) inside ``A.T @ ...`` and never measures it on
its own.  This profiler exists to show what moving ``csr_matrix.transpose_csr()`` from torch ops
(int64 key, torch.sort, unique_consecutive, bincount, cumsum) into the engine bought, on the
matrices of the benchmark configurations (harness/configs.py): config 4's A (N = 65536, density
5e-3, fp64) and config 2's (N = 16384, density 1e-3, fp64).

Per matrix:
  (a) this tree's ``transpose_csr()``: wall ms per call (device events around the call, workspace
      allocation included) and the device ms of its kernels from spg_get_timing;
  (b) ``transpose_csr()`` of another checkout, given with ``--parent ROOT`` (the commit before
      spg_csr2csc: the torch conversion), in processes of its own;
  (c) ``torch.sparse_csr_tensor(...).to_sparse_csc()`` as an outside figure.
Also: the queried workspace bytes against the rise of ``torch.cuda.max_memory_allocated`` over one
call of each, and the bytes/s of (a) over the least traffic a transpose can do,
2 * nnz * (4 + sizeof(T)) + the two row pointers.

Every figure is the median of RUNS (environment, default 20) calls after WARMUP (default 5); min
and max are printed beside it.  (a) and (b) run in fresh child processes, ROUNDS (default 3) of
each, alternating, so the spread between processes shows beside the spread inside one; the
results of the two trees are compared by a digest of their arrays.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"config4": (65536, 5e-3), "config2": (16384, 1e-3)}


def stats(times):
    times = sorted(times)
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1]}


def worker(root, case, runs, warmup, outside):
    """One tree's figures for one matrix, as a JSON line."""
    sys.path.insert(0, root)
    import torch
    from spmm_amd import _lib, cusparse, gen
    from spmm_amd.sparse import csr_matrix
    n, density = CASES[case]
    dev = torch.device("cuda", 0)
    if n <= 16384:
        A = csr_matrix(gen.scipy_pair(n, density, seed=42)[0], device=dev)
    else:
        A = gen.random_csr(n, n, density, seed=42, device=dev)
    assert A.has_canonical_format
    engine = bool(getattr(cusparse, "has_csr2csc", lambda: False)())

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

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del r
        return int(p)

    import spmm_amd
    res = {"case": case, "root": os.path.dirname(os.path.dirname(os.path.abspath(spmm_amd.__file__))), "engine": engine, "N": n, "nnz": A.nnz, "device": torch.cuda.get_device_name(0)}
    res["wall_ms"] = timed(A.transpose_csr)
    res["peak_bytes"] = peak(A.transpose_csr)
    T = A.transpose_csr()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (T.indptr.to(torch.int64), T.indices, T.data):
        h.update(t.cpu().numpy().tobytes())
    res["digest"] = h.hexdigest()[:16]
    res["result_bytes"] = int(sum(t.numel() * t.element_size() for t in (T.indptr, T.indices, T.data)))
    if engine:
        import ctypes
        hd = _lib.get_handle(0)
        hd.set_stream(torch.cuda.current_stream().cuda_stream)
        dev_ms = []
        for _ in range(runs):
            hd.set_timing(True)
            A.transpose_csr()
            t = hd.get_timing()
            dev_ms.append(sum(ms for ms, launches in t.values() if launches))
            res["launches"] = {k: v[1] for k, v in t.items() if v[1]}
        hd.set_timing(False)
        res["device_ms"] = stats(dev_ms)
        va, vt = cusparse._csr_view(A), cusparse._csr_view(T)
        need = ctypes.c_size_t(0)
        _lib.check(hd.lib.spg_csr2csc(hd.ptr, ctypes.byref(va), ctypes.byref(vt), ctypes.byref(need), None))
        res["workspace_bytes"] = int(need.value)
        esz = A.data.element_size()
        res["min_traffic_bytes"] = 2 * A.nnz * (4 + esz) + A.indptr.element_size() * (A.shape[0] + 1 + A.shape[1] + 1)
        res["source_id"] = _lib.source_id()
    if outside:
        S = torch.sparse_csr_tensor(A.indptr, A.indices, A.data, size=A.shape)
        res["torch_to_sparse_csc_ms"] = timed(S.to_sparse_csc)
        res["torch_version"] = torch.__version__
    print("RESULT " + json.dumps(res), flush=True)


def child(root, case, runs, warmup, outside):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", os.path.abspath(root), "--case", case]
    if outside:
        cmd.append("--outside")
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
    ap.add_argument("--parent", help="root of the checkout to compare against (its transpose_csr)")
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--rounds", type=int, default=int(os.environ.get("ROUNDS", "3")))
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--case")
    ap.add_argument("--outside", action="store_true")
    args = ap.parse_args()
    runs, warmup = int(os.environ.get("RUNS", "20")), int(os.environ.get("WARMUP", "5"))
    if args.worker:
        return worker(args.root, args.case, runs, warmup, args.outside)
    print(f"RUNS={runs} WARMUP={warmup} ROUNDS={args.rounds}")
    for case in args.cases:
        new, old = [], []
        for r in range(args.rounds):   # alternating, each in a fresh process
            new.append(child(args.root, case, runs, warmup, outside=(r == 0)))
            if args.parent:
                old.append(child(args.parent, case, runs, warmup, outside=False))
        a = new[0]
        if not a["engine"]:
            sys.exit("this tree's library does not export spg_csr2csc")
        print(f"== {case}: N={a['N']} nnz={a['nnz']} fp64 on {a['device']} (source_id {a['source_id']})")
        for r, x in enumerate(new):
            print(f"(a) spg_csr2csc   round {r}: wall {fmt(x['wall_ms'])}; device {fmt(x['device_ms'])}")
        for r, x in enumerate(old):
            if x["engine"] or x["root"] != os.path.abspath(args.parent):
                sys.exit("--parent must be a checkout without spg_csr2csc")
            print(f"(b) parent torch  round {r}: wall {fmt(x['wall_ms'])}")
        print(f"(c) torch to_sparse_csc ({a['torch_version']}): wall {fmt(a['torch_to_sparse_csc_ms'])}")
        print(f"    launches per call: {a['launches']}")
        am = [x["wall_ms"]["median"] for x in new]
        print(f"    (a) medians over rounds: min {min(am):.3f} max {max(am):.3f} ms")
        if old:
            bm = [x["wall_ms"]["median"] for x in old]
            print(f"    (b) medians over rounds: min {min(bm):.3f} max {max(bm):.3f} ms")
            print(f"    (b)/(a), worst case for (a) [min (b) / max (a)]: {min(bm) / max(am):.2f}x; "
                  f"median/median: {sorted(bm)[len(bm) // 2] / sorted(am)[len(am) // 2]:.2f}x")
            same = all(x["digest"] == a["digest"] for x in old + new)
            print(f"    results identical between the trees (sha256 of indptr|indices|data): {same} ({a['digest']})")
            print(f"    peak bytes over one call: (a) {a['peak_bytes']} (workspace query {a['workspace_bytes']}, "
                  f"result {a['result_bytes']}); (b) {old[0]['peak_bytes']}")
        else:
            print(f"    peak bytes over one call: (a) {a['peak_bytes']} (workspace query {a['workspace_bytes']}, "
                  f"result {a['result_bytes']})")
        dm = sorted(x["device_ms"]["median"] for x in new)[len(new) // 2]
        print(f"    minimum traffic {a['min_traffic_bytes']} bytes; over device time {dm:.3f} ms = "
              f"{a['min_traffic_bytes'] / dm / 1e6:.1f} GB/s")


if __name__ == "__main__":
    main()
