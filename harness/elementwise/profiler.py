#!/usr/bin/env python3
"""Element-wise operations on the GPU: spg_csr_binop (multiply, maximum, minimum) and
spg_csr_mul_dense (full matrix, row vector, column vector), with spg_csrgeam on the same operands
beside them.

Ports nothing the reference times: the reference multiplies and takes maximum / minimum with
kernels of its own (modify_src/cupy-src/cupyx/scipy/sparse/_csr.py:297-342) and never measures
them.  This profiler records what they cost on the matrices of the benchmark configurations
(harness/configs.py): config 4's A and B (N = 65536, density 5e-3, fp64, about 328 entries per row)
and config 2's (N = 16384, density 1e-3, fp64, about 16 per row).  The addition is unchanged code
and the only comparator: a binop reads both operands' values in both of its passes and runs one
scan more, so it is expected to cost more than the addition.

Per case, in fresh child processes (ROUNDS of them, default 3), for each operation:
  wall ms per call (device events around the shim's call, the workspace and result allocations and
  the one host wait for nnz(C) included), the device ms of its kernels from spg_get_timing with the
  launches per phase, and the compulsory bytes -- the least traffic the operation can do:
    binop / csrgeam   (nnzA + nnzB + nnzC) * (4 + sizeof T) plus the three row pointers;
    mul_dense         nnz * (4 + 2 * sizeof T) plus the row pointer plus the elements of the dense
                      operand that are needed: nnz of them for a full matrix (one per stored entry,
                      not the whole n x n array), n for a row or a column vector.
Every figure is the median of RUNS (environment, default 20) calls after WARMUP (default 5); min
and max are printed beside it.  Each binop result is compared with the torch form of the same rule
(sparse._binop_torch) array for array, each dense product with sparse._mul_dense_torch; values
are compared by the project's rule (NaN where the other has NaN, every other component bit for bit).
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"config4": (65536, 5e-3), "config2": (16384, 1e-3)}
OPS = ("multiply", "maximum", "minimum")
DENSE = ("full", "row", "col")


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
    if not (cusparse.has_elementwise() and cusparse.has_csrgeam()):
        sys.exit("this tree's library does not export the element-wise entry points")
    hd = _lib.get_handle(0)
    hd.set_stream(torch.cuda.current_stream().cuda_stream)
    esz, isz = A.data.element_size(), A.indptr.element_size()

    def measure(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        wall = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = fn()
            b.record()
            b.synchronize()
            wall.append(a.elapsed_time(b))
            del r
        dev_ms, out = [], {}
        for _ in range(runs):
            hd.set_timing(True)
            fn()
            t = hd.get_timing()
            dev_ms.append(sum(ms for ms, launches in t.values() if launches))
            out["launches"] = {k: v[1] for k, v in t.items() if v[1]}
            out["phase_ms"] = {k: round(v[0], 4) for k, v in t.items() if v[1]}
        hd.set_timing(False)
        out["wall_ms"], out["device_ms"] = stats(wall), stats(dev_ms)
        return out

    def same_values(x, y):
        """NaN exactly where the other has NaN (sign and payload are unspecified), else the same bits."""
        if x.shape != y.shape:
            return False
        x, y = (torch.view_as_real(t) if t.is_complex() else t for t in (x, y))
        bits = torch.int32 if x.dtype == torch.float32 else torch.int64
        nx, ny = torch.isnan(x), torch.isnan(y)
        return bool(torch.equal(nx, ny) and torch.equal(x.contiguous().view(bits)[~nx], y.contiguous().view(bits)[~ny]))

    def same(C, T):
        return bool(torch.equal(C.indptr.to(torch.int64), T.indptr.to(torch.int64)) and torch.equal(C.indices, T.indices)
                    and same_values(C.data, T.data))

    res = {"case": case, "N": n, "nnzA": A.nnz, "nnzB": B.nnz, "device": torch.cuda.get_device_name(0),
           "torch_version": torch.__version__, "source_id": _lib.source_id(), "ops": {}}
    calls = {"csrgeam": lambda: cusparse.csrgeam2(A, B)}
    calls.update({op: (lambda op=op: cusparse.csrbinop(A, B, op)) for op in OPS})
    for name, fn in calls.items():
        r = measure(fn)
        C = fn()
        torch.cuda.synchronize()
        r["nnzC"] = C.nnz
        r["bytes"] = (A.nnz + B.nnz + C.nnz) * (4 + esz) + (2 * isz + C.indptr.element_size()) * (n + 1)
        if name in OPS:
            r["identical"] = same(C, sparse._binop_torch(A, B, name))
        res["ops"][name] = r
    g = torch.Generator(device="cpu").manual_seed(7)
    for which in DENSE:
        shape = {"full": (n, n), "row": (1, n), "col": (n, 1)}[which]
        if which == "full" and n * n * esz > 8 << 30:      # config 4's full operand would take 32 GiB
            continue
        D = torch.randn(shape, generator=g, dtype=A.data.dtype).to(dev)
        r = measure(lambda: cusparse.multiply_by_dense(A, D))
        C = cusparse.multiply_by_dense(A, D)
        torch.cuda.synchronize()
        r["nnzC"] = C.nnz
        r["bytes"] = A.nnz * (4 + 2 * esz) + isz * (n + 1) + min(D.numel(), A.nnz) * esz
        want = sparse._mul_dense_torch(A.data, A.indices, A.indptr, n, D)
        r["identical"] = same_values(C.data, want)
        res["ops"]["mul_dense_" + which] = r
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


def med(values):
    values = sorted(values)
    return values[len(values) // 2]


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
        print(f"== {case}: N={a['N']} nnzA={a['nnzA']} nnzB={a['nnzB']} fp64 on {a['device']} "
              f"(source_id {a['source_id']})")
        geam = med(x["ops"]["csrgeam"]["device_ms"]["median"] for x in rounds)
        for name, first in a["ops"].items():
            for r, x in enumerate(rounds):
                o = x["ops"][name]
                print(f"{name:16s} round {r}: wall {fmt(o['wall_ms'])}; device {fmt(o['device_ms'])}")
            dm = med(x["ops"][name]["device_ms"]["median"] for x in rounds)
            print(f"    nnzC={first['nnzC']}; launches per call: {first['launches']}; device ms per phase (last run): "
                  f"{first['phase_ms']}")
            print(f"    compulsory traffic {first['bytes']} bytes; over device time {dm:.3f} ms = "
                  f"{first['bytes'] / dm / 1e6:.1f} GB/s")
            if name in OPS:
                print(f"    device time over spg_csrgeam's on the same operands: {dm / geam:.2f}x")
            if "identical" in first:
                print(f"    identical to the torch form (structure, value bits): "
                      f"{all(x['ops'][name]['identical'] for x in rounds)}")


if __name__ == "__main__":
    main()
