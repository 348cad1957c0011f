#!/usr/bin/env python3
"""SpMM rates on config 4's A (N = 65536, density 5e-3, fp64, spmm_amd.gen seed 42) times a
dense 65536 x n, n in {8, 64, 256}, row-major and column-major (profiles/spmm_first.txt).

Per case: ms per product (device events around REPS back-to-back products, after a warm-up),
2 * nnz * n / t, and the compulsory bytes (A's three arrays + B + C once) over t as a fraction
of the 8 TB/s HBM figure DESIGN uses.  Beside them, in the same process: (a) n calls of
cusparse.spmv on B's columns, (b) torch.sparse_csr_tensor @ B (rocSPARSE), "n/a" when it does
not run.  The first case of each order is also compared bit for bit against (a).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from spmm_amd import _lib, cusparse, gen  # noqa: E402

HBM = 8.0e12


def ms_per_call(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--density", type=float, default=5e-3)
    ap.add_argument("--cols", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spmm_rates.py needs a GPU")
    N = args.n
    A = gen.random_csr(N, N, args.density, seed=42, device="cuda")
    nnz = A.nnz
    info = _lib.load().spg_build_info().decode()
    print(f"# {info}")
    print(f"# library sha256[:16]={_lib.build_id()} device={torch.cuda.get_device_name(0)}")
    print(f"# A: {N} x {N} fp64 CSR, nnz={nnz} (density {args.density}, seed 42); reps={args.reps}; HBM figure 8 TB/s")
    try:
        At = torch.sparse_csr_tensor(A.indptr.to(torch.int64), A.indices.to(torch.int64), A.data, size=(N, N))
    except Exception as e:   # noqa: BLE001
        At = None
        print(f"# torch.sparse_csr_tensor: {type(e).__name__}: {e}")
    print(f"{'order':5} {'n':>4} {'spmm ms':>10} {'GFLOP/s':>10} {'compulsory GB':>14} {'GB/s':>9} {'/8TB/s':>7} "
          f"{'n x spmv ms':>12} {'rocSPARSE ms':>13}")
    for order in ("row", "col"):
        for n in args.cols:
            g = torch.Generator(device="cuda")
            g.manual_seed(7 + n)
            B = torch.randn((N, n), dtype=torch.float64, device="cuda", generator=g)
            if order == "col":
                B = B.t().contiguous().t()
            C = torch.zeros((N, n), dtype=torch.float64, device="cuda")
            if order == "col":
                C = torch.zeros((n, N), dtype=torch.float64, device="cuda").t()
            t_spmm = ms_per_call(lambda: cusparse.spmm(A, B, c=C), args.reps)
            cols = [B[:, j].contiguous() for j in range(n)]
            ys = [torch.zeros(N, dtype=torch.float64, device="cuda") for _ in range(n)]

            def by_spmv():
                for j in range(n):
                    cusparse.spmv(A, cols[j], y=ys[j])
            t_spmv = ms_per_call(by_spmv, max(2, args.reps // 4), warmup=1)
            if n == args.cols[0]:
                same = all(torch.equal(C[:, j].contiguous().view(torch.int64), ys[j].view(torch.int64))
                           for j in range(n))
                print(f"# {order}-major n={n}: spmm bit-equal to spmv per column: {same}")
            t_roc = "n/a"
            if At is not None:
                try:
                    t_roc = f"{ms_per_call(lambda: At @ B, max(2, args.reps // 4), warmup=1):.3f}"
                except Exception as e:   # noqa: BLE001
                    print(f"# torch.sparse_csr_tensor @ B ({order}, n={n}): {type(e).__name__}")
            bytes_ = nnz * (8 + 4) + (N + 1) * 4 + 2 * N * n * 8
            rate = bytes_ / (t_spmm * 1e-3)
            print(f"{order:5} {n:4d} {t_spmm:10.3f} {2.0 * nnz * n / (t_spmm * 1e-3) / 1e9:10.1f} "
                  f"{bytes_ / 1e9:14.4f} {rate / 1e9:9.1f} {rate / HBM:7.3f} {t_spmv:12.3f} {t_roc:>13}")


if __name__ == "__main__":
    main()
