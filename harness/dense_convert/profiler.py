#!/usr/bin/env python3
"""Dense <-> CSR conversion on the GPU: spg_csr2dense and spg_dense2csr against the torch
compositions they replace.

Ports nothing the reference times: the reference converts with ``C.toarray()`` (cupyx's
csr2dense kernel, modify_src/cupy-src/cupyx/scipy/sparse/_csr.py:383-428) in its
numerical_error/ scripts and others/test_cupy.py, and with ``csr_matrix(dense)``
(_csr.py:60-80) around others/spmm/, and never measures either on its own.  This profiler shows
what the engine's two conversions cost on an N x N matrix of a given density against torch on the
same device, in the same process and run:

  csr2dense  (a) ``A.todense()`` (spg_csr2dense, the result's allocation included);
             (t) ``torch.zeros`` + ``index_put_(accumulate=True)`` with the row ids precomputed;
  dense2csr  (a) ``cusparse.dense2csr(D)`` (spg_dense2csr_nnz + spg_dense2csr, allocations and
                 the one host wait included);
             (t) ``D.nonzero()`` + a gather of the values (no row pointer is built).

Per direction: wall ms per call from device events around it (median of RUNS calls after WARMUP,
environment, defaults 20 and 5; min and max beside it), the device ms of the engine's kernels
from spg_get_timing, and GB/s over the compulsory bytes: one write of D for csr2dense; two reads
of D plus one write of C (indices, values, row pointer) for dense2csr.  torch's figures are
given over the same byte counts.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))


def stats(times):
    times = sorted(times)
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1]}


def fmt(s, nbytes):
    return (f"{s['median']:.3f} ms (min {s['min']:.3f}, max {s['max']:.3f}) "
            f"{nbytes / s['median'] / 1e6:.1f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--densities", type=float, nargs="+", default=[1e-3, 1e-2, 1e-1])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--order", choices=["C", "F"], default="C")
    args = ap.parse_args()
    runs, warmup = int(os.environ.get("RUNS", "20")), int(os.environ.get("WARMUP", "5"))

    import numpy as np
    import torch
    from spmm_amd import _lib, cusparse, gen
    if not (torch.cuda.is_available() and cusparse.has_dense_convert()):
        sys.exit("needs a GPU and a library that exports spg_csr2dense / spg_dense2csr")
    dev = torch.device("cuda", 0)
    hd = _lib.get_handle(0)

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

    def device_ms(fn):
        hd.set_stream(torch.cuda.current_stream().cuda_stream)
        out = []
        for _ in range(runs):
            hd.set_timing(True)
            r = fn()
            t = hd.get_timing()
            out.append(sum(ms for ms, launches in t.values() if launches))
            del r
        hd.set_timing(False)
        return stats(out)

    n = args.n
    print(f"RUNS={runs} WARMUP={warmup} N={n} order={args.order} on {torch.cuda.get_device_name(0)} "
          f"(source_id {_lib.source_id()}, torch {torch.__version__})")
    for dname in args.dtypes:
        for density in args.densities:
            A = gen.random_csr(n, n, density, seed=42, device=dev).astype(np.dtype(dname))
            assert A.has_canonical_format
            esz = A.data.element_size()
            rows = A._row_ids()
            cols = A.indices.to(torch.int64)
            torch.cuda.synchronize()
            res = {"N": n, "density": density, "dtype": dname, "order": args.order, "nnz": A.nnz}

            def torch_todense():
                d = torch.zeros((n, n), dtype=A.data.dtype, device=dev)
                d.index_put_((rows, cols), A.data, accumulate=True)
                return d
            b_dense = n * n * esz
            res["csr2dense_bytes"] = b_dense
            res["csr2dense_ms"] = timed(lambda: A.todense(order=args.order))
            res["csr2dense_device_ms"] = device_ms(lambda: A.todense(order=args.order))
            res["torch_todense_ms"] = timed(torch_todense)
            D = A.todense(order=args.order)
            assert torch.equal(D, torch_todense())      # (canonical A: nothing to add up)

            def torch_fromdense():
                nz = D.nonzero()
                return nz, D[nz[:, 0], nz[:, 1]]
            b_csr = 2 * n * n * esz + A.nnz * (4 + esz) + 4 * (n + 1)
            res["dense2csr_bytes"] = b_csr
            res["dense2csr_ms"] = timed(lambda: cusparse.dense2csr(D))
            res["dense2csr_device_ms"] = device_ms(lambda: cusparse.dense2csr(D))
            res["torch_fromdense_ms"] = timed(torch_fromdense)
            C = cusparse.dense2csr(D)
            assert C.nnz == int((A.data != 0).sum()) and torch.equal(C.indptr.to(torch.int64), A.indptr.to(torch.int64))
            print(f"== {dname} density {density:g}: nnz {A.nnz}")
            print(f"csr2dense  (a) engine wall   {fmt(res['csr2dense_ms'], b_dense)}")
            print(f"           (a) engine device {fmt(res['csr2dense_device_ms'], b_dense)}")
            print(f"           (t) zeros + index_put_(accumulate) {fmt(res['torch_todense_ms'], b_dense)}")
            print(f"dense2csr  (a) engine wall   {fmt(res['dense2csr_ms'], b_csr)}")
            print(f"           (a) engine device {fmt(res['dense2csr_device_ms'], b_csr)}")
            print(f"           (t) nonzero + gather {fmt(res['torch_fromdense_ms'], b_csr)}")
            print("RESULT " + json.dumps(res), flush=True)
            del A, D, C, rows, cols
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
