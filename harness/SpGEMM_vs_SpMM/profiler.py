#!/usr/bin/env python3
"""SpGEMM (A @ B_sparse) against SpMM (A @ B_dense) on the same matrices, on the GPU: this
project's version of the measurement of the reference's others/spmm/spMM.py (n in
{128..1024} x density {0.01, 0.1, 0.5}) and others/spmm/diff_matrix_size.py (n in
{2**11..2**14} at density 0.001, with peak device memory), fp32 as there.

Per (n, density): A and B are seeded random CSR matrices (B with its own seed), B_dense is
B densified on the device (row-major, torch's layout).  Each product is timed with device
events around one ``@``; the figure is the median of RUNS (environment, default 5) after
WARMUP (default 2) untimed products of each kind.  Peak bytes are the rise of
``torch.cuda.max_memory_allocated`` over ``memory_allocated`` across one product with its
result kept alive (workspace + result; the reference reads the drop of free device memory).
The printed lines keep the reference's shapes.  ``--plot`` writes the three figures when
matplotlib is installed; nothing else needs it.
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from spmm_amd.sparse import csr_matrix  # noqa: E402

SMALL_SIZES, SMALL_DENSITIES = [128, 256, 512, 1024], [0.01, 0.1, 0.5]
LARGE_SIZES, LARGE_DENSITIES = [2 ** 11, 2 ** 12, 2 ** 13, 2 ** 14], [0.001]


def random_csr(n, density, seed):
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, format="csr", dtype=np.float32, random_state=rng)
    M.sort_indices()
    return M


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
        del out
    times.sort()
    return times[len(times) // 2]


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()   # kept alive across the reading
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def measure(n, density, runs, warmup, seed):
    A = csr_matrix(random_csr(n, density, seed), device="cuda")
    B = csr_matrix(random_csr(n, density, seed + 1), device="cuda")
    B_dense = torch.from_numpy(B.get().toarray()).cuda()
    spgemm = lambda: A @ B          # noqa: E731
    spmm = lambda: A @ B_dense      # noqa: E731
    return {"spgemm_ms": median_ms(spgemm, runs, warmup), "spmm_ms": median_ms(spmm, runs, warmup),
            "spgemm_peak": peak_bytes(spgemm), "spmm_peak": peak_bytes(spmm)}


def plot(results, sizes, densities, prefix):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:   # noqa: BLE001
        print("matplotlib is not installed: no figures")
        return
    for key, ylabel, name in (("ms", "Median time (ms)", "time_spgemm_vs_spmm"),
                              ("peak", "Peak device memory (MB)", "vram_peak_spgemm_vs_spmm")):
        fig, axes = plt.subplots(1, len(densities), figsize=(5 * len(densities), 4), squeeze=False)
        for ax, d in zip(axes[0], densities):
            scale = 1.0 if key == "ms" else 1.0 / 2 ** 20
            ax.plot(sizes, [results[(n, d)][f"spgemm_{key}"] * scale for n in sizes], marker="o",
                    label="SpGEMM (A@B_sparse)")
            ax.plot(sizes, [results[(n, d)][f"spmm_{key}"] * scale for n in sizes], marker="s",
                    label="SpMM (A@B_dense)")
            ax.set_xscale("log", base=2)
            ax.set_yscale("log")
            ax.set_title(f"density = {d}")
            ax.set_xlabel("Matrix size (n x n)")
            ax.set_ylabel(ylabel)
            ax.grid(True, which="both", linestyle="--", linewidth=0.5)
            ax.legend()
        fig.tight_layout()
        fig.savefig(f"{prefix}{name}.png", dpi=200, bbox_inches="tight")
        plt.close(fig)
    fig = plt.figure(figsize=(6, 4))
    ax = fig.gca()
    for d in densities:
        ax.plot(sizes, [results[(n, d)]["spgemm_ms"] / results[(n, d)]["spmm_ms"] for n in sizes], marker="o",
                label=f"density={d}")
    ax.axhline(1.0, linestyle="--")
    ax.set_xscale("log", base=2)
    ax.set_xlabel("Matrix size (n x n)")
    ax.set_ylabel("SpGEMM / SpMM time ratio")
    ax.legend()
    fig.tight_layout()
    fig.savefig(f"{prefix}time_ratio_spgemm_over_spmm.png", dpi=200, bbox_inches="tight")
    plt.close(fig)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", choices=["small", "large", "both"], default="both")
    ap.add_argument("--sizes", type=int, nargs="+", help="override the grid's sizes")
    ap.add_argument("--densities", type=float, nargs="+", help="override the grid's densities")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--plot", action="store_true")
    args = ap.parse_args()
    runs = int(os.environ.get("RUNS", "5"))
    warmup = int(os.environ.get("WARMUP", "2"))
    if not torch.cuda.is_available():
        sys.exit("SpGEMM_vs_SpMM/profiler.py needs a GPU")
    grids = []
    if args.grid in ("small", "both"):
        grids.append(("small", args.sizes or SMALL_SIZES, args.densities or SMALL_DENSITIES))
    if args.grid in ("large", "both"):
        grids.append(("large", args.sizes or LARGE_SIZES, args.densities or LARGE_DENSITIES))
    print(f"RUNS={runs} WARMUP={warmup} dtype=float32 device={torch.cuda.get_device_name(0)}")
    for name, sizes, densities in grids:
        results = {}
        for n in sizes:
            for d in densities:
                r = results[(n, d)] = measure(n, d, runs, warmup, args.seed)
                if name == "small":   # spMM.py's line
                    print(f"n={n:4d}, density={d:.2f}, Spgemm={r['spgemm_ms']:.4f} ms, "
                          f"spMM median= {r['spmm_ms']:.4f}")
                else:                 # diff_matrix_size.py's line
                    print(f"n={n:4d}, density={d}, SpGEMM={r['spgemm_ms']:.4f} ms, SpMM={r['spmm_ms']:.4f} ms | "
                          f"Peak VRAM SpGEMM={r['spgemm_peak'] / 2 ** 20} MB, SpMM={r['spmm_peak'] / 2 ** 20} MB "
                          f"({r['spgemm_peak']} / {r['spmm_peak']} bytes)")
        if args.plot:
            plot(results, sizes, densities, f"{name}_")


if __name__ == "__main__":
    main()
