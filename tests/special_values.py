"""IEEE special values for the parity tests: value recipes, the comparison rule and the
case table shared by tests/test_special_values_cpu.py and tests/test_gpu_special_values.py.

A plain helper module (no pytest hooks).  Everything is generated from seeds.

Recipes (`values`): they replace a matrix's values and leave its structure alone.
  tiny   +-sqrt(finfo.tiny) * 2^U(a, b): products land around finfo.tiny, about half of them
         denormal, and the partial sums move in and out of the denormal range;
  huge   +-sqrt(finfo.max) * 2^U(-3, 0.25): most products finite, some overflow, sums overflow
         to +-inf and inf - inf gives NaN;
  ints   +-{1, 2}: many columns cancel exactly to +0.0 and stay in C as structural entries;
  mixed  standard_normal with p_inf of the entries +inf, p_inf -inf, p_nan NaN, 5 % +0.0 and
         5 % -0.0.

Comparison rule (`assert_same_special`): structure equal; per real component (complex values
as (re, im) pairs) the NaN masks equal and every component that is not NaN bit-equal (so +-0,
denormals and +-inf are compared by their bits).  NaN sign and payload are NOT compared: x86
gives 0xFFF8... for inf - inf and the GPU need not.  That is the only relaxation, and the NaN
cap below bounds what it can hide.

Conditions (`check_conditions`), asserted on the oracle's output so that no case passes
vacuously: NaN components <= 10 % in every case; tiny: denormal >= 10 %; huge: inf >= 0.5 %;
ints: exact zeros >= 0.1 %; mixed: NaN >= 0.05 %.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import scipy.sparse as sp

REGIMES = ("tiny", "huge", "ints", "mixed")
DTYPES = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}

NAN_CAP = 0.10
FLOORS = {"tiny": ("denormal", 0.10), "huge": ("inf", 0.005), "ints": ("zero", 0.001), "mixed": ("nan", 0.0005)}


def real_dtype(dt):
    return np.dtype(dt).type(0).real.dtype


def values(regime, n, rng, real_dtype, scale=1.0, exps=None, p_inf=0.004, p_nan=0.002, sign=0):
    """n values of `real_dtype` for `regime`.  `scale` multiplies the magnitudes of tiny and
    huge (a power of two keeps the recipe's mantissas); `exps` = (a, b) is tiny's (huge's)
    exponent range; `sign` = +1 / -1 makes every tiny, huge or ints value positive / negative
    (0: random signs)."""
    fi = np.finfo(real_dtype)
    sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0) if sign == 0 else np.full(n, float(sign))
    if regime == "tiny":
        a, b = exps or (-2.0, 2.0)
        v = sgn * float(np.sqrt(fi.tiny)) * np.exp2(rng.uniform(a, b, n)) * scale
    elif regime == "huge":
        a, b = exps or (-3.0, 0.25)
        v = sgn * float(np.sqrt(float(fi.max))) * np.exp2(rng.uniform(a, b, n)) * scale
    elif regime == "ints":
        v = sgn * rng.integers(1, 3, n)
    elif regime == "mixed":
        v = rng.standard_normal(n)
        u = rng.random(n)
        edges = np.cumsum([p_inf, p_inf, p_nan, 0.05, 0.05])
        for lo, hi, x in zip(np.concatenate([[0.0], edges[:-1]]), edges, (np.inf, -np.inf, np.nan, 0.0, -0.0)):
            v = np.where((u >= lo) & (u < hi), x, v)
    else:
        raise ValueError(regime)
    return v.astype(real_dtype)


def draw(regime, shape, rng, dt, **kw):
    """An array of `shape` and dtype `dt` (complex: real and imaginary parts drawn in turn)."""
    n = int(np.prod(shape))
    rd = real_dtype(dt)
    v = values(regime, n, rng, rd, **kw)
    if np.dtype(dt).kind == "c":
        im = values(regime, n, rng, rd, **kw)
        out = np.empty(n, dtype=dt)
        out.real, out.imag = v, im
        v = out
    return v.reshape(shape)


def fill(S, regime, rng, dt, **kw):
    """A copy of the CSR structure S with values of dtype `dt` from `regime`."""
    return sp.csr_matrix((draw(regime, (S.nnz,), rng, dt, **kw), S.indices, S.indptr), shape=S.shape)


def _comps(x):
    x = np.ascontiguousarray(x)
    return x.view(real_dtype(x.dtype)).ravel()


def _bits(c):
    return c.view(np.uint32 if c.dtype == np.float32 else np.uint64)


def assert_values_special(got, ref, what="values"):
    """NaN exactly where ref has NaN; every other component bit-equal."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype, f"{what}: dtype {got.dtype} != {ref.dtype}"
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    g, r = _comps(got), _comps(ref)
    gn, rn = np.isnan(g), np.isnan(r)
    gb, rb = _bits(g), _bits(r)
    bad = (gn != rn) | (~rn & ~gn & (gb != rb))
    if bad.any():
        at = np.flatnonzero(bad)
        w = 2 * g.dtype.itemsize
        first = ", ".join(f"[{i}] got {int(gb[i]):#0{w + 2}x} ({g[i]!r}) want {int(rb[i]):#0{w + 2}x} ({r[i]!r})"
                          for i in at[:5])
        raise AssertionError(f"{what}: {at.size} of {g.size} components differ (component index): {first}")


def assert_same_special(got, ref):
    """got, ref: (indptr, indices, data[, ...]) of a CSR result."""
    p, j, x = got[:3]
    rp, rj, rx = ref[:3]
    assert np.array_equal(np.asarray(p, dtype=np.int64), np.asarray(rp, dtype=np.int64)), "row pointer"
    assert np.array_equal(j, rj), "column indices"
    assert_values_special(x, rx)


def classes(ref_values):
    """Shares of the components that are NaN, inf, denormal and exactly zero."""
    c = _comps(ref_values)
    n = max(c.size, 1)
    a = np.abs(c)
    return {"nan": float(np.isnan(c).sum()) / n, "inf": float(np.isinf(c).sum()) / n,
            "denormal": float(((a > 0) & (a < np.finfo(c.dtype).tiny)).sum()) / n,
            "zero": float((c == 0).sum()) / n}


def check_conditions(regime, ref_values, floors=True):
    sh = classes(ref_values)
    assert sh["nan"] <= NAN_CAP, (regime, sh)
    if floors:
        name, lo = FLOORS[regime]
        assert sh[name] >= lo, (regime, sh)
    return sh


def cmul(a, s):
    """a * s with numpy's complex rule (ac - bd) + (ad + bc)i spelled out on the real parts,
    every product and sum rounded on its own (numpy's own complex loops may fuse them)."""
    s = np.asarray(s)
    if s.dtype.kind != "c":
        with np.errstate(all="ignore"):
            return s.dtype.type(a) * s
    rd = real_dtype(s.dtype)
    a = complex(a)
    ar, ai = rd.type(a.real), rd.type(a.imag)
    out = np.empty_like(s)
    with np.errstate(all="ignore"):
        out.real = ar * s.real - ai * s.imag
        out.imag = ar * s.imag + ai * s.real
    return out


def axpby(alpha, s, beta, y):
    """The engine's epilogue on the host: (alpha == 1 ? s : alpha * s) [+ beta * y if beta != 0]."""
    v = s if alpha == 1 else cmul(alpha, s)
    if beta != 0:
        with np.errstate(all="ignore"):
            v = v + cmul(beta, y)     # complex add is componentwise
    return v


# ---------------------------------------------------------------------------------------------
# The case table: one structure per kernel path of spgemm, A cut to 128 rows (the planner looks
# at entries per row, not at the row count).  Structures come from the shapes the GPU suite
# already uses to reach each path (tests/test_gpu_parity.py); `expect` is what plan_info must say.
#
# STRUCTS: name -> (rows of A, k, n, density of A, density of B).
#   general: B is test_complex_bitexact's 2000 x 200000 at 2e-4 (40 entries per row).  That
#            test's A (density 2e-4, 0.4 entries per row) gives C one product per entry, so no
#            real sum could ever cancel and the `ints` floor would be out of reach; A here has
#            75 entries per row (3000 products per C row over 200000 columns, ~0.75 % of the
#            entries sum two products).  The margin to the tile path is thin: want_tile takes a
#            shape once (1 - exp(-avgA * avgB / n)) * 4096 reaches 64, and here it is about 60
#            (avgA 73.5 after duplicates, avgB 40).  Fewer entries per row starve the `ints`
#            floor (0.13 % zeros now, floor 0.1 %), so a retune of want_tile's threshold will
#            flip this case to the tile path and fail its path assert: pick A's density anew then.
#   dense2048: an empty A row and 40 empty B rows (test_tile_path_dense_2048).
#   sparse8192: A at 0.0075 (300 per row) with one 3000-entry row (test_tile_path_sparse_8192).
STRUCTS = {
    "short": (128, 2048, 2048, 0.004, 0.004),
    "general": (128, 2000, 200000, 0.0375, 2e-4),
    "owner": (128, 4096, 4096, 0.01, 0.01),
    "runs32": (128, 2048, 2048, 0.2, 0.2),
    "dense1024": (128, 4096, 4096, 0.02, 0.02),
    "dense2048": (128, 17000, 17000, 0.01, 0.01),
    "sparse8192": (128, 40000, 40000, 0.0075, 7.5e-4),
}


def _rand_struct(rng, m, n, density):
    nnz = int(round(density * m * n))
    M = sp.csr_matrix((np.ones(nnz), (rng.integers(0, m, nnz), rng.integers(0, n, nnz))), shape=(m, n))
    M.sum_duplicates()
    M.sort_indices()
    M.data[:] = 1.0
    return M


@functools.lru_cache(maxsize=None)
def structure(name):
    """(A, B) structures (values 1.0), canonical, built once per process."""
    m, k, n, da, db = STRUCTS[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A, B = _rand_struct(rng, m, k, da), _rand_struct(rng, k, n, db)
    if name == "dense2048":
        A = A.tolil(); A[5, :] = 0; A = sp.csr_matrix(A)
        keep = np.ones(k, bool); keep[100:140] = False
        B = sp.csr_matrix(sp.diags(keep.astype(float)) @ B)
        B.eliminate_zeros()
    if name == "sparse8192":
        A = A.tolil()
        A[7, :] = _rand_struct(rng, 1, k, 0.075)
        A = sp.csr_matrix(A)
    for M in (A, B):
        M.sum_duplicates()
        M.sort_indices()
        M.data[:] = 1.0
    return A, B


# Recipe parameters per structure and regime (defaults where absent), chosen so that the
# conditions hold, and the class shares of the oracle's alpha = 1 output measured with them
# (components; f32 / f64 first, complex where it differs).  Structures that sum many products per
# C entry need smaller tiny exponents (the sum of P denormal-range products leaves the range),
# a downward huge scale (else most sums overflow and inf - inf makes NaN past the cap) and
# smaller p_inf / p_nan (a C entry is NaN once any of its P products is).
#   products per C entry: short 1.0, general 1.0, owner 1.2, runs32 67, dense1024 2.0,
#   dense2048 2.1, sparse8192 1.2, SpMV / SpMM 20
#
# Measured shares in % of the components (the regime's own class; then NaN where not 0).
# Defaults: tiny exps (-2, 2), huge exps (-3, 0.25) scale 1, mixed p_inf 0.004 p_nan 0.002.
#   structure-dtype   tiny: denormal | huge: inf, nan | ints: zero | mixed: nan, inf
#   short-f32         48.4 | 1.24, 0    |  0.24 | 0.69, 1.09      defaults
#   short-f64         50.0 | 1.14, 0    |  0.45 | 0.47, 1.14      defaults
#   short-c64         30.0 | 4.42, 0.01 | 18.48 | 1.17, 2.62      defaults
#   short-c128        29.8 | 4.28, 0.01 | 19.16 | 1.10, 3.06      defaults
#   general-f64       49.9 | 1.26, 0    |  0.13 | 0.54, 1.46      defaults
#   general-c64       30.3 | 4.59, 0.01 | 18.57 | 1.06, 3.04      defaults
#   owner-f32         45.4 | 1.93, 0    |  3.30 | 0.81, 1.96      defaults
#   owner-c64         27.3 | 6.54, 0.04 | 16.90 | 1.42, 3.70      defaults
#   runs32-f32        51.0 | 19.93, 0   |  1.96 | 2.17, 4.02      tiny exps (-4, 0); huge scale 0.5;
#                                                                  mixed p_inf 2e-4 p_nan 1e-4
#       (with the defaults: tiny 3.5 % denormal, huge 26 % NaN, mixed 41 % NaN.  At scale 0.5 no
#        single product overflows, the sums do, and a sum that reached inf stays there: no NaN)
#   dense1024-f64     35.6 | 4.96, 0.02 |  8.15 | 1.08, 2.84      defaults
#   dense1024-c128    21.1 | 13.96, 0.23| 12.16 | 2.36, 5.60      defaults
#   dense2048-f64     34.7 | 5.32, 0.02 |  8.28 | 1.10, 2.84      defaults
#   sparse8192-f64    47.2 | 1.75, 0    |  2.16 | 0.68, 1.71      defaults
#   alpha = -0.75 / 0 (NaN %, the highest regime): short-f32 0.69 / 1.78, short-f64 0.47 / 1.61,
#       short-c64 4.43 / 7.72, short-c128 4.29 / 7.71, dense2048-f64 1.10 / 5.34
#   underflow (tiny, A > 0, B < 0): runs32-f32 +0.0 2.33, denormal 97.7; dense2048-f64 +0.0 30.2,
#       denormal 69.9.  Explicit +0.0 in A (dense1024-f64, ints): zero 11.8
#   SpMV (SpMM n = 17 within 1 of it): tiny exps (-3.5, 0.5); huge scale 0.6 (complex 0.5);
#       mixed p_inf 3e-4 p_nan 1e-4
#     f32   48.2 | 8.15, 0 | 3.17 | 1.07, 1.68      f64   48.7 | 7.45, 0 | 3.78 | 0.24, 1.39
#     c64   33.9 | 6.13, 0 | 2.28 | 1.45, 4.04      c128  34.6 | 6.48, 0 | 2.58 | 0.94, 5.31
#     alpha = -0.75, beta = 0.5 (NaN %): real as above; complex huge 6.1-6.5, mixed 5.5-6.3;
#     with y at the sums' scale (_y_params) tiny stays 44-60 % denormal and huge 5.6-8.2 % inf
#     (with the defaults: tiny 7 % denormal, huge 25 % NaN for complex, mixed 10-26 % NaN)
#     The floors of ints and mixed are asserted on the plain sums (alpha = 1, beta = 0) only; on
#     the alpha / beta forms of SpMV and SpMM they get the NaN cap alone (alpha * s + beta * y
#     hardly ever cancels to zero, and its NaNs are those of s and y).  tiny and huge keep their
#     floors there too.  The same holds for spgemm's alpha cases: floors on alpha = 1 and
#     alpha = -0.75, the cap alone on alpha = 0.
PARAMS = {
    "short": {},
    "general": {},
    "owner": {},
    "runs32": {"tiny": {"exps": (-4.0, 0.0)}, "huge": {"scale": 0.5},
               "mixed": {"p_inf": 2e-4, "p_nan": 1e-4}},
    "dense1024": {},
    "dense2048": {},
    "sparse8192": {},
    # SpMV / SpMM (20 products per output).  A complex alpha * s turns every inf component into
    # two NaNs (0 * inf in the cross terms), so the complex huge scale keeps inf under the cap.
    "spmv": {"tiny": {"exps": (-3.5, 0.5)}, "huge": {"scale": 0.6}, ("huge", "c"): {"scale": 0.5},
             "mixed": {"p_inf": 3e-4, "p_nan": 1e-4}},
}

# (id, structure, dtype, env, expect): env holds schedule-only switches read per plan.
CASES = [
    ("short-f32", "short", "f32", {}, {"path": "short"}),
    ("short-f64", "short", "f64", {}, {"path": "short"}),
    ("short-c64", "short", "c64", {}, {"path": "short"}),
    ("short-c128", "short", "c128", {}, {"path": "short"}),
    ("general-f64", "general", "f64", {}, {"path": "general"}),
    ("general-c64", "general", "c64", {}, {"path": "general"}),
    # 2048-column tiles with symbolic bitmaps, k_tile's owner rounds (fp32 / complex64 never
    # take the ordered-LDS kernels; B segments of 20 entries per tile, under the 48 of the runs)
    ("owner-f32", "owner", "f32", {}, {"path": "tile", "dense_tiles": False, "lds_ordered": False}),
    ("owner-c64", "owner", "c64", {}, {"path": "tile", "dense_tiles": False, "lds_ordered": False}),
    # k_tile_dn<float, .., 1024>: B segments of about 186 entries per 1024-column tile.  For fp32
    # plan_info's lds_ordered says that the entry runs and their ds_add_f32 are what runs (the
    # device's fp32 LDS check passed, the segments are long enough, SPG_F32_RUNS is not 0)
    ("runs32-f32", "runs32", "f32", {},
     {"path": "tile", "tile_width": 1024, "dense_tiles": True, "lds_ordered": True}),
    ("runs32-f32-norun", "runs32", "f32", {"SPG_F32_RUNS": "0"},
     {"path": "tile", "tile_width": 1024, "dense_tiles": True, "lds_ordered": False}),
    ("dense1024-f64", "dense1024", "f64", {},
     {"path": "tile", "tile_width": 1024, "dense_tiles": True, "lds_ordered": True}),
    ("dense1024-c128", "dense1024", "c128", {},
     {"path": "tile", "tile_width": 1024, "dense_tiles": True, "lds_ordered": True}),
    ("dense2048-f64", "dense2048", "f64", {},
     {"path": "tile", "tile_width": 2048, "dense_tiles": True, "lds_ordered": True}),
    ("sparse8192-f64", "sparse8192", "f64", {},
     {"path": "tile", "tile_width": 8192, "dense_tiles": False, "lds_ordered": True, "record_group": 8}),
    ("sparse8192-f64-rg1", "sparse8192", "f64", {"SPG_SP_RECORD_GROUP": "1"},
     {"path": "tile", "tile_width": 8192, "dense_tiles": False, "lds_ordered": True, "record_group": 1}),
]
CASE = {c[0]: c for c in CASES}
ALPHA_CASES = ["short-f32", "short-f64", "short-c64", "short-c128", "dense2048-f64"]
ALPHAS = [-0.75, 0.0]


def params(struct, regime, dt):
    """values() keyword arguments of a structure and regime ((regime, "c"): complex dtypes)."""
    P = PARAMS[struct]
    if np.dtype(dt).kind == "c" and (regime, "c") in P:
        return dict(P[(regime, "c")])
    return dict(P.get(regime, {}))


def seed_of(*parts):
    return zlib.crc32("|".join(str(p) for p in parts).encode())


def inputs(case, regime, variant=""):
    """(A, B) of a case and regime; `variant`: "" the plain recipe, "underflow" tiny with A all
    positive and B all negative and exponents low enough that most products underflow to -0.0,
    "azero" a tenth of A's entries an explicit +0.0.  Cases that differ only in their switches
    share their inputs."""
    return _inputs(CASE[case][1], CASE[case][2], regime, variant)


@functools.lru_cache(maxsize=16)
def _inputs(struct, dname, regime, variant):
    dt = DTYPES[dname]
    SA, SB = structure(struct)
    rng = np.random.default_rng(seed_of(struct, dname, regime, variant))
    kw = params(struct, regime, dt)
    if variant == "underflow":
        ex = UNDERFLOW_EXPS[struct]
        A = fill(SA, "tiny", rng, dt, exps=ex, sign=+1)
        B = fill(SB, "tiny", rng, dt, exps=ex, sign=-1)
    else:
        A = fill(SA, regime, rng, dt, **kw)
        B = fill(SB, regime, rng, dt, **kw)
    if variant == "azero":
        A.data[rng.random(A.nnz) < 0.1] = 0.0
    A.data.setflags(write=False)
    B.data.setflags(write=False)
    return A, B


# tiny exponents of the underflow variant: a product underflows to zero below
# finfo.tiny * 2^-(mantissa bits + 1), i.e. when the two exponents sum to less than -24 (f32) /
# -53 (f64).  runs32 sums 67 products per entry, so nearly all of them must underflow for an
# entry to see only -0.0 products (range sum in [-29, -23]: 94 % underflow); dense2048 sums
# about two (range sum in [-58, -48]: half of them underflow).
UNDERFLOW_EXPS = {"runs32": (-14.5, -11.5), "dense2048": (-29.0, -24.0)}


def reference(case, regime, alpha=1.0, variant=""):
    """The oracle's C for a case (OpenMP variant, 16 threads: identical values), computed once
    and never written."""
    return _reference(CASE[case][1], CASE[case][2], regime, float(alpha), variant)


@functools.lru_cache(maxsize=8)
def _reference(struct, dname, regime, alpha, variant):
    from oracle import oracle
    A, B = _inputs(struct, dname, regime, variant)
    ref = oracle.spgemm(A, B, alpha=alpha, keep_zeros=True, sort=True, threads=16)
    for a in ref:
        a.setflags(write=False)
    return ref


# SpMV / SpMM: a 4096 x 4096 A of density 0.005 (20 entries per row, so 20 products per output).
SPMV_N = 4096


@functools.lru_cache(maxsize=None)
def spmv_structure():
    return _rand_struct(np.random.default_rng(4096), SPMV_N, SPMV_N, 0.005)


def _y_params(regime, dt, kw):
    """The recipe of the y (C) that beta scales: the regime's own, with tiny's and huge's scale
    moved to where A x lives.  Drawn like x, a tiny y is ~sqrt(finfo.tiny), 2^63 (2^511) times
    the sums beside it, and alpha * s + beta * y would absorb every denormal of s: a flushed sum
    would pass.  tiny: scale sqrt(tiny), so y is ~tiny * 2^U(a, b), half of it denormal; huge:
    scale sqrt(max) / 4, so y is max * 2^U(-5, -1.75), finite, and the last add overflows too."""
    kw = dict(kw)
    fi = np.finfo(real_dtype(dt))
    if regime == "tiny":
        kw["scale"] = kw.get("scale", 1.0) * float(np.sqrt(fi.tiny))
    if regime == "huge":
        kw["scale"] = float(np.sqrt(float(fi.max))) / 4
    return kw


@functools.lru_cache(maxsize=8)
def spmv_inputs(regime, dname):
    """(A, x, y0) for SpMV."""
    dt = DTYPES[dname]
    rng = np.random.default_rng(seed_of("spmv", regime, dname))
    kw = params("spmv", regime, dt)
    A = fill(spmv_structure(), regime, rng, dt, **kw)
    x = draw(regime, (SPMV_N,), rng, dt, **kw)
    y0 = draw(regime, (SPMV_N,), rng, dt, **_y_params(regime, dt, kw))
    for a in (A.data, x, y0):
        a.setflags(write=False)
    return A, x, y0


# SpMM layouts (dtype, order, n).  Row-major operands take 16-byte accesses (V = 16 / sizeof
# elements per lane) when every row of B and C starts on a 16-byte boundary, V = 1 otherwise;
# at most 32 lanes wide they run k_spmm_row_packed (several rows per wave), else k_spmm_row.
#   n = 1, 17   packed, V = 1 (17 * sizeof is no multiple of 16; complex128 has V = 1 always)
#   n = 16      packed with V = 4 (fp32, 4 lanes) and V = 2 (fp64, 8 lanes)
#   n = 130     k_spmm_row: fp64 V = 2, a full strip of 128 columns and a 2-column one; fp32
#               V = 1 (520-byte rows), three strips; complex128 (16 bytes per element), three strips
#   n = 260     fp32 V = 4: a full strip of 256 columns and a 4-column one
#   rowld 131   fp64, B and C column slices of 132-wide parents (ld = 132, 16-byte aligned rows):
#               V = 2 with a partial vector (one valid column of two) in the last strip's lane 1
#   col 17      k_spmm_col, three column strips of 8 (complex128: five of 4), the last partial
SPMM_LAYOUTS = [(d, o, n) for d in ("f32", "f64", "c128") for o, n in [("row", 1), ("row", 17), ("row", 130), ("col", 17)]]
SPMM_LAYOUTS += [("f32", "row", 260), ("f32", "row", 16), ("f64", "row", 16), ("f64", "rowld", 131)]


@functools.lru_cache(maxsize=8)
def spmm_inputs(regime, dname, n):
    """(A, X, C0) for SpMM with n columns."""
    dt = DTYPES[dname]
    rng = np.random.default_rng(seed_of("spmm", regime, dname, n))
    kw = params("spmv", regime, dt)
    A = fill(spmv_structure(), regime, rng, dt, **kw)
    X = draw(regime, (SPMV_N, n), rng, dt, **kw)
    C0 = draw(regime, (SPMV_N, n), rng, dt, **_y_params(regime, dt, kw))
    for a in (A.data, X, C0):
        a.setflags(write=False)
    return A, X, C0
