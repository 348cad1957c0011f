"""IEEE special values on the CPU side (no GPU needed): the oracle against scipy on denormals,
+-0, +-inf and NaN, the sensitivity of the comparison rule, and the conditions that keep every
GPU case of tests/test_gpu_special_values.py from passing vacuously (tests/special_values.py).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle
from tests import special_values as sv

DNAMES = list(sv.DTYPES)


@functools.lru_cache(maxsize=None)
def _small(regime, dname):
    """300 x 400 by 400 x 500 at density 0.05 (about one product per C entry, C rows 63 % dense),
    a vector, a 17-column matrix: all from `regime` with the default parameters."""
    dt = sv.DTYPES[dname]
    rng = np.random.default_rng(sv.seed_of("small", regime, dname))
    SA = sp.random(300, 400, density=0.05, format="csr", random_state=rng)
    SB = sp.random(400, 500, density=0.05, format="csr", random_state=rng)
    SA.sort_indices()
    SB.sort_indices()
    A, B = sv.fill(SA, regime, rng, dt), sv.fill(SB, regime, rng, dt)
    return A, B, sv.draw(regime, (400,), rng, dt), sv.draw(regime, (400, 17), rng, dt)


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("regime", sv.REGIMES)
def test_oracle_spgemm_matches_scipy_on_special_values(regime, dname):
    A, B, _, _ = _small(regime, dname)
    p, j, x = oracle.spgemm(A, B, keep_zeros=True, sort=True)
    M = sp.csr_matrix((x.copy(), j.copy(), p.copy()), shape=(300, 500))
    M.eliminate_zeros()           # exact zeros (+-0; NaN != 0 stays), as scipy drops them
    C = A @ B
    C.sort_indices()
    assert C.dtype == x.dtype
    sv.assert_same_special((M.indptr, M.indices, M.data), (C.indptr, C.indices, C.data))
    # the OpenMP variant the GPU tests compare against: same values
    sv.assert_same_special(oracle.spgemm(A, B, keep_zeros=True, sort=True, threads=16), (p, j, x))
    sh = sv.classes(x)
    assert sh["nan"] <= sv.NAN_CAP and sh[sv.FLOORS[regime][0]] >= sv.FLOORS[regime][1], sh


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("regime", sv.REGIMES)
def test_oracle_spmv_spmm_match_scipy_on_special_values(regime, dname):
    A, _, x, X = _small(regime, dname)
    sv.assert_values_special(oracle.spmv(A, x), A @ x, "spmv")
    sv.assert_values_special(oracle.spmm(A, X), A @ X, "spmm")
    sv.assert_values_special(oracle.spmm(A, X[:, :1])[:, 0], oracle.spmv(A, X[:, 0].copy()), "spmm n=1")


# ---- the comparison rule ------------------------------------------------------------------

def _ref():
    """A small CSR result that holds every class: normal, denormal, +0.0, -0.0, +-inf, NaN."""
    p = np.array([0, 3, 3, 8], dtype=np.int64)
    j = np.array([0, 2, 5, 1, 2, 3, 4, 6], dtype=np.int32)
    return p, j


def _vals(dt):
    rd = sv.real_dtype(dt)
    fi = np.finfo(rd)
    v = np.array([1.5, fi.smallest_subnormal * 5, 0.0, -0.0, np.inf, -np.inf, np.nan, -2.25], dtype=rd)
    if np.dtype(dt).kind == "c":
        out = np.empty(8, dtype=dt)
        out.real, out.imag = v, v[::-1]
        return out
    return v.astype(dt)


def _mutations(x):
    """(name, mutated copy) of the reference values: each must be caught."""
    rd = sv.real_dtype(x.dtype)
    ut = np.uint32 if rd == np.float32 else np.uint64
    c = x.view(rd)                      # components; real: index k, complex: (re, im) pairs

    def put(k, v):
        y = c.copy()
        y[k] = v
        return y.view(x.dtype)

    ulp = c.copy()
    ulp.view(ut)[0] += 1
    step = 1 if c.size == 8 else 2      # component index of entry k's real part: k * step
    return [("one ulp", ulp.view(x.dtype)),
            ("denormal flushed to 0", put(1 * step, 0.0)),
            ("+0.0 -> -0.0", put(2 * step, -0.0)),
            ("-0.0 -> +0.0", put(3 * step, 0.0)),
            ("inf -> nan", put(4 * step, np.nan)),
            ("nan -> inf", put(6 * step, np.inf)),
            ("inf sign", put(5 * step, np.inf))]


@pytest.mark.parametrize("dname", DNAMES)
def test_comparator_is_sensitive(dname):
    dt = sv.DTYPES[dname]
    p, j = _ref()
    x = _vals(dt)
    sv.assert_same_special((p, j, x.copy()), (p, j, x))
    for name, y in _mutations(x):
        with pytest.raises(AssertionError):
            sv.assert_same_special((p, j, y), (p, j, x))
        with pytest.raises(AssertionError):
            sv.assert_values_special(y, x)
    # a structural zero removed (entry 2 of row 0 is a +0.0)
    p2 = np.array([0, 2, 2, 7], dtype=np.int64)
    with pytest.raises(AssertionError, match="row pointer"):
        sv.assert_same_special((p2, np.delete(j, 2), np.delete(x, 2)), (p, j, x))
    # a column index changed
    j2 = j.copy()
    j2[1] = 3
    with pytest.raises(AssertionError, match="column indices"):
        sv.assert_same_special((p, j2, x.copy()), (p, j, x))
    # a dtype changed
    if dname == "f64":
        with pytest.raises(AssertionError, match="dtype"):
            sv.assert_values_special(x.astype(np.float32), x)


@pytest.mark.parametrize("dname", DNAMES)
def test_comparator_ignores_only_nan_sign_and_payload(dname):
    dt = sv.DTYPES[dname]
    p, j = _ref()
    x = _vals(dt)
    rd = sv.real_dtype(dt)
    ut = np.uint32 if rd == np.float32 else np.uint64
    y = x.copy()
    c = y.view(rd)
    bits = c.view(ut)
    nan_at = np.flatnonzero(np.isnan(c))
    assert nan_at.size >= 1
    sign = ut(1) << ut(8 * rd.itemsize - 1)
    bits[nan_at] = bits[nan_at] ^ sign | ut(0x1234)    # other sign, other payload, still NaN
    assert np.isnan(c[nan_at]).all() and not np.array_equal(bits, x.view(rd).view(ut))
    sv.assert_same_special((p, j, y), (p, j, x))


def test_comparator_message_names_positions_and_bits():
    x = _vals(np.float64)
    y = x.copy()
    y[3] = 0.0
    with pytest.raises(AssertionError) as e:
        sv.assert_values_special(y, x)
    msg = str(e.value)
    assert "[3]" in msg and "0x0000000000000000" in msg and "0x8000000000000000" in msg


def test_classes_counts_components():
    sh = sv.classes(_vals(np.float64))
    assert sh == {"nan": 1 / 8, "inf": 2 / 8, "denormal": 1 / 8, "zero": 2 / 8}
    sh = sv.classes(_vals(np.complex64))
    assert sh == {"nan": 2 / 16, "inf": 4 / 16, "denormal": 2 / 16, "zero": 4 / 16}


def test_recipes_are_deterministic_and_typed():
    for regime in sv.REGIMES:
        for rd in (np.float32, np.float64):
            a = sv.values(regime, 1000, np.random.default_rng(3), rd)
            b = sv.values(regime, 1000, np.random.default_rng(3), rd)
            assert a.dtype == rd and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    m = sv.values("mixed", 200000, np.random.default_rng(1), np.float64, p_inf=0.01, p_nan=0.02)
    assert abs(np.isposinf(m).mean() - 0.01) < 2e-3 and abs(np.isneginf(m).mean() - 0.01) < 2e-3
    assert abs(np.isnan(m).mean() - 0.02) < 2e-3
    z = m == 0
    assert abs((z & ~np.signbit(m)).mean() - 0.05) < 3e-3 and abs((z & np.signbit(m)).mean() - 0.05) < 3e-3
    t = sv.values("tiny", 1000, np.random.default_rng(2), np.float32, sign=-1)
    assert (t < 0).all() and (np.abs(t) >= np.finfo(np.float32).tiny).all()


# ---- the conditions of every GPU case, from the oracle alone ----------------------------------

@pytest.mark.parametrize("regime", sv.REGIMES)
@pytest.mark.parametrize("case", [c[0] for c in sv.CASES])
def test_gpu_case_conditions(case, regime):
    """NaN cap and the regime's floor on the oracle's C of every spgemm case.  For the cases
    that also run with alpha = -0.75 and alpha = 0: the cap on the scaled output (the floors
    belong to the sums, which alpha = 1 shows: 0 * s is +-0 or NaN whatever s was), and alpha = 0
    keeps the structure."""
    ref = sv.reference(case, regime)
    sv.check_conditions(regime, ref[2])
    if case in sv.ALPHA_CASES:
        for alpha in sv.ALPHAS:
            r = sv.reference(case, regime, alpha=alpha)
            assert np.array_equal(r[0], ref[0]) and np.array_equal(r[1], ref[1])
            sv.check_conditions(regime, r[2], floors=alpha != 0)
            if alpha == 0:
                c = r[2].view(sv.real_dtype(r[2].dtype))
                assert (np.isnan(c) | (c == 0)).all()
                assert np.signbit(c[c == 0]).any()       # 0 * (-x) = -0.0


@pytest.mark.parametrize("case", ["runs32-f32", "dense2048-f64"])
def test_gpu_underflow_case_conditions(case):
    """tiny with A > 0 and B < 0: every product is negative or, underflowing, -0.0; the sums
    start from +0.0, so an entry that sees only -0.0 products is +0.0 (at least 0.1 % of C, the
    `ints` floor) and every other entry is a negative denormal."""
    A, B = sv.inputs(case, "tiny", "underflow")
    assert (A.data > 0).all() and (B.data < 0).all()
    x = sv.reference(case, "tiny", variant="underflow")[2]
    sh = sv.classes(x)
    assert sh["zero"] >= 0.001 and sh["denormal"] >= 0.10 and sh["nan"] == 0, sh
    assert not np.signbit(x[x == 0]).any() and (x <= 0).all()


def test_gpu_explicit_zero_case_conditions():
    """A tenth of A's entries an explicit +0.0 (ints elsewhere): their products are +-0.0, and C
    keeps entries reached by nothing else as +0.0."""
    A, _ = sv.inputs("dense1024-f64", "ints", "azero")
    assert 0.05 < (A.data == 0).mean() < 0.15 and not np.signbit(A.data[A.data == 0]).any()
    x = sv.reference("dense1024-f64", "ints", variant="azero")[2]
    sv.check_conditions("ints", x)
    assert not np.signbit(x[x == 0]).any()


@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("regime", sv.REGIMES)
def test_gpu_spmv_spmm_conditions(regime, dname):
    """The cap and the floor on A x and on A X for every width the GPU file runs; on the alpha /
    beta forms the cap, and tiny's and huge's floors too: their y lives where the sums do
    (special_values._y_params), so the last add still decides denormals and overflow."""
    after = regime in ("tiny", "huge")
    A, x, y0 = sv.spmv_inputs(regime, dname)
    s = oracle.spmv(A, x)
    sv.check_conditions(regime, s)
    sv.check_conditions(regime, sv.axpby(-0.75, s, 0.5, y0), floors=after)
    for n in sorted({n for d, _, n in sv.SPMM_LAYOUTS if d == dname}):
        A, X, C0 = sv.spmm_inputs(regime, dname, n)
        S = oracle.spmm(A, X)
        sv.check_conditions(regime, S)
        sv.check_conditions(regime, sv.axpby(1, S, 0.5, C0), floors=after)
    if regime == "tiny":   # beta * y does not swamp the sums: the scaled y is no larger than they are
        assert np.abs(y0).max() <= 4 * np.abs(s).max()
