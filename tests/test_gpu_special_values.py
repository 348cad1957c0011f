"""IEEE special values on every kernel path, against the CPU oracle (and through it scipy:
tests/test_special_values_cpu.py pins the oracle to scipy on the same recipes).

Every other GPU parity test draws its values from uniform[0, 1) or standard_normal.  Here the
inputs are denormals, +-0, +-inf, NaN, products that underflow or overflow and sums that cancel
exactly (tests/special_values.py: the recipes, the case table with one structure per kernel path,
the conditions that keep a case from passing vacuously).  The comparison is bit for bit except
for a NaN's sign and payload (special_values.assert_same_special).  What these values reach:
the ordered LDS adds of k_tile_dn / k_tile_sp (ds_add_f64 / ds_add_f32 must round like v_add with
denormals kept), the -0.0 start of the dense-tile accumulators and its re-walk, padding products
into dummy slots, the alpha scaling, the complex product without infinity recovery, and the
16-byte paths of k_spmm_row.  Each spgemm case asserts its kernel path through plan_info first.
"""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from tests import special_values as sv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# ALG1, ALG2 and ALG3 with its chunks kept on small inputs (as tests/test_gpu_parity.py's "3c")
ALGS = [(1, 0.2), (2, 0.2), ("3c", 0.1)]
CASE_IDS = [c[0] for c in sv.CASES]


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _upload(A, B):
    from spmm_amd.sparse import csr_matrix
    return csr_matrix(A.copy(), device=DEV), csr_matrix(B.copy(), device=DEV)   # (the cached inputs are read-only)


def _spgemm(dA, dB, alg, alpha=1.0, cf=0.2):
    from spmm_amd import cusparse
    env = {"SPG_ALG3_CHUNK_ALWAYS": "1"} if alg == "3c" else {}
    with _env(env):
        C = cusparse.spgemm(dA, dB, alpha=alpha, alg=3 if alg == "3c" else alg, chunk_fraction=cf)
    torch.cuda.synchronize()
    return C.indptr.cpu().numpy().astype(np.int64), C.indices.cpu().numpy(), C.data.cpu().numpy()


def _assert_path(case, dA, dB):
    """plan_info must report the case's kernel path (ALG2's plan; ALG1 and ALG3 pick the same
    kernels).  lds_ordered tells the ordered-LDS kernels from k_tile's owner rounds: for fp64 and
    complex128 tiles k_tile_dn / k_tile_sp, for fp32 dense tiles the entry runs of
    k_tile_dn<float, .., 1024> -- 1 only if the device's own ds_add_f32 check passed."""
    from spmm_amd import cusparse
    _, struct, dname, _, expect = sv.CASE[case]
    info = cusparse.plan_info(dA, dB, alg=2)
    got = {k: info[k] for k in expect}
    assert got == expect, (case, info)
    if struct == "short":
        assert cusparse.plan_info(dA, dB, alg=1)["path"] == "short", case     # the fused ALG1 pass
    return info


def _check_case(case, regime, alpha=1.0, variant=""):
    A, B = sv.inputs(case, regime, variant)
    ref = sv.reference(case, regime, alpha=alpha, variant=variant)
    dA, dB = _upload(A, B)
    with _env(sv.CASE[case][3]):
        _assert_path(case, dA, dB)
        for alg, cf in ALGS:
            try:
                sv.assert_same_special(_spgemm(dA, dB, alg, alpha=alpha, cf=cf), ref)
            except AssertionError as e:
                raise AssertionError(f"{case} {regime} alg={alg} alpha={alpha} {variant}: {e}") from None


@pytest.mark.parametrize("regime", sv.REGIMES)
@pytest.mark.parametrize("case", CASE_IDS)
def test_spgemm_special_values(case, regime):
    _check_case(case, regime)


@pytest.mark.parametrize("alpha", sv.ALPHAS)
@pytest.mark.parametrize("regime", sv.REGIMES)
@pytest.mark.parametrize("case", sv.ALPHA_CASES)
def test_spgemm_special_values_alpha(case, regime, alpha):
    """alpha = -0.75 scales inf, denormals and -0.0; alpha = 0 turns inf into NaN, negative sums
    into -0.0 and keeps the structure (no shortcut on alpha's value)."""
    _check_case(case, regime, alpha=alpha)


@pytest.mark.parametrize("case", ["runs32-f32", "dense2048-f64"])
def test_spgemm_underflow_to_negative_zero(case):
    """tiny with A > 0 and B < 0: every underflowing product is -0.0, the value the dense tiles'
    accumulator slots start from.  A column reached only by such products reads as untouched and
    must still come out as a structural +0.0 (the re-walk), through natural arithmetic."""
    _check_case(case, "tiny", variant="underflow")


def test_spgemm_explicit_zero_in_a():
    """A tenth of A's entries an explicit +0.0: 0 * (-x) = -0.0 products on the dense fp64 tiles."""
    _check_case("dense1024-f64", "ints", variant="azero")


# ---- the owner-round fallback (SPG_LDS_ORDERED=0 is read when a handle is created) ------------

# (runs32-f32: with the fp32 flag cleared too, the entry runs' shape takes the owner rounds)
FALLBACK = [(case, regime) for case in ("dense2048-f64", "sparse8192-f64", "runs32-f32") for regime in ("tiny", "mixed")]

_FRESH = """
import json, os, sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from tests import special_values as sv
from spmm_amd import cusparse
from spmm_amd.sparse import csr_matrix
arrs, infos = {{}}, {{}}
for case, regime in {runs!r}:
    A, B = sv.inputs(case, regime)
    dA, dB = csr_matrix(A.copy(), device="cuda:0"), csr_matrix(B.copy(), device="cuda:0")
    infos[case] = cusparse.plan_info(dA, dB, alg=2)
    for alg in (2, 3):
        os.environ["SPG_ALG3_CHUNK_ALWAYS"] = "1" if alg == 3 else "0"
        C = cusparse.spgemm(dA, dB, alg=alg, chunk_fraction=0.1)
        torch.cuda.synchronize()
        key = case + "|" + regime + "|" + str(alg)
        arrs[key + "|p"] = C.indptr.cpu().numpy().astype(np.int64)
        arrs[key + "|j"] = C.indices.cpu().numpy()
        arrs[key + "|x"] = C.data.cpu().numpy()
np.savez({out!r}, **arrs)
json.dump(infos, open({info!r}, "w"))
"""


def test_owner_round_fallback_special_values(tmp_path):
    """The lean fp64 shapes and the fp32 entry runs' shape on k_tile's owner rounds (a fresh
    process with SPG_LDS_ORDERED=0, which clears both LDS flags), tiny and mixed, ALG2 and
    chunked ALG3."""
    out, info = str(tmp_path / "out.npz"), str(tmp_path / "info.json")
    code = _FRESH.format(root=ROOT, runs=FALLBACK, out=out, info=info)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPG_LDS_ORDERED="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for case, i in json.load(open(info)).items():
        assert i["path"] == "tile" and not i["lds_ordered"] and i["tile_width"] <= 4096, (case, i)
    got = np.load(out)
    for case, regime in FALLBACK:
        ref = sv.reference(case, regime)
        for alg in (2, 3):
            key = f"{case}|{regime}|{alg}"
            try:
                sv.assert_same_special((got[key + "|p"], got[key + "|j"], got[key + "|x"]), ref)
            except AssertionError as e:
                raise AssertionError(f"{key}: {e}") from None


# ---- spg_numeric_tiles: the values travel through spg_tile_values ----------------------------

@pytest.mark.parametrize("regime", ["mixed", "tiny"])
def test_numeric_tiles_special_values(regime):
    from spmm_amd import cusparse, distributed
    case = "dense2048-f64"
    A, B = sv.inputs(case, regime)
    ref = sv.reference(case, regime)
    dA, dB = _upload(A, B)
    seen = {}

    def feed(geom):
        assert geom is not None and geom["tile_width"] == 2048, geom
        groups = distributed.tile_groups(geom["offsets"], 2)
        seen["groups"] = groups
        return geom["tile_values"](), groups

    C = cusparse._spgemm(dA, dB, alg=2, by_tiles=feed)
    torch.cuda.synchronize()
    assert len(seen["groups"]) == 2
    sv.assert_same_special((C.indptr.cpu().numpy(), C.indices.cpu().numpy(), C.data.cpu().numpy()), ref)


# ---- SpMV and SpMM ---------------------------------------------------------------------------

@pytest.mark.parametrize("alpha,beta", [(1, 0), (-0.75, 0.5)])
@pytest.mark.parametrize("dname", list(sv.DTYPES))
@pytest.mark.parametrize("regime", sv.REGIMES)
def test_spmv_special_values(regime, dname, alpha, beta):
    """y = alpha A x + beta y with x and y from the regime: the oracle's sums, then the engine's
    epilogue spelled out on the host (special_values.axpby)."""
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    A, x, y0 = sv.spmv_inputs(regime, dname)
    want = sv.axpby(alpha, oracle.spmv(A, x), beta, y0)
    y = torch.from_numpy(y0.copy()).to(DEV)
    out = cusparse.spmv(csr_matrix(A.copy(), device=DEV), torch.from_numpy(x.copy()).to(DEV), y=y, alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    sv.assert_values_special(out.cpu().numpy(), want, f"spmv {regime} {dname} alpha={alpha} beta={beta}")


# special_values.SPMM_LAYOUTS says which kernel and access width each (dtype, order, n) reaches
@pytest.mark.parametrize("beta", [0, 0.5])
@pytest.mark.parametrize("dname,order,n", sv.SPMM_LAYOUTS)
@pytest.mark.parametrize("regime", sv.REGIMES)
def test_spmm_special_values(regime, dname, order, n, beta):
    from spmm_amd import cusparse
    from spmm_amd.sparse import csr_matrix
    A, X, C0 = sv.spmm_inputs(regime, dname, n)
    want = sv.axpby(1, oracle.spmm(A, X), beta, C0)
    Xd, c = torch.from_numpy(X.copy()).to(DEV), torch.from_numpy(C0.copy()).to(DEV)
    if order == "col":
        Xd, c = Xd.t().contiguous().t(), c.t().contiguous().t()
    if order == "rowld":   # column slices of parents one column wider: ld = n + 1
        Xd = torch.cat([Xd, torch.zeros_like(Xd[:, :1])], dim=1)[:, :n]
        c = torch.cat([c, torch.zeros_like(c[:, :1])], dim=1)[:, :n]
        assert Xd.stride() == (n + 1, 1) and c.stride() == (n + 1, 1)
    out = cusparse.spmm(csr_matrix(A.copy(), device=DEV), Xd, c=c, beta=beta)
    assert out is c
    torch.cuda.synchronize()
    sv.assert_values_special(out.cpu().numpy(), want, f"spmm {regime} {dname} {order} n={n} beta={beta}")
