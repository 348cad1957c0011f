"""Every compiled kernel instantiation at its structural edges, bit for bit against the CPU oracle.

One case per (kernel, value type) of tests/instantiations.py: inputs with hand-placed edge rows
(A rows on each side of the 64-entry batch and of the NB*64-entry register queue, B rows on the
first / last column of a tile, a whole tile, exactly one window and one entry more, the short-row
kernel's entry, product and flag-list limits), steered to the kernel by filler rows.  Every case
runs through the C ABI with A/B row pointers and C row pointers of 32 and 64 bits in all four
combinations -- nnz(C) never picks C's width here -- under ALG1, ALG2 and ALG3 with its chunks
kept, once with alpha != 1 at (64, 64), and once through cusparse.spgemm with int64 indptr
tensors.  plan_info must report the case's kernel path in every run; the row pointer, the column
indices and the value bits must equal the oracle's, and the four width combinations each other,
byte for byte.  tests/test_instantiations_cpu.py shows the inputs are not vacuous.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import instantiations as inst

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import sys
sys.path.insert(0, {root!r})
from tests import instantiations as inst
inst.child_main({case!r}, {out!r})
"""


def _run(case, tmp_path):
    env = inst.CASE[case].env
    if not any(k in env for k in inst.CHILD_ENV):
        return inst.run_cross(case)
    out = str(tmp_path / "cross.npz")         # a switch read once per process: a fresh one
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, case=case, out=out)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return inst.load_child(out)


@pytest.mark.parametrize("case", inst.CASE_IDS)
def test_instantiation(case, tmp_path):
    c = inst.CASE[case]
    A, _, _ = inst.inputs(case)
    ref = inst.reference(case)
    out, infos = _run(case, tmp_path)
    # the kernel path of every run, and ALG3's chunks
    for key, info in infos.items():
        got = {k: info[k] for k in c.expect}
        assert got == c.expect, (case, key, info)
        rows = info["chunk_rows"]
        if key[0] == "3c":
            assert len(rows) - 1 >= 3 and rows[0] == 0 and rows[-1] == A.shape[0], (case, key, rows)
            assert all(a < b for a, b in zip(rows, rows[1:])), rows
        else:
            assert rows == [0, A.shape[0]], (case, key, rows)
    # every (ALG, IP, CP) against the oracle
    assert set(infos) == {(alg, ip, cp) for alg in inst.ALGS for ip, cp in inst.WIDTHS}
    for key in infos:
        p, j, x = out[key]
        assert p.dtype == (np.int32 if key[2] == 32 else np.int64), (key, p.dtype)
        inst.assert_same((p, j, x), ref, f"{case} alg={key[0]} IP={key[1]} CP={key[2]}")
    # the width combinations against each other, byte for byte; an int64 row pointer equals the
    # int32 one element for element
    for alg in inst.ALGS:
        p0, j0, x0 = out[(alg, 32, 32)]
        for ip, cp in inst.WIDTHS[1:]:
            p, j, x = out[(alg, ip, cp)]
            assert np.array_equal(p.astype(np.int64), p0.astype(np.int64)) and len(p) == len(p0), (case, alg, ip, cp)
            assert j.tobytes() == j0.tobytes() and x.tobytes() == x0.tobytes(), (case, alg, ip, cp)
        assert out[(alg, 32, 64)][0].tobytes() == out[(alg, 64, 64)][0].tobytes()
        assert out[(alg, 64, 32)][0].tobytes() == p0.tobytes()
    # alpha != 1 (complex for complex types) at (64, 64), and the Python entry point with int64 indptr
    inst.assert_same(out["alpha"], inst.reference(case, inst.alpha_of(c.dname)), f"{case} alpha")
    inst.assert_same(out["python"], ref, f"{case} cusparse.spgemm, int64 indptr")
