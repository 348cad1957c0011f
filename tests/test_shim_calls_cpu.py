"""What the Python shim (spmm_amd/cusparse.py) asks of the engine, call by call, on the CPU.

The shim's entry points are driven on small CPU tensors against a fake library: a plain object
whose ``spg_*`` attributes record every call and answer from a script (status, nnz(C), workspace
size, whether ALG1 left the result in the workspace).  Per call the trace keeps the function name;
for every struct argument its scalar fields (extents, nnz, ld, order, both type codes, start / step
/ count); for every pointer argument and pointer field only whether it is null; integers and floats
by value.  Handle look-ups and stream settings are in the trace too, and each case ends with the
dtypes and shapes of what the entry point returned.

  (a) recording   every trace equals tests/golden/shim_calls.json, recorded from the module as it
                  stood before its copies of the call frame were folded into one.  No tolerance: the
                  order and the arguments of every library call are part of the module's behaviour;
  (b) exceptions  for each public function, the inputs that trip each of its checks one at a time
                  (unavailable, wrong type, non-canonical, shape mismatch, CPU tensors): the type and
                  the exact message, against the same recording.

The seams the fake comes in by: ``cusparse._lib.get_handle``, ``cusparse._current_stream_ptr``,
``torch.cuda.current_device``, ``cusparse._available`` and ``_fastpath.get``.  No device, no library.
"""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from spmm_amd import _fastpath, _lib, cusparse
from spmm_amd.sparse import coo_matrix, csc_matrix, csr_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shim_calls.json")
OVERFLOW = _lib.STATUS_OVERFLOW
PLAN = 0x7000          # the fake plan handle
F64, C64, I32, I64 = torch.float64, torch.complex64, torch.int32, torch.int64


# ------------------------------------------------------------------ the fake library

def _struct(s):
    out = {"struct": type(s).__name__}
    for name, ct in s._fields_:
        v = getattr(s, name)
        out[name] = ("ptr" if v else "null") if ct is ctypes.c_void_p else v
    return out


def _arg(a):
    """One argument of a library call as the trace keeps it."""
    if a is None:
        return "null"
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    if isinstance(a, ctypes.Array):
        return {"array": len(a)}
    obj = a._obj                                   # (ctypes.byref)
    if isinstance(obj, _lib.SpgPlanInfo):
        return {"out": "SpgPlanInfo"}
    if isinstance(obj, ctypes.Structure):
        return _struct(obj)
    if isinstance(obj, ctypes.Array):              # a complex scalar: (real, imag)
        return {"ref": type(obj)._type_.__name__, "value": list(obj)}
    if isinstance(obj, ctypes.c_void_p):
        return {"ref": "void*"}
    return {"ref": type(obj).__name__, "value": obj.value}


class _FakeLib:
    """Records every spg_* call into `trace` and answers from `script`: {name: [answer, ...]}, one
    answer per call of that name in order, ``{}`` (success, nothing written) once they run out."""

    def __init__(self, script, trace):
        self._script = {k: list(v) for k, v in script.items()}
        self._trace = trace

    def __getattr__(self, name):
        if not name.startswith("spg_"):
            raise AttributeError(name)

        def call(*args):
            self._trace.append([name] + [_arg(a) for a in args])
            left = self._script.get(name)
            r = left.pop(0) if left else {}
            refs = [a._obj for a in args if hasattr(a, "_obj")]
            for o in refs:
                if isinstance(o, ctypes.c_int64) and "nnz" in r:
                    o.value = r["nnz"]
                elif isinstance(o, ctypes.c_size_t) and "size" in r:
                    o.value = r["size"]
                elif isinstance(o, _lib.SpgPlanInfo):
                    for k, v in r.get("info", {}).items():
                        setattr(o, k, v)
            voids = [o for o in refs if isinstance(o, ctypes.c_void_p)]
            if name == "spg_plan" and voids:
                voids[0].value = PLAN
            if name == "spg_spgemm_ws" and r.get("status", 0) == 0:
                pj, px, plan = voids
                if r.get("in_ws"):             # ALG1: C's indices and values inside the workspace
                    pj.value, px.value = args[6].value, args[6].value + 256
                else:
                    plan.value = PLAN
            if name == "spg_tile_value_offsets":
                for i in range(len(args[2])):
                    args[2][i] = 2 * i
            return r.get("status", 0)
        return call


class _FakeHandle:
    def __init__(self, lib, trace):
        self.lib, self.ptr, self._trace = lib, ctypes.c_void_p(0x5150), trace

    def set_stream(self, stream_ptr):
        self._trace.append(["set_stream", stream_ptr])


@contextlib.contextmanager
def _seams(script, trace, available=True):
    handle = _FakeHandle(_FakeLib(script, trace), trace)

    def get_handle(dev):
        trace.append(["get_handle", dev])
        return handle
    saved = [(cusparse._lib, "get_handle"), (cusparse, "_current_stream_ptr"), (torch.cuda, "current_device"),
             (cusparse, "_available"), (_fastpath, "get")]
    saved = [(o, n, getattr(o, n)) for o, n in saved]
    cusparse._lib.get_handle = get_handle
    cusparse._current_stream_ptr = lambda dev: 77
    torch.cuda.current_device = lambda: 0
    cusparse._available = available
    _fastpath.get = lambda: None
    try:
        yield
    finally:
        for o, n, v in saved:
            setattr(o, n, v)


def _describe(x):
    if isinstance(x, torch.Tensor):
        return [str(x.dtype), list(x.shape), list(x.stride())]
    if isinstance(x, (csr_matrix, csc_matrix)):
        return {"format": x.format, "shape": list(x.shape), "canonical": x._canonical, "data": _describe(x.data),
                "indices": _describe(x.indices), "indptr": _describe(x.indptr)}
    if isinstance(x, (tuple, list)):
        return [_describe(v) for v in x]
    assert x is None or isinstance(x, int), x
    return x


def _drive(script, thunk, available=True):
    """{calls, result or raises} of one entry point under the fake."""
    trace = []
    s = cusparse.last_stats
    s.alg, s.workspace_bytes, s.peak_bytes, s.num_products, s.nnz = 0, 0, 0, -1, 0
    with _seams(script, trace, available):
        try:
            out = {"result": _describe(thunk(trace))}
        except Exception as e:     # noqa: BLE001  (the type and the message are what is recorded)
            out = {"raises": [type(e).__name__, str(e)]}
    out["calls"] = trace
    out["last_stats"] = [s.alg, s.workspace_bytes, s.peak_bytes, s.num_products, s.nnz]
    return json.loads(json.dumps(out))


# ------------------------------------------------------------------ the operands

def _A(nnz=5, ipd=I32, dt=F64, canonical=True):
    """3 x 4 with 5 stored entries, or its empty counterpart."""
    if nnz == 0:
        return csr_matrix._from_parts(torch.empty(0, dtype=dt), torch.empty(0, dtype=I32),
                                      torch.zeros(4, dtype=ipd), (3, 4), canonical=canonical)
    return csr_matrix._from_parts(torch.arange(1.0, 6.0).to(dt), torch.tensor([0, 2, 1, 0, 3], dtype=I32),
                                  torch.tensor([0, 2, 3, 5], dtype=ipd), (3, 4), canonical=canonical)


def _B(ipd=I32, dt=F64):
    """4 x 3 with 4 stored entries."""
    return csr_matrix._from_parts(torch.arange(1.0, 5.0).to(dt), torch.tensor([0, 1, 2, 0], dtype=I32),
                                  torch.tensor([0, 1, 2, 3, 4], dtype=ipd), (4, 3), canonical=True)


def _csc(a):
    return csc_matrix((a.data, a.indices, a.indptr), shape=(a.shape[1], a.shape[0]), canonical=True)


def _coo():
    return coo_matrix((torch.arange(1.0, 6.0), (torch.tensor([0, 0, 1, 2, 2]), torch.tensor([0, 2, 1, 0, 3]))),
                      shape=(3, 4))


def _wide_pair():
    """Operands whose expected product count reaches 2**31 (the int64-first rule): 65536 x 1 by 1 x 32768."""
    a = csr_matrix._from_parts(torch.ones(65536), torch.zeros(65536, dtype=I32), torch.arange(65537, dtype=I32),
                               (65536, 1), canonical=True)
    b = csr_matrix._from_parts(torch.ones(32768), torch.arange(32768, dtype=I32), torch.tensor([0, 32768], dtype=I32),
                               (1, 32768), canonical=True)
    return a, b


# ------------------------------------------------------------------ the cases

def _args_of(m):
    return m.data, m.indices, m.indptr


def _two_phase(name, ovf):
    """The script of a size query, a structure call (after an OVERFLOW when `ovf`) and 2 entries."""
    return {name: [{"size": 512}] + ([{"status": OVERFLOW}] if ovf else []) + [{"nnz": 2}]}


def _tiles(groups, info, returns="groups"):
    """A `by_tiles` callback that logs the geometry it is given into the trace."""
    def by_tiles_of(trace):
        def by_tiles(geom):
            seen = None if geom is None else {k: (v.tolist() if k == "offsets" else str(v) if k == "dtype" else v)
                                              for k, v in geom.items() if k != "tile_values"}
            trace.append(["by_tiles", seen])
            if geom is None or returns is None:
                return None
            return geom["tile_values"](), groups
        return by_tiles
    return by_tiles_of


TILE_INFO = {"path": 2, "n_chunks": 1, "tile_width": 64, "tiles_per_row": 4, "record_group": 2}
PLAN_SCRIPT = {"spg_plan": [{"size": 1024}], "spg_spgemm_ws": [{"nnz": 3, "size": 2048}]}
TILE_SCRIPT = {"spg_plan": [{"size": 1024}], "spg_symbolic": [{"nnz": 3}], "spg_peak_bytes": [{"size": 4096}]}


def _cases():
    """{name: (script, thunk(trace))} in a fixed order."""
    c = {}
    cs = cusparse
    A, E = _A(), _A(0)
    c["csr2csc"] = ({"spg_csr2csc": [{"size": 512}]}, lambda tr: cs._csr2csc_arrays(*_args_of(A), 3, 4))
    c["csr2csc_int64_indptr"] = ({"spg_csr2csc": [{"size": 512}]},
                                 lambda tr: cs._csr2csc_arrays(*_args_of(_A(ipd=I64)), 3, 4))
    c["csr2csc_empty"] = ({}, lambda tr: cs._csr2csc_arrays(*_args_of(E), 3, 4))

    canon = _two_phase("spg_canonicalize_nnz", False)
    rows = torch.tensor([0, 0, 1, 2, 2])
    c["canonicalize_csr"] = (canon, lambda tr: cs._canonicalize_arrays(*_args_of(A), None, (3, 4), 3))
    c["canonicalize_coo"] = (canon, lambda tr: cs._canonicalize_arrays(A.data, A.indices.to(I64), None, rows, (3, 4), 0))
    c["canonicalize_indptr_dtype"] = (canon, lambda tr: cs._canonicalize_arrays(*_args_of(A), None, (3, 4), 4, I64))
    c["canonicalize_empty"] = ({}, lambda tr: cs._canonicalize_arrays(*_args_of(E), None, (3, 4), 3))
    c["canonicalize_empty_indptr_dtype"] = ({}, lambda tr: cs._canonicalize_arrays(*_args_of(E), None, (3, 4), 3, I64))
    c["canonicalize_overflow_raises"] = (_two_phase("spg_canonicalize_nnz", True),
                                         lambda tr: cs._canonicalize_arrays(*_args_of(A), None, (3, 4), 3))

    for ovf in (False, True):
        tag = "_overflow" if ovf else ""
        ex = _two_phase("spg_csr_extract_nnz", ovf)
        c["extract_range_range" + tag] = (ex, lambda tr: cs._extract_arrays(*_args_of(A), (3, 4), (0, 2, 2), (1, 1, 3)))
        c["extract_list_none" + tag] = (ex, lambda tr: cs._extract_arrays(*_args_of(A), (3, 4),
                                                                         torch.tensor([2, 0, 2]), None))
        dn = _two_phase("spg_dense2csr_nnz", ovf)
        c["dense2csr_row_major" + tag] = (dn, lambda tr: cs._dense2csr_arrays(torch.arange(12.0).reshape(3, 4)))
        c["dense2csr_col_major" + tag] = (dn, lambda tr: cs._dense2csr_arrays(torch.arange(12.0).reshape(4, 3).t()))
        c["dense2csr_neither" + tag] = (dn, lambda tr: cs._dense2csr_arrays(torch.arange(24.0).reshape(3, 8)[:, ::2]))
    c["extract_empty_source"] = ({"spg_csr_extract_nnz": [{"size": 512}, {"nnz": 0}]},
                                 lambda tr: cs._extract_arrays(*_args_of(E), (3, 4), None, torch.empty(0, dtype=I32)))
    c["extract_int64_indptr"] = (_two_phase("spg_csr_extract_nnz", False),
                                 lambda tr: cs._extract_arrays(*_args_of(_A(ipd=I64)), (3, 4), (2, -1, 3), None))
    c["dense2csr_complex"] = (_two_phase("spg_dense2csr_nnz", False),
                              lambda tr: cs._dense2csr_arrays(torch.ones(2, 3, dtype=C64)))
    c["dense2csr_zero_rows"] = ({"spg_dense2csr_nnz": [{"size": 512}, {"nnz": 0}]},
                                lambda tr: cs._dense2csr_arrays(torch.empty(0, 4)))

    c["todense_row_major"] = ({}, lambda tr: cs._todense_into(*_args_of(A), 3, 4, torch.empty(3, 4)))
    c["todense_col_major"] = ({}, lambda tr: cs._todense_into(*_args_of(A), 3, 4, torch.empty(4, 3).t()))
    c["todense_padded"] = ({}, lambda tr: cs._todense_into(*_args_of(A), 3, 4, torch.empty(3, 9)[:, :4]))
    c["todense_int64_indptr"] = ({}, lambda tr: cs._todense_into(*_args_of(_A(ipd=I64)), 3, 4, torch.empty(3, 4)))
    c["todense_empty"] = ({}, lambda tr: cs._todense_into(*_args_of(E), 3, 4, torch.empty(3, 4)))
    c["todense_zero_extent"] = ({}, lambda tr: cs._todense_into(E.data, E.indices, E.indptr[:1], 0, 4, torch.empty(0, 4)))

    B = _B()
    c["spgemm_alg2"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(A, B, alpha=2.0, alg=2))
    c["spgemm_default_alg"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(A, B))
    c["spgemm_alg3"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(A, B, alg=3, chunk_fraction=0.5))
    c["spgemm_public"] = (PLAN_SCRIPT, lambda tr: cs.spgemm(A, B, alpha=-0.5, alg=2))
    c["spgemm_alg1_in_workspace"] = ({"spg_plan": [{"size": 1024}],
                                      "spg_spgemm_ws": [{"nnz": 3, "size": 2048, "in_ws": True}]},
                                     lambda tr: cs._spgemm(A, B, alg=1))
    c["spgemm_overflow"] = ({"spg_plan": [{"size": 1024}], "spg_spgemm_ws": [{"status": OVERFLOW}, {"nnz": 3, "size": 2048}]},
                            lambda tr: cs._spgemm(A, B, alg=2))
    c["spgemm_mixed_indptr"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(_A(ipd=I64), B, alg=2))
    c["spgemm_mixed_values"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(_A(dt=torch.float32), B, alg=2))
    c["spgemm_complex"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(_A(dt=C64), _B(dt=C64), alpha=1 + 2j, alg=2))
    c["spgemm_empty"] = ({"spg_plan": [{"size": 0}], "spg_spgemm_ws": [{"nnz": 0}]}, lambda tr: cs._spgemm(E, B, alg=2))
    c["spgemm_before_numeric"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(A, B, alg=2,
                                                                     before_numeric=lambda: tr.append(["before_numeric"])))
    c["spgemm_before_numeric_alg1"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(
        A, B, alg=1, before_numeric=lambda: tr.append(["before_numeric"])))
    c["spgemm_numeric_fails"] = (dict(PLAN_SCRIPT, spg_numeric=[{"status": 6}]), lambda tr: cs._spgemm(A, B, alg=2))
    c["spgemm_wide"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(*_wide_pair(), alg=2))

    no_tiles = dict(TILE_SCRIPT, spg_plan_info=[{"info": {"path": 0, "n_chunks": 1}}])
    tiles = dict(TILE_SCRIPT, spg_plan_info=[{"info": TILE_INFO}])
    c["tiles_geom_none"] = (no_tiles, lambda tr: cs._spgemm(A, B, alg=2, by_tiles=_tiles(None, None)(tr)))
    c["tiles_two_groups"] = (tiles, lambda tr: cs._spgemm(A, B, alpha=2.0, alg=2,
                                                          by_tiles=_tiles([(0, 1), (1, 2)], TILE_INFO)(tr)))
    c["tiles_values_last"] = (tiles, lambda tr: cs._spgemm(A, B, alg=2, by_tiles=_tiles([(0, 2)], TILE_INFO)(tr),
                                                           values_first=False))
    c["tiles_overflow"] = (dict(tiles, spg_symbolic=[{"status": OVERFLOW}, {"nnz": 3}]),
                           lambda tr: cs._spgemm(A, B, alg=2, by_tiles=_tiles([(0, 2)], TILE_INFO)(tr)))
    c["tiles_row_major_fallback"] = (tiles, lambda tr: cs._spgemm(A, B, alg=2, by_tiles=_tiles(None, TILE_INFO, None)(tr)))
    c["tiles_gap_raises"] = (tiles, lambda tr: cs._spgemm(A, B, alg=2, by_tiles=_tiles([(1, 2)], TILE_INFO)(tr)))
    c["tiles_alg1"] = (PLAN_SCRIPT, lambda tr: cs._spgemm(A, B, alg=1, by_tiles=_tiles(None, None)(tr)))
    c["tiles_wide"] = (no_tiles, lambda tr: cs._spgemm(*_wide_pair(), alg=2, by_tiles=_tiles(None, None)(tr)))
    c["tiles_direct"] = (tiles, lambda tr: cs._spgemm_by_tiles(cs._handle_for(A), A, B, 1, _lib.SPG_ALG2, 0.2,
                                                               _tiles([(0, 2)], TILE_INFO)(tr), False))

    c["num_products"] = ({"spg_plan": [{"size": 1024}], "spg_num_products": [{"nnz": 42}]},
                         lambda tr: cs.num_products(A, B))
    c["cols16_split"] = ({}, lambda tr: cs._cols16_split(A))
    c["cols16_split_empty"] = ({}, lambda tr: cs._cols16_split(E))
    c["cols16_join"] = ({}, lambda tr: cs._cols16_join(A.indptr, torch.empty((3, 0), dtype=I32),
                                                       torch.zeros(5, dtype=torch.int16), (3, 4)))

    x4, x3, b4, b3 = torch.ones(4), torch.ones(3), torch.ones(4, 2), torch.ones(3, 2)
    c["spmv_csr"] = ({}, lambda tr: cs.spmv(A, x4))
    c["spmv_csc"] = ({}, lambda tr: cs.spmv(_csc(A), x3))
    c["spmv_coo"] = ({}, lambda tr: cs.spmv(_coo(), x4))
    c["spmv_transa"] = ({}, lambda tr: cs.spmv(A, x3, transa=True))
    c["spmv_given_y"] = ({}, lambda tr: cs.spmv(A, x4, y=torch.zeros(3, dtype=F64), alpha=2, beta=0.5))
    c["spmv_complex"] = ({}, lambda tr: cs.spmv(_A(dt=C64), x4, alpha=1 + 2j, beta=-1j))
    c["spmv_numpy_x"] = ({}, lambda tr: cs.spmv(A, np.ones(4, dtype=np.float32)))
    c["spmv_empty"] = ({}, lambda tr: cs.spmv(E, x4))
    c["spmm_csr"] = ({}, lambda tr: cs.spmm(A, b4))
    c["spmm_csc"] = ({}, lambda tr: cs.spmm(_csc(A), b3))
    c["spmm_coo"] = ({}, lambda tr: cs.spmm(_coo(), b4))
    c["spmm_transa"] = ({}, lambda tr: cs.spmm(A, b3, transa=True))
    c["spmm_transb"] = ({}, lambda tr: cs.spmm(A, torch.ones(2, 4), transb=True))
    c["spmm_given_c"] = ({}, lambda tr: cs.spmm(A, b4, c=torch.zeros(2, 3, dtype=F64).t(), alpha=2, beta=0.5))
    c["spmm_complex"] = ({}, lambda tr: cs.spmm(_A(dt=C64), b4, alpha=1 + 2j))
    c["spmm_empty"] = ({}, lambda tr: cs.spmm(E, b4))

    # csrgeam2's frame under its device check.  The module the recording was made from had no
    # tensor-level entry for the addition, so these were recorded when _csrgeam_arrays was split
    # out, after their calls compared equal to those of the earlier csrgeam2 run on the same CPU
    # tensors with its device check lifted.
    geam = _two_phase("spg_csrgeam_nnz", False)
    A2 = _A(ipd=I64)

    def geam_of(a, b, alpha=1, beta=1):
        return lambda tr: cs._csrgeam_arrays(*_args_of(a), *_args_of(b), (3, 4), alpha, beta)
    c["csrgeam_arrays"] = (geam, geam_of(A, A, 2.0, -0.5))
    c["csrgeam_arrays_mixed_indptr"] = (geam, geam_of(A, A2))
    c["csrgeam_arrays_empty_b"] = (geam, geam_of(A, E))
    c["csrgeam_arrays_complex"] = (geam, geam_of(_A(dt=C64), _A(dt=C64), 1 + 2j, -1j))
    c["csrgeam_arrays_overflow_raises"] = (_two_phase("spg_csrgeam_nnz", True), geam_of(A, A))
    c["csrgeam_arrays_bad_scalar"] = (geam, geam_of(A, A, "two", 1))
    return c


def _errors():
    """{name: (available, thunk)}: per public function, the inputs that trip each check in turn."""
    cs = cusparse
    A, B, T = _A(), _B(), torch.ones(3, 4)
    loose = _A(canonical=False)
    e = {}

    def each(name, fn, **inputs):
        e[f"{name}:unavailable"] = (False, lambda: fn(*next(iter(inputs.values()))))
        for label, args in inputs.items():
            e[f"{name}:{label}"] = (True, lambda args=args: fn(*args))

    each("spgemm", cs.spgemm, type_a=(_csc(A), B), type_b=(A, _csc(B)), canonical_a=(loose, B),
         canonical_b=(A, _A(canonical=False)), shape=(A, A), chunk_fraction=(A, B, 1, 3, 0.0))
    each("spmv", cs.spmv, type=(T, torch.ones(4)), shape=(A, torch.ones(3)), canonical=(loose, torch.ones(4)),
         y_size=(A, torch.ones(4), torch.zeros(4, dtype=F64)), y_type=(A, torch.ones(4), torch.zeros(3)))
    each("spmm", cs.spmm, type=(T, torch.ones(4, 2)), shape=(A, torch.ones(3, 2)), canonical=(loose, torch.ones(4, 2)),
         c_shape=(A, torch.ones(4, 2), torch.zeros(2, 3, dtype=F64)), c_type=(A, torch.ones(4, 2), torch.zeros(3, 2)),
         c_strides=(A, torch.ones(4, 2), torch.zeros(6, 4, dtype=F64)[::2, ::2]))
    each("csr2csc", cs.csr2csc, type=(_csc(A),), cpu=(A,))
    each("csc2csr", cs.csc2csr, type=(A,), cpu=(_csc(A),))
    each("csrgeam2", cs.csrgeam2, type_a=(_csc(A), A), type_b=(A, _csc(A)), canonical_a=(loose, A),
         canonical_b=(A, loose), shape=(A, B), cpu=(A, A))
    each("canonicalize", cs.canonicalize, type=(_csc(A),), cpu=(A,), cpu_coo=(_coo(),))
    each("csrsort", cs.csrsort, type=(_coo(),), cpu=(A,))
    each("extract", cs.extract, type=(_coo(),), cpu=(A, [0], None), cpu_csc=(_csc(A),))
    each("csr2dense", cs.csr2dense, type=(_csc(A),), cpu=(A,))
    each("csc2dense", cs.csc2dense, type=(A,), cpu=(_csc(A),))
    each("sparseToDense", cs.sparseToDense, type=(T,), cpu_csr=(A,), cpu_csc=(_csc(A),), cpu_coo=(_coo(),))
    each("dense2csr", cs.dense2csr, type=(A,), ndim=(torch.ones(4),), dtype=(torch.ones(3, 4, dtype=I32),), cpu=(T,))
    each("dense2csc", cs.dense2csc, type=(A,), ndim=(torch.ones(4),), dtype=(torch.ones(3, 4, dtype=I32),), cpu=(T,))
    each("denseToSparse", cs.denseToSparse, cpu_csr=(T,), cpu_csc=(T, "csc"), cpu_coo=(T, "coo"), format=(T, "bsr"),
         type_coo=(A, "coo"))
    e["validate_csr:cpu"] = (True, lambda: cs.validate_csr(A))
    e["check_availability:name"] = (True, lambda: cs.check_availability("gemm"))
    e["spgemm:by_tiles_alg1"] = (True, lambda: cs._spgemm(A, B, alg=1, by_tiles=lambda geom: ()))
    return e


def _record():
    cases = {name: _drive(script, thunk) for name, (script, thunk) in _cases().items()}
    errors = {name: _drive({}, lambda tr, f=thunk: f(), available) for name, (available, thunk) in _errors().items()}
    return {"cases": cases, "errors": errors}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_lists_these_cases(golden):
    assert list(golden["cases"]) == list(_cases()) and list(golden["errors"]) == list(_errors())


@pytest.mark.parametrize("name", list(_cases()))
def test_calls_equal_the_recording(golden, name):
    script, thunk = _cases()[name]
    got, want = _drive(script, thunk), golden["cases"][name]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"{name}: call {i} is {g}, recorded {w}"
    assert got == want


@pytest.mark.parametrize("name", list(_errors()))
def test_exceptions_equal_the_recording(golden, name):
    available, thunk = _errors()[name]
    got, want = _drive({}, lambda tr: thunk(), available), golden["errors"][name]
    assert "raises" in want, f"{name}: the recording holds no exception"
    assert got.get("raises") == want["raises"]
    assert got == want       # and the same library calls, if any, before it


if __name__ == "__main__":      # records tests/golden/shim_calls.json anew (only when the shim's calls are meant to change)
    rec = _record()
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        for si, (section, entries) in enumerate(rec.items()):
            f.write(json.dumps(section) + ": {\n")
            f.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in entries.items()))
            f.write("\n}" + ("," if si + 1 < len(rec) else "") + "\n")
        f.write("}\n")
