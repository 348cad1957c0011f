"""Packed segments of the dense-tile kernels (k_seg_place / k_tile_dn, spmm_amd/csrc/seg_place.hpp).

Plans whose numeric kernel is k_tile_dn find the records of every (tile, B row) segment through
an 8-byte {byte offset, record count} pair, and large products of short segments keep every
segment at a byte offset chosen so that it crosses no 128-byte line it need not.  The planner
places only products of 4e9 expected products and more (spgemm.hip, placed_segments); the tests
here are small, so they run under SPG_SEG_PLACE=1, the schedule-only switch that places the
segments of every such plan.  The inputs are crafted for that placement:

  A  96 x 1100, about 170 entries per row, one row of exactly 64 and one of exactly 65 entries
  B  1100 x 16384 fp64 (8 tiles of 2048 columns; K = 1100 is no multiple of the 64 B rows one
     lane places), every tile segment 0, 1, 12, 13, 25 or 26 records long (10 / 120 / 130 / 250 /
     260 bytes: either side of one and of two lines), tile 3 empty in every row, and the last
     block of the last tile ending exactly on a line (26 + 26 + 12 records = 640 bytes), so the
     sentinel records start right behind its last record.

test_crafted_inputs (no GPU) checks these properties on a host model of the placement, among them
that segments would start at every even residue modulo 128.  On the GPU every result is compared
bit for bit with scipy's A @ B: ALG1 / ALG2 / ALG3 (and ALG3 with its chunks kept) on workspaces
of exactly the queried size and C arrays that are guarded and poisoned with 0x00 and 0xFF
(tests/guarded.py, through tests/instantiations.py), spg_symbolic twice before spg_numeric,
spg_numeric_tiles over the first, a middle and the last tile alone and then over all tiles, a
spg_numeric on the same plan after that, all of it with 32- and 64-bit row pointers; and one
fp32 (entry runs) and one complex128 product on dense 1024-column tiles, whose segments are
several lines long, placed (the switch) and, as the planner leaves them, at compact offsets.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import instantiations as inst

M, K, N, TW = 96, 1100, 16384, 2048
G = N // TW
CRAFT = (0, 1, 12, 13, 25, 26)
EMPTY_TILE = 3
PLACE = {"SPG_SEG_PLACE": "1"}
LINE, BLK = 128, 64


def _segments_to_csr(counts, tw, n, rng, dt):
    """B from per-(row, tile) segment lengths: random distinct columns inside each tile."""
    rows = []
    for k in range(counts.shape[0]):
        cols = [g * tw + np.sort(rng.choice(min(tw, n - g * tw), int(c), replace=False))
                for g, c in enumerate(counts[k]) if c]
        rows.append(np.concatenate(cols) if cols else np.zeros(0, np.int64))
    return inst._csr(rows, (counts.shape[0], n), rng, dt)


def _a_matrix(rng, m, k, per_row, dt, exact=()):
    rows = []
    for i in range(m):
        cnt = dict(exact).get(i, int(rng.integers(per_row - 12, per_row + 13)))
        rows.append(np.sort(rng.choice(k, cnt, replace=False)))
    return inst._csr(rows, (m, k), rng, dt)


@functools.lru_cache(maxsize=1)
def crafted():
    rng = np.random.default_rng(inst.seed_of("dn_packed_segments"))
    counts = rng.choice(CRAFT, size=(K, G))
    counts[:, EMPTY_TILE] = 0
    last_blk = K // BLK * BLK                      # rows 1088 .. 1099: the last block of every tile
    counts[last_blk:, G - 1] = 0
    counts[K - 3:, G - 1] = (26, 26, 12)           # 640 bytes from the block's line-aligned start
    B = _segments_to_csr(counts, TW, N, rng, np.float64)
    A = _a_matrix(rng, M, K, 170, np.float64, exact=((5, 64), (6, 65)))
    C = (A @ B).tocsr()
    C.sort_indices()
    ref = (C.indptr.copy(), C.indices.copy(), C.data.copy())
    for a in (A.data, A.indices, A.indptr, B.data, B.indices, B.indptr) + ref:
        a.setflags(write=False)
    return A, B, counts, ref


def _place(x, L):
    if L == 0:
        return x
    here = (x + L - 1) // LINE - x // LINE + 1
    return -(-x // LINE) * LINE if here > -(-L // LINE) else x


def placed_model(counts, rb):
    """The device passes on the host: per tile, blocks of 64 rows placed from a line boundary.
    Returns per tile (start residues before placing, placed starts, end in bytes, end of the last
    block before its rounding)."""
    out = []
    for g in range(counts.shape[1]):
        base, res, starts, raw_end = 0, [], [], 0
        for k0 in range(0, counts.shape[0], BLK):
            x = 0
            for c in counts[k0:k0 + BLK, g]:
                L = int(c) * rb
                at = _place(x, L)
                if L:
                    res.append(x % LINE)
                starts.append(base + at)
                x = at + L
            raw_end = base + x
            base += -(-x // LINE) * LINE
        out.append((res, starts, base, raw_end))
    return out


def test_crafted_inputs():
    A, B, counts, _ = crafted()
    lens = np.diff(A.indptr)
    assert lens[5] == 64 and lens[6] == 65 and 160 <= lens.mean() <= 180
    per_row = np.diff(B.indptr)
    assert 82 <= per_row.mean() <= 170 and K % BLK != 0
    assert set(np.unique(counts)) == set(CRAFT)
    assert not counts[:, EMPTY_TILE].any() and all(counts[:, g].any() for g in range(G) if g != EMPTY_TILE)
    # B's segments are the crafted ones
    tiles = B.indices // TW
    got = np.zeros_like(counts)
    np.add.at(got, (np.repeat(np.arange(K), per_row), tiles), 1)
    assert np.array_equal(got, counts)
    model = placed_model(counts, 10)
    compact, placed = set(), set()
    for g, (res, starts, end, raw_end) in enumerate(model):
        rank = np.concatenate([[0], np.cumsum(counts[:, g])])[:-1]
        compact |= set(((10 * rank[counts[:, g] > 0]) % LINE).tolist())
        for c, at in zip(counts[:, g], starts):
            L = int(c) * 10
            if L:
                placed.add(at % LINE)
            if 0 < L <= LINE:
                assert at // LINE == (at + L - 1) // LINE
        assert end % LINE == 0
    # every even start residue: where the segments start back to back (what the placement is
    # handed), and after placing still both record alignments (0 and 2 modulo 4) and many offsets
    assert compact == set(range(0, LINE, 2))
    assert {r % 4 for r in placed} == {0, 2} and 0 in placed and len(placed) >= 32, sorted(placed)
    assert model[EMPTY_TILE][2] == 0                          # the empty tile takes no line
    assert model[G - 1][3] == model[G - 1][2]                 # the last block ends on a line, unrounded
    # the placed size, block by block as the device places it, is within the plan-time bound
    # (seg_bound; spgemm.hip brec_span rounds it up to a line), tile by tile and in all
    for g in range(G):
        nz = int(counts[:, g].sum())
        assert model[g][2] <= 10 * nz + 126 * min(nz, K), g
    assert sum(m[2] for m in model) <= -(-(10 * B.nnz + 126 * min(B.nnz, K * G)) // LINE) * LINE
    # this shape's segments are short enough to be placed, but its product is far too small for
    # the planner to do so: the GPU tests set SPG_SEG_PLACE=1 (spgemm.hip placed_segments)
    assert B.nnz / K * TW / N * 10 <= 256 and A.nnz * B.nnz / K < 4e9
    # the planner takes dense 2048-column tiles for this shape (restated planner, no GPU)
    want = inst.plan(M, A.nnz, K, B.nnz, N, "f64")
    assert (want["path"], want["tile_width"], want["dense_tiles"], want["lds_ordered"]) == ("tile", 2048, True, True)
    assert all(abs(v / t - 1.0) > inst.MARGIN for _, v, t in want["margins"]), want["margins"]


torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def uploaded():
    A, B, _, _ = crafted()
    return inst.Uploaded(A), inst.Uploaded(B)


@gpu
@pytest.mark.parametrize("ip", [32, 64])
@pytest.mark.parametrize("alg", [1, 2, 3, "3c"])
def test_spgemm_bit_exact(alg, ip):
    _, _, _, ref = crafted()
    dA, dB = uploaded()
    for fill in inst.POISON_FILLS:
        info = {}
        got = inst.run_abi(dA, dB, alg, 1.0, inst.CF, ip, 64 if fill else 32, env=PLACE, info=info, fill=fill)
        assert (info["path"], info["tile_width"], info["tiles_per_row"], info["dense_tiles"], info["lds_ordered"],
                info["record_group"]) == ("tile", TW, G, True, True, 1), info
        inst.assert_same(got, ref, f"alg={alg} IP={ip} fill={fill:#04x}")


@gpu
@pytest.mark.parametrize("ip", [32, 64])
def test_symbolic_twice_then_numeric(ip):
    _, _, _, ref = crafted()
    dA, dB = uploaded()
    for fill in inst.POISON_FILLS:
        ex = {}
        got = inst.run_abi(dA, dB, 2, 1.0, inst.CF, ip, 64, first_cp=32, env=PLACE, fill=fill, extra=ex)
        inst.assert_same(got, ref, f"repeated spg_symbolic IP={ip} fill={fill:#04x}")
        assert np.array_equal(ex["first"][0].astype(np.int64), ref[0].astype(np.int64))
        assert ex["first"][1] == ex["nnz"] == len(ref[1])


@gpu
@pytest.mark.parametrize("fill", inst.POISON_FILLS)
@pytest.mark.parametrize("ip", [32, 64])
def test_numeric_tiles_then_numeric(ip, fill):
    """spg_numeric_tiles with tile-major values over the first, a middle and the last tile alone
    (only that tile's columns of C are written, and they are scipy's; every other entry still
    holds the poison byte), over all tiles one by one, then spg_numeric on the same plan."""
    from spmm_amd import _lib
    from tests.guarded import guarded
    _, _, _, ref = crafted()
    dA, dB = uploaded()
    dA_, dB_, h, va, vb = inst._handle_views(dA, dB, ip)
    lib, dev = h.lib, dA.device
    al = inst._scalar(np.float64, 1.0)
    rp, rj, rx = ref
    ws = guarded(inst.workspace_bytes(dA, dB, 2, inst.CF, ip, PLACE), "uint8", fill, dev, "workspace")
    wsb = ctypes.c_size_t(ws.nbytes)
    plan = ctypes.c_void_p()
    with inst.environ(PLACE):      # (read per plan)
        _lib.check(lib.spg_plan(h.ptr, ctypes.byref(va), ctypes.byref(vb), 2, inst.CF, ctypes.byref(wsb),
                                ctypes.c_void_p(ws.data_ptr()), ctypes.byref(plan)), "spg_plan")
    try:
        offs = (ctypes.c_int64 * (G + 1))()
        _lib.check(lib.spg_tile_value_offsets(h.ptr, plan, offs, G + 1), "spg_tile_value_offsets")
        tile_of = dB_.indices.cpu().numpy() // TW
        assert list(offs) == [int((tile_of < g).sum()) for g in range(G + 1)]     # the compact tile-major order
        tm = guarded(dB.nnz, np.float64, fill, dev, "tile-major values")
        _lib.check(lib.spg_tile_values(h.ptr, plan, ctypes.c_void_p(tm.data_ptr())), "spg_tile_values")
        indptr = guarded(M + 1, "int64", fill, dev, "C.indptr")
        nnz = ctypes.c_int64(0)
        _lib.check(lib.spg_symbolic(h.ptr, plan, ctypes.c_void_p(indptr.data_ptr()), 64, ctypes.byref(nnz)), "spg_symbolic")
        nz = int(nnz.value)
        assert nz == len(rj)

        def fresh():
            gj, gx = guarded(nz, "int32", fill, dev, "C.indices"), guarded(nz, np.float64, fill, dev, "C.values")
            return gj, gx, _lib.SpgCsr(M, N, nz, indptr.data_ptr(), gj.data_ptr(), gx.data_ptr(), 64, va.value_type)

        def tiles(vc, t0, t1):
            _lib.check(lib.spg_numeric_tiles(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc),
                                             ctypes.c_void_p(tm.data_ptr()), t0, t1), "spg_numeric_tiles")
            torch.cuda.synchronize()

        for t in (0, G // 2, G - 1):
            gj, gx, vc = fresh()
            tiles(vc, t, t + 1)
            j, x = gj.t.cpu().numpy(), gx.t.cpu().numpy()
            mine = rj // TW == t
            assert np.array_equal(j[mine], rj[mine]) and np.array_equal(x[mine].view(np.uint64), rx[mine].view(np.uint64)), t
            assert (j[~mine].view(np.uint8) == fill).all() and (x[~mine].view(np.uint8) == fill).all(), t
            for g in (ws, indptr, tm, gj, gx):
                g.check(f"tile {t} alone: {g.name}")
        gj, gx, vc = fresh()
        for t in range(G):
            tiles(vc, t, t + 1)
        inst.assert_same((indptr.t.cpu().numpy(), gj.t.cpu().numpy(), gx.t.cpu().numpy()), ref, "all tiles one by one")
        gj2, gx2, vc2 = fresh()
        _lib.check(lib.spg_numeric(h.ptr, plan, ctypes.byref(al), ctypes.byref(vc2)), "spg_numeric")
        torch.cuda.synchronize()
        inst.assert_same((indptr.t.cpu().numpy(), gj2.t.cpu().numpy(), gx2.t.cpu().numpy()), ref, "spg_numeric after tiles")
        for g in (ws, indptr, tm, gj, gx, gj2, gx2):
            g.check(f"after tiles: {g.name}")
    finally:
        lib.spg_plan_destroy(plan)
    dA.check_unchanged("A")
    dB.check_unchanged("B")


# dense 1024-column tiles of the other record forms: fp32 entry runs (6-byte records, segments of
# 48 records and more) and complex128 (20-byte records); both sides of a line again, in their units
OTHER = {"f32": dict(k=520, n=2048, per_a=80, craft=(0, 21, 22, 64, 85, 128)),
         "c128": dict(k=520, n=2048, per_a=80, craft=(0, 1, 6, 7, 12, 13, 32))}


@functools.lru_cache(maxsize=2)
def other(dname):
    o = OTHER[dname]
    dt = inst.DTYPES[dname]
    rng = np.random.default_rng(inst.seed_of("dn_packed_segments", dname))
    counts = rng.choice(o["craft"], size=(o["k"], o["n"] // 1024))
    B = _segments_to_csr(counts, 1024, o["n"], rng, dt)
    A = _a_matrix(rng, M, o["k"], o["per_a"], dt, exact=((5, 64), (6, 65)))
    C = (A @ B).tocsr()
    C.sort_indices()
    return A, B, (C.indptr, C.indices, C.data)


@gpu
@pytest.mark.parametrize("dname", list(OTHER))
def test_other_dense1024(dname):
    A, B, ref = other(dname)
    want = inst.plan(M, A.nnz, B.shape[0], B.nnz, B.shape[1], dname)
    assert (want["tile_width"], want["dense_tiles"], want["lds_ordered"]) == (1024, True, True), want
    dA, dB = inst.Uploaded(A), inst.Uploaded(B)
    for fill in inst.POISON_FILLS:
        for alg, ip, env in ((2, 32, PLACE), ("3c", 64, PLACE), (2, 64, {})):
            info = {}
            got = inst.run_abi(dA, dB, alg, 1.0, inst.CF, ip, 32, env=env, info=info, fill=fill)
            assert (info["path"], info["tile_width"], info["dense_tiles"], info["lds_ordered"]) == ("tile", 1024, True, True)
            inst.assert_same(got, ref, f"{dname} alg={alg} IP={ip} fill={fill:#04x} {env}")
