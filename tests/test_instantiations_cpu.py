"""The inputs of tests/test_gpu_instantiations.py, checked without a GPU (tests/instantiations.py):
every case carries the edge rows it claims, the planner's rules restated in Python send it to the
kernel it names with a margin on every threshold, the oracle's C shows the intended item counts,
deleting the entry at any seam position changes C (so a kernel that mis-loads that entry cannot
pass), at least 20 % of a tile case's C entries sum two or more products, and the oracle agrees
with scipy bit for bit on these inputs.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle
from tests import instantiations as inst

# cases that differ only in their switches share their inputs: one representative each
UNIQUE = list({(c.struct, c.dname): c.id for c in inst.CASES}.values())
WIDE = [c for c in UNIQUE if inst.STRUCTS[inst.CASE[c].struct].kind != "short"]
TILE = [c for c in UNIQUE if inst.STRUCTS[inst.CASE[c].struct].kind == "tile"]
SHORT = [c for c in UNIQUE if inst.STRUCTS[inst.CASE[c].struct].kind == "short"]


def _row(M, i):
    return M.indices[M.indptr[i]:M.indptr[i + 1]]


def _crow(ref, i):
    p, j, x = ref
    return j[p[i]:p[i + 1]], x[p[i]:p[i + 1]]


def test_case_table_covers_every_kernel_and_dtype():
    have = {(c.id.rsplit("-", 1)[0] if not c.id.endswith("rg1") else "sparse8192-rg1", c.dname) for c in inst.CASES}
    want = ([("short", d) for d in inst.DTYPES] + [("short-kshort", "f64"), ("short64-kshort", "f64")] + [("general", d) for d in inst.DTYPES] +
            [("owner-sparse", "f32"), ("owner-sparse", "c64"), ("owner-dense", "f32"), ("owner-dense", "c64"),
             ("runs32", "f32"), ("dense1024", "f64"), ("dense1024", "c128"), ("dense2048", "f64"),
             ("sparse4096", "f64"), ("sparse4096", "c128"), ("sparse8192", "f64"), ("sparse8192-rg1", "f64")])
    assert set(want) <= have, set(want) - have
    syms = {c.sym for c in inst.CASES}
    assert {"k_tile_sym_seg", "k_tile_sym8c"} <= syms
    for c in inst.CASES:
        assert 128 <= inst.inputs(c.id)[0].shape[0] <= 192


@pytest.mark.parametrize("case", inst.CASE_IDS)
def test_planner_selects_the_case_with_margin(case):
    c = inst.CASE[case]
    pl = inst.plan_case(case)
    assert {k: pl[k] for k in c.expect} == c.expect, pl
    assert pl["sym"] == c.sym, pl
    for name, v, th in pl["margins"]:
        assert abs(v / th - 1.0) >= inst.MARGIN, (case, name, v, th)
    S = inst.STRUCTS[c.struct]
    if S.kind == "tile":
        assert pl["tile_width"] == S.tw                       # the geometry the special rows were built for
        assert pl["tiles_per_row"] >= 3 and S.n % S.tw != 0   # an inner tile and a ragged last tile
        if pl["dense_tiles"]:
            assert S.caps == ()
        elif pl["record_group"] == 8:
            assert 2032 in S.caps and S.n % (8 * 8192) != 0   # SpCfgRG's window; padding tiles in the last group
        else:
            assert (2048 if S.tw == 8192 else 1024) in S.caps  # SpCfg2048 / SpCfg1024 / k_tile's TILE_CAP


@pytest.mark.parametrize("case", UNIQUE)
def test_inputs_are_canonical_and_typed(case):
    A, B, _ = inst.inputs(case)
    dt = inst.DTYPES[inst.CASE[case].dname]
    for M in (A, B):
        assert M.dtype == dt and M.indices.dtype == np.int32
        assert oracle.has_canonical_format(M) and M.has_canonical_format
        assert np.isfinite(M.data.view(M.data.real.dtype)).all() and (M.data != 0).all()
    A2, B2, _ = inst._inputs.__wrapped__(inst.CASE[case].struct, inst.CASE[case].dname)   # from seeds: the same again
    assert np.array_equal(A2.indices, A.indices) and np.array_equal(B2.data.view(np.uint8), B.data.view(np.uint8))


@pytest.mark.parametrize("case", WIDE)
def test_a_row_lengths_and_their_places(case):
    A, B, meta = inst.inputs(case)
    dname = inst.CASE[case].dname
    q = inst.nb_of(dname) * 64
    lens = np.diff(A.indptr)
    want = inst.a_lengths(dname)
    assert want == [0, 1, 63, 64, 65, 127, 128, 129, q - 1, q, q + 1, q + 64, 2 * q + 1]
    edge_lens = {int(lens[i]) for lab, i in meta.edge.items() if lab.startswith("len")}
    assert set(want) <= edge_lens, set(want) - edge_lens
    assert lens[0] == 2 * q + 1 and lens[-1] == q + 1                   # first and last row are edge rows
    assert 0 in meta.edge.values() and A.shape[0] - 1 in meta.edge.values()
    i = meta.edge[f"len{q + 64}"]
    assert lens[i - 1] == 0 and lens[i + 1] == 0                        # an empty row on each side of a long row
    assert lens[1] == 0                                                 # and after the longest
    # length rows and fillers use ordinary (non-empty, random) B rows only
    blen = np.diff(B.indptr)
    special = set(meta.special.values())
    for lab, i in meta.edge.items():
        if lab.startswith("len"):
            assert not special & set(_row(A, i).tolist()) and (blen[_row(A, i)] > 0).all()
    # the seam row: special rows at entries 0, 63, 64, q - 1, q, all on two columns of the inner tile
    S = inst.STRUCTS[inst.CASE[case].struct]
    seam = _row(A, meta.edge["seam"])
    assert len(seam) == q + 1
    for pos, lab in [(0, "lo.g.straddle"), (63, "mid.first"), (64, "mid.last"), (q - 1, "hi.g.first"), (q, "hi.g.last")]:
        assert seam[pos] == meta.special[lab]
        assert set(_row(B, seam[pos]).tolist()) & {S.tw, 2 * S.tw - 1}
    hits = np.concatenate([_row(B, j) for j in seam])
    assert (hits == S.tw).sum() >= 3 and (hits == 2 * S.tw - 1).sum() >= 3


@pytest.mark.parametrize("case", TILE)
def test_special_b_rows_have_their_shapes(case):
    A, B, meta = inst.inputs(case)
    S = inst.STRUCTS[inst.CASE[case].struct]
    k, n, tw = S.k, S.n, S.tw
    G = (n + tw - 1) // tw
    lo_rows = [r for lab, r in meta.special.items() if lab.startswith("lo.")]
    hi_rows = [r for lab, r in meta.special.items() if lab.startswith("hi.")]
    assert min(lo_rows) == 0 and max(hi_rows) == k - 1                  # at both ends of B's row range
    assert sorted(lo_rows) == list(range(len(lo_rows))) and sorted(hi_rows) == list(range(k - len(hi_rows), k))
    for end in ("lo", "hi"):
        for t, g in (("g", 1), ("l", G - 1)):
            c0, w = g * tw, min(tw, n - g * tw)
            r = lambda lab: _row(B, meta.special[f"{end}.{t}.{lab}"]).tolist()
            assert r("empty") == [] and r("first") == [c0] and r("last") == [c0 + w - 1] and r("nminus1") == [n - 1]
            assert r("straddle") == ([c0, c0 + w - 1, c0 + w] if t == "g" else [c0 - 1, c0, c0 + w - 1])
            assert r("full") == list(range(c0, c0 + w)) == r("full2")
            for m in (63, 64, 65):
                e = r(f"e{m}")
                assert len(e) == m and c0 <= e[0] and e[-1] < c0 + w
            for cap in S.caps:
                assert r(f"cap{cap}") == list(range(c0, c0 + cap)) and r(f"capnext{cap}") == [c0 + cap]
    # a full row is one segment longer than a marker group (dn_mkb * 64 products: 8 * 64, or
    # 16 * 64 from 2048 slots on) on every tile but the ragged one
    assert tw > (16 if tw >= 2048 else 8) * 64
    if S.rg:
        rows = _row(A, meta.edge["lasttile"])
        assert len(rows) == inst.nb_of("f64") * 64 + 1
        assert all(_row(B, j).min() >= (G - 1) * tw for j in rows)


@pytest.mark.parametrize("case", TILE)
def test_oracle_items_have_the_intended_counts(case):
    A, B, meta = inst.inputs(case)
    ref = inst.reference(case)
    S = inst.STRUCTS[inst.CASE[case].struct]
    labs = {i: lab for lab, i in meta.edge.items()}
    seen = set()
    for i, lo, hi, nnz in meta.items:
        cols, _ = _crow(ref, i)
        inside = int(((cols >= lo) & (cols < hi)).sum())
        if nnz is None:                       # every product in [lo, hi): the last real tile
            assert inside == len(cols) > 0, labs[i]
        else:
            assert inside == nnz == len(cols), (labs[i], inside, nnz)
        seen.add(labs[i].split(".")[0])
    assert {"full", "fullfull", "onlyempty"} <= seen
    for cap in S.caps:
        assert {f"cap{cap}", f"cap{cap}+1"} <= seen
    # the dense full-row item holds TW entries; two full rows sum every column twice
    i = meta.edge["fullfull.g"]
    cols, _ = _crow(ref, i)
    assert len(cols) == S.tw and oracle.num_products(A[i], B) == 2 * S.tw


@pytest.mark.parametrize("case", SHORT)
def test_short_case_rows_sit_on_the_kernel_limits(case):
    A, B, meta = inst.inputs(case)
    ref = inst.reference(case)
    s = meta.spill
    n = B.shape[1]
    assert (inst.ROW_ENTRIES, inst.ROW_PREG, inst.ROW_LCAP, 32 * inst.ROW_NW) == (64, 640, 64, 16384)
    # (short64 is `short` without the 65-entry row: its longest A row has exactly 64 entries)
    with65 = inst.CASE[case].struct != "short64"
    assert ("len65" in s) == with65 and np.diff(A.indptr).max() == (65 if with65 else 64)
    for m in (63, 64, 65) if with65 else (63, 64):
        assert s[f"len{m}"][0] == m and s[f"len{m}"][4] == (m <= 64)
    for P in (128, 129, 256, 257, 384, 385, 512, 513, 640, 641):
        e, prod, L, nz, taken = s[f"p{P}"]
        assert prod == P and e <= 64 and L == 0 and nz == P and taken == (P <= 640), (P, s[f"p{P}"])
    assert s["p640"][0] == 64 and s["p641"][0] == 64
    assert s["flag64"][2] == 64 and s["flag64"][4] and s["flag65"][2] == 65 and not s["flag65"][4]
    assert s["flag64"][1] == 64 and s["flag64"][3] == 62           # two columns hit twice
    spilled = ["p641", "len65", "flag65"] if with65 else ["p641", "flag65"]
    assert [lab for lab, v in s.items() if not v[4]] == spilled                       # spilled, each for one reason
    # the oracle shows the same counts; 640 distinct outputs exceed the stage window of every type
    # that has one within 640 (fp64 / complex64 517 or 602, complex128 387)
    for lab, i in meta.edge.items():
        assert len(_crow(ref, i)[0]) == s[lab][3], lab
    cols, _ = _crow(ref, meta.edge["p640"])
    assert len(cols) == 640 > 602 and cols[0] == 0 and cols[-1] == n - 1
    assert _crow(ref, meta.edge["p630+empty"])[0][-1] == n - 1 and meta.edge["p630+empty"] == A.shape[0] - 1
    assert meta.edge["p640"] == 0
    lens = np.diff(A.indptr)
    assert lens[1] == 0 and (lens == 0).sum() >= 2 and len(_crow(ref, meta.edge["onlyempty"])[0]) == 0


@pytest.mark.parametrize("case", UNIQUE)
def test_deleting_a_seam_entry_changes_c(case):
    """The fault a mis-loaded batch would make: for every edge row and q in {0, 63, 64, NB*64 - 1,
    NB*64, last}, A without entry q of that row gives another C row (structure or bits)."""
    A, B, meta = inst.inputs(case)
    ref = inst.reference(case)
    q = inst.nb_of(inst.CASE[case].dname) * 64
    blen = np.diff(B.indptr)
    variants, rows, data = [], [], []
    for lab, i in meta.edge.items():
        js, xs = _row(A, i), A.data[A.indptr[i]:A.indptr[i + 1]]
        for pos in sorted({0, 63, 64, q - 1, q, len(js) - 1}):
            if 0 <= pos < len(js):
                if blen[js[pos]] == 0:
                    assert not lab.startswith("len") and lab != "seam", lab   # only where an empty B row is meant
                    continue
                variants.append((lab, i, pos))
                rows.append(np.delete(js, pos))
                data.append(np.delete(xs, pos))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    Av = sp.csr_matrix((np.concatenate(data), np.concatenate(rows).astype(np.int32), indptr),
                       shape=(len(rows), A.shape[1]))
    got = oracle.spgemm(Av, B, keep_zeros=True, sort=True)
    for v, (lab, i, pos) in enumerate(variants):
        cols, vals = _crow(ref, i)
        gc, gv = _crow(got, v)
        same = np.array_equal(gc, cols) and np.array_equal(inst._bits(gv), inst._bits(vals))
        assert not same, (case, lab, pos)
    if "seam" in meta.edge:
        assert {p for lab, _, p in variants if lab == "seam"} == {0, 63, 64, q - 1, q}


@pytest.mark.parametrize("case", TILE)
def test_a_fifth_of_c_sums_several_products(case):
    A, B, _ = inst.inputs(case)
    ref = inst.reference(case)
    P = oracle.num_products(A, B)
    assert len(ref[1]) <= 0.8 * P, (len(ref[1]), P)


@pytest.mark.parametrize("case", UNIQUE)
def test_oracle_matches_scipy(case):
    A, B, _ = inst.inputs(case)
    p, j, x = inst.reference(case)
    M = sp.csr_matrix((x.copy(), j.copy(), p.copy()), shape=(A.shape[0], B.shape[1]))
    M.eliminate_zeros()
    C = A @ B
    C.sort_indices()
    inst.assert_same((M.indptr, M.indices, M.data), (C.indptr, C.indices, C.data), case)
    # and the alpha != 1 reference keeps the structure
    r = inst.reference(case, inst.alpha_of(inst.CASE[case].dname))
    assert np.array_equal(r[0], p) and np.array_equal(r[1], j) and not np.array_equal(inst._bits(r[2]), inst._bits(x))


def test_comparison_is_exact():
    p, j = np.array([0, 2, 3]), np.array([0, 4, 1], dtype=np.int32)
    x = np.array([1.0, -0.0, 2.5])
    inst.assert_same((p.astype(np.int32), j, x.copy()), (p, j, x))
    for y in (np.array([1.0, 0.0, 2.5]), np.nextafter(x, 9.0)):
        with pytest.raises(AssertionError):
            inst.assert_same((p, j, y), (p, j, x))
    with pytest.raises(AssertionError):
        inst.assert_same((np.array([0, 1, 3]), j, x), (p, j, x))
    with pytest.raises(AssertionError):
        inst.assert_same((p, np.array([0, 3, 1], dtype=np.int32), x), (p, j, x))
