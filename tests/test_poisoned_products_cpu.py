"""The inputs of tests/test_gpu_poisoned_products.py are not vacuous (no GPU needed): the two
shared inputs that stress ALG1's single pass do what their names say, the short cases keep their
output within the single pass's estimate (so the workspace hand-off is reached), the poison
schedule gives both row-pointer widths both fills, the tile groupings cover every tile in both
orders, and the 16-bit column matrices hold the rows the split can get wrong -- an empty row, a
row only in the last block, entries on both sides of every block edge -- with a host split that
joins back to the indices."""
import numpy as np
import pytest

from tests import instantiations as inst


def test_estimate_overflow_pair():
    A, B = inst.estimate_overflow_pair()
    assert A.has_canonical_format and B.has_canonical_format
    p = inst.plan(A.shape[0], A.nnz, B.shape[0], B.nnz, B.shape[1], "f64")
    assert p["path"] == "short"
    nnz_c = (abs(A) @ abs(B)).nnz
    assert nnz_c > inst.alg1_estimate(A, B)
    assert nnz_c > 10 * A.nnz * (B.nnz / B.shape[0])
    assert inst.estimate_overflow_pair()[0] is A        # generated once


def test_long_row_pair():
    A, B = inst.long_row_pair()
    assert A.has_canonical_format and B.has_canonical_format
    p = inst.plan(A.shape[0], A.nnz, B.shape[0], B.nnz, B.shape[1], "f64")
    assert p["path"] == "short"
    lens = np.diff(A.indptr)
    assert lens.max() >= 300 > inst.ROW_ENTRIES and (lens > inst.ROW_ENTRIES).sum() == 1
    assert (abs(A) @ abs(B)).nnz <= inst.alg1_estimate(A, B)     # only the row makes the pass hand over


@pytest.mark.parametrize("case", [c.id for c in inst.CASES if c.expect["path"] == "short"])
def test_short_cases_fit_the_single_pass_estimate(case):
    A, B, _ = inst.inputs(case)
    assert len(inst.reference(case)[1]) <= inst.alg1_estimate(A, B)


def test_short64_holds_the_single_pass_on_k_short():
    """short64-kshort-f64: k_short's single pass refuses only A rows of more than 64 entries (it
    takes any product count up to 65535), and gives up past the estimate: neither happens here, so
    ALG1 keeps the C that pass wrote."""
    case = "short64-kshort-f64"
    A, B, meta = inst.inputs(case)
    assert inst.CASE[case].env == {"SPG_SHORT_KERNEL": "short"}
    assert np.diff(A.indptr).max() == 64 and A.shape[0] == inst.ROWS
    assert max(v[1] for v in meta.spill.values()) == 641 < 65535
    assert len(inst.reference(case)[1]) <= inst.alg1_estimate(A, B)
    assert inst.plan_case(case)["path"] == "short"
    # the same rows as `short` but for the 65-entry one
    edges = set(inst.inputs("short-kshort-f64")[2].edge)
    assert set(meta.edge) == edges - {"len65"} and "len65" in edges


def test_poison_schedule():
    seen = {(fill, inst.POISON_WIDTHS[(ai + fi) % 2]) for ai in range(len(inst.ALGS))
            for fi, fill in enumerate(inst.POISON_FILLS)}
    assert seen == {(f, w) for f in (0x00, 0xFF) for w in ((32, 64), (64, 32))}
    assert inst.STALE_ORDER == (1, 2, "3c", 2)


@pytest.mark.parametrize("tiles", [1, 2, 5, 9])
def test_tile_groupings(tiles):
    g = dict(inst.tile_groupings(tiles))
    for name, ranges in g.items():
        covered = sorted(t for a, b in ranges for t in range(a, b))
        assert covered == list(range(tiles)), name
        starts = [a for a, _ in ranges]
        assert starts == sorted(starts, reverse=name.endswith("descending")), name
    if tiles == 1:
        assert list(g) == ["all/ascending"]
    else:
        assert set(g) == {"per-tile/ascending", "per-tile/descending", "two/ascending", "two/descending", "all/ascending"}
        assert len(g["per-tile/ascending"]) == tiles and len(g["two/ascending"]) == 2


@pytest.mark.parametrize("case,tiles", [("dense2048-f64", 9), ("sparse8192-f64", 1), ("sparse8192-f64-rg1", 5)])
def test_tile_cases_have_value_tiles(case, tiles):
    """dense2048: 17000 columns in 2048-column tiles, record group 1; sparse8192: 5 tiles in one
    record group of 8, so its only call is the whole product; with record group 1 they are 5."""
    p = inst.plan_case(case)
    assert -(-p["tiles_per_row"] // p["record_group"]) == tiles


@pytest.mark.parametrize("cols", inst.COLS16_WIDTHS)
def test_cols16_matrix(cols):
    assert inst.COLS16_WIDTHS == (65535, 65536, 65537, 140000)
    M = inst.cols16_matrix(cols)
    assert M.has_canonical_format and M.shape[1] == cols and M.indices.dtype == np.int32
    assert inst.cols16_matrix(cols) is M
    nb = -(-cols // 65536)
    last0 = (nb - 1) * 65536
    row = lambda name: M.indices[M.indptr[inst.COLS16_ROWS[name]]:M.indptr[inst.COLS16_ROWS[name] + 1]]
    starts, lo16 = inst.cols16_split_host(M)
    assert starts.shape == (M.shape[0], nb - 1) and starts.dtype == np.uint32 and lo16.dtype == np.uint16
    # the empty rows, also among the random ones; every start of an empty row is its length, 0
    assert len(row("empty")) == 0 and len(row("empty2")) == 0
    assert (starts[np.diff(M.indptr) == 0] == 0).all()
    # a row with entries only in the last block: every start is 0; only in the first: its length
    assert len(row("last-block")) == min(40, cols - last0) and row("last-block").min() >= last0
    assert (starts[inst.COLS16_ROWS["last-block"]] == 0).all()
    assert row("first-block").max() < 65536 and (starts[inst.COLS16_ROWS["first-block"]] == 50).all()
    # an entry on each side of every block edge, the last column alone, a row through every block
    want = sorted({c for b in range(nb) for c in (b * 65536, min(cols, (b + 1) * 65536) - 1)})
    assert list(row("edges")) == want and list(row("last-column")) == [cols - 1]
    for b in range(1, nb):
        assert {b * 65536 - 1, b * 65536} <= set(row("edges"))
    assert set(row("all-blocks") >> 16) == set(range(nb)) or cols == 65537   # (one column in its last block)
    assert set(M.indices >> 16) == set(range(nb))
    assert list(starts[inst.COLS16_ROWS["edges"]]) == [2 * (b + 1) for b in range(nb - 1)]
    # the split carries the columns exactly: (block << 16 | lo16) joins back to the indices
    assert np.array_equal(inst.cols16_join_host(M, starts, lo16), M.indices)
    assert np.array_equal(((M.indices >> 16) << 16) | lo16, M.indices)
