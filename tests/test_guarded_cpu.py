"""tests/guarded.py on CPU tensors: the interior is aligned and of the size asked for, both bands
are poisoned, check() passes on an untouched buffer and fails on a single changed byte at either
end of either band, naming the buffer and the offset from the interior."""
import numpy as np
import pytest

from tests.guarded import ALIGN, BAND, guarded

torch = pytest.importorskip("torch")

DTYPES = ["int32", "int64", "uint16", "float32", "float64", "complex64", "complex128"]


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0xA5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [0, 1, 13, (7, 3)])
def test_layout_and_poison(shape, dtype, fill):
    g = guarded(shape, dtype, fill, "cpu", name="buf")
    item = np.dtype(dtype).itemsize
    want_shape = (shape,) if isinstance(shape, int) else shape
    assert tuple(g.t.shape) == want_shape
    assert g.t.element_size() == item and str(g.t.dtype) == "torch." + dtype
    assert g.nbytes == int(np.prod(want_shape)) * item == g.t.numel() * item
    assert g.data_ptr() % ALIGN == 0 and (g.nbytes == 0 or g.data_ptr() == g.t.data_ptr())
    assert g.data_ptr() == g.parent.data_ptr() + g.front and g.front >= BAND
    assert g.parent.numel() >= g.back + BAND
    assert bool((g.parent == fill).all())
    g.check()
    # the poison as the dtype reads it
    if g.t.numel() and fill == 0xFF:
        host = g.t.numpy() if dtype != "uint16" else g.bytes().numpy().view(np.uint16)
        if np.dtype(dtype).kind in "fc":
            assert np.isnan(host).all()
        elif np.dtype(dtype).kind == "i":
            assert (host == -1).all()
        else:
            assert (host == 0xFFFF).all()
    # writing the whole interior leaves the guards alone
    g.bytes().fill_(fill ^ 0x5A)
    g.check()
    assert g.t.is_contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [0, 5])
def test_check_sees_one_byte_at_each_end_of_each_band(dtype, count):
    item = np.dtype(dtype).itemsize
    g = guarded(count, dtype, 0xFF, "cpu")
    nb = count * item
    # (offset from the interior's start, band): first and last byte of each band
    for off, band in ((-BAND, "front"), (-1, "front"), (nb, "back"), (nb + BAND - 1, "back")):
        g.refill()
        g.check("C.values")
        g.parent[g.front + off] = 0x7F
        with pytest.raises(AssertionError) as e:
            g.check("C.values")
        msg = str(e.value)
        assert "C.values" in msg and band in msg and f"byte offset {off} " in msg, msg
    g.refill()
    g.check()


def test_first_changed_byte_is_reported():
    g = guarded(16, "float64", 0x00, "cpu", name="y")
    g.parent[g.back + 9] = 1
    g.parent[g.back + 3] = 1
    with pytest.raises(AssertionError, match=r"y: back guard band changed, 2 bytes, first at byte offset 131 "):
        g.check()
    # a byte equal to the fill is no change; 0x00 poison reads as zeros
    g.refill()
    assert bool((g.t == 0).all())
    g.check()


def test_band_is_the_reach():
    """A store further than BAND bytes in front of the interior is outside the check (the
    alignment padding in front of the band is checked too, so the reach is at least BAND)."""
    g = guarded(4, "int32", 0xFF, "cpu")
    assert BAND == 4096 and BAND <= g.front < BAND + ALIGN
