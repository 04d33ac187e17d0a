"""CPU self-test of tests/_guard.py: the layout the guarded op-level tests rely on, and that each check reports what it is for."""
import pytest
import torch

from _guard import FILL, MIN_BORDER, Guarded, all_written


@pytest.mark.parametrize("shape,dtype", [((2, 5, 7, 9, 8), torch.float32), ((3, 11, 13, 24), torch.bfloat16), ((7, 3, 5), torch.float64),
                                         ((10007,), torch.float32), ((1, 40, 40, 40, 16), torch.float32)])
def test_payload_is_aligned_exact_and_between_nan_borders(shape, dtype):
    g = Guarded(shape, dtype, device="cpu")
    item = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= s
    assert g.ptr % 256 == 0 and g.tensor.data_ptr() == g.ptr
    assert g.nbytes == n * item and g.tensor.shape == shape and g.tensor.dtype == dtype
    front, back = g.borders()
    slab = (n // shape[0]) * item
    assert front.numel() >= max(MIN_BORDER, 2 * slab) and back.numel() >= max(MIN_BORDER, 2 * slab)
    # the back border starts at the very next byte behind the payload: no rounding, no slack
    assert back.data_ptr() == g.ptr + g.nbytes
    assert front.data_ptr() + front.numel() == g.ptr
    assert front.numel() + g.nbytes + back.numel() == g.raw.numel()
    assert bool((g.raw == FILL).all())
    assert bool(torch.isnan(g.tensor.float()).all())            # 0xFF.. is a NaN in every float format used
    g.check("fresh")


def test_values_land_in_the_payload_only():
    v = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    g = Guarded((2, 3, 4), torch.float32, values=v.numpy().astype("float64"), device="cpu")
    assert torch.equal(g.tensor, v)
    g.check("input")
    all_written(g, "input")
    g.fill(0x00)
    assert bool((g.tensor == 0).all())
    g.check("scratch")


@pytest.mark.parametrize("side", ["front", "back"])
@pytest.mark.parametrize("where", ["adjacent", "far"])
def test_one_changed_border_byte_is_reported(side, where):
    g = Guarded((4, 6, 8), torch.float32, values=torch.zeros(4, 6, 8), device="cpu")
    front, back = g.borders()
    b = front if side == "front" else back
    at = {("front", "adjacent"): b.numel() - 1, ("front", "far"): 0, ("back", "adjacent"): 0, ("back", "far"): b.numel() - 1}[(side, where)]
    b[at] = 0xFE
    with pytest.raises(AssertionError, match=r"dx: %s border" % side):
        g.check("dx")
    b[at] = FILL
    g.check("dx")


def test_unwritten_output_element_is_reported():
    for dtype in (torch.float32, torch.bfloat16, torch.float64):
        g = Guarded((3, 5, 8), dtype, device="cpu")
        g.tensor[...] = 1.0
        all_written(g, "y")
        g.bytes[-torch.empty((), dtype=dtype).element_size():] = FILL       # the last element back to its initial state
        with pytest.raises(AssertionError, match="y: 1 of 120 elements never written"):
            all_written(g, "y")
