"""tests/_views.py, the pitched / unaligned window helper of the layout tests
(test_gpu_views_*.py), on CPU tensors: content, strides, alignment residues,
guard margins, and that guards_intact sees one changed byte in each margin."""
import numpy as np
import pytest
import torch

import _views as V

DTYPES = [np.uint8, np.uint16, np.float16, np.float32]


def _arr(shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.uniform(-100, 100, shape).astype(dtype)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def test_layout_table_holds_the_required_entries():
    want = {"a16_pitched": (0, 0), "vec4": (4, 0), "odd_base": (1, 0), "odd_both": (3, None)}
    for name, (base, pitch) in want.items():
        assert V.LAYOUTS[name].base == base and V.layout_of(name) [0] == base
        if pitch is not None:
            assert V.LAYOUTS[name].pitch == pitch and V.layout_of(name)[1] == pitch
    assert V.LAYOUTS["odd_pitch"].base == 0 and V.LAYOUTS["odd_pitch"].pitch % 2 == 1
    assert V.LAYOUTS["odd_both"].pitch % 4 == 2
    assert V.layout_of("odd_base", 1, 3)[0] == 3  # one BGR pixel
    for e in (2, 4):
        assert V.layout_of("odd_base", e)[0] == e  # one element
        assert V.layout_of("odd_pitch", e)[1] % 16 != 0 and V.layout_of("odd_pitch", e)[1] % e == 0
        assert V.layout_of("odd_both", e)[1] % 16 != 0 and V.layout_of("odd_both", e)[1] % e == 0


@pytest.mark.parametrize("layout", list(V.LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(7, 13), (1, 1), (5, 9, 3), (4, 6, 4), (3, 8, 2)])
def test_window(layout, dtype, shape):
    arr = _arr(shape, dtype)
    parent, view = V.window(arr, layout, seed=3)
    e = arr.dtype.itemsize
    cn = shape[2] if len(shape) == 3 else 1
    # the view equals the input
    assert tuple(view.shape) == shape and np.array_equal(V.host(view).view(np.uint8), arr.view(np.uint8))
    # strides and alignment are what the table says
    base, pitch = V.layout_of(layout, e, cn)
    assert view.data_ptr() % 16 == base
    assert (view.stride(0) * e) % 16 == pitch
    assert view.stride(-1) == 1 and (len(shape) == 2 or view.stride(1) == cn)
    assert view.stride(0) * e > shape[1] * cn * e
    if e == 1 and cn == 1:
        assert (base, pitch) == V.LAYOUTS[layout][:2]
    # the guard margins hold, and the window lies strictly inside its allocation
    top, bottom, left, right = V.margins(parent, view)
    assert top >= 2 and bottom >= 2 and left >= e * cn and right >= 16
    assert left % (e * cn) == 0
    st = parent.untyped_storage()
    assert parent.data_ptr() > st.data_ptr() and parent.data_ptr() + parent.numel() < st.data_ptr() + st.nbytes()
    # the guards are noise, not a constant
    outside = parent[~V.window_mask(parent, view)]
    assert len(torch.unique(outside)) > 8
    assert int(V.window_mask(parent, view).sum()) == arr.nbytes
    # guards_intact: true untouched and after a write inside the window, false after one byte in each margin
    before = V.snapshot(parent)
    assert V.guards_intact(parent, before, view)
    view.view(torch.int16 if dtype == np.uint16 else view.dtype)[0, 0] = 1
    assert V.guards_intact(parent, before, view)
    start = view.data_ptr() - parent.data_ptr()
    p = view.stride(0) * e
    row = shape[1] * cn * e
    h = shape[0]
    for pos in (start - p,               # the row above
                start + h * p,           # the row below
                start - 1,               # the byte left of the first pixel
                start + (h - 1) * p + row,   # the byte right of the last pixel
                0, parent.numel() - 1):  # the parent's corners
        old = int(parent[pos])
        parent[pos] = old ^ 0x55
        assert not V.guards_intact(parent, before, view), pos
        parent[pos] = old
    assert V.guards_intact(parent, before, view)


def test_windows_of_one_seed_repeat_and_of_two_seeds_differ():
    arr = _arr((6, 10), np.uint8)
    a, _ = V.window(arr, "odd_both", seed=1)
    b, _ = V.window(arr, "odd_both", seed=1)
    c, _ = V.window(arr, "odd_both", seed=2)
    assert torch.equal(a, b) and not torch.equal(a, c)
