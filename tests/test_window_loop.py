"""CPU (but for the pointer): what the two sliding-window testers share on the host (pointasnl_amd/window_loop.py) pinned to
the expressions it replaced and to the two numpy restatements (tests/window_flow_ref.py, tests/kitti_window_flow_ref.py)."""
import numpy as np
import pytest

import kitti_window_flow_ref as K
import window_flow_ref as R
from pointasnl_amd import window_loop as L


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def loop(stride, width):
    t = L.WindowLoop()
    t.stride, t.block_size = float(stride), float(width)
    return t


@pytest.mark.parametrize("magnitude", [0.01, 1.0, 50.0, 300.0])
@pytest.mark.parametrize("stride", [0.1, 0.3, 0.5, 1.7, 4.0])
def test_centres_have_the_bits_of_the_per_window_expression(magnitude, stride):
    rng = np.random.default_rng(int(magnitude * 100 + stride * 10))
    nx, ny = 7, 5
    for _ in range(10):
        coordmin = ((rng.random(3) * 2 - 1) * magnitude).astype(np.float32)
        coordmax = (coordmin + np.array([nx * stride, ny * stride, 2.9])).astype(np.float32)
        found = np.flatnonzero(rng.random(nx * ny) < 0.6)
        got = loop(stride, 1.5).centers(coordmin, coordmax, nx, ny)
        assert got.dtype == np.float64 and got.shape == (nx * ny, 2)
        want = []
        for w in found:  # ScanNet's window tester before the shared base, literally
            i, j = divmod(int(w), ny)
            curmin = coordmin + [i * stride, j * stride, 0]
            curmax = curmin + [1.5, 1.5, coordmax[2] - coordmin[2]]
            want.append((curmin[0:2] + curmax[0:2]) / 2.0)
        assert np.asarray(want).dtype == np.float64
        np.testing.assert_array_equal(bits(got[found]), bits(np.asarray(want)))
    got = loop(4, 10).centers(coordmin, coordmax, nx, ny)
    want = []
    for i in range(nx):
        for j in range(ny):
            curmin, curmax = K.window_box(coordmin, coordmax, i, j, 10, 4)
            want.append((curmin[0:2] + curmax[0:2]) / 2.0)  # as kitti_window_flow_ref.windows
    assert got.dtype == np.float64
    np.testing.assert_array_equal(bits(got), bits(np.asarray(want)))


def test_merge_is_the_scannet_restatements():
    centers = [np.array([x, 0.75]) for x in (0.75, 1.3, 1.75, 2.25, 2.8)]  # off the lattice: no equal distances
    sizes = [5000, 100, 4096, 9000, 10]
    want = R.merge(sizes, centers, 4096)
    assert want == [[0], [2, 1], [3, 4]]
    assert L.merge_blocks(sizes, centers, 4096, nearest=L.nearest_block_literal) == want
    rng = np.random.default_rng(0)
    centers = [np.array([0.31 + i * 0.5 + 0.75, -2.2 + j * 0.5 + 0.75]) for i in range(6) for j in range(5)]  # equal distances are the rule
    sizes = rng.integers(1, 9000, len(centers))
    want = R.merge(sizes, centers, 4096)
    assert 1 < len(want) < len(centers)
    assert L.merge_blocks(sizes, np.array(centers), 4096, nearest=L.nearest_block_literal) == want
    with pytest.raises(ValueError):
        L.merge_blocks([], [], 4096, nearest=L.nearest_block_literal)
    with pytest.raises(ValueError):
        L.merge_blocks([10, 20, 30], centers[:3], 4096, nearest=L.nearest_block_literal)


@pytest.mark.parametrize("length", [256, 300, 4097])
def test_both_row_draws_are_one(length):
    a, b = np.random.RandomState(0), np.random.RandomState(0)
    short, refused = L.draw_rows(length, 256, a, pad_short=True), L.draw_rows(length, 256, b)
    assert short.shape[0] % 256 == 0
    np.testing.assert_array_equal(short, refused)
    np.testing.assert_array_equal(short, R.draw_rows(length, 256, np.random.RandomState(0)))
    assert a.randint(1 << 30) == b.randint(1 << 30)


def test_a_make_up_longer_than_the_block_pads_short_or_raises():
    with pytest.raises(ValueError):
        L.draw_rows(100, 256, np.random.RandomState(0))
    a, b = np.random.RandomState(0), np.random.RandomState(0)
    got = L.draw_rows(100, 256, a, pad_short=True)
    assert got.shape == (200,)
    np.testing.assert_array_equal(got, R.draw_rows(100, 256, b))
    assert a.randint(1 << 30) == b.randint(1 << 30)


@pytest.mark.gpu
def test_pointer_takes_a_byte_offset():
    import torch

    from pointasnl_amd import _hip

    t = torch.zeros((4,), dtype=torch.int32, device="cuda")
    assert _hip.ptr(t).value == t.data_ptr() and _hip.ptr(t, 8).value == t.data_ptr() + 8
    assert _hip.ptr(None).value in (None, 0)
