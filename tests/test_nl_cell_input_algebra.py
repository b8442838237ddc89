"""The non-local cell attended in input space (csrc/nl_input.hip), checked on the CPU: a numpy mirror of the kernel's order of
operations (tests/nl_cell_input_ref.py: fp32, a key range per wave, blocks of 16 keys, online rescale, merge of the ranges)
against oracle.cells' cell in fp64, at DESIGN 5's atol = rtol = 1e-5.  n = 1 is the case in which a softmax over one key is 1
whatever the score: the result is then V_0 exactly, so the Q . bk term the input-space form drops cannot be missed."""
import numpy as np
import pytest

import nl_cell_input_ref as R
from oracle import cells

SHAPES = [(3, 260, 700, 3, 6, 32), (2, 77, 333, 6, 9, 64), (1, 5, 1, 3, 6, 32)]


@pytest.mark.parametrize("shape", SHAPES)
def test_mirror_of_the_kernel_order_matches_the_fp64_cell(shape):
    b, p, n, c, cz, cb = shape
    h = R.problem(*shape)
    want = R.restated(h, cb)
    # the whole cell as oracle.cells.point_nonlocal_cell states it, with an identity back-projection: relu of the above
    g = {k: v.astype(np.float64) for k, v in h.items()}
    params = {"s/conv_kv": {"w": g["wkv"], "b": g["bkv"]}, "s/conv_query": {"w": g["wq"], "b": g["bq"]},
              "s/conv_back_project": {"w": np.eye(cb), "b": np.zeros(cb)}}
    cell = cells.point_nonlocal_cell(g["feature"], g["new_point"], [cb, cb], params, "s")
    np.testing.assert_allclose(cell, np.maximum(want, 0), rtol=1e-12, atol=1e-12)
    for split in sorted({R.split_of(b, p, n, c), 4, 8, 16}):
        got = R.mirror(h, cb, split)
        print(f"{shape} split {split}: worst error / bound = {R.worst_ratio(got, want):.4f}")
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(np.maximum(got, 0), cell, rtol=1e-5, atol=1e-5)


def test_one_key_gives_its_value_row_whatever_the_score():
    shape = (1, 5, 1, 3, 6, 32)
    h = R.problem(*shape)
    v0 = h["feature"][0, 0].astype(np.float64) @ h["wkv"][:, 32:].astype(np.float64) + h["bkv"][32:]
    np.testing.assert_allclose(R.restated(h, 32), np.broadcast_to(v0, (1, 5, 32)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.mirror(h, 32, 4), np.broadcast_to(v0, (1, 5, 32)), rtol=1e-5, atol=1e-5)


def test_split_rule_on_the_reference_shapes():
    assert R.split_of(64, 512, 1024, 3) == 4     # classifier layer 1: 2048 waves
    assert R.split_of(16, 1024, 8192, 3) == 8    # ScanNet layer 1: 2048 waves
    assert R.split_of(8, 1280, 10240, 3) == 16   # SemanticKITTI: 2560 waves
    assert R.split_of(1, 64, 3, 3) == 4 and R.split_of(1, 64, 600, 3) == 8 and R.split_of(1, 10, 2100, 5) == 8
