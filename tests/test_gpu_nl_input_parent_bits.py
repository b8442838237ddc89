"""The input-space non-local cell's forward (csrc/nl_input.hip) and fused backward (csrc/nl_input_grad.hip) after their shared
machinery -- staged stream, block step, query projection, key ranges, wave fold, split rule -- moved into csrc/nl_input_core.hpp:
nothing of their arithmetic changed, so every output must equal, bit for bit, what the commit before computed
(tests/golden/nl_input_core.npz, recorded by tests/golden/make_nl_input_core.py).  Both entry points sum in a fixed order without
atomics: the comparison is equality, no tolerance.

Per shape of tests/nl_input_core_cases.py: the digest of the forward's output and of each of the six gradients of one C-ABI call
with every output requested; a second run over different stale output and workspace bytes gives the same bytes; and on the two
ABI shapes the three subset calls (weights only, grad_feature only, grad_new_point only: the other `flags` paths) give the
parent's bits, which are the full call's."""
import os

import numpy as np
import pytest

import nl_cell_input_grad_ref as R
import nl_input_core_cases as C
from guarded import ALT_BYTE, ALT_WS_BYTE, NAN_BYTE, WS_BYTE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nl_input_core.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def full_runs():
    """the full call's gradients per shape, shared by the two tests"""
    return {}


def full_run(full_runs, shape):
    if shape not in full_runs:
        h, g = R.problem(*shape)
        full_runs[shape] = C.run_grad(shape, h, g, R.NAMES, NAN_BYTE, WS_BYTE)
    return full_runs[shape]


def show_rows(what, got, want):
    print(f"{what}: first / last query row\n  got  {got.tolist()}\n  want {want.tolist()}")


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_forward_and_full_backward_equal_the_parent(shape, golden, full_runs):
    h, g = R.problem(*shape)
    key = C.shape_id(shape) + "/"
    out, full = C.run_forward(shape, h, NAN_BYTE), full_run(full_runs, shape)
    # a pure function of the inputs, whatever the outputs and the workspace held
    assert C.run_forward(shape, h, ALT_BYTE).tobytes() == out.tobytes()
    again = C.run_grad(shape, h, g, R.NAMES, ALT_BYTE, ALT_WS_BYTE)
    for k in R.NAMES:
        assert again[k].tobytes() == full[k].tobytes(), k
    # the parent commit's bits
    rec = C.record(out, full, {})
    for name in ("out_rows", "grad_new_point_rows"):
        if not np.array_equal(rec[name], golden[key + name]):
            show_rows(f"{key}{name}", rec[name], golden[key + name])
    np.testing.assert_array_equal(rec["out_rows"], golden[key + "out_rows"])
    np.testing.assert_array_equal(rec["grad_new_point_rows"], golden[key + "grad_new_point_rows"])
    assert str(rec["out_sha256"]) == str(golden[key + "out_sha256"])
    for k in R.NAMES:
        assert str(rec[f"grad_{k}_sha256"]) == str(golden[key + f"grad_{k}_sha256"]), k


@pytest.mark.parametrize("subset", list(C.SUBSETS))
@pytest.mark.parametrize("shape", C.ABI_SHAPES, ids=C.shape_id)
def test_subset_calls_equal_the_parent_and_the_full_call(shape, subset, golden, full_runs):
    h, g = R.problem(*shape)
    full = full_run(full_runs, shape)
    need = C.SUBSETS[subset]
    got = C.run_grad(shape, h, g, need, NAN_BYTE, WS_BYTE)
    again = C.run_grad(shape, h, g, need, ALT_BYTE, ALT_WS_BYTE)
    assert set(got) == set(need)
    for k in need:
        assert again[k].tobytes() == got[k].tobytes(), k
        assert got[k].tobytes() == full[k].tobytes(), k
        assert C.digest(got[k]) == str(golden[f"{C.shape_id(shape)}/{subset}/grad_{k}_sha256"]), k
        assert str(golden[f"{C.shape_id(shape)}/{subset}/grad_{k}_sha256"]) == str(golden[f"{C.shape_id(shape)}/grad_{k}_sha256"]), k
