"""The AdaptiveSampling cell's forward (csrc/as_cell.hip) and fused backward (csrc/as_grad.hip) after their shared pieces -- the
key-major tile softmax, the narrow projection, the column softmax of the re-weighting tail, the 16-lane reductions, the grid
and scale rules -- moved into csrc/as_core.hpp: nothing of their arithmetic changed, so every output must equal, bit for bit,
what the commit before computed (tests/golden/as_core.npz, recorded by tests/golden/make_as_core.py).  Every entry sums in a
fixed order without atomics: the comparison is equality, no tolerance.

Per case of tests/as_core_cases.py: the digest of each output of one C-ABI call (the gradient entries: with every output
requested) and the end rows of the first in clear; a second run over different stale output and workspace bytes gives the same
bytes; and for the gradient entries every subset call (the other outputs NULL) gives the full call's bits."""
import os

import numpy as np
import pytest

import as_core_cases as C
from guarded import ALT_BYTE, ALT_WS_BYTE, NAN_BYTE, WS_BYTE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "as_core.npz")
GRAD_CASES = [case for case in C.CASES if C.SUBSETS.get(case[0])]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def full_runs():
    """the first run's outputs per case, shared by the two tests"""
    return {}


def full_run(full_runs, case):
    if case not in full_runs:
        full_runs[case] = C.run(case, NAN_BYTE, WS_BYTE)
    return full_runs[case]


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_every_output_equals_the_parent(case, golden, full_runs):
    outs = full_run(full_runs, case)
    # a pure function of the inputs, whatever the outputs and the workspace held
    again = C.run(case, ALT_BYTE, ALT_WS_BYTE)
    assert set(again) == set(outs)
    for k in outs:
        assert again[k].tobytes() == outs[k].tobytes(), k
    # the parent commit's bits
    rec, key = C.record(outs), C.case_id(case) + "/"
    if not np.array_equal(rec["rows"], golden[key + "rows"]):
        print(f"{key}{sorted(outs)[0]}: first / last row\n  got  {rec['rows'].tolist()}\n  want {golden[key + 'rows'].tolist()}")
    np.testing.assert_array_equal(rec["rows"], golden[key + "rows"])
    assert rec["sha256"].shape == golden[key + "sha256"].shape
    for name, got, want in zip(sorted(outs), rec["sha256"], golden[key + "sha256"]):
        assert got == want, name


@pytest.mark.parametrize("case", GRAD_CASES, ids=C.case_id)
def test_subset_calls_equal_the_full_call(case, full_runs):
    full = full_run(full_runs, case)
    for need in C.SUBSETS[case[0]].values():
        got = C.run(case, NAN_BYTE, WS_BYTE, need)
        again = C.run(case, ALT_BYTE, ALT_WS_BYTE, need)
        assert set(got) == set(need)
        for k in need:
            assert again[k].tobytes() == got[k].tobytes(), k
            assert got[k].tobytes() == full[k].tobytes(), k  # (which the first test holds to the parent's digest)
