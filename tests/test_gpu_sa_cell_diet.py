"""The persistent set-abstraction cells (pasnl_sa_cell on xyz-only rows, pasnl_sa_cell_pre) after their loads, waits and
skip-maxima folds were re-ordered: nothing of their arithmetic changed, so every output must equal, bit for bit, what the commit
before computed (tests/golden/sa_cell_diet.npz, recorded by tests/golden/make_sa_cell_diet.py), and stay within 1e-5 of the
output scale of the fp64 restatement in oracle/cells.py, with skip maxima and centre outputs exact.

Cases (tests/sa_cell_diet_cases.py): the 128-channel pre-projected cell with two tiles per group, a 64-channel one with a ragged
last wave and one that takes the XCD map, a one-chunk row, two with more groups than resident waves (linear and XCD map), index
tables whose neighbours are all one point or whose neighbour 0 is the last row of its cloud; the xyz-only 64-channel cell with
fewer groups than one workgroup stride, with 528 groups, with several groups per wave, and with the XCD map.  Each in both
centre forms, each run twice over different stale bytes in guarded output views."""
import os

import numpy as np
import pytest

import sa_cell_diet_cases as C
from guarded import ALT_BYTE, NAN_BYTE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sa_cell_diet.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def reference():
    """inputs and the fp64 oracle of every case, computed once"""
    out = {}
    for case in C.CASES:
        d = C.inputs(case)
        out[case] = (d, C.oracle(case, d))
    return out


@pytest.mark.parametrize("centre0", [False, True], ids=["table", "centre0"])
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_cell_against_parent_and_oracle(case, centre0, golden, reference):
    d, (want, want_skip, want_nf) = reference[case]
    r = C.run(case, d, centre0, NAN_BYTE)
    again = C.run(case, d, centre0, ALT_BYTE)
    # nothing outside the views, and nothing of the stale bytes inside them
    assert r.guards and again.guards
    assert r.out.tobytes() == again.out.tobytes() and r.skip.tobytes() == again.skip.tobytes()
    # skip maxima, centres and neighbour 0's rows: exact
    np.testing.assert_array_equal(r.skip, want_skip)
    if centre0:
        assert r.cen.tobytes() == again.cen.tobytes() and r.nf.tobytes() == again.nf.tobytes()
        np.testing.assert_array_equal(r.cen, d["centres"])
        np.testing.assert_array_equal(r.nf, want_nf)
    # the fp64 oracle, at the form's tolerance
    scale = np.abs(want).max()
    err = np.abs(r.out - want).max() / scale
    print(f"{C.case_id(case)} centre0={centre0}: rel err {err:.3e}")
    assert err < 1e-5
    # the parent commit's bits
    key = f"{C.case_id(case)}/{'centre0' if centre0 else 'table'}/"
    rec = C.record(case, r, centre0)
    assert str(rec["skip_sha256"]) == str(golden[key + "skip_sha256"])
    if not centre0:
        np.testing.assert_array_equal(rec["out_groups"].view(np.uint32), golden[key + "out_groups"].view(np.uint32))
    assert str(rec["out_sha256"]) == str(golden[key + "out_sha256"])
    # and the other centre form's (recorded with its own digest; the same bits)
    assert str(golden[f"{C.case_id(case)}/table/out_sha256"]) == str(golden[f"{C.case_id(case)}/centre0/out_sha256"])


def test_centre_forms_agree(reference):
    """the centres a group reads from its own tile are the table's: the same bits from both entries"""
    for case in (C.CASES[0], next(c for c in C.CASES if c[0] == "xyz3")):
        d, _ = reference[case]
        a, b = C.run(case, d, False, NAN_BYTE), C.run(case, d, True, NAN_BYTE)
        assert a.out.tobytes() == b.out.tobytes() and a.skip.tobytes() == b.skip.tobytes()
