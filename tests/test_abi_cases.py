"""tests/abi_cases.py before any GPU is involved: every entry point in scope has a case, every case is ragged against the
widths it declares, and every record is consistent with itself (shapes of the expected values, the symbols it says it calls)."""
import numpy as np
import pytest

import abi_cases as A

IDS = [c.id for c in A.CASES]


def test_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


def test_every_entry_point_in_scope_has_a_case():
    from pointasnl_amd import _hip

    scope = [s for s in _hip.SYMBOLS if A.in_scope(s)]
    assert len(scope) == 67, "a new symbol needs a case or a line in the exclusion list"
    missing = [s for s in scope if s not in A.covered()]
    assert not missing, missing
    # the exclusion list names symbols that exist, and no case needs one of them
    for s in list(A.EXCLUDED) + list(A.EXCLUDED_LOOP_ENTRIES):
        assert s in _hip.SYMBOLS, s
    assert not [s for s in A.covered() if not A.in_scope(s)]


@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_case_is_ragged_as_declared(case):
    assert case.ragged, "a case names the widths it is ragged against"
    for what, dim, width in case.ragged:
        assert dim > 0 and width > 1 and dim % width != 0, (what, dim, width)


@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_case_record_is_consistent(case):
    """the declared dimensions are dimensions of the call; outputs, states and expected values have one shape; the symbols a
    case calls beside its entry are the ones it lists"""
    built = case.built()
    ints = set()
    for a in built.args:
        if isinstance(a, (int, np.integer)):
            ints.add(int(a))
        elif isinstance(a, A.L):
            ints.add(int(a.v))
    products = set(ints)
    for o in built.outs:
        products.update(int(d) for d in o.shape)
        products.update(int(np.prod(o.shape[:i])) for i in range(1, len(o.shape) + 1))
    for a in ints:
        products.update({a + 3, a + 4, a + 6})
    products.update([3 * p for p in products])
    for what, dim, width in case.ragged:
        assert dim in products, (what, dim)
    uses = set()
    names = [o.name for o in built.outs]
    assert len(set(names)) == len(names)
    for o in built.outs:
        st = o.states()
        assert st.shape == tuple(o.shape) and set(np.unique(st)) <= {A.DEFINED, A.KEPT, A.UNSPECIFIED}
        if (st == A.DEFINED).any():
            want = built.want[o.name]
            if o.cmp != A.BF16X3:
                assert want.shape == tuple(o.shape), (o.name, want.shape, o.shape)
            if o.cmp == A.BITS:
                assert want.dtype == np.dtype(o.dtype), (o.name, want.dtype)
            else:
                assert np.isfinite(want[st == A.DEFINED] if o.cmp != A.BF16X3 else want).all()
        if o.bytes_fn:
            uses.add(o.bytes_fn)
    refs = [a.name for a in built.args if isinstance(a, A.Ref)]
    assert sorted(refs) == sorted(names), "every output is handed to the entry once"
    for a in built.args:
        if isinstance(a, A.Prep):
            uses.add(a.entry)
            assert sum(x is A.DST for x in a.args) == 1
            if a.bytes_fn:
                uses.add(a.bytes_fn)
    assert (built.ws is not None) == any(a is A.WS for a in built.args) == any(a is A.WSB for a in built.args)
    if built.ws:
        uses.add(built.ws[0])
    assert uses - {case.entry} == set(case.uses) - {case.entry}, (uses, case.uses)
    assert not case.no_ws or built.ws
