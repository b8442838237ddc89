"""CPU side of tests/test_gpu_grad_edges.py: the restated host arithmetic of the deterministic backward (csrc/grouping.hip:
grad_det, grad_lists_kernel, grad_segsum_kernel) on the shapes the GPU module runs, and that those inputs can tell a right kernel
from a wrong one -- a sum taken in another order than the sequential loop's has other bits.  Oracle and numpy alone."""
import numpy as np
import pytest

import grad_edge_cases as E

CASES = E.list_cases()


def test_restated_arithmetic():
    assert E.GL_THREADS == 1024 and E.ROUND == 64 and E.SLAB == 512
    # the limit: n * 4 <= 150 * 1024
    assert E.MAX_TARGETS == 38400 and E.accepted(38400) and not E.accepted(38401)
    # scan ownership
    assert [E.per(n) for n in E.SCAN] == [1, 1, 2, 2, 2, 3, 8, 10, 38, 38]
    for n, want in {**E.SCAN, **E.SCAN_INTERP}.items():
        p, last, owned, idle = E.scan_owner(n)
        assert (p, last, owned, idle) == want
        assert last * p + owned == n and 1 <= owned <= p and last + idle == E.GL_THREADS - 1
    assert E.scan_owner(1025)[1:] == (512, 1, 511)      # thread 512 owns target 1024 alone
    assert E.scan_owner(38400)[1:] == (1010, 20, 13)    # thread 1010 owns the last 20, threads 1011..1023 nothing
    # the cases cover: a last thread with a partial range, a last thread with a full one, thread 1023 with and without targets
    assert {E.SCAN[n][2] < E.SCAN[n][0] for n in E.SCAN if E.SCAN[n][0] > 1} == {True, False}
    assert {E.SCAN[n][3] > 0 for n in E.SCAN} == {True, False}
    # rounds and slabs
    assert tuple(E.rounds(length) for length in E.LENGTHS) == E.ROUNDS
    assert [E.rounds(length) for length in (64, 65, 128, 129)] == [1, 2, 2, 3]
    assert [E.slabs(c) for c in E.SLAB_C] == [1, 1, 1, 1, 1, 1, 2, 3] == list(E.SLAB_C.values())
    # workspace
    assert E.workspace_bytes(2, 38400, 9600) == 4 * (2 * 38401 + 2 * 9600)
    assert E.workspace_bytes(3, 7, 0) == 4 * 3 * 8
    assert E.workspace_bytes(0, 7, 5) == E.workspace_bytes(-1, 7, 5) == E.workspace_bytes(2, 0, 5) == E.workspace_bytes(2, -3, 5) == 0


def test_gradient_generator_spans_four_decades():
    g = E.grads(np.random.default_rng(0), (4000,))
    assert g.dtype == np.float32 and np.isfinite(g).all()
    mag = np.log10(np.abs(g[g != 0]))
    assert (mag < -1.5).mean() > 0.1 and (mag > 1.5).mean() > 0.05


@pytest.mark.parametrize("name", list(CASES))
def test_lists_are_the_oracles_and_order_sensitive(name):
    """The helper's view of a case (contribution e adds terms()[e] to target flat_idx()[e]) summed in ascending e IS the oracle's
    row, bit for bit; summed in descending order, or in a fixed random order (what a kernel that forgot to sort its slots would
    do), it is not: for EVERY row with 8 or more contributions and for at least half of the rows with 3 to 7."""
    case = CASES[name]()
    want = case.want
    assert want.shape == (case.b, case.n, case.c) and want.dtype == np.float32
    counts = case.counts()
    assert (want[counts == 0] == 0).all()  # exact zeros (+0.0 == -0.0: the bits are compared below)
    assert (want[counts == 0].view(np.uint32) == 0).all()
    rows = E.order_sensitivity(case, min_len=1)
    assert len(rows) == (counts > 0).sum()
    for i, t, length, asc, _, _ in rows:
        assert counts[i, t] == length
        np.testing.assert_array_equal(asc.view(np.uint32), want[i, t].view(np.uint32))
    long_rows = [(d, p) for _, _, length, _, d, p in rows if length >= 8]
    short_rows = [(d, p) for _, _, length, _, d, p in rows if 3 <= length <= 7]
    assert all(d for d, _ in long_rows) and all(p for _, p in long_rows)
    if short_rows:
        assert 2 * sum(d for d, _ in short_rows) >= len(short_rows)
        assert 2 * sum(p for _, p in short_rows) >= len(short_rows)


@pytest.mark.parametrize("op", ["gather", "group"])
@pytest.mark.parametrize("n", list(E.SCAN))
def test_scan_cases(op, n):
    case = E.scan_case(op, n)
    assert case.b == 2 and case.n == n and case.entries == (n // 4 if op == "gather" else 64 * 32)
    p = E.per(n)
    counts = case.counts()
    for i, lo in enumerate(case.note["zero_block"]):
        # no contribution inside the block, some on both sides of it, and the block lies across two threads' ranges
        assert (counts[i, lo:lo + E.ZERO_BLOCK] == 0).all() and counts[i, :lo].sum() > 0 and counts[i, lo + E.ZERO_BLOCK:].sum() > 0
        assert lo // p < (lo + E.ZERO_BLOCK - 1) // p
        assert ((lo + 2) // p) % 64 == 0 and (lo + 2) % p == 0  # ... the second one lane 0 of a wave
    assert case.valid().all() and counts.sum() == 2 * case.entries


@pytest.mark.parametrize("m", list(E.SCAN_INTERP))
def test_scan_interp_cases(m):
    case = E.scan_interp_case(m)
    assert case.n == m and case.entries == 2100 and case.valid().all()
    assert (case.w > 0).all() and (case.counts() == 0).any() and case.counts().max() >= 3


@pytest.mark.parametrize("op", ["gather", "group", "interp"])
def test_round_cases(op):
    case = E.round_case(op)
    counts = case.counts()
    np.testing.assert_array_equal(counts, case.note["lengths"])
    for i in range(2):
        assert sorted(counts[i]) == sorted(list(E.LENGTHS) + [0] * 4)
    assert (counts[0] != counts[1]).any()                      # another assignment in the second cloud
    flat = case.flat_idx()
    assert counts[0, flat[0, 0]] == 1000                      # e = 0 in a list longer than one round
    for i in range(2):                                         # positions shuffled over the whole range: every long list
        for t in np.nonzero(counts[i] >= 63)[0]:               # reaches into the first and the last tenth of it
            e = np.nonzero(flat[i] == t)[0]
            assert e.min() < case.entries // 10 and e.max() > case.entries - case.entries // 10
            assert (np.diff(e) > 1).any()
    if op == "interp":
        assert case.idx.shape == (2, 594, 3) and (case.w > 0).all()


@pytest.mark.parametrize("op", ["group", "interp"])
@pytest.mark.parametrize("c", list(E.SLAB_C))
def test_slab_cases(op, c):
    case = E.slab_case(op, c)
    counts = case.counts()
    assert case.n == 40 and case.c == c and E.slabs(c) == E.SLAB_C[c]
    for i in range(2):
        assert 65 in counts[i] and 129 in counts[i]
    assert E.rounds(65) == 2 and E.rounds(129) == 3


@pytest.mark.parametrize("op", ["gather", "group", "interp"])
def test_out_of_range_cases(op):
    case = E.oob_case(op)
    n, flat, valid, counts = case.n, case.flat_idx(), case.valid(), case.counts()
    assert set(np.unique(flat[~valid])) == set(E.invalid_values(n))
    for i in (0, 1):
        assert 0.08 < (~valid[i]).mean() < 0.35
        assert counts[i, case.note["victim"][i]] == 0 and (case.want[i, case.note["victim"][i]] == 0).all()
        assert counts[i].max() > 128
    assert not valid[2].any() and (case.want[2] == 0).all()
    # the redirect changes nothing where every index is valid: dropping the invalid contributions by hand gives the same rows
    terms = case.terms()
    for i in (0, 1):
        for t, e in zip(*case.lists(i)):
            np.testing.assert_array_equal(E.seq_sum(terms[i, e]).view(np.uint32), case.want[i, t].view(np.uint32))


@pytest.mark.parametrize("op", ["gather", "group", "interp"])
def test_distinct_cases(op):
    case = E.distinct_case(op)
    counts = case.counts()
    assert counts.max() == 1 and (counts == 0).any() and case.valid().all()


@pytest.mark.parametrize("op", ["gather", "group", "interp"])
def test_gamma_bound_holds_for_the_oracles_own_sums(op):
    """|fl(sum) - sum| <= gamma(L) * sum |term| for an fp32 sum of L terms in ANY order: what the GPU module asks of the atomic
    variants holds for the sequential loop as well, and it is no empty bound -- the order does matter at this size."""
    case = E.round_case(op)
    bound, s64 = E.fp64_sums_and_bounds(case)
    err = np.abs(case.want.astype(np.float64) - s64)
    assert (err <= bound).all()
    assert (bound[case.counts() == 0] == 0).all()
    assert err.max() > 0
