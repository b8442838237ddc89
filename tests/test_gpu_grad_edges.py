"""The backward of gather_point / group_point / three_interpolate (include/pasnl.h: "Deterministic backward of ..."; grad_det,
grad_lists_kernel and grad_segsum_kernel of csrc/grouping.hip) on the branches the shapes of test_gpu_ops.py never take: scan
ownership of more than one target per thread, the 64-at-a-time walk at and next to its round boundaries, a second and third slab of
512 channels; and the lines of the header nothing else holds it to: out-of-range indices are ignored, every destination row is
written and nothing beside it, the workspace is exactly pasnl_grad_workspace_bytes, 38400 targets are the limit and 38401 are
refused before any launch.  Then the atomic variants of all three operators.

tests/grad_edge_cases.py restates the host arithmetic with the constants of grouping.hip and builds the inputs; every case names the
branch it is meant for and asserts that the restated arithmetic puts it there before anything is launched.  The reference of every
deterministic comparison is the oracle's sequential fp32 loop, compared as bit patterns; the one tolerance in this module is the
derived bound of an fp32 sum in any order, for the atomic variants on long lists (tests/test_grad_edge_cases.py holds the
oracle's own sums to it)."""
import ctypes

import numpy as np
import pytest
import torch

import grad_edge_cases as E
from guarded import GUARD, NAN_BYTE, WS_BYTE, Guarded  # noqa: F401

pytestmark = pytest.mark.gpu

OPS = ["gather", "group", "interp"]


@pytest.fixture(scope="module")
def P():
    import pointasnl_amd

    return pointasnl_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------------------------------------
# the two ways in: the autograd functions of the Python mirror, and the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def backward(P, case):
    """the gradient of a case through the mirror's autograd function (valid indices only: the forward gathers with them)"""
    assert case.valid().all()
    x = torch.zeros((case.b, case.n, case.c), dtype=torch.float32, device="cuda", requires_grad=True)
    if case.op == "gather":
        out = P.tf_sampling.gather_point(x, dev(case.idx))
    elif case.op == "group":
        out = P.tf_grouping.group_point(x, dev(case.idx))
    else:
        out = P.tf_interpolate.three_interpolate(x, dev(case.idx), dev(case.w))
    out.backward(dev(case.g))
    return x.grad.cpu().numpy()


ENTRY = {"gather": ("pasnl_gather_point_grad_det", "pasnl_gather_point_grad"),
         "group": ("pasnl_group_point_grad_det", "pasnl_group_point_grad"),
         "interp": ("pasnl_three_interpolate_grad_det", "pasnl_three_interpolate_grad")}


def abi_dims(op, b, targets, c, shape):
    """the integer arguments of an entry; shape = (m,) | (m, nsample) | (n_unknown, 3)"""
    if op == "gather":
        return (b, targets, shape[0])
    if op == "group":
        return (b, targets, c, shape[0], shape[1])
    return (b, shape[0], c, targets)


def entries_of(op, shape):
    return shape[0] if op == "gather" else shape[0] * shape[1]


def ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else 0 if t is None else t.data_ptr())


def call(op, dims, g, idx, w, dst, ws=None, ws_bytes=None):
    """one call of the C ABI on torch's current stream -> status.  ws_bytes None: the atomic entry."""
    from pointasnl_amd import _hip

    fn = getattr(_hip.lib(), ENTRY[op][0 if ws_bytes is not None else 1])
    args = list(dims) + [ptr(g), ptr(idx)] + ([ptr(w)] if op == "interp" else []) + [ptr(dst)]
    if ws_bytes is not None:
        args += [ptr(ws), ctypes.c_size_t(ws_bytes)]
    return fn(*args, _hip.stream_ptr())


def lib_workspace_bytes(b, targets, entries):
    from pointasnl_amd import _hip

    return int(_hip.lib().pasnl_grad_workspace_bytes(int(b), int(targets), ctypes.c_long(int(entries))))


def run_abi(case, det=True, ws_bytes=None):
    """a case through the C ABI: destination inside a NaN-filled buffer, workspace a view of exactly pasnl_grad_workspace_bytes
    bytes inside a patterned one -> (status, gradient, destination, workspace)"""
    shape = case.idx.shape[1:]
    dims = abi_dims(case.op, case.b, case.n, case.c, shape)
    g, idx, w = dev(case.g), dev(case.idx), dev(case.w) if case.w is not None else None
    dst = Guarded(4 * case.b * case.n * case.c, NAN_BYTE)
    assert np.isnan(dst.floats((-1,))).all()
    if det:
        nbytes = lib_workspace_bytes(case.b, case.n, case.entries)
        assert nbytes == E.workspace_bytes(case.b, case.n, case.entries)
        ws = Guarded(nbytes, WS_BYTE)
        status = call(case.op, dims, g, idx, w, dst.ptr, ws.ptr, nbytes if ws_bytes is None else ws_bytes)
    else:
        ws = None
        status = call(case.op, dims, g, idx, w, dst.ptr)
    torch.cuda.synchronize()
    return status, dst.floats((case.b, case.n, case.c)), dst, ws


# ---------------------------------------------------------------------------------------------------------------------------
# 1. scan ownership: per = ceil(targets / 1024) targets per thread of grad_lists_kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["gather", "group"])
@pytest.mark.parametrize("n", list(E.SCAN))
def test_scan_ownership(P, n, op):
    """per = 1 | 2 | 3 | 8 | 10 | 38: a second and later iteration of the loops over j < per; `t < n` false in the middle of the
    last owner's range (1025, 2047, 38399, 38400); st[n] written by a thread whose whole range lies beyond n (1023, 1025, 2049,
    38399, 38400).  A block of targets without contributions lies across two threads' ranges and two waves' partial sums."""
    assert E.accepted(n) and E.scan_owner(n) == E.SCAN[n]
    case = E.scan_case(op, n)
    assert case.b == 2 and case.n == n
    got = backward(P, case)
    assert_bits(got, case.want)
    for i, lo in enumerate(case.note["zero_block"]):
        assert (bits(got[i, lo:lo + E.ZERO_BLOCK]) == 0).all()


@pytest.mark.parametrize("m", list(E.SCAN_INTERP))
def test_scan_ownership_three_interpolate(P, m):
    """the weighted form (rep = 3) onto 1025 and 2049 known points, indices and weights of a real three_nn / three_weights"""
    assert E.accepted(m) and E.scan_owner(m) == E.SCAN_INTERP[m] and E.per(m) >= 2
    case = E.scan_interp_case(m)
    got = backward(P, case)
    assert_bits(got, case.want)
    assert (bits(got[case.counts() == 0]) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. round boundaries of the list walk
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_round_boundaries(P, op):
    """Lists of exactly 0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200 and 1000 contributions, their positions shuffled over the whole
    range (slot order != ascending order), another assignment in the second cloud; contribution e = 0 sits in the list of 1000,
    whose later rounds start from `prev`.  gather_point uses 3 of a wave's 64 lanes, the other two 70 channels (two 64-channel
    registers of the slab); three_interpolate is the weighted form.  Twice: run-to-run identical."""
    assert tuple(E.rounds(length) for length in E.LENGTHS) == E.ROUNDS == (0, 1, 1, 1, 1, 1, 2, 2, 2, 3, 4, 16)
    case = E.round_case(op)
    counts = case.counts()
    for i in range(case.b):
        assert sorted(counts[i][counts[i] > 0]) == sorted(E.LENGTHS[1:])
    assert counts[0, case.flat_idx()[0, 0]] > E.ROUND and E.slabs(case.c) == 1
    got = backward(P, case)
    assert_bits(got, case.want)
    assert_bits(backward(P, case), got)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. channel slabs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["group", "interp"])
@pytest.mark.parametrize("c", list(E.SLAB_C))
def test_channel_slabs(P, c, op):
    """c on both sides of a lane row (63 | 64 | 65) and of the slab (511 | 512 | 513), and three slabs (1025): the loop over c0
    runs a second and a third time, each with `first` and `prev` of its own over lists of 65 and 129 (two and three rounds)."""
    assert E.slabs(c) == E.SLAB_C[c] and [E.slabs(x) for x in E.SLAB_C] == [1, 1, 1, 1, 1, 1, 2, 3]
    case = E.slab_case(op, c)
    counts = case.counts()
    assert case.n == 40 and all(65 in counts[i] and 129 in counts[i] for i in range(case.b))
    assert E.rounds(65) == 2 and E.rounds(129) == 3
    assert_bits(backward(P, case), case.want)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. out-of-range indices (deterministic entries only: the atomic ones do not check bounds, like the reference)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_out_of_range_indices_are_ignored(op):
    """A tenth of the indices is one of -1, n, n + 1, 2^31 - 1, -2^31: the valid contributions keep their order, so every row is
    the oracle's on n + 1 targets with the invalid ones redirected to the row that is dropped.  One target loses every
    contribution (an exact zero row); a whole cloud has no valid index (all zeros, st[n] = 0)."""
    case = E.oob_case(op)
    valid, counts = case.valid(), case.counts()
    assert set(np.unique(case.flat_idx()[~valid])) == set(E.invalid_values(case.n))
    assert valid[:2].any() and not valid[2].any() and counts.max() > 2 * E.ROUND
    status, got, dst, ws = run_abi(case)
    assert status == E.OK
    assert_bits(got, case.want)
    for i, t in enumerate(case.note["victim"]):
        assert counts[i, t] == 0 and (bits(got[i, t]) == 0).all()
    assert (bits(got[2]) == 0).all()
    assert dst.guards_intact() and ws.guards_intact()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. every row written, nothing else
# ---------------------------------------------------------------------------------------------------------------------------
def written_case(op, kind):
    if kind == "lists":
        return E.round_case(op)
    return E.scan_interp_case(2049) if op == "interp" else E.scan_case(op, 2049)


@pytest.mark.parametrize("kind", ["per3", "lists"])
@pytest.mark.parametrize("op", OPS)
def test_every_row_written_and_nothing_else(op, kind):
    """Destination and workspace are views inside larger buffers: no NaN is left in the destination (no memset needed), the bytes
    in front of and behind both views keep their pattern -- with a workspace of exactly pasnl_grad_workspace_bytes bytes."""
    case = written_case(op, kind)
    if kind == "per3":
        assert E.per(case.n) == 3 and (case.counts() == 0).any()
    else:
        assert case.counts().max() == 1000 and E.rounds(1000) == 16
    status, got, dst, ws = run_abi(case)
    assert status == E.OK
    assert not np.isnan(got).any()
    assert_bits(got, case.want)
    assert dst.guards_intact() and ws.guards_intact()


@pytest.mark.parametrize("op,shape", [("gather", (0,)), ("group", (0, 5)), ("group", (5, 0)), ("interp", (0, 3))])
def test_no_contributions_gives_zero_rows(op, shape):
    """m = 0 / nsample = 0 / n = 0: entries == 0.  Every row is written (zeros), no source pointer is needed, status 0."""
    b, n, c = 2, 2049, 3 if op == "gather" else 5
    assert entries_of(op, shape) == 0 and E.per(n) == 3
    nbytes = lib_workspace_bytes(b, n, 0)
    assert nbytes == E.workspace_bytes(b, n, 0) == 4 * b * (n + 1)
    dst, ws = Guarded(4 * b * n * c, NAN_BYTE), Guarded(nbytes, WS_BYTE)
    status = call(op, abi_dims(op, b, n, c, shape), None, None, None, dst.ptr, ws.ptr, nbytes)
    torch.cuda.synchronize()
    assert status == E.OK
    assert (bits(dst.floats((b, n, c))) == 0).all()
    assert dst.guards_intact() and ws.guards_intact()


@pytest.mark.parametrize("op", OPS)
def test_no_clouds_touches_nothing(op):
    """b = 0: status 0, neither destination nor workspace is written"""
    case = E.distinct_case(op)
    g, idx, w = dev(case.g), dev(case.idx), dev(case.w) if case.w is not None else None
    dst, ws = Guarded(4 * case.n * case.c, NAN_BYTE), Guarded(1024, WS_BYTE)
    assert lib_workspace_bytes(0, case.n, case.entries) == 0
    status = call(op, abi_dims(op, 0, case.n, case.c, case.idx.shape[1:]), g, idx, w, dst.ptr, ws.ptr, 1024)
    torch.cuda.synchronize()
    assert status == E.OK and dst.untouched() and ws.untouched()


def test_workspace_bytes():
    """pasnl_grad_workspace_bytes(b, t, e) == 4 * (b * (t + 1) + b * e): start[b][t + 1] and list[b][e]; 0 for non-positive b or t"""
    for b, t, e in [(1, 1, 0), (2, 2049, 512), (2, 38400, 9600), (3, 16, 1782), (64, 1024, 3 * 8192), (1, 38400, 2 ** 31 - 1)]:
        assert lib_workspace_bytes(b, t, e) == E.workspace_bytes(b, t, e) == 4 * (b * (t + 1) + b * e)
    for b, t, e in [(0, 16, 4), (-1, 16, 4), (2, 0, 4), (2, -5, 4), (0, 0, 0)]:
        assert lib_workspace_bytes(b, t, e) == E.workspace_bytes(b, t, e) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------
CANARY = -7.0


def negative_count(op, shape):
    return {"gather": (-1,), "group": (shape[0], -1), "interp": (-1, 3)}[op]


@pytest.mark.parametrize("kind,want", [("workspace", E.EWORKSPACE), ("targets", E.EUNSUPPORTED), ("negative", E.EINVAL)])
@pytest.mark.parametrize("op", OPS)
def test_refusals(op, kind, want):
    """One byte less workspace than pasnl_grad_workspace_bytes: PASNL_EWORKSPACE.  38401 targets (38400 run in
    test_scan_ownership): PASNL_EUNSUPPORTED.  A negative count: PASNL_EINVAL.  Each before any launch -- the destination keeps its
    canary -- and the next valid call is correct."""
    case = E.distinct_case(op)
    shape = case.idx.shape[1:]
    g, idx, w = dev(case.g), dev(case.idx), dev(case.w) if case.w is not None else None
    n = E.MAX_TARGETS + 1 if kind == "targets" else case.n
    assert E.accepted(n) == (kind != "targets") and E.accepted(E.MAX_TARGETS)
    # destination and workspace are large enough for the call as stated: a call that is wrongly accepted stays inside them
    nbytes = lib_workspace_bytes(case.b, n, case.entries)
    assert nbytes == E.workspace_bytes(case.b, n, case.entries) > 0
    dst = torch.full((case.b, n, case.c), CANARY, dtype=torch.float32, device="cuda")
    ws = torch.full((nbytes,), WS_BYTE, dtype=torch.uint8, device="cuda")
    dims = abi_dims(op, case.b, n, case.c, negative_count(op, shape) if kind == "negative" else shape)
    status = call(op, dims, g, idx, w, dst, ws, nbytes - 1 if kind == "workspace" else nbytes)
    torch.cuda.synchronize()
    assert status == want
    assert bool((dst == CANARY).all()) and bool((ws == WS_BYTE).all())
    status, got, _, _ = run_abi(case)
    assert status == E.OK
    assert_bits(got, case.want)


def test_mirror_refuses_38401_targets(P):
    """gather_point over 38401 points: the forward runs, the backward raises PasnlUnsupported; 38400 is test_scan_ownership's"""
    from pointasnl_amd import _hip

    n = E.MAX_TARGETS + 1
    assert not E.accepted(n) and E.accepted(n - 1)
    x = torch.zeros((1, n, 3), dtype=torch.float32, device="cuda", requires_grad=True)
    out = P.tf_sampling.gather_point(x, dev(np.array([[0, 5, n - 1, 5]], np.int32)))
    with pytest.raises(_hip.PasnlUnsupported, match="GatherPointGrad"):
        out.backward(torch.ones_like(out))
    case = E.distinct_case("gather")
    assert_bits(backward(P, case), case.want)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the atomic variants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_atomic_variants_distinct_targets(op):
    """No target has more than one contribution (idx a partial permutation, three-neighbour indices distinct over the cloud): a
    row is one term, so the atomic entries give the oracle's bits; rows without contribution are the entry's own memset, from a
    NaN-filled destination."""
    case = E.distinct_case(op)
    counts = case.counts()
    assert counts.max() == 1 and (counts == 0).any()
    status, got, dst, _ = run_abi(case, det=False)
    assert status == E.OK
    assert not np.isnan(got).any() and (bits(got[counts == 0]) == 0).all()
    assert_bits(got, case.want)
    assert dst.guards_intact()


@pytest.mark.parametrize("op", OPS)
def test_atomic_variants_long_lists(P, op):
    """The lists of test_round_boundaries through the atomic entries (the mirror with DETERMINISTIC_GRADS off): per element
    |got - s64| <= gamma(L) * sum |term|, L the row's list length, s64 the fp64 sum of the same fp32 terms (for three_interpolate
    the fp32 product g * w, which IS float64(g) * float64(w) rounded: the library is built without contraction and an atomic add
    has no product to contract with), gamma(L) = L u / (1 - L u), u = 2^-24 -- the bound of an fp32 sum in any order."""
    from pointasnl_amd import _hip

    case = E.round_case(op)
    counts = case.counts()
    assert counts.max() == 1000 and abs(E.gamma(1000) - 1000 * 2.0 ** -24) < 1e-8
    bound, s64 = E.fp64_sums_and_bounds(case)
    _hip.DETERMINISTIC_GRADS = False
    try:
        got = backward(P, case)
    finally:
        _hip.DETERMINISTIC_GRADS = True
    assert got.dtype == np.float32 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - s64)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"atomic {op}: largest |got - s64| / bound = {worst:.3g}")
    assert (err <= bound).all()
    assert (bits(got[counts == 0]) == 0).all()
    assert_bits(got[counts == 1], case.want[counts == 1])
    assert_bits(backward(P, case), case.want)  # and the switch is back: the ordered sums again
