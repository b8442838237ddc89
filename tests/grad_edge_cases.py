"""Inputs and restated host arithmetic for the backward of gather_point / group_point / three_interpolate
(csrc/grouping.hip: grad_det -> grad_lists_kernel + grad_segsum_kernel).  Plain numpy + the oracle: no GPU, no torch.

Shared by tests/test_grad_edge_cases.py (CPU: the restated arithmetic, and that the inputs can tell a right kernel from a wrong
one) and tests/test_gpu_grad_edges.py (GPU: the kernels against the oracle, bit for bit).

A `Case` is one call of one operator seen as the kernels see it: `b` clouds, `n` TARGET rows per cloud (the rows of the
gradient), `entries` CONTRIBUTIONS per cloud, contribution e of cloud i adding the term row `terms()[i, e]` to target
`flat_idx()[i, e]`.  (targets, contributions) = (n, m) for gather_point, (n, m*nsample) for group_point, (m, 3*n) for
three_interpolate, whose term is the fp32 product grad_out[e // 3] * weight[e]."""
import dataclasses
import functools
import zlib

import numpy as np

from oracle import ops as O
from oracle import ref

# ---------------------------------------------------------------------------------------------------------------------------
# the host arithmetic of grad_det / grad_lists_kernel / grad_segsum_kernel, restated (constants of csrc/grouping.hip)
# ---------------------------------------------------------------------------------------------------------------------------
GL_THREADS = 1024                   # grad_lists_kernel: threads of the one workgroup a cloud gets
ROUND = 64                          # grad_segsum_kernel: contributions consumed per walk over a list ("64 smallest at a time")
CH = 8                              # grad_segsum_kernel: 64-channel slabs accumulated per walk
SLAB = CH * 64                      # channels per pass of the loop over c0
LDS_HISTOGRAM_BYTES = 150 * 1024    # grad_det: n * sizeof(int) <= 150 * 1024
MAX_TARGETS = LDS_HISTOGRAM_BYTES // 4

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -3, -5  # include/pasnl.h


def accepted(n):
    """grad_det's PASNL_EUNSUPPORTED test on the targets of a cloud"""
    return n * 4 <= LDS_HISTOGRAM_BYTES


def per(n):
    """targets owned by every thread of grad_lists_kernel's scan: thread t owns [t * per, t * per + per)"""
    return (n + GL_THREADS - 1) // GL_THREADS


def scan_owner(n):
    """(per, the thread that owns the last target, how many targets it owns, how many threads behind it own nothing)"""
    p = per(n)
    last = (n - 1) // p
    return p, last, n - last * p, GL_THREADS - 1 - last


def rounds(length):
    """walks of grad_segsum_kernel over a list of `length` contributions (per channel slab)"""
    return (length + ROUND - 1) // ROUND


def slabs(c):
    """passes of grad_segsum_kernel's loop over c0"""
    return (c + SLAB - 1) // SLAB


def workspace_bytes(b, targets, entries):
    """pasnl_grad_workspace_bytes: start[b][targets + 1] and list[b][entries], ints"""
    if b <= 0 or targets <= 0 or entries < 0:
        return 0
    return 4 * (b * (targets + 1) + b * entries)


U = 2.0 ** -24  # unit roundoff of fp32


def gamma(length):
    """|fl(sum of L fp32 terms, any order) - exact sum| <= gamma(L) * sum |term|  (Higham, Accuracy and Stability, (4.4))"""
    return length * U / (1.0 - length * U)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def grads(rng, shape):
    """standard_normal * 10 ** uniform(-2, 2) per element: magnitudes over four decades, so that nearly every change of the order
    of an fp32 sum changes its bits (with same-scale values too many wrong orders give the right ones)"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-2.0, 2.0, shape)).astype(np.float32)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


# Seeds other than 0.  A case has to meet the order-sensitivity conditions of tests/test_grad_edge_cases.py; with three-channel rows
# and a handful of lists of three to seven terms (the scan cases of gather_point) not every draw does, and then the seed moves,
# never the condition.
SEEDS = {("scan", "gather", 1023): 1, ("scan", "gather", 2049): 1, ("scan", "gather", 8192): 1, ("oob", "gather"): 13,
         ("slab", "group", 1): 9, ("slab", "interp", 1): 3}


def case_rng(*key):
    return np.random.default_rng(seed_of(key, SEEDS.get(key, 0)))


@dataclasses.dataclass(eq=False)
class Case:
    op: str            # "gather" | "group" | "interp"
    b: int
    n: int             # targets per cloud
    c: int
    idx: np.ndarray    # int32: (b, m) | (b, m, nsample) | (b, n_unknown, 3)
    g: np.ndarray      # float32: (b, m, 3) | (b, m, nsample, c) | (b, n_unknown, c)
    w: np.ndarray = None  # float32 (b, n_unknown, 3), three_interpolate only
    note: dict = dataclasses.field(default_factory=dict)  # what the builder placed where (zero blocks, list lengths, ...)

    @property
    def entries(self):
        return int(np.prod(self.idx.shape[1:]))

    def flat_idx(self):
        return self.idx.reshape(self.b, self.entries).astype(np.int64)

    def valid(self):
        f = self.flat_idx()
        return (f >= 0) & (f < self.n)

    def counts(self):
        """(b, n) list lengths: valid contributions per target"""
        f, v = self.flat_idx(), self.valid()
        return np.stack([np.bincount(f[i][v[i]], minlength=self.n) for i in range(self.b)])

    def terms(self):
        """(b, entries, c) fp32: what contribution e adds to its target's row"""
        if self.op == "interp":
            return np.repeat(self.g, 3, axis=1) * self.w.reshape(self.b, self.entries, 1)
        return self.g.reshape(self.b, self.entries, self.c)

    def lists(self, i):
        """cloud i: (targets with a non-empty list, their contributions e in ascending order)"""
        f = self.flat_idx()[i]
        e = np.nonzero(self.valid()[i])[0]
        e = e[np.argsort(f[e], kind="stable")]
        if len(e) == 0:
            return e, []
        cut = np.nonzero(np.diff(f[e]))[0] + 1
        return f[e][np.concatenate([[0], cut])], np.split(e, cut)

    def _oracle(self, n, idx):
        b = self.b
        if self.op == "gather":
            return O.gather_point_grad(np.zeros((b, n, 3), np.float32), idx, self.g)
        if self.op == "group":
            return O.group_point_grad(np.zeros((b, n, self.c), np.float32), idx, self.g)
        pts = np.zeros((b, n, self.c), np.float32)
        want = O.three_interpolate_grad(pts, idx, self.w, self.g)
        if ref.available("libref_interp.so"):  # the reference's own loop (tf_interpolate.cpp:131-153) agrees with its restatement
            np.testing.assert_array_equal(ref.three_interpolate_grad(pts, idx, self.w, self.g).view(np.uint32), want.view(np.uint32))
        return want

    @functools.cached_property
    def want(self):
        """(b, n, c): the oracle's sequential fp32 loop.  It does not check bounds (nor does the reference), so with out-of-range
        indices it runs on n + 1 targets with every invalid index redirected to target n, and that row is dropped: the valid
        contributions keep their order, so every other row is what "out-of-range indices are ignored" means, bit for bit."""
        v = self.valid().reshape(self.idx.shape)
        if v.all():
            out = self._oracle(self.n, self.idx)
        else:
            out = self._oracle(self.n + 1, np.where(v, self.idx, self.n).astype(np.int32))[:, :self.n].copy()
        out.setflags(write=False)
        return out


def seq_sum(t):
    """fp32 sum of the rows of t (L, c) in the given order, one addition at a time"""
    acc = np.zeros(t.shape[1], np.float32)
    for row in t:
        acc = acc + row
    return acc


def slot_order(length, rng):
    """stand-in for the order in which a list's contributions took their slots: a random permutation that is neither the
    ascending order nor the ascending order with its first two swapped ((a + b) + ... == (b + a) + ... bit for bit)"""
    while length >= 3:
        p = rng.permutation(length)
        if (p[2:] != np.arange(2, length)).any():
            return p
    return np.arange(length)  # one or two terms: no order to tell apart


def fp64_sums_and_bounds(case):
    """(gamma(L) * sum |term|, fp64 sum of the fp32 terms), each (b, n, c), L the row's list length.  (The fp64 sum's own error,
    L * 2**-53 of the same sum |term|, is 2**-29 of the bound.)"""
    terms, flat, valid = case.terms().astype(np.float64), case.flat_idx(), case.valid()
    s64 = np.zeros((case.b, case.n, case.c))
    sabs = np.zeros_like(s64)
    for i in range(case.b):
        np.add.at(s64[i], flat[i][valid[i]], terms[i][valid[i]])
        np.add.at(sabs[i], flat[i][valid[i]], np.abs(terms[i][valid[i]]))
    return gamma(case.counts().astype(np.float64))[..., None] * sabs, s64


def order_sensitivity(case, min_len=3):
    """For every row with at least `min_len` contributions: (cloud, target, length, ascending sum, does the descending sum differ
    in some channel's bits, does the sum in a fixed random order differ)."""
    rng = np.random.default_rng(seed_of("slots", case.op, case.n, case.c))
    terms = case.terms()
    out = []
    for i in range(case.b):
        for t, e in zip(*case.lists(i)):
            if len(e) < min_len:
                continue
            rows = terms[i, e]
            asc = seq_sum(rows)
            desc = seq_sum(rows[::-1])
            perm = seq_sum(rows[slot_order(len(e), rng)])
            out.append((i, int(t), len(e), asc, bool((asc.view(np.uint32) != desc.view(np.uint32)).any()),
                        bool((asc.view(np.uint32) != perm.view(np.uint32)).any())))
    return out


def _make(op, rng, b, n, c, flat, shape):
    """a Case of `op` whose contribution e of cloud i goes to target flat[i, e]; shape = (m,) | (m, nsample) | (n_unknown, 3)"""
    idx = np.ascontiguousarray(flat.reshape((b,) + shape)).astype(np.int32)
    if op == "gather":
        assert c == 3
        return Case(op, b, n, 3, idx, grads(rng, (b, shape[0], 3)))
    if op == "group":
        return Case(op, b, n, c, idx, grads(rng, (b,) + shape + (c,)))
    w = rng.uniform(0.05, 1.0, (b,) + shape).astype(np.float32)  # random positive weights
    return Case(op, b, n, c, idx, grads(rng, (b, shape[0], c)), w)


# ---- 1. scan ownership ---------------------------------------------------------------------------------------------------
# n: (per, thread that owns the last target, targets it owns, threads behind it that own nothing)
SCAN = {
    1023: (1, 1022, 1, 1), 1024: (1, 1023, 1, 0), 1025: (2, 512, 1, 511), 2047: (2, 1023, 1, 0), 2048: (2, 1023, 2, 0),
    2049: (3, 682, 3, 341), 8192: (8, 1023, 8, 0), 10240: (10, 1023, 10, 0), 38399: (38, 1010, 19, 13), 38400: (38, 1010, 20, 13),
}
SCAN_INTERP = {1025: (2, 512, 1, 511), 2049: (3, 682, 3, 341)}
ZERO_BLOCK = 5  # targets without any contribution, two on one side of a thread-ownership boundary and three on the other


def zero_block(rng, n):
    """[lo, lo + ZERO_BLOCK) around the first target of a thread that is lane 0 of its wave: the block crosses from one thread's
    targets into the next one's, and from one wave's partial sum into the next"""
    p, last, _, _ = scan_owner(n)
    thread = 64 * int(rng.integers(1, (n - 3) // p // 64 + 1))
    lo = thread * p - 2
    assert 0 < lo and lo + ZERO_BLOCK <= n and (lo // p) != ((lo + ZERO_BLOCK - 1) // p)
    return lo


@functools.lru_cache(maxsize=None)
def scan_case(op, n):
    """b = 2; indices uniform over all targets but a ZERO_BLOCK per cloud.  gather_point: m = n / 4 contributions;
    group_point: c = 5, m = 64, nsample = 32."""
    rng = case_rng("scan", op, n)
    b = 2
    shape, c = ((n // 4,), 3) if op == "gather" else ((64, 32), 5)
    entries = int(np.prod(shape))
    lo = [zero_block(rng, n) for _ in range(b)]
    flat = rng.integers(0, n - ZERO_BLOCK, (b, entries))
    for i in range(b):
        flat[i] += ZERO_BLOCK * (flat[i] >= lo[i])
    case = _make(op, rng, b, n, c, flat, shape)
    case.note["zero_block"] = lo
    return case


@functools.lru_cache(maxsize=None)
def scan_interp_case(m):
    """three_interpolate onto m known points from 700 unknown ones: 2100 contributions from a real three_nn / three_weights"""
    rng = case_rng("scan", "interp", m)
    b, n, c = 2, 700, 6
    x1, x2 = rng.random((b, n, 3), dtype=np.float32), rng.random((b, m, 3), dtype=np.float32)
    d, i = O.three_nn(x1, x2)
    return Case("interp", b, m, c, i, grads(rng, (b, n, c)), O.three_weights(d))


# ---- 2. round boundaries of the list walk --------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1000)
ROUNDS = (0, 1, 1, 1, 1, 1, 2, 2, 2, 3, 4, 16)
ROUND_TARGETS = 16
ROUND_SHAPE = {"gather": ((1782,), 3), "group": ((891, 2), 70), "interp": ((594, 3), 70)}


@functools.lru_cache(maxsize=None)
def round_case(op):
    """b = 2.  Twelve of a cloud's 16 targets get lists of exactly LENGTHS contributions (another assignment in the second
    cloud), at positions e shuffled over the whole range.  Their total, 1782 = 3 * 594, needs no padding to fill the rows of
    three_interpolate's (b, n, 3) indices, which are constructed (real three-neighbour indices never make long lists), with
    random positive weights.  Contribution e = 0 of cloud 0 belongs to the list of 1000."""
    rng = case_rng("round", op)
    shape, c = ROUND_SHAPE[op]
    entries = int(np.prod(shape))
    assert entries == sum(LENGTHS)
    b = 2
    flat = np.zeros((b, entries), np.int64)
    lengths = np.zeros((b, ROUND_TARGETS), np.int64)
    for i in range(b):
        lengths[i, rng.permutation(ROUND_TARGETS)[:len(LENGTHS)]] = LENGTHS
        flat[i] = np.repeat(np.arange(ROUND_TARGETS), lengths[i])[rng.permutation(entries)]
    longest = int(np.argmax(lengths[0]))
    j = int(np.nonzero(flat[0] == longest)[0][0])
    flat[0, [0, j]] = flat[0, [j, 0]]
    case = _make(op, rng, b, ROUND_TARGETS, c, flat, shape)
    case.note["lengths"] = lengths
    return case


# ---- 3. channel slabs ----------------------------------------------------------------------------------------------------
SLAB_C = {1: 1, 63: 1, 64: 1, 65: 1, 511: 1, 512: 1, 513: 2, 1025: 3}
SLAB_TARGETS = 40


@functools.lru_cache(maxsize=None)
def slab_case(op, c):
    """b = 2, 40 targets, 300 contributions: a list of 65 and one of 129 (two and three rounds in every slab), the other 106
    uniform over the remaining 38 targets.  With a single channel a row is ONE sum, and one sum of three to twenty terms keeps its
    bits under a change of order too often for the conditions of the CPU module; there the 106 make a list of 64 and 21 lists of
    two, which are exempt."""
    assert op in ("group", "interp")
    rng = case_rng("slab", op, c)
    b, entries = 2, 300
    shape = (60, 5) if op == "group" else (100, 3)
    flat = np.zeros((b, entries), np.int64)
    for i in range(b):
        targets = rng.permutation(SLAB_TARGETS)
        if c == 1:
            rest = np.repeat(targets[2:24], [64] + [2] * 21)
        else:
            rest = targets[2:][rng.integers(0, SLAB_TARGETS - 2, entries - 65 - 129)]
        flat[i] = np.concatenate([np.full(65, targets[0]), np.full(129, targets[1]), rest])[rng.permutation(entries)]
    return _make(op, rng, b, SLAB_TARGETS, c, flat, shape)


# ---- 4. out-of-range indices ---------------------------------------------------------------------------------------------
OOB_TARGETS = 30
OOB_SHAPE = {"gather": ((1500,), 3), "group": ((300, 5), 7), "interp": ((500, 3), 7)}


def invalid_values(n):
    return np.array([-1, n, n + 1, 2 ** 31 - 1, -2 ** 31], np.int64)


@functools.lru_cache(maxsize=None)
def oob_case(op):
    """b = 3, 30 targets, 1500 contributions, half of them onto targets 0..3 (lists of some 190) and half uniform.  In clouds 0
    and 1 a tenth of the indices, and every index of one `victim` target, is replaced by a value of invalid_values(n); in cloud 2
    every index is."""
    rng = case_rng("oob", op)
    shape, c = OOB_SHAPE[op]
    b, n, entries = 3, OOB_TARGETS, int(np.prod(shape))
    flat = np.where(rng.random((b, entries)) < 0.5, rng.integers(0, 4, (b, entries)), rng.integers(0, n, (b, entries)))
    bad = invalid_values(n)[rng.integers(0, 5, (b, entries))]
    victim = [2, 17]  # a long list and a short one
    mask = rng.random((b, entries)) < 0.1
    for i, t in enumerate(victim):
        assert (flat[i] == t).sum() >= 3
        mask[i] |= flat[i] == t
    mask[2] = True
    case = _make(op, rng, b, n, c, np.where(mask, bad, flat), shape)
    case.note["victim"] = victim
    return case


# ---- 5 / 7. shapes without any list longer than one ------------------------------------------------------------------------
DISTINCT_SHAPE = {"gather": ((200,), 3), "group": ((40, 5), 70), "interp": ((66, 3), 70)}


@functools.lru_cache(maxsize=None)
def distinct_case(op):
    """b = 2, 300 targets, some 200 contributions all onto different targets (idx a partial permutation; three_interpolate's
    three-neighbour indices made distinct over the whole cloud): the sum of a row is one term, whatever the order"""
    rng = case_rng("distinct", op)
    shape, c = DISTINCT_SHAPE[op]
    b, n, entries = 2, 300, int(np.prod(shape))
    flat = np.stack([rng.permutation(n)[:entries] for _ in range(b)])
    return _make(op, rng, b, n, c, flat, shape)


def list_cases():
    """every case with lists, by a readable id: what the CPU module checks for order sensitivity"""
    out = {}
    for n in SCAN:
        for op in ("gather", "group"):
            out[f"scan-{op}-{n}"] = functools.partial(scan_case, op, n)
    for m in SCAN_INTERP:
        out[f"scan-interp-{m}"] = functools.partial(scan_interp_case, m)
    for op in ("gather", "group", "interp"):
        out[f"round-{op}"] = functools.partial(round_case, op)
        out[f"oob-{op}"] = functools.partial(oob_case, op)
    for c in SLAB_C:
        for op in ("group", "interp"):
            out[f"slab-{op}-{c}"] = functools.partial(slab_case, op, c)
    return out
