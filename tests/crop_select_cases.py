"""Inputs and a numpy mirror for the crop's radix selection (csrc/crop.hip) and the LDS sort behind it (csrc/test_loop.hpp:
op_sort, reached through pasnl_crop_order_permute and pasnl_scene_order_gather).  Plain numpy + the oracle: no GPU, no torch.

Shared by tests/test_crop_select_cases.py (CPU: every case is where it claims to be in the pass structure, the oracle agrees with
a second statement of the selection, and the cases tell the mirror from four wrong versions of it) and
tests/test_gpu_crop_select.py (GPU: the kernels against the oracle, bit for bit).

The KEY of a point is the bit pattern of its float64 squared distance ((dx*dx)+(dy*dy))+(dz*dz) with bit 63 cleared (cr_key: a
NaN with the sign set ranks and is returned as the positive NaN of the same payload).  `select` restates the selection: five
passes over the digits at bits 50 / 37 / 24 / 11 / 0 (13, 13, 13, 13 and 11 bits wide), each finding the bin of the r-th key
among the keys that match the prefix found so far, ending early when that bin is taken whole; then everything below the prefix
and the first r (ascending index) of what is on it."""
import functools

import numpy as np

from oracle import ops as O

# ---------------------------------------------------------------------------------------------------------------------------
# constants of csrc/crop.hip and csrc/test_loop.hpp
# ---------------------------------------------------------------------------------------------------------------------------
SHIFTS = (50, 37, 24, 11, 0)
WIDTHS = (13, 13, 13, 13, 11)
CR_THREADS, CR_ITEMS = 256, 8
CR_BLOCK = CR_THREADS * CR_ITEMS      # points per workgroup
CR_WAVE = 64 * CR_ITEMS               # points per wave
PER = (1 << 13) // CR_THREADS         # cr_find_bin: 32 consecutive bins per thread
OP_CAP = 14336                        # op_sort: the most (d2, position) pairs a workgroup's LDS holds

SIGN = np.uint64(1) << np.uint64(63)
U64 = np.uint64

MUTANTS = ("last10", "no_before", "tie_le", "early")


def bits_of(d2):
    """float64 -> key bits (bit 63 cleared)"""
    return np.ascontiguousarray(d2, dtype=np.float64).view(np.uint64) & ~SIGN


def crop_d2(points, centre):
    with np.errstate(invalid="ignore", over="ignore"):
        return O.crop_d2(points, centre)


def key_bits(points, centre):
    return bits_of(crop_d2(points, centre))


def digit(keys, p):
    return ((np.asarray(keys, np.uint64) >> U64(SHIFTS[p])) & U64((1 << WIDTHS[p]) - 1)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# the mirror
# ---------------------------------------------------------------------------------------------------------------------------
def find_bin(hist, r):
    """cr_find_bin: (bin, keys before it, keys in it) of the r-th key of a histogram; an r outside [1, total] finds nothing and
    answers (0, 0, 0)"""
    cum = np.cumsum(hist)
    if r < 1 or r > int(cum[-1]):
        return 0, 0, 0
    b = int(np.searchsorted(cum, r))
    return b, int(cum[b] - hist[b]), int(hist[b])


def select(keys, k, mutant=None):
    """The selection of the k smallest keys (ties at the k-th: lowest indices) as the kernels do it -> (records, indices).
    One record per pass that ran: p, bin (the boundary bin), before, inbin, r (after the pass), nonempty (bins that hold a
    matching key), last (the highest of them).

    mutant: one of MUTANTS, a wrong version --
      last10     the last digit's histogram is taken over 10 bits
      no_before  passes 3 and 4 do not take `before` off the rank
      tie_le     the tie cut keeps position <= r instead of < r (one key more)
      early      the early end tests the rank BEFORE `before` is taken off (r >= inbin)"""
    keys = np.asarray(keys, np.uint64)
    n, k = len(keys), int(k)
    if k <= 0:
        return [], np.zeros(0, np.int32)
    if k >= n:
        return [], np.arange(n, dtype=np.int32)
    prefix, shift, r, done, recs = 0, 63, k, False, []
    for p in range(5):
        if done:
            break
        width = 10 if (mutant == "last10" and p == 4) else WIDTHS[p]
        match = (keys >> U64(shift)) == U64(prefix)
        dig = ((keys[match] >> U64(SHIFTS[p])) & U64((1 << width) - 1)).astype(np.int64)
        hist = np.bincount(dig, minlength=1 << WIDTHS[p])
        b, before, inbin = find_bin(hist, r)
        prev_r = r
        prefix, shift = (prefix << WIDTHS[p]) | b, SHIFTS[p]
        r = prev_r if (mutant == "no_before" and p >= 3) else prev_r - before
        done = (prev_r >= inbin if mutant == "early" else r == inbin) or p == 4
        filled = np.nonzero(hist)[0]
        recs.append(dict(p=p, bin=b, before=before, inbin=inbin, r=r, nonempty=len(filled), last=int(filled[-1]) if len(filled) else -1))
    t = keys >> U64(shift)
    below, on = t < U64(prefix), t == U64(prefix)
    rank = np.cumsum(on) - on
    take = rank <= r if mutant == "tie_le" else rank < r
    return recs, np.nonzero(below | (on & take))[0].astype(np.int32)


def trace(keys, k):
    return select(keys, k)[0]


def deciding_pass(recs):
    """the last pass that had more than one bin to choose from"""
    return max((rec["p"] for rec in recs if rec["nonempty"] >= 2), default=-1)


def lexsort_select(keys, k):
    """the second statement: a full sort by (key, index)"""
    n = len(keys)
    return np.sort(np.lexsort((np.arange(n), keys))[:max(0, min(int(k), n))]).astype(np.int32)


def cut_position(keys, sel):
    """where the tie cut falls: the last selected index among the keys equal to the largest selected key -> (index, block,
    wave of the block, item of the thread, ties kept, ties in all)"""
    kmax = keys[sel].max()
    on = np.nonzero(keys == kmax)[0]
    kept = np.intersect1d(on, sel)
    i = int(kept[-1])
    return dict(index=i, block=i // CR_BLOCK, wave=(i % CR_BLOCK) // CR_WAVE, item=i % CR_ITEMS, kept=len(kept), ties=len(on))


# ---------------------------------------------------------------------------------------------------------------------------
# direct-form cases: one call of pasnl_knn_crop each
# ---------------------------------------------------------------------------------------------------------------------------
def direct(name, points, centres, ks=None, radius=0.0, n=None, stride=0, kcap=None, claims=None):
    points = np.ascontiguousarray(points, np.float32)
    centres = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
    n = len(points) if n is None else n
    return dict(name=name, points=points, centres=centres, b=len(centres), ks=None if ks is None else [int(k) for k in ks],
                radius=float(radius), n=n, stride=stride, kcap=n if kcap is None else kcap, claims=claims or [{}] * len(centres))


def scan_of(case, c):
    """the n points crop c of a direct-form case searches"""
    lo = c * case["stride"]
    return case["points"][lo:lo + case["n"]]


def want(case, c):
    """the oracle's answer for crop c: (ascending indices, key bits of their d2)"""
    p = scan_of(case, c)
    with np.errstate(invalid="ignore", over="ignore"):
        if case["radius"] > 0:
            sel, d2 = O.radius_crop(p, case["centres"][c], case["radius"])
        else:
            sel, d2 = O.knn_crop(p, case["centres"][c], min(case["ks"][c], case["kcap"]))
    return sel, bits_of(d2)


def ball(rng, count, lo, hi):
    """`count` points with a distance from the origin in [lo, hi)"""
    v = rng.standard_normal((count, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (lo + (hi - lo) * rng.random((count, 1)))).astype(np.float32)


# ---- digit_p: the selection is decided in pass p, among many bins
RING_U = {1: 2.0 ** -7, 2: 2.0 ** -14, 3: 2.0 ** -20, 4: 2.0 ** -26}
RING_JL = np.array([(j, l) for j in range(45) for l in range(45) if j * j + l * l < 2048])
VARIANTS = ("one_of_many", "inside_tie", "whole", "last_bin")


def ring_points(x0, u):
    return np.stack([np.full(len(RING_JL), x0), RING_JL[:, 0] * u, RING_JL[:, 1] * u], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ring_x0(p):
    """The first float32 x0 >= 1 + 12345 * 2^-23 for which the ring's keys (centre: the origin) differ in digit p and nowhere
    else, and no other digit of theirs is zero.  (x0 * x0 and the ring's terms are exact in double.)"""
    m = 2 ** 23 + 12345
    for m in range(m, m + 200000):
        x0 = np.float32(m * 2.0 ** -23)
        kx = bits_of(np.array([np.float64(x0) * np.float64(x0)]))
        dx = [int(digit(kx, q)[0]) for q in range(5)]
        span = 2045 * (2 if p in (1, 3) else 1)  # the ring adds (j*j + l*l) * u*u: up to 2045 units of bit 38 | 24 | 12 | 0
        if any(dx[q] == 0 for q in range(5) if q != p) or dx[p] + span >= (1 << WIDTHS[p]):
            continue
        keys = key_bits(ring_points(x0, RING_U[p]), np.zeros(3, np.float32))
        if all(len(np.unique(digit(keys, q))) == 1 for q in range(5) if q != p) and len(np.unique(digit(keys, p))) == len(np.unique(keys)):
            return x0
    raise AssertionError("no x0")


def digit_cloud(p, far=5000, near=300):
    """the ring of pass p among `near` nearer and `far` farther points, in a fixed random order -> (points, ring's indices)"""
    rng = np.random.default_rng(1000 + p)
    pts = np.concatenate([ring_points(ring_x0(p), RING_U[p]), ball(rng, near, 0.05, 0.9), ball(rng, far, 2.0, 10.0)])
    order = rng.permutation(len(pts))
    first = int(np.argmax(order >= len(RING_JL)))   # row 0 is no point of the ring: the ring does not start on a block's edge
    order[[0, first]] = order[[first, 0]]
    inv = np.empty_like(order)
    inv[order] = np.arange(len(pts))
    return pts[order], np.sort(inv[:len(RING_JL)])


def ring_ranks(keys, ring):
    """ranks r0 inside the ring for the four variants: the ring's distinct keys, their counts and the keys in front of each"""
    vals, counts = np.unique(keys[ring], return_counts=True)
    front = np.cumsum(counts) - counts
    g = len(vals)

    def first(start, least):
        return next(i for i in range(start, g) if counts[i] >= least)

    a, b, c = first(g // 3, 2), first(g // 2, 3), first(2 * g // 3, 2)
    assert counts[-1] >= 2
    return {"one_of_many": int(front[a]) + 1, "inside_tie": int(front[b]) + 2, "whole": int(front[c] + counts[c]),
            "last_bin": int(front[-1]) + 1}


@functools.lru_cache(maxsize=None)
def digit_case(p):
    pts, ring = digit_cloud(p)
    keys = key_bits(pts, np.zeros(3, np.float32))
    nearer = int((keys < keys[ring].min()).sum())
    r0 = ring_ranks(keys, ring)
    claims = [dict(kind="digit", p=p, variant=v, ring=ring, nearer=nearer, r0=r0[v]) for v in VARIANTS]
    return direct(f"digit_p{p}", pts, np.zeros((4, 3)), [nearer + r0[v] for v in VARIANTS], claims=claims)


# ---- findbin: the pass-0 boundary bin on the seams of cr_find_bin
def bin_range(b):
    e, m = b >> 2, b & 3
    return 2.0 ** (e - 1023) * (1 + m / 4), 2.0 ** (e - 1023) * (1 + (m + 1) / 4)


def a_in_bin(b, count):
    """`count` float32 values a whose square (exact in double) has its leading 13 key bits equal to b; with count >= 3 the first
    and the last are the smallest and the largest such float32"""
    if b == 0:
        return np.zeros(count, np.float32)
    if b == 8188:
        return np.full(count, np.inf, np.float32)
    lo, hi = bin_range(b)
    a = [np.float32(np.sqrt(lo + (hi - lo) * (i + 0.5) / count)) for i in range(count)]
    if count >= 3:
        first, last = np.float32(np.sqrt(lo)), np.float32(np.sqrt(hi))
        while np.float64(first) * np.float64(first) < lo:
            first = np.nextafter(first, np.float32(np.inf))
        while np.float64(last) * np.float64(last) >= hi:
            last = np.nextafter(last, np.float32(0))
        a[0], a[-1] = first, last
    a = np.array(a, np.float32)
    assert len(np.unique(a)) == count and (digit(bits_of(a.astype(np.float64) ** 2), 0) == b).all()
    return a


# boundary bin -> (bin % 32, thread % 64) it is aimed at.  A float32 `a` reaches bins 0 (a = 0), about 2900..5119 and 8188 (inf):
# the seam between waves 1 and 2 (threads 127 | 128), the first thread of wave 0 and the last of wave 3.
SEAMS = {0: (0, 0), 4064: (0, 63), 4095: (31, 63), 4096: (0, 0), 4127: (31, 0), 8188: (28, 63)}


@functools.lru_cache(maxsize=None)
def findbin_case(b):
    rng = np.random.default_rng(2000 + b)
    below = [x for x in (0, 0, 0, 3900, 3900, 4500, b - 33, b - 33, b - 2, b - 1, b - 1) if x < b and (x == 0 or 2950 < x < 5100)]
    above = [x for x in (b + 1, b + 1, b + 2, b + 33, 4500, 5000, 5000, 8188) if x > b and (2950 < x < 5100 or x == 8188)]
    inbin = 4 if b == 8188 else 5
    a = np.concatenate([a_in_bin(x, 1) for x in below] + [a_in_bin(b, inbin)] + [a_in_bin(x, 1) for x in above]
                       + ([np.array([np.nan], np.float32)] if b == 8188 else []))
    a = np.where(np.isnan(a), a, a * rng.choice(np.array([-1, 1], np.float32), len(a)))  # (the NaN keeps its clear sign bit)
    pts = np.zeros((len(a), 3), np.float32)
    pts[:, 0] = a
    pts = pts[rng.permutation(len(a))]
    claims = [dict(kind="findbin", bin=b, seam=SEAMS[b], at=at) for at in ("first", "last")]
    return direct(f"findbin_{b}", pts, np.zeros((2, 3)), [len(below) + 1, len(below) + inbin], claims=claims)


# ---- tiecut: the cut inside a run of equal keys
TIE_N = 3 * CR_BLOCK + 5


def tie_ks(ties):
    return [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4096, 4097, ties - 1]


@functools.lru_cache(maxsize=None)
def tiecut_case(cloud):
    if cloud == "copies":  # every key equal: the cut is at index k - 1
        pts = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (TIE_N, 1))
        ks = tie_ks(TIE_N)
        centres = np.tile(np.array([[1.0, 2.0, -0.5]], np.float32), (len(ks), 1))
        claims = [dict(kind="tiecut", cloud=cloud, ties=TIE_N, nearer=0) for _ in ks]
        return direct("tiecut_copies", pts, centres, ks, claims=claims)
    rng = np.random.default_rng(3000)  # 5000 points at distance 1 (the six unit points) among 1500 nearer and 2500 farther
    unit = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    pts = np.concatenate([unit[rng.integers(0, 6, 5000)], ball(rng, 1500, 0.05, 0.9), ball(rng, 2500, 2.0, 10.0)])
    pts = pts[rng.permutation(len(pts))]
    ks = [1500 + k for k in tie_ks(5000)]
    claims = [dict(kind="tiecut", cloud=cloud, ties=5000, nearer=1500) for _ in ks]
    return direct("tiecut_scattered", pts, np.zeros((len(ks), 3)), ks, claims=claims)


# ---- edges_n_k: done and live start states in one launch
EDGE_N = (1, 8, 2047, 2048, 2049, 4096, 4097)


@functools.lru_cache(maxsize=None)
def edges_case(n):
    rng = np.random.default_rng(4000 + n)
    pts = (rng.standard_normal((n, 3)) * 3).astype(np.float32)
    centres = np.stack([pts[0], pts[n // 2], pts[n - 1] + np.float32(0.125), pts[n // 3] - np.float32(0.5)])
    ks = [0, n, min(n, n // 3 + 1), n - 1]
    return direct(f"edges_n{n}", pts, centres, ks, claims=[dict(kind="edges")] * 4)


# ---- radius_extremes
@functools.lru_cache(maxsize=None)
def radius_case(kind):
    rng = np.random.default_rng(5000)
    if kind == "on_radius":  # points exactly ON the radius: r * r is the key of a member of the p = 4 ring
        pts, ring = digit_cloud(4)
        keys = key_bits(pts, np.zeros(3, np.float32))
        for i in ring[len(ring) // 2:]:
            d2 = keys[i:i + 1].view(np.float64)[0]
            r = np.sqrt(d2)
            if r * r == d2 and (keys == keys[i]).sum() >= 2:
                return direct("radius_on_radius", pts, np.zeros((1, 3)), radius=r, claims=[dict(kind="radius", on=int(i))])
        raise AssertionError("no ring member whose key is a square")
    pts = (rng.standard_normal((3000, 3)) * 3).astype(np.float32)
    centre = np.array([0.5, -0.25, 1.0], np.float32)
    pts[[3, 700, 2047, 2048, 2999]] = centre   # coincident with the centre
    pts[5] = np.inf
    pts[6, 1] = np.nan
    return direct(f"radius_{kind}", pts, [centre, pts[1]], radius={"tiny": 1e-200, "huge": 1e200}[kind], claims=[dict(kind="radius")] * 2)


# ---- stride_gt_n: scan_stride > n, the rows between the crops are copies of the centres
@functools.lru_cache(maxsize=None)
def stride_case():
    rng = np.random.default_rng(6000)
    n, pad = 2500, 37
    centres = np.array([[0.5, 0.5, 0.5], [-1.0, 0.25, 2.0]], np.float32)
    buf = (rng.standard_normal((2 * (n + pad), 3)) * 2).astype(np.float32)
    for lo in (n, 2 * n + pad):
        buf[lo:lo + pad] = centres[np.arange(pad) % 2]
    return direct("stride_gt_n", buf, centres, [900, 2049], n=n, stride=n + pad, claims=[dict(kind="stride")] * 2)


# ---- nonfinite: +inf, NaN and NaN with the sign bit set
NEG_NAN32 = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
NONFINITE = dict(inf=(5, 100, 280), nan=(50, 250), neg_nan=(10, 200))


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    rng = np.random.default_rng(7000)
    n = 300
    pts = (rng.standard_normal((n, 3)) * 2).astype(np.float32)
    pts[list(NONFINITE["inf"]), 0] = np.inf
    pts[list(NONFINITE["nan"]), 0] = np.nan
    pts[list(NONFINITE["neg_nan"]), 0] = NEG_NAN32
    assert (pts[list(NONFINITE["neg_nan"]), 0].view(np.uint32) == 0xFFC00000).all()
    return direct("nonfinite", pts, np.tile(np.array([[0.5, 0.0, -0.5]], np.float32), (4, 1)), [n, n - 1, n - 2, n - 3],
                  claims=[dict(kind="nonfinite")] * 4)


DIRECT = {}
DIRECT.update({f"digit_p{p}": functools.partial(digit_case, p) for p in (1, 2, 3, 4)})
DIRECT.update({f"findbin_{b}": functools.partial(findbin_case, b) for b in SEAMS})
DIRECT.update({f"tiecut_{c}": functools.partial(tiecut_case, c) for c in ("copies", "scattered")})
DIRECT.update({f"edges_n{n}": functools.partial(edges_case, n) for n in EDGE_N})
DIRECT.update({f"radius_{k}": functools.partial(radius_case, k) for k in ("tiny", "huge", "on_radius")})
DIRECT.update({"stride_gt_n": stride_case, "nonfinite": nonfinite_case})


# ---------------------------------------------------------------------------------------------------------------------------
# desc_multi: three scans in one flat buffer, through the descriptor entries
# ---------------------------------------------------------------------------------------------------------------------------
SCAN_DESC = np.dtype([("offset", "<i8"), ("cloud", "<i4"), ("pick", "<i4"), ("n", "<i4"), ("k", "<i4"),
                      ("cx", "<f4"), ("cy", "<f4"), ("cz", "<f4"), ("pad", "<i4")])   # pasnl_scan_crop_t
SCENE_DESC = np.dtype([("offset", "<i8"), ("cloud", "<i4"), ("pick", "<i4"), ("n", "<i4"), ("k", "<i4"),
                       ("cx", "<f8"), ("cy", "<f8"), ("cz", "<f8")])                  # pasnl_scene_crop_t
assert SCAN_DESC.itemsize == 40 and SCENE_DESC.itemsize == 48


def descriptors(dtype, offsets, ns, ks, centres):
    d = np.zeros(len(ns), dtype)
    d["offset"], d["cloud"], d["n"], d["k"] = offsets, np.arange(len(ns)), ns, ks
    d["cx"], d["cy"], d["cz"] = centres[:, 0], centres[:, 1], centres[:, 2]
    return d


@functools.lru_cache(maxsize=None)
def desc_multi():
    """scans of 700, 2048 and 5000 points (the last: the p = 3 ring); k = 0, k >= n and a live k"""
    rng = np.random.default_rng(8000)
    ring_pts, ring = digit_cloud(3, far=5000 - 300 - len(RING_JL))
    scans = [(rng.standard_normal((700, 3)) * 2).astype(np.float32), (rng.standard_normal((2048, 3)) * 2).astype(np.float32), ring_pts]
    ns = [len(s) for s in scans]
    offsets = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    keys = key_bits(ring_pts, np.zeros(3, np.float32))
    nearer = int((keys < keys[ring].min()).sum())
    ks = [0, 3000, nearer + ring_ranks(keys, ring)["one_of_many"]]
    centres = np.array([scans[0][5], scans[1][9] + np.float32(0.25), [0, 0, 0]], np.float32)
    return dict(points=np.concatenate(scans), offsets=offsets, ns=ns, nmax=max(ns), ks=ks, kcap=max(ns), centres=centres, ring=ring,
                scan_desc=descriptors(SCAN_DESC, offsets[:-1], ns, ks, centres),
                scene_desc=descriptors(SCENE_DESC, offsets[:-1], ns, ks, centres.astype(np.float64)))


def want_desc(case, c):
    lo = int(case["offsets"][c])
    with np.errstate(invalid="ignore", over="ignore"):
        sel, d2 = O.knn_crop(case["points"][lo:lo + case["ns"][c]], case["centres"][c], min(case["ks"][c], case["kcap"]))
    return sel, bits_of(d2)


# ---------------------------------------------------------------------------------------------------------------------------
# sort_sweep: op_sort at every small count, around the powers of two and at its capacity
# ---------------------------------------------------------------------------------------------------------------------------
SORT_M = sorted(set(range(1, 131)) | {2 ** j + e for j in range(8, 14) for e in (-1, 0, 1)} | {OP_CAP - 1, OP_CAP})
ARRANGEMENTS = ("random", "sorted", "reversed")
SORT_SCAN_N = 16000                      # points per scan: more than OP_CAP, idx is distinct
SORT_VALUES = np.array([0.0, 0.25, 1.5, 7.0, np.inf])
SORT_PAD_D2 = 5e-324                     # behind the count in a d2 row: would sort in front of everything but 0


def sort_groups(batch=64):
    """(m, arrangement) pairs by ascending m in launches of at most `batch` crops; m = OP_CAP on its own"""
    small = [(m, a) for m in SORT_M if m < OP_CAP for a in ARRANGEMENTS]
    return [small[i:i + batch] for i in range(0, len(small), batch)] + [[(OP_CAP, a) for a in ARRANGEMENTS]]


@functools.lru_cache(maxsize=None)
def sort_points():
    """two scans of SORT_SCAN_N points in one flat buffer"""
    return (np.random.default_rng(9000).standard_normal((2 * SORT_SCAN_N, 3)) * 4).astype(np.float32)


def sort_group(g):
    """launch g of the sweep: descriptors' fields, idx / d2 rows of kcap, perm rows of num_point = kcap, and the expected
    selection.  Crop c searches scan c % 2; its d2 holds at most 5 distinct values, so (key, position) decides."""
    pairs = sort_groups()[g]
    b, kcap = len(pairs), max(m for m, _ in pairs)
    rng = np.random.default_rng(9100 + g)
    idx = np.zeros((b, kcap), np.int32)
    d2 = np.full((b, kcap), SORT_PAD_D2)
    perm = np.zeros((b, kcap), np.int32)
    select = np.zeros((b, kcap), np.int32)
    for c, (m, arr) in enumerate(pairs):
        idx[c, :m] = np.sort(rng.choice(SORT_SCAN_N, m, replace=False))
        v = SORT_VALUES[rng.integers(0, rng.integers(1, len(SORT_VALUES) + 1), m)]
        d2[c, :m] = {"random": v, "sorted": np.sort(v), "reversed": np.sort(v)[::-1]}[arr]
        perm[c] = np.arange(kcap) % m
        perm[c, :m] = rng.permutation(m)
        order = np.lexsort((np.arange(m), bits_of(d2[c, :m])))
        select[c] = idx[c, order[perm[c]]]
    scan = np.arange(b) % 2
    centres = rng.standard_normal((b, 3)) * 2
    return dict(b=b, kcap=kcap, ms=[m for m, _ in pairs], offsets=(scan * SORT_SCAN_N).astype(np.int64), idx=idx, d2=d2, perm=perm,
                select=select, centres=centres)
