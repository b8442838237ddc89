"""One record per store path of the forward entry points of include/pasnl.h (the model path and the input stage): the
arguments of one call through the C ABI, every device output with the shape and dtype the header states, the workspace-size
function where the entry takes a workspace, the expected result, and -- as data -- the tile, chunk or wave widths the shape
is ragged against.  Plain numpy + the oracle: no GPU, no torch.

Shared by tests/test_abi_cases.py (CPU: every in-scope symbol has a case, every case is ragged as it says) and
tests/test_gpu_abi_bounds.py (GPU: outputs and workspaces as guarded views of exactly the stated sizes, two runs over different
stale bytes).

Sizes are the header's, not what the Python mirror allocates.  An output is described by `Out`: its shape is the shape of the
BUFFER the test hands in, and `state` says per element what the header promises:
    DEFINED      written by the entry, compared with `want` and bit-identical between the two runs
    KEPT         not written: holds the bytes it held before the call (rows past a count, columns of a wider table that
                 belong to somebody else, outputs the header says are ignored)
    UNSPECIFIED  the header leaves the contents open (scratch, swap residue): excluded from every comparison but the guards

The expected values come from the oracle the entry's parity test uses: oracle.ops bit for bit for indices, gathers, maxima
and subsampling; the fp64 restatement with the layer arithmetic of oracle.cells for attention, cells and dense."""
import dataclasses
import os
import sys
import zlib

import numpy as np

from oracle import cells
from oracle import ops as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import clouds  # noqa: E402
from golden import ref_cases as RC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

OK, EWORKSPACE = 0, -3  # include/pasnl.h

DEFINED, KEPT, UNSPECIFIED = 1, 0, 2

# comparisons (the ones the entries' parity tests make; nothing new)
BITS = ("bits",)                                # bit patterns
ATT = ("allclose", 1e-5, 1e-5)                  # test_gpu_cells.py: attention cores, rtol / atol
AS_FEAT = ("allclose", 1e-5, 2e-5)              # test_gpu_cells.py: test_adaptive_sampling_fused's new_feature
SCALE = ("scale", 1e-5)                         # max |got - want| <= 1e-5 * max |want|   (cells)
SCALE1 = ("scale1", 1e-5)                       # max |got - want| <= 1e-5 * max(1, max |want|)   (tails, dense)
PROJ = ("scale", 1e-6)                          # test_gpu_sa_cell_pre.py: test_projection_table
BF16X3 = ("bf16x3",)                            # test_gpu_dense.py: the three planes add up to the weight within 2^-23


# ---------------------------------------------------------------------------------------------------------------------------
# argument markers
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class L:      # a C long
    v: int


@dataclasses.dataclass
class F:      # a C float
    v: float


@dataclasses.dataclass
class D:      # a C double
    v: float


@dataclasses.dataclass
class Ref:    # the device pointer of output `name`, `offset` elements into its buffer
    name: str
    offset: int = 0


class _Marker:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


WS = _Marker("WS")      # the workspace pointer
WSB = _Marker("WSB")    # its size as size_t (the test hands in the size function's value, or one byte less)
DST = _Marker("DST")    # inside Prep.args: the buffer the preparation writes


@dataclasses.dataclass(eq=False)
class Prep:
    """an INPUT that another entry point produces on the device (packed weights, the projection table): `entry(*args)` writes
    `nbytes` bytes (DST), which `bytes_fn(*bytes_args)` has to equal when given.  The preparation runs into a guarded buffer of
    exactly that size too."""
    entry: str
    args: list
    nbytes: int
    bytes_fn: str = None
    bytes_args: tuple = ()


@dataclasses.dataclass(eq=False)
class Out:
    name: str
    shape: tuple
    dtype: object
    cmp: tuple = BITS
    state: object = None        # None: every element DEFINED; else an int8 array that broadcasts to shape
    bytes_fn: str = None        # the header's size function for this buffer, if it has one ...
    bytes_args: tuple = ()      # ... and its arguments: the test asserts it returns exactly the bytes of `shape`

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.int64)) * np.dtype(self.dtype).itemsize

    @property
    def row_bytes(self):
        return int(self.shape[-1]) * np.dtype(self.dtype).itemsize

    def states(self):
        if self.state is None:
            return np.full(self.shape, DEFINED, np.int8)
        return np.broadcast_to(np.asarray(self.state, np.int8), self.shape)


@dataclasses.dataclass(eq=False)
class Built:
    args: list                  # ints, markers, numpy inputs (copied to the device), None (a NULL pointer), Prep
    outs: list
    want: dict                  # name -> array of the output's shape (read where the state is DEFINED)
    ws: tuple = None            # (size function, its arguments) where the entry takes a workspace
    ws_zero: int = 0            # leading workspace bytes the header requires the CALLER to have zeroed (pasnl_dense_rows)
    exact: list = dataclasses.field(default_factory=list)   # (output, index, array): that part of the output, bit for bit
    alias: list = dataclasses.field(default_factory=list)   # (output a, index, output b): a[index] has the bits of b


@dataclasses.dataclass(eq=False)
class Case:
    id: str
    entry: str
    ragged: tuple               # ((what, dim, width), ...): dim % width != 0 -- the last tile / chunk / wave is partial
    build: object               # () -> Built
    uses: tuple = ()            # further symbols the case calls (size functions, preparations)
    no_ws: bool = False         # the size function returns 0 for this shape: the entry takes its path without a workspace
    _built: Built = None

    def built(self):
        if self._built is None:
            self._built = self.build()
        return self._built


CASES = []


def case(id, entry, ragged, uses=(), no_ws=False):
    def deco(fn):
        CASES.append(Case(id, entry, tuple(ragged), fn, tuple(uses), no_ws))
        return fn
    return deco


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def randn(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def weight(rng, k, n):
    return (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)


def layer(x, w, b, act="relu"):
    return cells._layer(x, {"w": w, "b": b}, act)


def strided_state(rows, stride, lo, hi):
    st = np.full((rows, stride), KEPT, np.int8)
    st[:, lo:hi] = DEFINED
    return st


def place(rows, stride, lo, values):
    full = np.zeros((rows, stride), values.dtype)
    full[:, lo:lo + values.shape[1]] = values
    return full


# ---------------------------------------------------------------------------------------------------------------------------
# sampling.hip
# ---------------------------------------------------------------------------------------------------------------------------
# 64 lanes a wave, 256 threads a workgroup, idx rows of m ints and new_xyz rows of 3 floats stored in 16-byte pieces
FPS_SHAPES = [(3, 300, 77, "ball"), (2, 2050, 65, "ball"), (641, 70, 5, "lattice")]


def _fps(b, n, m, kind, gather):
    def build():
        xyz = clouds(11 + n, b, n, kind)
        want = O.farthest_point_sample(m, xyz)
        if not gather:
            return Built([b, n, m, xyz, Ref("idx")], [Out("idx", (b, m), np.int32)], {"idx": want})
        return Built([b, n, m, xyz, Ref("idx"), Ref("new_xyz")],
                     [Out("idx", (b, m), np.int32), Out("new_xyz", (b, m, 3), np.float32)],
                     {"idx": want, "new_xyz": O.gather_point(xyz, want)})
    return build


for _b, _n, _m, _kind in FPS_SHAPES:
    _r = (("n", _n, 64), ("m", _m, 4), ("b*m*3", _b * _m * 3, 4))
    case(f"fps_{_b}x{_n}x{_m}", "pasnl_farthest_point_sample", _r)(_fps(_b, _n, _m, _kind, False))
    case(f"fps_gather_{_b}x{_n}x{_m}", "pasnl_farthest_point_sample_gather", _r)(_fps(_b, _n, _m, _kind, True))


@case("gather_point_3x100x77", "pasnl_gather_point", (("b*m", 3 * 77, 64), ("b*m*3", 3 * 77 * 3, 4)))
def _gather_point():
    b, n, m = 3, 100, 77
    inp = clouds(3, b, n)
    idx = rng_of("gather_point").integers(0, n, (b, m)).astype(np.int32)
    return Built([b, n, m, inp, idx, Ref("out")], [Out("out", (b, m, 3), np.float32)], {"out": O.gather_point(inp, idx)})


def _prob(b, n, m):
    def build():
        rng = rng_of("prob", n)
        p, r = rng.random((b, n), dtype=np.float32), rng.random((b, m), dtype=np.float32)
        return Built([b, n, m, p, r, Ref("temp"), Ref("out")],
                     [Out("temp", (b, n), np.float32, state=UNSPECIFIED), Out("out", (b, m), np.int32)],
                     {"out": O.prob_sample(p, r)})
    return build


case("prob_sample_2x100x10", "pasnl_prob_sample", (("n", 100, 64), ("m", 10, 4)))(_prob(2, 100, 10))
case("prob_sample_2x9192x33", "pasnl_prob_sample", (("n", 9192, 1024), ("m", 33, 4)))(_prob(2, 9192, 33))


# ---------------------------------------------------------------------------------------------------------------------------
# ball_grid.hip / grouping.hip
# ---------------------------------------------------------------------------------------------------------------------------
# idx rows: 32 entries staged per lane, stored as 16-byte pieces (4 ints) that cover whole 128-byte rows (32 ints); 64 queries
# a workgroup
def _ball(b, n, m, ns, r, kind, seed=21):
    def build():
        xyz1 = clouds(seed, b, n, kind)
        xyz2 = clouds(seed + 1, b, m, kind)
        idx, cnt = O.query_ball_point(r, ns, xyz1, xyz2)
        return Built([b, n, m, F(r), ns, xyz1, xyz2, Ref("idx"), Ref("pts_cnt")],
                     [Out("idx", (b, m, ns), np.int32), Out("pts_cnt", (b, m), np.int32)], {"idx": idx, "pts_cnt": cnt})
    return build


for _ns in (32, 16, 5, 64):
    case(f"ball_3x300x77_ns{_ns}", "pasnl_query_ball_point", (("m", 77, 64), ("b*m*nsample", 3 * 77 * _ns, 32 * 64)))(
        _ball(3, 300, 77, _ns, 0.2, "ball"))
case("ball_n2048_m2047", "pasnl_query_ball_point", (("m", 2047, 64), ("b*m*nsample", 2047 * 5, 32)))(
    _ball(1, 2048, 2047, 5, 0.1, "cube"))
case("ball_n2049_brute_force", "pasnl_query_ball_point", (("n", 2049, 64), ("m", 77, 64), ("nsample", 5, 4)))(
    _ball(2, 2049, 77, 5, 0.15, "cube"))
case("ball_every_point_hits", "pasnl_query_ball_point", (("m", 77, 64), ("n", 300, 64), ("nsample", 37, 4)))(
    _ball(3, 300, 77, 37, 5.0, "ball"))
case("ball_unit_cube_100", "pasnl_query_ball_point", (("m", 33, 64), ("n", 100, 64), ("nsample", 21, 4)))(
    _ball(2, 100, 33, 21, 0.5, "cube"))


def _group_inputs(key, b, n, c, m, k):
    rng = rng_of(key, c)
    xyz = clouds(5, b, n)
    feat = randn(rng, b, n, c)
    idx = rng.integers(0, n, (b, m, k)).astype(np.int32)
    return rng, xyz, feat, idx


def gathered_rows(xyz, feat, idx, centres):
    """[xyz[i] - centre | xyz[i] | feature[i]] per neighbour, float32 and exact (one subtraction)"""
    bi = np.arange(xyz.shape[0])[:, None, None]
    gx = xyz[bi, idx]
    return np.concatenate([gx - centres[:, :, None, :], gx, feat[bi, idx]], axis=-1)


def neighbour0(xyz, feat, idx):
    bi = np.arange(xyz.shape[0])[:, None]
    cen = xyz[bi, idx[:, :, 0]]
    return cen, np.concatenate([cen, feat[bi, idx[:, :, 0]]], axis=-1)


for _c in (7, 131):
    _b, _n, _m, _k = 2, 100, 33, 5

    def _group_point(c=_c, b=_b, n=_n, m=_m, k=_k):
        _, _, feat, idx = _group_inputs("group", b, n, c, m, k)
        return Built([b, n, c, m, k, feat, idx, Ref("out")], [Out("out", (b, m, k, c), np.float32)],
                     {"out": O.group_point(feat, idx)})

    def _sa_group(c=_c, b=_b, n=_n, m=_m, k=_k):
        _, xyz, feat, idx = _group_inputs("sa_group", b, n, c, m, k)
        new_xyz = clouds(6, b, m)
        x = gathered_rows(xyz, feat, idx, new_xyz)
        return Built([b, n, c, m, k, xyz, feat, idx, new_xyz, Ref("new_point"), Ref("skip_max")],
                     [Out("new_point", (b, m, k, 6 + c), np.float32), Out("skip_max", (b, m, 6 + c), np.float32)],
                     {"new_point": x, "skip_max": x.max(axis=2)})

    def _take0(c=_c, b=_b, n=_n, m=_m, k=_k):
        _, xyz, feat, idx = _group_inputs("take0", b, n, c, m, k)
        cen, nf = neighbour0(xyz, feat, idx)
        return Built([b, n, c, m, k, xyz, feat, idx, Ref("new_xyz"), Ref("new_feature")],
                     [Out("new_xyz", (b, m, 3), np.float32), Out("new_feature", (b, m, 3 + c), np.float32)],
                     {"new_xyz": cen, "new_feature": nf})

    _r = (("c", _c, 4), ("6+c", 6 + _c, 4), ("b*m", _b * _m, 64))
    case(f"group_point_c{_c}", "pasnl_group_point", _r + (("b*m*k", _b * _m * _k, 64),))(_group_point)
    case(f"sa_group_c{_c}", "pasnl_sa_group", _r + (("b*m*k", _b * _m * _k, 64),))(_sa_group)
    case(f"take_neighbor0_c{_c}", "pasnl_take_neighbor0", _r + (("3+c", 3 + _c, 4),))(_take0)


@case("select_top_k_2x7x33x5", "pasnl_select_top_k", (("n", 33, 4), ("b*m", 14, 64)))
def _select_top_k():
    b, m, n, k = 2, 7, 33, 5
    dist = rng_of("topk").random((b, m, n), dtype=np.float32)
    dist[:, :, ::7] = np.round(dist[:, :, ::7] * 4) / 4
    wi, wo = O.select_top_k(k, dist)
    return Built([b, n, m, k, dist, Ref("outi"), Ref("out")],
                 [Out("outi", (b, m, n), np.int32), Out("out", (b, m, n), np.float32)], {"outi": wi, "out": wo})


# ---------------------------------------------------------------------------------------------------------------------------
# grouping.hip (brute-force kNN), knn_grid.hip, knn_tree.hip
# ---------------------------------------------------------------------------------------------------------------------------
# one wave (64 lanes) per query or several queries per wave; lists of 32 / 64 entries per register set; rows of k entries
def _knn(b, n, m, k, i64, entry="pasnl_knn_batch", cap=None):
    def build():
        sup = clouds(31, b, n, "ball")
        qry = clouds(32, b, m, "ball")
        idx, d = O.knn_batch(sup, qry, k, return_dist=True)
        dt = np.int64 if i64 else np.int32
        outs = [Out("idx", (b, m, k), dt), Out("dist2", (b, m, k), np.float32)]
        args = [b, n, m, k, sup, qry, Ref("idx"), int(i64), Ref("dist2")]
        if entry == "pasnl_knn_batch":
            return Built(args, outs, {"idx": idx.astype(dt), "dist2": d})
        args += [WS, WSB] + ([cap] if cap is not None else [])
        return Built(args, outs, {"idx": idx.astype(dt), "dist2": d}, ws=("pasnl_knn_workspace_bytes", (b, n)))
    return build


for _k, _i64 in ((1, False), (16, True), (33, False)):
    case(f"knn_batch_n300_k{_k}", "pasnl_knn_batch", (("m", 77, 4), ("n", 300, 64), ("b*m*k", 3 * 77 * _k, 64)))(
        _knn(3, 300, 77, _k, _i64))
for _n in (2049, 8193):
    _r = (("n", _n, 64), ("m", 77, 4), ("k", 17, 4))
    # n = 2049 < PASNL_KNN_GRID_MIN_N: pasnl_knn_workspace_bytes is 0 and the search is forwarded to pasnl_knn_batch
    case(f"knn_batch_ws_n{_n}", "pasnl_knn_batch_ws", _r, uses=("pasnl_knn_workspace_bytes",), no_ws=_n < 4096)(
        _knn(2, _n, 77, 17, False, "pasnl_knn_batch_ws"))
    case(f"knn_batch_ws_bg_n{_n}", "pasnl_knn_batch_ws_bg", _r, uses=("pasnl_knn_workspace_bytes",), no_ws=_n < 4096)(
        _knn(2, _n, 77, 17, True, "pasnl_knn_batch_ws_bg", cap=7))


def _tie_inputs(kind):
    if kind == "lattice":  # tests/golden/ref_knn.npz: the reference library's own lists on a lattice with off-lattice queries
        seed, b, n, m, k, gk = RC.KNN_TIE_CASES[6]
        assert (seed, gk) == (807, "lattice_q_off")
        sup, qry = RC.knn_tie_cloud(seed, b, n, m, gk)
        want = np.load(os.path.join(GOLDEN, "ref_knn.npz"))[f"knn_tie_{seed}"].astype(np.int64)
        _, d = O.knn_batch(sup, qry, k + 1 if k < n else k, return_dist=True)
        assert (d[..., 1:] == d[..., :-1]).any(axis=-1).all(), "every query has a tie in or right behind its list"
        return b, n, m, k, sup, qry, want
    b, n, m, k = 2, 300, 77, 17
    sup, qry = clouds(31, b, n, "ball"), clouds(32, b, m, "ball")
    want, d = O.knn_batch(sup, qry, k + 1, return_dist=True)
    assert not (d[..., 1:] == d[..., :-1]).any(), "tie-free: the canonical order is the reference's order"
    return b, n, m, k, sup, qry, want[..., :k].copy()


def _knn_tree(kind, i64):
    def build():
        b, n, m, k, sup, qry, want = _tie_inputs(kind)
        dt = np.int64 if i64 else np.int32
        return Built([b, n, m, k, sup, qry, Ref("idx"), int(i64), WS, WSB], [Out("idx", (b, m, k), dt)],
                     {"idx": want.astype(dt)}, ws=("pasnl_knn_tree_workspace_bytes", (b, n, m, k)))
    return build


def _knn_ref(kind, i64):
    def build():
        b, n, m, k, sup, qry, want = _tie_inputs(kind)
        dt = np.int64 if i64 else np.int32
        # depth_flag: set to 1 for a tree deeper than 96 levels, never cleared -- here it keeps what it held
        return Built([b, n, m, k, sup, qry, Ref("idx"), int(i64), Ref("depth_flag"), WS, WSB, 0],
                     [Out("idx", (b, m, k), dt), Out("depth_flag", (1,), np.int32, state=KEPT)],
                     {"idx": want.astype(dt)}, ws=("pasnl_knn_batch_ref_workspace_bytes", (b, n, m, k)))
    return build


_TIE_R = {"lattice": (("n", 700, 64), ("m", 90, 64), ("m", 90, 4)), "ball": (("n", 300, 64), ("m", 77, 64), ("k", 17, 4))}
for _kind in ("lattice", "ball"):
    case(f"knn_batch_tree_{_kind}", "pasnl_knn_batch_tree", _TIE_R[_kind], uses=("pasnl_knn_tree_workspace_bytes",))(
        _knn_tree(_kind, _kind == "ball"))
    case(f"knn_batch_ref_{_kind}", "pasnl_knn_batch_ref", _TIE_R[_kind], uses=("pasnl_knn_batch_ref_workspace_bytes",))(
        _knn_ref(_kind, _kind == "lattice"))


@case("knn_distance_pick_2x300x33x5", "pasnl_knn_distance_pick", (("n", 300, 64), ("nq", 33, 4), ("k", 5, 4)))
def _knn_pick():
    b, n, nq, k = 2, 300, 33, 5
    x = clouds(900 + n, b, n, "ball")
    rnd = O.mt19937(77, b * nq).reshape(b, nq)
    wi, wq = O.knn_batch_distance_pick(x, nq, k, seed=77)
    return Built([b, n, nq, k, x, rnd, Ref("idx"), Ref("queries")],
                 [Out("idx", (b, nq, k), np.int64), Out("queries", (b, nq, 3), np.float32)], {"idx": wi, "queries": wq})


# ---------------------------------------------------------------------------------------------------------------------------
# interpolation.hip
# ---------------------------------------------------------------------------------------------------------------------------
# three_nn: 64 unknown points a wave, the known cloud in quarters rounded up to 4 points; fp_interpolate_cat: tiles of 16 rows,
# channels in pieces of 4
def _three_nn(b, n, m):
    def build():
        x1, x2 = clouds(61, b, n, "cube"), clouds(62, b, m, "cube")
        d, i = O.three_nn(x1, x2)
        return Built([b, n, m, x1, x2, Ref("dist"), Ref("idx")],
                     [Out("dist", (b, n, 3), np.float32), Out("idx", (b, n, 3), np.int32)], {"dist": d, "idx": i})
    return build


case("three_nn_2x70x5", "pasnl_three_nn", (("n", 70, 64), ("m", 5, 4), ("b*n*3", 420, 64)))(_three_nn(2, 70, 5))
case("three_nn_1x33x1281", "pasnl_three_nn", (("n", 33, 64), ("m", 1281, 4), ("b*n*3", 99, 4)))(_three_nn(1, 33, 1281))


def _interp_inputs(b, m, c2, n):
    rng = rng_of("interp", m, c2)
    p2 = randn(rng, b, m, c2)
    x1, x2 = clouds(73, b, n, "cube"), clouds(74, b, m, "cube")
    x1[0, :3] = x2[0, :3]  # zero distances: the 1e-10 floor of the weights
    d, i = O.three_nn(x1, x2)
    return rng, p2, d, i


@case("three_interpolate_c7", "pasnl_three_interpolate", (("c", 7, 4), ("n", 33, 16), ("b*n*c", 2 * 33 * 7, 64)))
def _three_interpolate():
    b, m, c, n = 2, 50, 7, 33
    _, pts, d, i = _interp_inputs(b, m, c, n)
    w = O.three_weights(d)
    return Built([b, m, c, n, pts, i, w, Ref("out")], [Out("out", (b, n, c), np.float32)],
                 {"out": O.three_interpolate(pts, i, w)})


@case("three_weights_66", "pasnl_three_weights", (("rows", 66, 64), ("rows*3", 198, 4)))
def _three_weights():
    _, _, d, _ = _interp_inputs(2, 50, 7, 33)
    return Built([66, d, Ref("weight")], [Out("weight", (66, 3), np.float32)], {"weight": O.three_weights(d).reshape(66, 3)})


def _fp_cat(b, m, c2, n, c1):
    def build():
        rng, p2, d, i = _interp_inputs(b, m, c2, n)
        p1 = randn(rng, b, n, c1) if c1 else None
        want = O.three_interpolate(p2, i, O.three_weights(d))
        if c1:
            want = np.concatenate([want, p1], axis=2)
        return Built([b, m, c2, n, c1, p2, i, d, p1, Ref("out")], [Out("out", (b, n, c2 + c1), np.float32)], {"out": want})
    return build


case("fp_interpolate_cat_2x50x7x33x5", "pasnl_fp_interpolate_cat", (("n", 33, 16), ("c2", 7, 4), ("c1", 5, 4), ("c2+c1", 12, 16)))(
    _fp_cat(2, 50, 7, 33, 5))
case("fp_interpolate_cat_3x40x64x17x0", "pasnl_fp_interpolate_cat", (("n", 17, 16), ("b*n", 51, 16)))(_fp_cat(3, 40, 64, 17, 0))


# ---------------------------------------------------------------------------------------------------------------------------
# cells.hip: non-local attention
# ---------------------------------------------------------------------------------------------------------------------------
# query tiles of 32 and 64, key blocks of 32, pairs of 32-query tiles (64) in the two-tile kernel
def _nl(b, p, n, cb, variant, ws=False, spike=False):
    def build():
        rng = rng_of("nl", p, n, cb)
        q, kv = randn(rng, b, p, cb), randn(rng, b, n, 2 * cb)
        if spike:  # a key that dominates late: the rescale path, across parts where the keys are split
            kv[0, n - 3, :cb] = q[0, min(40, p - 1)] * 5.0
        want = cells.nl_attention_core(q.astype(np.float64), kv.astype(np.float64), cb)
        outs = [Out("out", (b, p, cb), np.float32, ATT)]
        if not ws:
            return Built([b, p, n, cb, q, kv, Ref("out"), variant], outs, {"out": want})
        return Built([b, p, n, cb, q, kv, Ref("out"), variant, WS, WSB], outs, {"out": want},
                     ws=("pasnl_nl_attention_workspace_bytes", (b, p, n, cb)))
    return build


for _cb, _variants in ((32, (1, 2, 3)), (64, (1, 2, 3)), (128, (2, 3))):
    for _v in _variants:
        case(f"nl_attention_2x45x77_cb{_cb}_v{_v}", "pasnl_nl_attention", (("p", 45, 32), ("p", 45, 64), ("n", 77, 32)))(
            _nl(2, 45, 77, _cb, _v))
case("nl_attention_pair_130x33x64", "pasnl_nl_attention", (("p", 33, 32), ("p", 33, 64)))(_nl(130, 33, 64, 32, 0, spike=True))
case("nl_attention_pair_3x2800x256", "pasnl_nl_attention", (("p", 2800, 64), ("p", 2800, 32 * 3)))(
    _nl(3, 2800, 256, 32, 0, spike=True))
case("nl_attention_ws_1x100x4096", "pasnl_nl_attention_ws", (("p", 100, 64), ("p", 100, 32)),
     uses=("pasnl_nl_attention_workspace_bytes",))(_nl(1, 100, 4096, 32, 0, ws=True, spike=True))


# ---------------------------------------------------------------------------------------------------------------------------
# as_cell.hip: the AdaptiveSampling cell
# ---------------------------------------------------------------------------------------------------------------------------
def _as_att(g, as_, cb, form):
    def build():
        rng = rng_of("as_att", g, as_, cb, form)
        if form == "proj":
            w = 15
            x = randn(rng, g, as_, w)
            wkvq, bkvq = randn(rng, w, 3 * cb, scale=0.5), randn(rng, 3 * cb, scale=0.1)
            kvq64 = x.astype(np.float64) @ wkvq.astype(np.float64) + bkvq
            want = cells.nl_attention_core(kvq64[..., 2 * cb:], kvq64[..., :2 * cb], cb)
            args = [g, as_, cb, w, x, wkvq, bkvq, Ref("out")]
        elif form == "qkv":
            kvq = randn(rng, g, as_, 3 * cb)
            k64 = kvq.astype(np.float64)
            want = cells.nl_attention_core(k64[..., 2 * cb:], k64[..., :2 * cb], cb)
            args = [g, as_, cb, kvq, Ref("out")]
        else:
            q, kv = randn(rng, g, as_, cb), randn(rng, g, as_, 2 * cb)
            want = cells.nl_attention_core(q.astype(np.float64), kv.astype(np.float64), cb)
            args = [g, as_, cb, q, kv, Ref("out")]
        return Built(args, [Out("out", (g, as_, cb), np.float32, ATT)], {"out": want})
    return build


# one group per wave or per 16 lanes: 4 groups a wave, 4 waves a workgroup; rows of cb floats in 16-byte pieces
case("as_attention_7x16x40", "pasnl_as_attention", (("g", 7, 4), ("cb", 40, 64)))(_as_att(7, 16, 40, "plain"))
case("as_attention_3x1x33", "pasnl_as_attention", (("g", 3, 4), ("cb", 33, 4), ("as", 1, 4)))(_as_att(3, 1, 33, "plain"))
case("as_attention_qkv_65x5x33", "pasnl_as_attention_qkv", (("g", 65, 4), ("cb", 33, 4), ("as", 5, 4)))(_as_att(65, 5, 33, "qkv"))
case("as_attention_proj_65x4x32x15", "pasnl_as_attention_proj", (("g", 65, 4), ("g", 65, 16), ("w", 15, 4)))(
    _as_att(65, 4, 32, "proj"))


@case("as_gather_2x100x7x33x9x5", "pasnl_as_gather", (("6+c", 13, 4), ("b*m", 66, 64), ("b*m*as", 330, 64)))
def _as_gather():
    b, n, c, m, k, as_ = 2, 100, 7, 33, 9, 5
    _, xyz, feat, idx = _group_inputs("as_gather", b, n, c, m, k)
    cen, _ = neighbour0(xyz, feat, idx)
    return Built([b, n, c, m, k, as_, xyz, feat, idx, Ref("out")], [Out("out", (b, m, as_, 6 + c), np.float32)],
                 {"out": gathered_rows(xyz, feat, idx[:, :, :as_], cen)})


def reweight64(logits, xyz, feat):
    """pointasnl_util.py:154-155,167-171 in fp64: softmax over the neighbours, then the re-weighted sums"""
    w = cells._softmax(logits.astype(np.float64), 1)
    return (xyz.astype(np.float64) * w[..., :1]).sum(axis=1), (feat.astype(np.float64) * w[..., 1:]).sum(axis=1)


def _as_outs(g, ch):
    return [Out("new_xyz", (g, 3), np.float32, ATT), Out("new_feature", (g, ch), np.float32, AS_FEAT)]


@case("as_reweight_65x5x9x13", "pasnl_as_reweight", (("g", 65, 64), ("ch", 13, 4), ("g*3", 195, 4)))
def _as_reweight():
    g, as_, ns, ch = 65, 5, 9, 13
    rng = rng_of("as_reweight")
    logits, gx, gf = randn(rng, g, as_, 1 + ch), randn(rng, g, ns, 3, scale=0.2), randn(rng, g, ns, ch)
    wx, wf = reweight64(logits, gx[:, :as_], gf[:, :as_])
    return Built([g, as_, ns, ch, logits, gx, gf, Ref("new_xyz"), Ref("new_feature")], _as_outs(g, ch),
                 {"new_xyz": wx, "new_feature": wf})


@case("as_reweight_x_65x5x13", "pasnl_as_reweight_x", (("g", 65, 64), ("ch", 13, 4), ("g*3", 195, 4)))
def _as_reweight_x():
    g, as_, ch = 65, 5, 13
    rng = rng_of("as_reweight_x")
    logits, x = randn(rng, g, as_, 1 + ch), randn(rng, g, as_, 3 + ch)
    wx, wf = reweight64(logits, x[..., 3:6], x[..., 3:])
    return Built([g, as_, ch, logits, x, Ref("new_xyz"), Ref("new_feature")], _as_outs(g, ch), {"new_xyz": wx, "new_feature": wf})


def _as_cell(g, form):
    """the AdaptiveSampling cell after the gather (pointasnl_util.py:112-173) in fp64: projections, micro attention, mlp2
    (cb -> 32 -> 1 + ch), softmax over the neighbours, re-weighted sums"""
    def build():
        rng = rng_of("as_cell", g, form)
        as_ = 5
        if form == "narrow":
            w, cb = 13, 32
        else:
            w, cb = 73, 33          # the reference's bottleneck (3 + c) / 2 = 33 at c = 64: ch = 67 + 3
        ch = w - 3
        x = randn(rng, g, as_, w)
        x[..., :6] *= 0.2
        wkvq, bkvq = weight(rng, w, 3 * cb), randn(rng, 3 * cb, scale=0.1)
        wa, ba, wb, bb = weight(rng, cb, 32), randn(rng, 32, scale=0.1), weight(rng, 32, 1 + ch), randn(rng, 1 + ch, scale=0.1)
        if form == "narrow":
            kvq64 = x.astype(np.float64) @ wkvq.astype(np.float64) + bkvq
            head = [g, as_, cb, w, ch, x, wkvq, bkvq]
        else:
            kvq = (x @ wkvq + bkvq).astype(np.float32)   # the projection GEMM's output is an INPUT of the wide cell
            kvq64 = kvq.astype(np.float64)
            if form == "wide_ld":
                ld = 104
                padded = np.full((g * as_, ld), 7.0, np.float32)
                padded[:, :3 * cb] = kvq.reshape(g * as_, 3 * cb)
                head = [g, as_, cb, w, ch, padded, ld, x]
            else:
                head = [g, as_, cb, w, ch, kvq, x]
        att = cells.nl_attention_core(kvq64[..., 2 * cb:], kvq64[..., :2 * cb], cb)
        logits = layer(layer(att, wa, ba), wb, bb, None)
        wx, wf = reweight64(logits, x[..., 3:6], x[..., 3:])
        return Built(head + [wa, ba, wb, bb, Ref("new_xyz"), Ref("new_feature")], _as_outs(g, ch), {"new_xyz": wx, "new_feature": wf})
    return build


for _g in (1, 65):
    _r = (("g", _g, 4), ("g*3", _g * 3, 4))
    case(f"as_cell_narrow_g{_g}", "pasnl_as_cell_narrow", _r + (("ch", 10, 4), ("w", 13, 4)))(_as_cell(_g, "narrow"))
    case(f"as_cell_wide_g{_g}", "pasnl_as_cell_wide", _r + (("ch", 70, 4), ("cb", 33, 4)))(_as_cell(_g, "wide"))
    case(f"as_cell_wide_ld_g{_g}", "pasnl_as_cell_wide_ld", _r + (("ch", 70, 4), ("cb", 33, 4)))(_as_cell(_g, "wide_ld"))


# ---------------------------------------------------------------------------------------------------------------------------
# cells.hip: the set-abstraction cells
# ---------------------------------------------------------------------------------------------------------------------------
def cell_weights(rng, c, c1, conv1=True):
    w0, b0 = weight(rng, 6 + c, c1), randn(rng, c1, scale=0.1)
    w1, b1 = (weight(rng, c1, c1), randn(rng, c1, scale=0.1)) if conv1 else (None, None)
    ww, bw = randn(rng, 3, 32), randn(rng, 32, scale=0.1)
    return w0, b0, w1, b1, ww, bw


def cell64(x, w0, b0, w1, b1, ww, bw):
    """pointasnl_util.py:264-274 in fp64 on the gathered rows x (..., k, 6 + c): H2^T G per group, flattened (c2 * 32)"""
    x64 = x.astype(np.float64)
    h = layer(x64, w0, b0)
    if w1 is not None:
        h = layer(h, w1, b1)
    g = layer(x64[..., :3], ww, bw)
    out = np.swapaxes(h, -1, -2) @ g
    return out.reshape(-1, out.shape[-2] * 32)


@case("sa_local_cell_5x96x30x64", "pasnl_sa_local_cell", (("groups", 5, 4), ("w", 36, 32), ("w", 36, 16)))
def _sa_local_cell():
    g, k, c, c1 = 5, 96, 30, 64
    rng = rng_of("sa_local_cell")
    x = randn(rng, g, k, 6 + c)
    x[..., :3] *= 0.2
    w0, b0, w1, b1, ww, bw = cell_weights(rng, c, c1)
    return Built([g, k, 6 + c, c1, c1, x, w0, b0, w1, b1, ww, bw, Ref("out")], [Out("out", (g, c1 * 32), np.float32, SCALE)],
                 {"out": cell64(x, w0, b0, w1, b1, ww, bw)})


def _sa_cell(b, n, c, m, k, c1, form="plain", conv1=True, xyz_only=False):
    """form: plain (new_xyz given) | null (new_xyz = NULL) | centre0 | packed | packed0 (packed, new_xyz = NULL) | pre | pre0"""
    def build():
        rng, xyz, feat, idx = _group_inputs("sa_cell", b, n, c, m, k)
        if xyz_only:
            feat = xyz.copy()
        centre0 = form in ("null", "centre0", "packed0", "pre0")
        cen, nf = neighbour0(xyz, feat, idx)
        centres = cen if centre0 else clouds(6, b, m)
        w0, b0, w1, b1, ww, bw = cell_weights(rng, c, c1, conv1)
        x = gathered_rows(xyz, feat, idx, centres)
        want = {"out": cell64(x, w0, b0, w1, b1, ww, bw), "skip_max": x.max(axis=2)}
        outs = [Out("out", (b * m, c1 * 32), np.float32, SCALE), Out("skip_max", (b, m, 6 + c), np.float32)]
        extra = [Out("new_xyz", (b, m, 3), np.float32), Out("new_feature", (b, m, 3 + c), np.float32)]
        head = [b, n, c, m, k, c1, c1, xyz, feat]
        new_xyz = None if centre0 else centres
        if form in ("plain", "null"):
            return Built(head + [idx, new_xyz, w0, b0, w1, b1, ww, bw, Ref("out"), Ref("skip_max")], outs, want)
        if form == "centre0":
            want.update(new_xyz=cen, new_feature=nf)
            return Built(head + [idx, w0, b0, w1, b1, ww, bw, Ref("out"), Ref("skip_max"), Ref("new_xyz"), Ref("new_feature")],
                         outs + extra, want)
        if form in ("packed", "packed0"):
            def pk(kk, nn, w):
                nbytes = (kk + 15) // 16 * 16 * nn * 4
                return Prep("pasnl_mlp3_pack_weights", [kk, nn, f32(w), DST], nbytes, "pasnl_mlp3_packed_weights_bytes", (kk, nn))
            if centre0:
                want.update(new_xyz=cen, new_feature=nf)
            else:  # new_xyz given: new_xyz_out and new_feature_out are ignored
                extra[0].state = extra[1].state = KEPT
            return Built(head + [idx, new_xyz, w0, b0, w1, b1, ww, bw, pk(c, c1, w0[6:]), pk(c1, c1, w1) if conv1 else None,
                                 Ref("out"), Ref("skip_max"), Ref("new_xyz"), Ref("new_feature")], outs + extra, want)
        proj = Prep("pasnl_sa_project", [b, n, c, c1, xyz, feat, w0, b0, DST], b * n * c1 * 4)
        if form == "pre":
            return Built(head + [proj, idx, new_xyz, w0, w1, b1, ww, bw, Ref("out"), Ref("skip_max")], outs, want)
        want.update(new_xyz=cen, new_feature=nf)
        return Built(head + [proj, idx, w0, w1, b1, ww, bw, Ref("out"), Ref("skip_max"), Ref("new_xyz"), Ref("new_feature")],
                     outs + extra, want)
    return build


# 4 waves a workgroup and a group per wave (b*m against 4), rows of 6 + c floats staged in chunks of 32 (and loaded in 16-byte
# pieces), skip maxima staged per wave; the wide kernels: one workgroup per group
_SA = "pasnl_sa_cell"
case("sa_cell_1x77x11x9x32x32", _SA, (("b*m", 9, 4), ("6+c", 17, 32), ("6+c", 17, 4)))(_sa_cell(1, 77, 11, 9, 32, 32))
case("sa_cell_one_group_c1_128", _SA, (("b*m", 1, 4), ("6+c", 10, 32), ("6+c", 10, 4)))(_sa_cell(1, 50, 4, 1, 32, 128))
case("sa_cell_wide_1x80x512x3_c1_512", _SA, (("b*m", 3, 4), ("6+c", 518, 32), ("6+c", 518, 4)))(_sa_cell(1, 80, 512, 3, 32, 512))
case("sa_cell_16_channels_m1", _SA, (("b*m", 1, 4), ("6+c", 9, 4)))(_sa_cell(1, 64, 3, 1, 32, 16, xyz_only=True))
case("sa_cell_single_convolution", _SA, (("b*m", 33, 4), ("6+c", 262, 32), ("6+c", 262, 4)))(
    _sa_cell(1, 128, 256, 33, 32, 256, conv1=False))
case("sa_cell_new_xyz_null", _SA, (("b*m", 9, 4), ("6+c", 17, 32), ("6+c", 17, 4)))(_sa_cell(1, 77, 11, 9, 32, 32, "null"))
case("sa_cell_centre0_3x300x3x70x32x64", "pasnl_sa_cell_centre0", (("b*m", 210, 4), ("6+c", 9, 4), ("3+c", 6, 4), ("m", 70, 64)))(
    _sa_cell(3, 300, 3, 70, 32, 64, "centre0"))
case("sa_cell_centre0_1x77x11x9", "pasnl_sa_cell_centre0", (("b*m", 9, 4), ("6+c", 17, 4), ("3+c", 14, 4)))(
    _sa_cell(1, 77, 11, 9, 32, 32, "centre0"))
_PK = ("pasnl_mlp3_pack_weights", "pasnl_mlp3_packed_weights_bytes")
case("sa_cell_packed_1x80x512x3", "pasnl_sa_cell_packed", (("b*m", 3, 4), ("6+c", 518, 32), ("6+c", 518, 4)), uses=_PK)(
    _sa_cell(1, 80, 512, 3, 32, 512, "packed"))
case("sa_cell_packed_centre0_1x200x256x25", "pasnl_sa_cell_packed", (("b*m", 25, 4), ("6+c", 262, 32), ("3+c", 259, 4)), uses=_PK)(
    _sa_cell(1, 200, 256, 25, 32, 256, "packed0"))
case("sa_cell_packed_single_convolution", "pasnl_sa_cell_packed", (("b*m", 33, 4), ("6+c", 262, 32)), uses=_PK)(
    _sa_cell(1, 128, 256, 33, 32, 256, "packed", conv1=False))
_PJ = ("pasnl_sa_project",)
case("sa_cell_pre_1x100x28x5x96x64", "pasnl_sa_cell_pre", (("b*m", 5, 4), ("6+c", 34, 32), ("n", 100, 32)), uses=_PJ)(
    _sa_cell(1, 100, 28, 5, 96, 64, "pre"))
case("sa_cell_pre_one_group_c1_128", "pasnl_sa_cell_pre", (("b*m", 1, 4), ("6+c", 10, 32), ("n", 50, 32)), uses=_PJ)(
    _sa_cell(1, 50, 4, 1, 32, 128, "pre"))
case("sa_cell_pre_centre0_1x256x64x37", "pasnl_sa_cell_pre_centre0", (("b*m", 37, 4), ("6+c", 70, 32), ("3+c", 67, 4)), uses=_PJ)(
    _sa_cell(1, 256, 64, 37, 32, 32, "pre0"))


@case("sa_project_3x77x36x64", "pasnl_sa_project", (("n", 77, 32), ("b*n", 231, 32), ("3+c", 39, 4)))
def _sa_project():
    b, n, c, c1 = 3, 77, 36, 64
    rng = rng_of("sa_project")
    xyz, feat = clouds(7, b, n), randn(rng, b, n, c)
    w0, b0 = randn(rng, 6 + c, c1), randn(rng, c1)
    want = np.concatenate([xyz, feat], axis=-1).astype(np.float64) @ w0[3:].astype(np.float64) + b0
    return Built([b, n, c, c1, xyz, feat, w0, b0, Ref("proj")], [Out("proj", (b, n, c1), np.float32, PROJ)], {"proj": want})


# ---------------------------------------------------------------------------------------------------------------------------
# cells.hip: the set-abstraction tail, the decoder cell
# ---------------------------------------------------------------------------------------------------------------------------
def tail_pack(k, c, w):
    nbytes = (k + 31) // 32 * 32 * c * 4
    return Prep("pasnl_sa_tail_pack_weights", [k, c, f32(w), DST], nbytes, "pasnl_sa_tail_packed_weights_bytes", (k, c))


def _tail(rows, w, cb, c, form):
    """form: plain | res | cat | packed (residual and concat rows) | packed_plain (neither: residual, new_xyz, out_cat NULL)"""
    def build():
        rng = rng_of("tail", rows, w, c)
        A, S, N = randn(rng, rows, c), randn(rng, rows, w), randn(rng, rows, max(cb, 1))
        ws, bs, wb, bb = weight(rng, w, c), randn(rng, c), weight(rng, max(cb, 1), c), randn(rng, c)
        wagg, bagg, xyz, R = weight(rng, c, c), randn(rng, c), randn(rng, rows, 3), randn(rng, rows, c)
        want = A.astype(np.float64) + np.maximum(S.astype(np.float64) @ ws + bs, 0)
        if cb:
            want = want + np.maximum(N.astype(np.float64) @ wb + bb, 0)
        want = np.maximum(want @ wagg.astype(np.float64) + bagg, 0)
        if form in ("res", "packed"):
            want = want + R
        att = [N if cb else None]
        out = Out("out", (rows, c), np.float32, SCALE1)
        # out_cat = [0 | new_xyz | out]: column 0 and the coordinates bit for bit; the copy of `out` is held to the fp64 product
        # here and, by the test, to the bits of `out`
        cat = Out("out_cat", (rows, c + 4), np.float32, SCALE1)
        want_cat = np.concatenate([np.zeros((rows, 1)), xyz.astype(np.float64), want], axis=1)
        front = (slice(None), slice(0, 4))
        cat_checks = dict(exact=[("out_cat", front, np.concatenate([np.zeros((rows, 1), np.float32), xyz], axis=1))],
                          alias=[("out_cat", (slice(None), slice(4, None)), "out")])
        head = [rows, w, cb, c, A, S] + att
        if form in ("packed", "packed_plain"):
            full = form == "packed"
            args = head + [tail_pack(w, c, ws), bs, tail_pack(cb, c, wb) if cb else None, bb if cb else None, tail_pack(c, c, wagg),
                           bagg, R if full else None, xyz if full else None, Ref("out_cat") if full else None, Ref("out")]
            return Built(args, [out, cat] if full else [out], {"out": want, "out_cat": want_cat}, **(cat_checks if full else {}))
        args = head + [ws, bs, wb if cb else None, bb if cb else None, wagg, bagg]
        if form == "res":
            return Built(args + [R, Ref("out")], [out], {"out": want})
        if form == "cat":
            return Built(args + [Ref("out"), xyz, Ref("out_cat")], [out, cat], {"out": want, "out_cat": want_cat}, **cat_checks)
        return Built(args + [Ref("out")], [out], {"out": want})
    return build


# row tiles of 32 and 64 rows, contraction chunks of 32, column tiles of 128
for _rows, _w, _cb, _c in ((77, 134, 64, 256), (2049, 257, 33, 96)):
    _r = (("rows", _rows, 32), ("rows", _rows, 64), ("w", _w, 32)) + ((("c", _c, 128), ("cb", _cb, 32)) if _c % 128 else ())
    _u = ("pasnl_sa_tail_pack_weights", "pasnl_sa_tail_packed_weights_bytes")
    case(f"sa_tail_{_rows}x{_w}x{_cb}x{_c}", "pasnl_sa_tail", _r)(_tail(_rows, _w, _cb, _c, "plain"))
    case(f"sa_tail_res_{_rows}x{_w}x{_cb}x{_c}", "pasnl_sa_tail_res", _r)(_tail(_rows, _w, _cb, _c, "res"))
    case(f"sa_tail_cat_{_rows}x{_w}x{_cb}x{_c}", "pasnl_sa_tail_cat", _r + (("c+4", _c + 4, 32),))(_tail(_rows, _w, _cb, _c, "cat"))
    case(f"sa_tail_packed_{_rows}x{_w}x{_cb}x{_c}", "pasnl_sa_tail_packed", _r + (("c+4", _c + 4, 32),), uses=_u)(
        _tail(_rows, _w, _cb, _c, "packed"))
case("sa_tail_packed_plain_77x134x0x256", "pasnl_sa_tail_packed", (("rows", 77, 32), ("w", 134, 32)),
     uses=("pasnl_sa_tail_pack_weights", "pasnl_sa_tail_packed_weights_bytes"))(_tail(77, 134, 0, 256, "packed_plain"))


def _tail_pack(k, c):
    def build():
        w = randn(rng_of("tail_pack", k, c), k, c)
        chunks = (k + 31) // 32
        padded = np.zeros((chunks * 32, c), np.float32)
        padded[:k] = w
        # packed[((chunk * 2 + h) * c + col) * 16 + t] = w[32 chunk + 2 t + h][col], zero beyond k
        want = padded.reshape(chunks, 16, 2, c).transpose(0, 2, 3, 1).copy()   # [chunk][h][col][t]
        return Built([k, c, w, Ref("packed")],
                     [Out("packed", (chunks, 2, c, 16), np.float32, bytes_fn="pasnl_sa_tail_packed_weights_bytes", bytes_args=(k, c))],
                     {"packed": want})
    return build


case("sa_tail_pack_weights_134x96", "pasnl_sa_tail_pack_weights", (("k", 134, 32), ("c", 96, 64)),
     uses=("pasnl_sa_tail_packed_weights_bytes",))(_tail_pack(134, 96))
case("sa_tail_pack_weights_33x32", "pasnl_sa_tail_pack_weights", (("k", 33, 32), ("c", 32, 64)),
     uses=("pasnl_sa_tail_packed_weights_bytes",))(_tail_pack(33, 32))


def decode64(xyz, feat, idx, ww, bw):
    b = xyz.shape[0]
    bi = np.arange(b)[:, None, None]
    gx = xyz[bi, idx].astype(np.float64)
    fmat = np.concatenate([gx, feat[bi, idx].astype(np.float64)], axis=-1)
    g = layer(gx - xyz[:, :, None, :].astype(np.float64), ww, bw)
    return np.swapaxes(fmat, 2, 3) @ g   # (b, n, 3 + c, 32)


def tiled_order(c, v):
    """position q of pasnl_decode_cell_tiled's row -> position (channel * 32 + j) of the plain row (include/pasnl.h)"""
    order = np.empty((3 + c) * 32, np.int64)
    q = np.arange(96)
    order[q] = (q // 32) * 32 + q % 32
    for t in range(c // 32):
        for g in range(4):
            for h in range(2):
                for m in range(32):
                    for i in range(4):
                        q = 96 + t * 1024 + (2 * g + h) * 128 + 4 * m + i
                        order[q] = (3 + 32 * v * (t // v) + v * m + t % v) * 32 + 8 * g + 4 * h + i
    assert sorted(order) == list(range((3 + c) * 32))
    return order


def _decode(b, n, c, k, tiled=False):
    def build():
        rng = rng_of("decode", n, c)
        xyz, feat = clouds(8, b, n), randn(rng, b, n, c)
        idx = rng.integers(0, n, (b, n, k)).astype(np.int32)
        ww, bw = randn(rng, 3, 32), randn(rng, 32, scale=0.1)
        want = decode64(xyz, feat, idx, ww, bw).reshape(b, n, (3 + c) * 32)
        if tiled:  # c % 128 == 0 and a 16-byte aligned feature table: V = 4 (pasnl_decode_cell_tiled_v4)
            want = want[:, :, tiled_order(c, 4 if c % 128 == 0 else 1)]
        return Built([b, n, c, k, xyz, feat, idx, ww, bw, Ref("out")], [Out("out", (b, n, (3 + c) * 32), np.float32, SCALE)],
                     {"out": want})
    return build


# a point per wave, 4 waves a workgroup; 32-channel tiles; feature rows in 16-byte pieces
case("decode_cell_3x17x256x16", "pasnl_decode_cell", (("b*n", 51, 4), ("n", 17, 4), ("3+c", 259, 32)))(_decode(3, 17, 256, 16))
case("decode_cell_1x40x5x32", "pasnl_decode_cell", (("3+c", 8, 32), ("c", 5, 4), ("n", 40, 64)))(_decode(1, 40, 5, 32))
case("decode_cell_tiled_1x257x256", "pasnl_decode_cell_tiled", (("b*n", 257, 4), ("n", 257, 64)))(_decode(1, 257, 256, 16, True))


# ---------------------------------------------------------------------------------------------------------------------------
# mlp_pool.hip
# ---------------------------------------------------------------------------------------------------------------------------
@case("max_pool_rows_10x7x33", "pasnl_max_pool_rows", (("c", 33, 4), ("c", 33, 64), ("b*c", 330, 256)))
def _max_pool():
    x = randn(rng_of("max_pool"), 10, 7, 33)
    return Built([10, 7, 33, x, Ref("out")], [Out("out", (10, 33), np.float32)], {"out": x.max(axis=1)})


@case("max_pool_rows_strided_5x77x33_in_48", "pasnl_max_pool_rows_strided", (("c", 33, 4), ("c", 33, 64), ("out_stride", 48, 33)))
def _max_pool_strided():
    b, n, c, stride, lo = 5, 77, 33, 48, 8
    x = randn(rng_of("max_pool_strided"), b, n, c)
    return Built([b, n, c, x, Ref("out", lo), L(stride)], [Out("out", (b, stride), np.float32, state=strided_state(b, stride, lo, lo + c))],
                 {"out": place(b, stride, lo, x.max(axis=1))})


def mlp3_pack(k, n, w):
    nbytes = (k + 15) // 16 * 16 * n * 4
    return Prep("pasnl_mlp3_pack_weights", [k, n, f32(w), DST], nbytes, "pasnl_mlp3_packed_weights_bytes", (k, n))


@case("mlp3_pack_weights_132x128", "pasnl_mlp3_pack_weights", (("k", 132, 16), ("k", 132, 32)), uses=("pasnl_mlp3_packed_weights_bytes",))
def _mlp3_pack():
    k, n = 132, 128
    w = randn(rng_of("mlp3_pack"), k, n)
    bts = (k + 15) // 16
    padded = np.zeros((bts * 16, n), np.float32)
    padded[:k] = w
    # packed[((bt * 2 + h) * n + col) * 8 + u] = w[16 bt + 2 u + h][col], zero beyond k
    want = padded.reshape(bts, 8, 2, n).transpose(0, 2, 3, 1).copy()   # [bt][h][col][u]
    return Built([k, n, w, Ref("packed")],
                 [Out("packed", (bts, 2, n, 8), np.float32, bytes_fn="pasnl_mlp3_packed_weights_bytes", bytes_args=(k, n))],
                 {"packed": want})


@case("mlp3_max_pool_2x77x132", "pasnl_mlp3_max_pool", (("n", 77, 32), ("k0", 132, 16), ("out_stride", 520, 512)),
      uses=("pasnl_mlp3_pack_weights", "pasnl_mlp3_packed_weights_bytes", "pasnl_mlp3_max_pool_workspace_bytes"))
def _mlp3():
    b, n, c, (c1, c2, c3), lo = 2, 77, 128, (128, 256, 512), 8
    k0, stride = 4 + c, c3 + lo
    rng = rng_of("mlp3")
    x = np.concatenate([np.zeros((b, n, 1), np.float32), clouds(31, b, n), randn(rng, b, n, c)], axis=-1)  # [0 | xyz | points]
    w0, w1, w2 = weight(rng, k0, c1), weight(rng, c1, c2), weight(rng, c2, c3)
    w0[0] = 0   # the alignment column has a zero row
    b0, b1, b2 = randn(rng, c1, scale=0.1), randn(rng, c2, scale=0.1), randn(rng, c3, scale=0.1)
    want = layer(layer(layer(x.astype(np.float64), w0, b0), w1, b1), w2, b2).max(axis=1)
    return Built([b, n, k0, c1, c2, c3, x, mlp3_pack(k0, c1, w0), b0, mlp3_pack(c1, c2, w1), b1, mlp3_pack(c2, c3, w2), b2,
                  Ref("out", lo), L(stride), WS, WSB],
                 [Out("out", (b, stride), np.float32, SCALE, state=strided_state(b, stride, lo, stride))],
                 {"out": place(b, stride, lo, want)}, ws=("pasnl_mlp3_max_pool_workspace_bytes", (b, n, c3)))


# ---------------------------------------------------------------------------------------------------------------------------
# dense.hip, dense_bf16x3.hip
# ---------------------------------------------------------------------------------------------------------------------------
def dense_inputs(rows, k, n, key, lda=None):
    rng = rng_of(key, rows, n)
    x, w = randn(rng, rows, k), weight(rng, k, n)
    b = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    want = x.astype(np.float64) @ w.astype(np.float64) + b
    if lda is not None:  # a row stride larger than K
        x = np.concatenate([x, np.full((rows, lda - k), 7.0, np.float32)], axis=1)
    return x, w, b, want


def _dense_rows(rows, k, n, relu):
    def build():
        x, w, b, want = dense_inputs(rows, k, n, "dense_rows")
        counters = ((n + 31) // 32 * 4 + 255) // 256 * 256
        return Built([rows, k, n, x, w, b, int(relu), Ref("out"), WS, WSB], [Out("out", (rows, n), np.float32, SCALE1)],
                     {"out": np.maximum(want, 0) if relu else want}, ws=("pasnl_dense_rows_workspace_bytes", (rows, k, n)),
                     ws_zero=counters)
    return build


# 32-column blocks, 32-row blocks, K slices of whole groups of 128
_U = ("pasnl_dense_rows_workspace_bytes",)
case("dense_rows_33x72x31", "pasnl_dense_rows", (("rows", 33, 32), ("n", 31, 32), ("kdim", 72, 128)), uses=_U)(_dense_rows(33, 72, 31, True))
case("dense_rows_1x8x1", "pasnl_dense_rows", (("rows", 1, 32), ("n", 1, 32), ("kdim", 8, 128)), uses=_U)(_dense_rows(1, 8, 1, False))
case("dense_rows_33x264x31_k_slices", "pasnl_dense_rows", (("rows", 33, 32), ("n", 31, 32), ("kdim", 264, 128)), uses=_U)(
    _dense_rows(33, 264, 31, True))


def _splitk(rows, k, n, relu):
    def build():
        x, w, b, want = dense_inputs(rows, k, n, "splitk", lda=k + 8)
        return Built([rows, k, n, k + 8, x, w, b, int(relu), Ref("out"), WS, WSB], [Out("out", (rows, n), np.float32, SCALE1)],
                     {"out": np.maximum(want, 0) if relu else want}, ws=("pasnl_dense_splitk_workspace_bytes", (rows, k, n)))
    return build


_U = ("pasnl_dense_splitk_workspace_bytes",)
case("dense_splitk_130x272x132", "pasnl_dense_splitk", (("rows", 130, 128), ("n", 132, 128), ("kdim", 272, 32)), uses=_U)(
    _splitk(130, 272, 132, False))
# one K slice: pasnl_dense_splitk_workspace_bytes is 0 and nothing meets in a workspace
case("dense_splitk_129x64x4", "pasnl_dense_splitk", (("rows", 129, 128), ("n", 4, 128)), uses=_U, no_ws=True)(_splitk(129, 64, 4, True))


@case("bf16x3_split_weights_96x128", "pasnl_bf16x3_split_weights", (("kdim", 96, 64),), uses=("pasnl_bf16x3_weights_bytes",))
def _bf16x3_split():
    k, n = 96, 128
    w = (randn(rng_of("bf16x3_split"), k, n) * np.logspace(-6, 6, n)).astype(np.float32)
    # three bf16 planes in operand order [plane][k / 8][n][k % 8]; held as raw 16-bit words
    return Built([k, n, w, Ref("wsplit")],
                 [Out("wsplit", (3, k // 8, n, 8), np.uint16, BF16X3, bytes_fn="pasnl_bf16x3_weights_bytes", bytes_args=(k, n))],
                 {"wsplit": w})


@case("dense_bf16x3_130x96x128", "pasnl_dense_bf16x3", (("rows", 130, 128), ("rows", 130, 32), ("kdim", 96, 64)),
      uses=("pasnl_bf16x3_split_weights", "pasnl_bf16x3_weights_bytes"))
def _bf16x3():
    rows, k, n = 130, 96, 128
    x, w, b, want = dense_inputs(rows, k, n, "bf16x3", lda=k + 4)
    split = Prep("pasnl_bf16x3_split_weights", [k, n, w, DST], 3 * k * n * 2, "pasnl_bf16x3_weights_bytes", (k, n))
    return Built([rows, k, n, k + 4, x, split, b, 0, Ref("out")], [Out("out", (rows, n), np.float32, SCALE1)], {"out": want})


@case("narrow_project2_77x9x32_5x1x128", "pasnl_narrow_project2", (("rows0", 77, 4), ("rows0", 77, 64), ("rows1", 5, 4), ("kdim0", 9, 4)))
def _narrow():
    rng = rng_of("narrow")
    jobs, args, outs, want = ((77, 9, 32), (5, 1, 128)), [], [], {}
    for j, (rows, k, n) in enumerate(jobs):
        x, w = randn(rng, rows, k), randn(rng, k, n)
        b = rng.uniform(-0.5, 0.5, n).astype(np.float32)
        args += [L(rows), k, n, x, w, b, Ref(f"out{j}")]
        outs.append(Out(f"out{j}", (rows, n), np.float32, SCALE1))
        want[f"out{j}"] = x.astype(np.float64) @ w.astype(np.float64) + b
    return Built(args, outs, want)


# ---------------------------------------------------------------------------------------------------------------------------
# subsample.hip, crop.hip: the input stage
# ---------------------------------------------------------------------------------------------------------------------------
def _grid_subsample(n, dl, fdim, ldim):
    def build():
        rng = rng_of("grid_subsample", n)
        p = rng.random((n, 3)).astype(np.float32)
        f = rng.random((n, fdim)).astype(np.float32)
        c = rng.integers(0, 4, (n, ldim)).astype(np.int32)
        wp, wf, wc = O.grid_subsample(p, f, c, dl)
        cnt = wp.shape[0]
        assert 0 < cnt < n or n == 1
        rows = (np.arange(n) < cnt).astype(np.int8)[:, None]   # rows past out_count are not written

        def full(a, width, dt):
            out = np.zeros((n, width), dt)
            out[:cnt] = a
            return out
        outs = [Out("out_points", (n, 3), np.float32, state=rows), Out("out_features", (n, fdim), np.float32, state=rows),
                Out("out_classes", (n, ldim), np.int32, state=rows), Out("out_count", (1,), np.int32)]
        return Built([L(n), fdim, ldim, p, f, c, F(dl), Ref("out_points"), Ref("out_features"), Ref("out_classes"), Ref("out_count"),
                      WS, WSB], outs,
                     {"out_points": full(wp, 3, np.float32), "out_features": full(wf, fdim, np.float32),
                      "out_classes": full(wc, ldim, np.int32), "out_count": np.array([cnt], np.int32)},
                     ws=("pasnl_grid_subsample_workspace_bytes", (L(n),)))
    return build


_U = ("pasnl_grid_subsample_workspace_bytes",)
case("grid_subsample_n1", "pasnl_grid_subsample", (("n", 1, 256),), uses=_U)(_grid_subsample(1, 0.1, 2, 1))
case("grid_subsample_n3000", "pasnl_grid_subsample", (("n", 3000, 256), ("n", 3000, 1024), ("fdim", 6, 4)), uses=_U)(
    _grid_subsample(3000, 0.5, 6, 2))


@case("knn_crop_2x2049", "pasnl_knn_crop", (("n", 2049, 256), ("n", 2049, 1024), ("kcap", 100, 64)), uses=("pasnl_knn_crop_workspace_bytes",))
def _knn_crop():
    b, n, kcap = 2, 2049, 100
    rng = rng_of("knn_crop")
    pts = (rng.random((b, n, 3)) * np.array([40.0, 40.0, 4.0])).astype(np.float32)
    centres = pts[np.arange(b), [5, 777]].copy()
    k = np.array([33, 100], np.int32)
    idx, d2 = np.zeros((b, kcap), np.int32), np.zeros((b, kcap), np.float64)
    for i in range(b):
        sel, dd = O.knn_crop(pts[i], centres[i], int(k[i]))
        idx[i, :k[i]], d2[i, :k[i]] = sel, dd
    state = (np.arange(kcap)[None, :] < k[:, None]).astype(np.int8)   # entries behind the count are not written
    return Built([b, L(n), L(n), pts, centres, k, kcap, D(0.0), Ref("out_idx"), Ref("out_d2"), Ref("out_count"), WS, WSB],
                 [Out("out_idx", (b, kcap), np.int32, state=state), Out("out_d2", (b, kcap), np.float64, state=state),
                  Out("out_count", (b,), np.int32)],
                 {"out_idx": idx, "out_d2": d2, "out_count": k.copy()}, ws=("pasnl_knn_crop_workspace_bytes", (b, L(n))))


# ---------------------------------------------------------------------------------------------------------------------------
# scope
# ---------------------------------------------------------------------------------------------------------------------------
# symbols of pointasnl_amd._hip.SYMBOLS that need no case here, each with its reason
EXCLUDED = {
    # host-only: they launch nothing and write no device memory
    "pasnl_version": "host only", "pasnl_strerror": "host only", "pasnl_device_count": "host only",
    "pasnl_decode_cell_tiled_v4": "host predicate on (c, pointer alignment)",
    # the backward: the deterministic entries are guarded in tests/test_gpu_grad_edges.py (destination, exact workspace); the
    # atomic ones are not bit-reproducible from run to run (their distinct-target form is guarded there too)
    "pasnl_grad_workspace_bytes": "tests/test_gpu_grad_edges.py", "pasnl_gather_point_grad_det": "tests/test_gpu_grad_edges.py",
    "pasnl_group_point_grad_det": "tests/test_gpu_grad_edges.py", "pasnl_three_interpolate_grad_det": "tests/test_gpu_grad_edges.py",
    "pasnl_gather_point_grad": "atomic", "pasnl_group_point_grad": "atomic", "pasnl_three_interpolate_grad": "atomic",
}
# the test loops (scan, scene, window, kwindow, block, kblock, modelnet): a follow-up of the same shape -- their kernels were
# rewritten one commit ago and came with fresh tests
EXCLUDED_PREFIXES = ("pasnl_scan_", "pasnl_scene_", "pasnl_window_", "pasnl_kwindow_", "pasnl_block_", "pasnl_kblock_",
                     "pasnl_modelnet_", "pasnl_cls_")
EXCLUDED_LOOP_ENTRIES = ("pasnl_knn_crop_indirect", "pasnl_crop_order_permute", "pasnl_knn_crop_scene", "pasnl_confusion_matrix")


def in_scope(symbol):
    return not (symbol in EXCLUDED or symbol in EXCLUDED_LOOP_ENTRIES or symbol.startswith(EXCLUDED_PREFIXES))


def covered():
    """every symbol a case calls: its entry, its size functions, its preparations"""
    seen = set()
    for c in CASES:
        seen.add(c.entry)
        seen.update(c.uses)
    return seen
