"""The shape thresholds of the two fixed dispatchers -- fps_dispatch (csrc/sampling.hip) and pasnl::knn_brute_launch
(csrc/grouping.hip) -- crossed from both sides, every kernel they can choose compared index for index with the oracle.

Which kernel runs is decided by the shape alone.  FPS_BRANCH / knn_branch below restate the two dispatchers' host arithmetic in
plain Python (the constants are those of sampling.hip, grouping.hip and common.hpp); every case names the branch it is meant for
and asserts that the restated arithmetic puts it there, so a moved threshold fails here instead of silently testing another kernel.
Every comparison is exact: integers, or bit patterns for the gathered coordinates."""
import functools

import numpy as np
import pytest
import torch

from conftest import clouds
from oracle import ops as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import pointasnl_amd

    return pointasnl_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------
# fps_dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------------
LDS_MAX_BYTES = 160 * 1024  # common.hpp


def pruned_lds(n, m):
    """fps_pruned_launch: the cloud (12 B a point), the 16-bit sort keys of an even number of points, rounded up to 16 bytes, then
    the larger of the 4096-cell histogram and the 64 + m words of slots and picks"""
    lds = 12 * n + 2 * ((n + 1) & ~1)
    lds = (lds + 15) & ~15
    return lds + max(4096 * 4, (64 + m) * 4)


def pruned_accepts(n, m):
    return pruned_lds(n, m) <= LDS_MAX_BYTES - 1024 and n <= 65535


def unpruned_lds(n, m, stride):
    """fps_launch: 2 x 16 slots of 8 bytes, `stride` floats a point, m picks"""
    return 2 * 16 * 8 + 4 * stride * n + 4 * m


def fps_branch(b, n, m):
    """(kernel, waves, points per lane or per-lane block, floats per LDS record) fps_dispatch chooses, None where it refuses"""
    def unpruned(waves, ppl):
        for stride in (4, 3):
            if unpruned_lds(n, m, stride) <= LDS_MAX_BYTES:
                return ("fps", waves, ppl, stride)
        return None

    if n <= 128:
        return unpruned(1, 2)
    if n <= 256:
        return unpruned(1, 4)
    if n <= 512:
        return unpruned(1, 8)
    if n <= 1024:
        return unpruned(1, 16) if b > 640 else unpruned(4, 4)
    if n <= 2048:
        return unpruned(4, 8)
    if n > 10240:
        return None
    nb = 4 if n <= 4096 else 8 if n <= 8192 else 10
    if pruned_accepts(n, m):
        return ("pruned", 16, nb, 3)
    return unpruned(4, 16) if n <= 4096 else unpruned(16, nb)


def check_fps(P, xyz, m, want, entry):
    """the plain entry against the oracle's picks, or the gather entry against the picks and O.gather_point of them, bit for bit"""
    b = xyz.shape[0]
    if entry == "plain":
        got = P.tf_sampling.farthest_point_sample(m, dev(xyz)).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (b, m)
        np.testing.assert_array_equal(got, want)
    else:
        idx, new_xyz = P.tf_sampling.farthest_point_sample_gather(m, dev(xyz))
        idx, new_xyz = idx.cpu().numpy(), new_xyz.cpu().numpy()
        assert idx.dtype == np.int32 and idx.shape == (b, m) and new_xyz.dtype == np.float32 and new_xyz.shape == (b, m, 3)
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_array_equal(new_xyz.view(np.uint32), O.gather_point(xyz, want).view(np.uint32))


# ---- 1. boundary sweep: both sides of 128 | 129, 256 | 257, 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097, 8192 | 8193 (the
# near sides 512, 1024, 2048, 8192 are test_gpu_ops.py's), ragged sizes inside 129..256, m around n / 4
SWEEP = [
    (127, ("fps", 1, 2, 4)), (128, ("fps", 1, 2, 4)),
    (129, ("fps", 1, 4, 4)), (200, ("fps", 1, 4, 4)), (255, ("fps", 1, 4, 4)), (256, ("fps", 1, 4, 4)),
    (257, ("fps", 1, 8, 4)), (511, ("fps", 1, 8, 4)),
    (513, ("fps", 4, 4, 4)), (1023, ("fps", 4, 4, 4)),
    (1025, ("fps", 4, 8, 4)), (2047, ("fps", 4, 8, 4)),
    (2049, ("pruned", 16, 4, 3)), (4095, ("pruned", 16, 4, 3)), (4096, ("pruned", 16, 4, 3)),
    (4097, ("pruned", 16, 8, 3)), (8191, ("pruned", 16, 8, 3)),
    (8193, ("pruned", 16, 10, 3)),
]
# (n, m) inside 129..256 beyond m = n / 4: every point sampled (the last rounds run on a field of zeros where clouds repeat a
# position), and a single pick (no round at all)
SWEEP_M = [(129, 129), (200, 200), (256, 256), (200, 1), (256, 1)]


@functools.lru_cache(maxsize=None)
def sweep_case(n, m, kind):
    b = 3 if n <= 1025 else 2
    xyz = clouds(1000 + n, b, n, kind)
    return xyz, O.farthest_point_sample(m, xyz)


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("kind", ["ball", "lattice"])
@pytest.mark.parametrize("n,branch", SWEEP, ids=[f"n{n}" for n, _ in SWEEP])
def test_fps_boundary_sweep(P, n, branch, kind, entry):
    m = n // 4
    xyz, want = sweep_case(n, m, kind)
    assert fps_branch(xyz.shape[0], n, m) == branch
    check_fps(P, xyz, m, want, entry)


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("kind", ["ball", "lattice"])
@pytest.mark.parametrize("n,m", SWEEP_M)
def test_fps_129_to_256_all_points_and_single_pick(P, n, m, kind, entry):
    xyz, want = sweep_case(n, m, kind)
    assert fps_branch(xyz.shape[0], n, m) == ("fps", 1, 4, 4)
    check_fps(P, xyz, m, want, entry)


@functools.lru_cache(maxsize=None)
def many_clouds_case(b, n, kind):
    xyz = clouds(2000 + n + b, b, n, kind)
    return xyz, O.farthest_point_sample(n // 4, xyz)


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("b,n,kind,branch", [
    (641, 513, "ball", ("fps", 1, 16, 4)), (641, 513, "lattice", ("fps", 1, 16, 4)),
    (641, 1024, "ball", ("fps", 1, 16, 4)), (641, 1024, "lattice", ("fps", 1, 16, 4)),
    (640, 513, "lattice", ("fps", 4, 4, 4)),  # the last batch size of the four-wave form
])
def test_fps_more_than_640_clouds_one_wave_each(P, b, n, kind, branch, entry):
    """b > 640 clouds of 513..1024 points: one wave per cloud, 16 points per lane -- at the smallest and the largest such cloud
    (lanes 1..63 hold 8 real points and 8 paddings at n = 513; no padding at all at n = 1024)."""
    xyz, want = many_clouds_case(b, n, kind)
    assert fps_branch(b, n, n // 4) == branch
    check_fps(P, xyz, n // 4, want, entry)


# ---- 2. the unpruned kernels behind the pruned one.  LDS_MAX_BYTES = 163840; the pruned kernel accepts up to 163840 - 1024 =
# 162816 bytes.  In every case below the 16-byte records do not fit either, so the kernel that runs is fps_kernel<.., .., 3>.
FALLBACK = {
    # n = 10240, m = 5120 (half of a lidar crop):
    #   pruned   12*10240 + 2*10240 = 143360 (a multiple of 16) + max(16384, 4*(64+5120) = 20736) = 164096 > 162816: declines
    #            (from m = 4801 on: 4*(64+m) > 162816 - 143360 = 19456)
    #   16-byte  256 + 163840 + 20480 = 184576 > 163840
    #   12-byte  256 + 122880 + 20480 = 143616 <= 163840: fps_kernel<16, 10, 3>  (up to m = 10176)
    "ball_10240_5120": (10240, 5120, ("fps", 16, 10, 3)),
    "lattice16_10240_5120": (10240, 5120, ("fps", 16, 10, 3)),
    # n = 9000, m = 9500 (ragged n, more samples than points):
    #   pruned   108000 + 18000 = 126000 (a multiple of 16) + 4*(64+9500) = 38256 -> 164256 > 162816: declines (from m = 9141 on)
    #   16-byte  256 + 144000 + 38000 = 182256 > 163840
    #   12-byte  256 + 108000 + 38000 = 146256 <= 163840: fps_kernel<16, 10, 3>
    "ball_9000_9500": (9000, 9500, ("fps", 16, 10, 3)),
    "duplicates_9000_9500": (9000, 9500, ("fps", 16, 10, 3)),
    # n = 8192, m = 12288:
    #   pruned   98304 + 16384 = 114688 + 4*(64+12288) = 49408 -> 164096 > 162816: declines (from m = 11969 on)
    #   16-byte  256 + 131072 + 49152 = 180480 > 163840
    #   12-byte  256 + 98304 + 49152 = 147712 <= 163840: fps_kernel<16, 8, 3>
    "ball_8192_12288": (8192, 12288, ("fps", 16, 8, 3)),
    "duplicates_8192_12288": (8192, 12288, ("fps", 16, 8, 3)),
    # n = 4096, m = 27000:
    #   pruned   49152 + 8192 = 57344 + 4*(64+27000) = 108256 -> 165600 > 162816: declines (from m = 26305 on)
    #   16-byte  256 + 65536 + 108000 = 173792 > 163840
    #   12-byte  256 + 49152 + 108000 = 157408 <= 163840: fps_kernel<4, 16, 3>  (up to m = 28608)
    "ball_4096_27000": (4096, 27000, ("fps", 4, 16, 3)),
    "duplicates_4096_27000": (4096, 27000, ("fps", 4, 16, 3)),
}


@functools.lru_cache(maxsize=None)
def fallback_case(case):
    n, m, _ = FALLBACK[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    if case.startswith("ball"):
        xyz = clouds(3000 + n, 2, n, "ball")
    elif case.startswith("lattice16"):
        xyz = (np.round(rng.random((1, n, 3)) * 16) / 16).astype(np.float32)  # 4913 positions: ties, then exhaustion at the end
    else:  # 100 distinct points, each many times over (test_gpu_ops.py's exhausted_3000, in a shuffled order): from the 101st
        # pick on every running distance is 0 and the reference's rule -- (k mod 512, k) lowest -- returns index 0
        base = clouds(45, 1, 100, "cube")
        xyz = base[:, rng.integers(0, 100, n)].copy()
        xyz[:, :100] = base  # every distinct point is there
    want = O.farthest_point_sample(m, xyz)
    if case.startswith("duplicates"):
        assert (want[:, 101:] == 0).all() and (want[:, 1:100] != 0).all()
    return xyz, m, want


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("case", list(FALLBACK))
def test_fps_unpruned_fallback(P, case, entry):
    """Clouds of more than 2048 points whose pick list leaves no room for the pruned kernel's layout: fps_dispatch falls through
    to fps_launch<4,16>, <16,8> or <16,10>, which -- with today's sizes -- fits only with 12-byte LDS records (STRIDE = 3)."""
    n, m, branch = FALLBACK[case]
    # the arithmetic of the comments above, from the restated formulas: the pruned kernel declines, the 16-byte records do not
    # fit, the 12-byte ones do
    assert n > 2048 and not pruned_accepts(n, m)
    assert unpruned_lds(n, m, 4) > LDS_MAX_BYTES >= unpruned_lds(n, m, 3)
    xyz, m, want = fallback_case(case)
    assert fps_branch(xyz.shape[0], n, m) == branch
    check_fps(P, xyz, m, want, entry)


def test_fps_refuses_what_no_kernel_holds(P):
    """n = 10240, m = 10240: pruned 143360 + 4*(64+10240) = 184576 > 162816; 16-byte records 256 + 163840 + 40960 > 163840; 12-byte
    records 256 + 122880 + 40960 = 164096 > 163840.  fps_dispatch answers PASNL_EUNSUPPORTED before any launch: the mirror raises
    PasnlUnsupported, the caller's buffers are untouched, and the device goes on working."""
    from pointasnl_amd import _hip

    n = m = 10240
    assert fps_branch(1, n, m) is None
    assert fps_branch(1, n, 10176) == ("fps", 16, 10, 3) and fps_branch(1, n, 10177) is None  # the last m that fits
    x = dev(clouds(7, 1, n))
    with pytest.raises(_hip.PasnlUnsupported, match="FarthestPointSample"):
        P.tf_sampling.farthest_point_sample(m, x)
    idx = torch.full((1, m), -7, dtype=torch.int32, device="cuda")
    new_xyz = torch.full((1, m, 3), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(_hip.PasnlUnsupported, match="FarthestPointSample"):
        P.tf_sampling.farthest_point_sample_gather(m, x, out=(idx, new_xyz))
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((new_xyz == -7.0).all())
    small = clouds(8, 2, 300)
    np.testing.assert_array_equal(P.tf_sampling.farthest_point_sample(40, dev(small)).cpu().numpy(), O.farthest_point_sample(40, small))


# ---------------------------------------------------------------------------------------------------------------------------
# pasnl::knn_brute_launch, restated
# ---------------------------------------------------------------------------------------------------------------------------
SEARCH_WAVES = 4       # grouping.hip
KNN_GRID_MIN_N = 4096  # include/pasnl.h: from here on tie_order="index" takes the grid search, not the brute-force kernels


def knn_branch(b, n, m, k):
    """("knn2", registers per lane R, queries per wave) or ("knn", SLOTS, queries per wave)"""
    if k <= 64 and not (k <= 16 and n > 2048):
        nq = b * m
        qw = 4 if nq >= 4 * 8192 else 2 if nq >= 2 * 8192 else 1
        return ("knn2", 1 if k <= 32 else 2, qw)
    if k <= 64:
        return ("knn", 1, 4)
    if k <= 128:
        return ("knn", 2, 2)
    return ("knn", 4, 1)


def sqdist_f32(sup, qry, idx):
    """the canonical fp32 squared distance ((dx*dx)+(dy*dy))+(dz*dz) of every listed neighbour"""
    d = np.take_along_axis(sup[:, None], idx[..., None], axis=2) - qry[:, :, None]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def check_knn(P, sup, qry, k, tie_free_cloud):
    from oracle import ref

    b, n, _ = sup.shape
    want, wd = O.knn_batch(sup, qry, k, return_dist=True)
    # canonical (distance, index) order, both row types
    got = P.nearest_neighbors.knn_batch(dev(sup), dev(qry), k, omp=True, tie_order="index")
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    got32 = P.nearest_neighbors.knn_batch(dev(sup), dev(qry), k, dtype=torch.int32, tie_order="index")
    assert got32.dtype == torch.int32
    np.testing.assert_array_equal(got32.cpu().numpy(), want.astype(np.int32))
    # the default: the reference's result.  The reference library itself where it is there; the canonical list for every query
    # whose first k + 1 distances are distinct (there the two orders are one); and for EVERY query, ties or not: k different
    # points at exactly the k smallest distances
    dflt = P.nearest_neighbors.knn_batch(dev(sup), dev(qry), k, omp=True).cpu().numpy()
    assert dflt.dtype == np.int64 and dflt.min() >= 0 and dflt.max() < n
    if ref.available("libref_knn.so"):
        np.testing.assert_array_equal(dflt, ref.knn_batch(sup, qry, k))
    d1 = O.knn_batch(sup, qry, k + 1, return_dist=True)[1] if k < n else wd
    free = (np.diff(d1, axis=-1) != 0).all(-1)
    if tie_free_cloud:
        # a check of the INPUT, so that the comparison below is not empty: with random fp32 coordinates two of a query's k + 1
        # smallest distances agree in all 24 bits for about (k+1)^2 / 2^24 of the queries (3e-4 at k = 64, 1e-3 at k = 129:
        # a tie or two among the 74 queries of the boundary grid is likely somewhere, four are not)
        assert free.mean() >= 0.95
    np.testing.assert_array_equal(dflt[free], want[free])
    np.testing.assert_array_equal(sqdist_f32(sup, qry, dflt).view(np.uint32), wd.view(np.uint32))
    assert (np.diff(np.sort(dflt, axis=-1), axis=-1) != 0).all()


# (b, m): b * m on both sides of 16384 and of 32768; m = 381, 1057 and 517 are no multiples of SEARCH_WAVES * qw = 4, 8, 16 (the
# last workgroup of every cloud is ragged), 256 and 512 are
QW_SHAPES = [(43, 381, 1), (64, 256, 2), (31, 1057, 2), (64, 512, 4), (64, 517, 4)]
assert [b * m for b, m, _ in QW_SHAPES] == [16383, 16384, 32767, 32768, 33088]


@pytest.mark.parametrize("k", [8, 32, 33, 64])
@pytest.mark.parametrize("n", [64, 300])
@pytest.mark.parametrize("b,m,qw", QW_SHAPES, ids=[f"{b}x{m}" for b, m, _ in QW_SHAPES])
def test_knn_queries_per_wave(P, b, m, qw, n, k):
    """One, two and four queries per wave (b*m below 16384, below 32768, from there on) for both register widths of knn2_kernel
    (k <= 32, k <= 64): small clouds, many queries drawn independently of the support."""
    assert knn_branch(b, n, m, k) == ("knn2", 1 if k <= 32 else 2, qw) and n < KNN_GRID_MIN_N
    assert (m % (SEARCH_WAVES * qw) != 0) == (m in (381, 1057, 517))
    sup, qry = clouds(61 + n, b, n, "ball"), clouds(62 + m, b, m, "ball")
    check_knn(P, sup, qry, k, tie_free_cloud=True)


@pytest.mark.parametrize("k", [32, 33])
@pytest.mark.parametrize("b,m,qw", [(43, 381, 1), (31, 1057, 2), (64, 517, 4)])
def test_knn_queries_per_wave_lattice(P, b, m, qw, k):
    """the same on lattice clouds: equal distances inside and at the end of nearly every list"""
    n = 300
    assert knn_branch(b, n, m, k) == ("knn2", 1 if k <= 32 else 2, qw)
    sup, qry = clouds(63, b, n, "lattice"), clouds(64 + m, b, m, "lattice")
    check_knn(P, sup, qry, k, tie_free_cloud=False)


@pytest.mark.parametrize("n,k,branch", [
    (2048, 16, ("knn2", 1, 1)), (2048, 17, ("knn2", 1, 1)), (2049, 16, ("knn", 1, 4)), (2049, 17, ("knn2", 1, 1)),
    (700, 64, ("knn2", 2, 1)), (700, 65, ("knn", 2, 2)), (700, 128, ("knn", 2, 2)), (700, 129, ("knn", 4, 1)),
])
@pytest.mark.parametrize("kind", ["ball", "lattice"])
def test_knn_k_and_n_boundaries(P, n, k, branch, kind):
    """k = 16 | 17 at n = 2048 | 2049 (the single-pass kernel takes k <= 16 over more than 2048 points), k = 64 | 65 (two-pass |
    insertion kernel), k = 128 | 129 (two | four list registers per lane); 37 queries: three ragged workgroups at one query per wave,
    a single one at two and four"""
    b, m = 2, 37
    assert knn_branch(b, n, m, k) == branch and n < KNN_GRID_MIN_N
    sup, qry = clouds(71 + n, b, n, kind), clouds(72 + k, b, m, kind)
    check_knn(P, sup, qry, k, tie_free_cloud=kind == "ball")
