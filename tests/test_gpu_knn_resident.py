"""The resident form of knn2_kernel (csrc/grouping.hip): clouds of at most 1024 points keep every distance of pass 1 in registers
and pass 2 collects the candidates d <= U from them.  Compared with the oracle's kNN in canonical (distance, index) order --
both index types, and the distances bit for bit -- and, through pasnl_knn_batch_ref's Python path (the default tie order), with
the reference's order.  Shapes: both register widths (k <= 32, k <= 64), 8 and 16 iterations, clouds that end inside a block of
four iterations and inside an iteration, one, two and four queries per wave, the first cloud of the streaming form (n = 1025),
lattice clouds (ties inside the list and at the K-th distance) and a cloud whose queries overflow the 128 candidates."""
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


def knn_form(b, n, m, k):
    """pasnl::knn_brute_launch restated for k <= 64 over at most 2048 points: (registers per lane R, queries per wave, iterations
    kept resident or 0 for the streaming form)"""
    nq = b * m
    qw = 4 if nq >= 4 * 8192 else 2 if nq >= 2 * 8192 else 1
    return (1 if k <= 32 else 2, qw, 8 if n <= 512 else 16 if n <= 1024 else 0)


def sqdist_f32(sup, qry, idx):
    d = np.take_along_axis(sup[:, None], idx[..., None], axis=2) - qry[:, :, None]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz


@functools.lru_cache(maxsize=None)
def case(b, n, m, k, kind):
    if kind == "copies":  # 200 copies of one point, spread over the cloud: every query sees >= 200 candidates under its bound
        sup = clouds(5000 + n, b, n, "ball")
        rng = np.random.default_rng(5)
        qry = clouds(5001 + m, b, m, "ball")
        for c in range(b):
            at = 8 + rng.choice(n - 8, 200, replace=False)
            sup[c, at] = sup[c, at[0]]
            qry[c, 1::3] = sup[c, at[0]] + np.float32(0.01)  # a third of the queries next to the copies,
        qry[:, ::3] = sup[:, 7:8]                             # a third on a support point, a third anywhere
    else:
        sup, qry = clouds(5000 + n, b, n, kind), clouds(5001 + m, b, m, kind)
    want, wd = O.knn_batch(sup, qry, k, return_dist=True)
    d1 = O.knn_batch(sup, qry, k + 1, return_dist=True)[1] if k < n else wd
    free = (np.diff(d1, axis=-1) != 0).all(-1)
    return sup, qry, want, wd, free


def check(P, b, n, m, k, kind):
    from oracle import ref
    from pointasnl_amd import _hip

    sup, qry, want, wd, free = case(b, n, m, k, kind)
    s, q = dev(sup), dev(qry)
    # canonical order, both index types, with the distances
    for dt, i64 in ((torch.int64, 1), (torch.int32, 0)):
        idx = torch.full((b, m, k), -1, dtype=dt, device="cuda")
        d = torch.full((b, m, k), -1.0, dtype=torch.float32, device="cuda")
        _hip.launch("pasnl_knn_batch", "knn", b, n, m, k, _hip.ptr(s), _hip.ptr(q), _hip.ptr(idx), i64, _hip.ptr(d))
        np.testing.assert_array_equal(idx.cpu().numpy(), want.astype(idx.cpu().numpy().dtype))
        np.testing.assert_array_equal(d.cpu().numpy().view(np.uint32), wd.view(np.uint32))
        got = P.nearest_neighbors.knn_batch(s, q, k, dtype=dt, tie_order="index")  # (no distances asked for)
        np.testing.assert_array_equal(got.cpu().numpy(), want.astype(idx.cpu().numpy().dtype))
    # the reference's order: the reference library itself where it is built; the canonical list wherever a query's first k + 1
    # distances are distinct; and for every query k different points at exactly the k smallest distances
    dflt = P.nearest_neighbors.knn_batch(s, q, k, omp=True).cpu().numpy()
    assert dflt.dtype == np.int64 and dflt.min() >= 0 and dflt.max() < n
    if ref.available("libref_knn.so"):
        np.testing.assert_array_equal(dflt, ref.knn_batch(sup, qry, k))
    if kind == "ball":
        assert free.mean() >= 0.95
    np.testing.assert_array_equal(dflt[free], want[free])
    np.testing.assert_array_equal(sqdist_f32(sup, qry, dflt).view(np.uint32), wd.view(np.uint32))
    assert (np.diff(np.sort(dflt, axis=-1), axis=-1) != 0).all()


SHAPES = [
    ((2, 1024, 70, 32), (1, 1, 16)), ((2, 1000, 33, 32), (1, 1, 16)), ((2, 512, 40, 64), (2, 1, 8)), ((3, 513, 20, 64), (2, 1, 16)),
    ((2, 64, 64, 32), (1, 1, 8)), ((2, 1025, 30, 32), (1, 1, 0)),
    ((64, 64, 512, 32), (1, 4, 8)), ((64, 64, 256, 32), (1, 2, 8)),
]


@pytest.mark.parametrize("kind", ["ball", "lattice"])
@pytest.mark.parametrize("shape,form", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_knn_resident(P, shape, form, kind):
    assert knn_form(*shape) == form
    check(P, *shape, kind)


@pytest.mark.parametrize("shape,form", [((2, 1024, 70, 32), (1, 1, 16)), ((2, 512, 40, 64), (2, 1, 8)), ((64, 300, 512, 32), (1, 4, 8))],
                         ids=["2x1024x70x32", "2x512x40x64", "64x300x512x32"])
def test_knn_resident_overflow_takes_the_fallback(P, shape, form):
    """200 copies of one point: at most 199 of them can be nearer than a query's K-th neighbour or all 200 lie under the bound,
    so every query whose bound reaches the copies holds more than 128 candidates and is answered by the insertion pass"""
    assert knn_form(*shape) == form
    b, n, m, k = shape
    sup, qry, want, wd, _ = case(b, n, m, k, "copies")
    # the input does what it is meant to: for some queries the copies are among the k nearest (then >= 200 points lie at or
    # under the K-th distance: more than the 128-entry buffer)
    cnt_at_kth = (sqdist_f32(sup, qry, np.broadcast_to(np.arange(n), (b, m, n))) <= wd[..., -1:]).sum(-1)
    assert (cnt_at_kth > 128).any() and (cnt_at_kth <= 128).any()
    check(P, b, n, m, k, "copies")
