"""GPU: the ScanNet sliding-window whole-scene test loop on the device (csrc/window_test.hip,
pointasnl_amd.ScanNet.window_tester and the drop-in dataset class) against the numpy restatement tests/window_flow_ref.py
run live on the same machine (it is pinned to the reference class in tests/test_window_tester_flow.py) and the golden run
tests/golden/window_flow.npz.  Every comparison is exact: bit patterns or integers."""
import os
import sys

import numpy as np
import pytest
import torch

import window_flow_ref as R
from scan_flow_ref import stand_in_forward_np
from window_flow_ref import WindowFlowRef, scene

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C = 21


@pytest.fixture(scope="module")
def W():
    from pointasnl_amd.ScanNet import window_tester as W

    return W


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def host(t):
    return t.cpu().numpy()


def scene6(seed, n, snapped=False, scale=1.0):
    p, c = scene(seed, n, snapped)
    return np.ascontiguousarray(np.hstack([(p * np.float32(scale)).astype(np.float32), c]))


def labels_of(seed, n):
    return np.random.default_rng(seed).integers(0, C, n).astype(np.int64)


@pytest.mark.parametrize("n,noise_ratio,snapped", [(200003, 0.2, False), (4097, 0.2, False), (700, 3.0, False), (5000, 0.2, True),
                                                   (3, 0.2, False)])
def test_noise_step_moves_the_scene_bit_for_bit(W, n, noise_ratio, snapped):
    """D:192-212 after one, two and three votes: the sequential float32 centroid (200 003 points: 49 staged tiles), max_length,
    the float64 move with the last of a repeated choice winning (noise_ratio 3: every point drawn about three times), and the
    labels zeroed for that call only."""
    pts = scene6(40, n, snapped)
    lab = labels_of(40, n)
    t = W.WindowTester([pts], labels=[lab], noise_ratio=noise_ratio, rng=np.random.RandomState(9))
    rng = np.random.RandomState(9)
    xyz = pts[:, 0:3]  # a strided view, as the reference's
    for vote in range(3):
        serial = t.move(0)
        choices, centroid, max_length = R.move(xyz, rng, noise_ratio)
        if noise_ratio > 1:
            assert len(np.unique(choices)) < len(choices) / 2
        stats = host(t.stats)
        np.testing.assert_array_equal(bits(stats[0:3]), bits(centroid[0]))
        np.testing.assert_array_equal(bits(stats[3:4]), bits(np.asarray([max_length], np.float32)))
        np.testing.assert_array_equal(bits(host(t.points(0))), bits(xyz))
        seg = lab.astype(np.int32)
        seg[choices] = 0
        np.testing.assert_array_equal(np.where(host(t.stamp[0]) == serial, 0, lab), seg)
    assert rng.randint(1 << 30) == t.rng.randint(1 << 30)


def check_windows(t, i, xyz, stride=0.5):
    coordmin, coordmax, (nx, ny), counts, found = R.windows(xyz, stride)
    gmin, gmax, grid, gcounts, members, masks = t.window_lists(i)
    np.testing.assert_array_equal(bits(gmin), bits(coordmin))
    np.testing.assert_array_equal(bits(gmax), bits(coordmax))
    assert grid == (nx, ny)
    np.testing.assert_array_equal(gcounts, counts)
    np.testing.assert_array_equal(members, np.concatenate([m for _, m, _, _ in found]))
    np.testing.assert_array_equal(masks.astype(bool), np.concatenate([m for _, _, m, _ in found]))
    return counts, found


@pytest.mark.parametrize("seed,n,snapped,scale", [(50, 30000, False, 1.0), (51, 20000, True, 1.0), (52, 70001, False, 1.7),
                                                  (53, 640, True, 0.5), (54, 65, False, 1.0)])
def test_windows_are_the_reference_comparisons(W, seed, n, snapped, scale):
    """D:214-242: bounds, per-window counts, ascending member lists and the 0.001-margin masks; `snapped` puts the points of
    the unmoved scene on a 0.04 m lattice, so many sit exactly on a window's bound (0.2 and 0.5 are lattice multiples)."""
    pts = scene6(seed, n, snapped, scale)
    t = W.WindowTester([pts], labels=[labels_of(seed, n)], rng=np.random.RandomState(seed))
    counts, found = check_windows(t, 0, pts[:, 0:3])  # the scene as given
    if snapped and n > 1000:
        near = 0  # float32 lattice coordinates within rounding of a float64 bound: the comparison's dtype decides
        cmin = np.min(pts[:, 0:3], axis=0)
        for a in range(2):
            lo = cmin[a] + np.arange(12) * 0.5 - 0.2
            near += np.count_nonzero(np.abs(pts[:, a, None].astype(np.float64) - lo[None, :]) < 1e-6)
        assert near > 100
    rng = np.random.RandomState(seed)
    t.move(0)
    R.move(pts[:, 0:3], rng)
    check_windows(t, 0, pts[:, 0:3])  # and after a move


def test_windows_and_moves_equal_the_golden_reference_run(W):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_window_flow as M

    gold = np.load(os.path.join(HERE, "golden", "window_flow.npz"))
    t = W.WindowTester([M.scene_points()], labels=[M.labels()], num_classes=M.NUM_CLASSES, block_points=M.BLOCK_POINTS,
                       stride=M.STRIDE, rng=np.random.RandomState(int(gold["seed"][0])))
    t.blocks(0)
    np.testing.assert_array_equal(bits(host(t.points(0))), bits(gold["moved1"]))
    t.blocks(0)
    np.testing.assert_array_equal(bits(host(t.points(0))), bits(gold["moved2"]))
    gmin, gmax, (nx, ny), counts, members, masks = t.window_lists(0)
    np.testing.assert_array_equal(bits(gmin), bits(gold["coordmin"]))
    np.testing.assert_array_equal(bits(gmax), bits(gold["coordmax"]))
    assert [nx, ny] == gold["grid"].tolist()
    np.testing.assert_array_equal(counts, gold["counts"])
    member_bits, mask_bits = np.zeros((nx * ny, M.N), bool), np.zeros((nx * ny, M.N), bool)
    at = 0
    for w in range(nx * ny):
        m = members[at:at + counts[w]]
        assert np.all(np.diff(m) > 0)
        member_bits[w, m] = True
        mask_bits[w, m[masks[at:at + counts[w]] != 0]] = True
        at += counts[w]
    np.testing.assert_array_equal(np.packbits(member_bits, axis=1), gold["members"])
    np.testing.assert_array_equal(np.packbits(mask_bits, axis=1), gold["masks"])


@pytest.mark.parametrize("n,block_points,min_block_points,with_rgb,scale", [
    (60000, 8192, 4096, True, 1.0), (30000, 2048, 4096, False, 1.0), (30000, 2048, 4096, True, 1.0), (9000, 256, 300, True, 1.0),
    (9000, 256, 300, False, 1.0), (5000, 512, 1500, True, 0.5)])
def test_blocks_are_the_restatements_four_arrays(W, n, block_points, min_block_points, with_rgb, scale):
    """D:183-300 end to end, two consecutive votes; min_block_points 300 leaves many windows unmerged, 1500 on the halved
    scene merges most of them"""
    ours, theirs = scene6(60, n, scale=scale), scene6(60, n, scale=scale)
    lab = labels_of(60, n)
    kw = dict(num_classes=C, block_points=block_points, with_rgb=with_rgb, min_block_points=min_block_points)
    t = W.WindowTester([ours if with_rgb else ours[:, 0:3]], labels=[lab], rng=np.random.RandomState(3), **kw)
    ref = WindowFlowRef([theirs], [lab], rng=np.random.RandomState(3), **kw)
    for vote in range(2):
        want = ref.getitem(0)
        got = [host(a) for a in t.blocks(0)]
        assert got[0].dtype == np.float32 and got[0].shape == want[0].shape == (want[1].shape[0], block_points, 6 if with_rgb else 3)
        np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2].astype(np.float64), want[2])
        np.testing.assert_array_equal(got[3].astype(np.int64), want[3])
        np.testing.assert_array_equal(bits(host(t.points(0))), bits(theirs[:, 0:3]))
        assert len(ref.last["parts"]) < len(ref.last["found"])  # something was merged
    assert ref.rng.randint(1 << 30) == t.rng.randint(1 << 30)


@pytest.mark.parametrize("with_rgb", [True, False])
def test_dataset_class_is_the_drop_in(with_rgb):
    from pointasnl_amd.ScanNet.scannet_dataset import ScannetDatasetWholeSceneSlidingWindow

    sizes = (30000, 21000)
    ours, theirs = [scene6(70 + i, n) for i, n in enumerate(sizes)], [scene6(70 + i, n) for i, n in enumerate(sizes)]
    labs = [labels_of(70 + i, n) for i, n in enumerate(sizes)]
    ds = ScannetDatasetWholeSceneSlidingWindow(None, split="test", num_class=C, block_points=2048, with_rgb=with_rgb, stride=0.5,
                                               scene_points_list=ours, semantic_labels_list=labs, scene_points_id=[None] * 2,
                                               scene_points_num=list(sizes), rng=np.random.RandomState(8))
    ref = WindowFlowRef(theirs, labs, num_classes=C, block_points=2048, with_rgb=with_rgb, rng=np.random.RandomState(8))
    assert len(ds) == 2 and ds.point_num == list(sizes)
    for i in (1, 0, 1):
        got, want = ds[i], ref.getitem(i)
        for a, b, dt in zip(got, want, (np.float32, np.int32, np.float64, np.int64)):
            assert a.dtype == b.dtype == dt and a.shape == b.shape
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(ours[i]), bits(theirs[i]))  # scene_points_list[i] is left moved, colours untouched
    assert ds.tester.rng.randint(1 << 30) == ref.rng.randint(1 << 30)


def test_run_end_to_end_against_restatement(W):
    """T:107-196 over two scenes and three votes.  The forward is stand_in_forward_np's device twin with ties and NaN rows
    injected; its logits differ from numpy's by a few ulps, so the restatement is fed the device's own logits batch by
    batch -- after checking that it asks for exactly the batch the device was given (zero rows included) -- which leaves the
    loop, not the sine, under test."""
    sizes, P, B, votes = (12000, 9001), 1024, 4, 3
    ours, theirs = [scene6(80 + i, n) for i, n in enumerate(sizes)], [scene6(80 + i, n) for i, n in enumerate(sizes)]
    labs = [labels_of(80 + i, n) for i, n in enumerate(sizes)]
    labs[1][labs[1] == 13] = 2  # a class one scene does not hold
    kw = dict(num_classes=C, block_points=P, batch_size=B, min_block_points=1500)
    t = W.WindowTester(ours, labels=labs, rng=np.random.RandomState(6), **kw)
    ref = WindowFlowRef(theirs, labs, rng=np.random.RandomState(6), **kw)
    wrng = np.random.default_rng(1)
    w, b = (wrng.standard_normal((3, C)) * 0.9).astype(np.float32), wrng.standard_normal(C).astype(np.float32)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    log = []

    def forward(x):
        lg = torch.sin(x[:, :, :3] @ wt + bt) * 4.0
        k = len(log)
        if k % 3 == 0:
            lg[0, :200, 5] = 7.0
            lg[0, :200, 9] = 7.0        # ties: the first maximum
            lg[2, :100, 0] = 99.0       # class 0 is never predicted
        if k % 4 == 1:
            lg[1, 7, :] = float("nan")  # a NaN row: numpy's argmax takes the first NaN
            lg[1, 8, 11] = float("nan")
            lg[3, 9, 1:] = float("-inf")
        log.append((x.clone(), lg.clone()))
        return lg

    fed = t.run(forward, num_votes=votes)
    replay = iter(log)

    def forward_np(x):
        xd, lg = next(replay)
        np.testing.assert_array_equal(bits(x), bits(host(xd)))
        lg = host(lg)
        ok = np.isfinite(lg) & (lg != 7.0) & (lg != 99.0)
        assert np.abs(lg - stand_in_forward_np(x[:, :, :3], w, b))[ok].max() < 1e-4
        return lg

    ref.run(forward_np, num_votes=votes)
    assert next(replay, None) is None and fed > 2 * votes * 20 and any(x[B - 1].abs().max() == 0 for x, _ in log)
    ids = [np.random.default_rng(i).permutation(2 * n)[:n] for i, n in enumerate(sizes)]
    for i in range(2):
        np.testing.assert_array_equal(host(t.pool(i)), ref.pools[i])
        assert ref.pools[i].max() >= votes  # a point is voted by several windows per vote
        np.testing.assert_array_equal(host(t.pred_label(i)), ref.pred[i])
        for a, c in zip(t.scene_counts(i), ref.counts[i]):
            np.testing.assert_array_equal(a, c)
        iou_map, mean = t.scene_iou(i)
        want_map, want_mean = R.scene_iou(*ref.counts[i])
        np.testing.assert_array_equal(bits(iou_map), bits(want_map))
        assert mean == want_mean
        np.testing.assert_array_equal(t.export(i, ids[i], 2 * sizes[i]), R.export(ref.pred[i], ids[i], 2 * sizes[i]))
        np.testing.assert_array_equal(bits(host(t.points(i))), bits(theirs[i][:, 0:3]))
    for a, c in zip(t.totals(), ref.total):
        np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(bits(t.class_iou()), bits(R.class_iou(ref.total[1], ref.total[2])))
    assert ref.rng.randint(1 << 30) == t.rng.randint(1 << 30)


def test_error_paths(W):
    from pointasnl_amd.ScanNet.scannet_dataset import ScannetDatasetWholeSceneSlidingWindow

    pts, lab = scene6(1, 3000), labels_of(1, 3000)
    with pytest.raises(NotImplementedError):
        W.WindowTester([pts], labels=[lab], split="train")
    with pytest.raises(NotImplementedError):
        ScannetDatasetWholeSceneSlidingWindow(None, split="train", scene_points_list=[pts], semantic_labels_list=[lab])
    with pytest.raises(ValueError):  # 300 points, about 2 700 memberships: merged into one block that is still under 4096
        W.WindowTester([pts[:300]], labels=[lab[:300]], block_points=256, rng=np.random.RandomState(0)).blocks(0)
    flat = pts.copy()
    flat[:, 1] = 2.0
    with pytest.raises(ValueError):  # zero extent in y: no window at all
        W.WindowTester([flat], labels=[lab], block_points=256, min_block_points=10, noise_ratio=0.0, rng=np.random.RandomState(0)).blocks(0)
    with pytest.raises(ValueError):  # all points coincide: the noise step divides by zero
        W.WindowTester([np.ones((50, 6), np.float32)], labels=[lab[:50]], block_points=16, min_block_points=4,
                       rng=np.random.RandomState(0)).blocks(0)
    with pytest.raises(ValueError):
        W.WindowTester([pts[:, 0:3]], labels=[lab], with_rgb=True)
    with pytest.raises(ValueError):
        W.WindowTester([pts], labels=[lab + 30])
    with pytest.raises(ValueError):
        W.merge_blocks([], [])
    ok = W.WindowTester([pts], labels=[lab], block_points=256, min_block_points=200, rng=np.random.RandomState(0))
    assert ok.blocks(0)[0].shape[1:] == (256, 6)


def test_pool_argmax_takes_the_first_maximum_and_zero_without_a_vote():
    import ctypes

    from pointasnl_amd import _hip

    rng = np.random.default_rng(2)
    pool = rng.integers(0, 4, (5000, C)).astype(np.int32)
    pool[:100] = 0            # no vote at all: class 0
    pool[100:200, 0] = 0
    pool[100:200, 4] = pool[100:200, 17] = 9  # ties: the first maximum
    pd = torch.from_numpy(pool).cuda()
    out = torch.empty((5000,), dtype=torch.int32, device="cuda")
    _hip.launch("pasnl_window_pool_labels", "labels", ctypes.c_long(5000), C, ctypes.c_void_p(pd.data_ptr()), ctypes.c_void_p(out.data_ptr()))
    np.testing.assert_array_equal(host(out), np.argmax(pool.astype(np.float64), 1))
    assert host(out)[:100].max() == 0 and (host(out)[100:200] == 4).all()


def spread(seed, n, extent):
    """n points uniform over `extent` metres, with colours -> (n,6) f32"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.hstack([rng.random((n, 3)) * extent, rng.random((n, 3))]).astype(np.float32))


@pytest.mark.parametrize("n", [2, 63, 64, 65, 257])
def test_windows_at_every_chunking(W, n):
    """D:214-242 with a two-lane wave (the smallest scene that has a grid), a wave one short of full, a full
    one, one point past the wave boundary, and five chunks (two workgroups of four): counts, lists and masks are the
    restatement's.  One point has zero extent and raises as it always did."""
    pts = spread(70 + n, n, (2.6, 2.1, 1.5))
    with pytest.raises(ValueError, match="zero extent"):
        W.WindowTester([pts[:1]], labels=[labels_of(n, 1)], noise_ratio=0.0, rng=np.random.RandomState(n)).window_lists(0)
    t = W.WindowTester([pts], labels=[labels_of(n, n)], noise_ratio=0.0, rng=np.random.RandomState(n))
    counts, found = check_windows(t, 0, pts[:, 0:3])
    assert counts.sum() > n and len(found) >= 2  # windows overlap: a point is listed more than once


def test_more_than_64_windows_per_axis(W):
    """300 points over 34 m x 2 m at stride 0.5: 66 or more windows in x, which the 64-bit masks of the earlier kernels
    refused; most windows are empty for any one wave.  Lists and masks are the restatement's; and the count kernel stores
    only non-zero counts, so the entry point must clear a stale histogram itself."""
    import ctypes

    from pointasnl_amd import _hip

    n = 300
    pts = spread(81, n, (34.0, 2.0, 1.5))
    t = W.WindowTester([pts], labels=[labels_of(81, n)], noise_ratio=0.0, rng=np.random.RandomState(81))
    _, _, nx, ny = t.grid(0)
    assert nx > 64
    counts, found = check_windows(t, 0, pts[:, 0:3])  # (raises PasnlUnsupported if the limit came back)
    per_chunk = [np.bincount(m // 64, minlength=5) for _, m, _, _ in found]
    assert any((c == 0).any() for c in per_chunk)  # windows that are empty for some chunks: their cells are never stored
    hist = torch.full((int(_hip.lib().pasnl_window_hist_bytes(ctypes.c_long(n), nx, ny)) // 4,), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    cnt = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    _hip.launch("pasnl_window_count", "count", ctypes.c_long(n), p(t.xyz[0]), p(t.bounds), nx, ny, ctypes.c_double(0.5), p(hist), p(cnt))
    np.testing.assert_array_equal(host(cnt), counts)
