"""GPU: the SemanticKITTI sliding-window whole-scan test loop on the device (csrc/kitti_window_test.hip,
pointasnl_amd.SemanticKITTI.window_tester and the drop-in dataset class) against the numpy restatement
tests/kitti_window_flow_ref.py run live on the same machine (it is pinned to the reference class in
tests/test_kitti_window_tester_flow.py) and the golden run tests/golden/kitti_window_flow.npz.  Every comparison is exact --
bit patterns or integers -- but the rotation's, which is held to one float32 ulp."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import kitti_window_flow_ref as R
from kitti_window_flow_ref import KittiWindowFlowRef, scan
from scan_flow_ref import stand_in_forward_np

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C = 20


@pytest.fixture(scope="module")
def W():
    from pointasnl_amd.SemanticKITTI import window_tester as W

    return W


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def host(t):
    return t.cpu().numpy()


def labels_of(seed, n):
    return np.random.default_rng(seed).integers(0, C, n).astype(np.int32)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def device_windows(xyz, block, stride, shape=None, woff=None, cap=None, slack=0):
    """pasnl_window_bounds -> pasnl_kwindow_count -> pasnl_kwindow_fill, called directly -> bounds (6,), (nx, ny), counts,
    the filled buffer (cap + slack entries, -7 where nothing was written)"""
    from pointasnl_amd import _hip

    n = xyz.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    b = torch.zeros((6,), dtype=torch.float32, device="cuda")
    _hip.launch("pasnl_window_bounds", "bounds", ctypes.c_long(n), ptr(x), ptr(b))
    bh = host(b)
    nx, ny = R.grid(bh[0:3], bh[3:6], stride) if shape is None else shape
    hist = torch.empty((int(_hip.lib().pasnl_kwindow_hist_bytes(ctypes.c_long(n), nx, ny)) // 4,), dtype=torch.int32, device="cuda")
    cnt = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
    _hip.launch("pasnl_kwindow_count", "count", ctypes.c_long(n), ptr(x), ptr(b), nx, ny, ctypes.c_double(block), ctypes.c_double(stride),
                ptr(hist), ptr(cnt))
    counts = host(cnt).astype(np.int64)
    if woff is None:
        woff = np.cumsum(counts) - counts
    cap = int(counts.sum()) if cap is None else cap
    out = torch.full((cap + slack,), -7, dtype=torch.int32, device="cuda")
    wo = torch.from_numpy(np.asarray(woff, np.int32)).cuda()
    _hip.launch("pasnl_kwindow_fill", "fill", ctypes.c_long(n), ptr(x), ptr(b), nx, ny, ctypes.c_double(block), ctypes.c_double(stride),
                ptr(hist), ptr(wo), ctypes.c_long(cap), ptr(out))
    return bh, (nx, ny), counts, host(out)


def check_windows(xyz, block, stride, shape=None):
    coordmin, coordmax, grid, members, _ = R.windows(xyz, block, stride, shape)
    bh, dgrid, counts, filled = device_windows(xyz, block, stride, shape)
    np.testing.assert_array_equal(bits(bh), bits(np.concatenate([coordmin, coordmax])))
    assert dgrid == grid
    np.testing.assert_array_equal(counts, [len(m) for m in members])  # empty windows: 0
    np.testing.assert_array_equal(filled, np.concatenate(members))
    return grid, counts, members


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_counts_and_member_lists_equal_the_restatement(n):
    """D:289-307 at the sizes where the chunking of 64 points per wave turns: one point (no extent: one window is forced),
    a wave short of one point, one full wave, one point into the second wave, 65 waves in 17 workgroups"""
    if n == 1:
        check_windows(np.array([[3.0, -2.0, 0.5]], np.float32), 10, 4, shape=(1, 1))
        return
    grid, counts, _ = check_windows(scan(30 + n, n, edge=min(8, n // 8))[0], 10, 4)
    assert grid == (7, 5) and counts.sum() > 3 * n


def test_more_than_64_windows_per_axis():
    """3000 points over 30 m with 1 m windows every 0.25 m: 120 x 120 windows, some of them empty, 47 waves"""
    pts = scan(41, 3000, 30.0, 30.0)[0]
    grid, counts, _ = check_windows(pts, 1.0, 0.25)
    assert grid == (120, 120) and np.count_nonzero(counts == 0) > 100 and counts.max() < 64


def test_points_beside_the_bounds_and_on_a_lattice():
    """curmin - 0.2 and curmax + 0.2 are float64 values no float32 equals (0.2 has no finite binary expansion), so the points
    that decide the comparison are the float32 values beside a bound: for every window bound of both axes the nearest float32
    and one ulp to either side are in the scan, and a float32 comparison would sort some of them to the wrong side.  The
    snapped scan puts thousands of points on the 0.05 m lattice that 0.2, 4 and 10 are multiples of."""
    pts = scan(42, 2000)[0]
    coordmin, coordmax = R.bounds(pts)
    extra = []
    for a in range(2):
        for i in range(7 if a == 0 else 5):
            curmin, curmax = R.window_box(coordmin, coordmax, i, i, 10, 4)
            for b in (curmin[a] - 0.2, curmax[a] + 0.2):
                if not coordmin[a] < b < coordmax[a]:
                    continue
                f = np.float32(b)
                for v in (np.nextafter(f, np.float32(-1e9)), f, np.nextafter(f, np.float32(1e9))):
                    p = pts[len(extra)].copy()
                    p[a] = v
                    extra.append(p)
    assert len(extra) > 30
    both = np.concatenate([pts, np.array(extra, np.float32)])
    np.testing.assert_array_equal(bits(np.concatenate(R.bounds(both))), bits(np.concatenate([coordmin, coordmax])))
    check_windows(both, 10, 4)
    snapped = scan(43, 5000, snapped=True)[0]
    check_windows(snapped, 10, 4)
    check_windows(snapped, 10, 3.3)


def test_one_window_skipped_windows_and_the_cap():
    pts = scan(44, 700, 3.0, 2.5, edge=0)[0]  # less than one stride wide: all points in the one window
    grid, counts, members = check_windows(pts, 10, 4)
    assert grid == (1, 1) and counts.tolist() == [700] and np.array_equal(members[0], np.arange(700))
    pts = scan(45, 3001)[0]
    _, _, _, members, _ = R.windows(pts, 10, 4)
    counts = np.array([len(m) for m in members])
    # woff = -1 skips: every third window is left out, the others are laid out in REVERSE window order
    keep = [w for w in range(35) if w % 3 != 0][::-1]
    woff = np.full(35, -1, np.int64)
    at = 0
    for w in keep:
        woff[w] = at
        at += counts[w]
    _, _, dcounts, filled = device_windows(pts, 10, 4, woff=woff, cap=at, slack=100)
    np.testing.assert_array_equal(dcounts, counts)
    np.testing.assert_array_equal(filled[:at], np.concatenate([members[w] for w in keep]))
    assert (filled[at:] == -7).all()
    # cap: nothing is written at or past it, whatever the offsets promise
    total, cap = int(counts.sum()), int(counts.sum()) // 2 + 3
    _, _, _, filled = device_windows(pts, 10, 4, cap=cap, slack=total)
    np.testing.assert_array_equal(filled[:cap], np.concatenate(members)[:cap])
    assert (filled[cap:] == -7).all()


def test_windows_equal_the_golden_run(W):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_kitti_window_flow as M

    gold = np.load(os.path.join(HERE, "golden", "kitti_window_flow.npz"))
    pts, rem = M.scan_points()
    t = W.KittiWindowTester([pts], labels=[M.labels()], remissions=[rem], num_classes=M.NUM_CLASSES, block_points=M.BLOCK_POINTS,
                            block_size=M.BLOCK_SIZE, stride=M.STRIDE, min_block_points=M.MIN_BLOCK_POINTS,
                            rng=np.random.RandomState(int(gold["seed"][0])))
    gmin, gmax, (nx, ny), counts, members = t.window_lists(0)
    np.testing.assert_array_equal(bits(gmin), bits(gold["coordmin"]))
    np.testing.assert_array_equal(bits(gmax), bits(gold["coordmax"]))
    assert [nx, ny] == gold["grid"].tolist()
    np.testing.assert_array_equal(counts, gold["counts"])
    member_bits = np.zeros((nx * ny, M.N), bool)
    at = 0
    for w in range(nx * ny):
        m = members[at:at + counts[w]]
        assert np.all(np.diff(m) > 0)
        member_bits[w, m] = True
        at += counts[w]
    np.testing.assert_array_equal(np.packbits(member_bits, axis=1), gold["members"])
    data, idx = t.blocks(0)
    assert data.shape[1:] == (M.BLOCK_POINTS, 4) and data.shape[0] * M.BLOCK_POINTS >= counts.sum()


def tie_proof(counts, min_block_points, block_points):
    """the merge's ties cannot end in a ragged chunk: all small windows together stay a small block, every other window can be
    made up to block_points on its own"""
    small = counts[counts <= min_block_points]
    return 0 < small.sum() <= min_block_points and counts[counts > min_block_points].min() >= block_points // 2


@pytest.mark.parametrize("with_remission", [False, True])
def test_gather_rows_remission_stale_rows_and_indices(W, with_remission):
    """D:334-351 through `blocks`, then a batch that runs past the last row: zeros there (data and indices)"""
    n, P = 5000, 256
    pts, rem = scan(50, n)
    kw = dict(num_classes=C, block_points=P, min_block_points=64)
    t = W.KittiWindowTester([pts], remissions=[rem] if with_remission else None, rng=np.random.RandomState(3), **kw)
    ref = KittiWindowFlowRef([pts], None, [rem] if with_remission else None, rng=np.random.RandomState(3), **kw)
    for vote in range(2):
        want = ref.getitem(0)
        got = [host(a) for a in t.blocks(0)]
        assert tie_proof(np.array([len(m) for m in ref.last["members"]]), 64, P)
        assert got[0].dtype == np.float32 and got[0].shape == want[0].shape == (want[1].shape[0], P, 4 if with_remission else 3)
        np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
        np.testing.assert_array_equal(got[1].astype(np.int64), want[1])
        assert len(ref.last["parts"]) < len(ref.last["members"])  # something was merged
    want = ref.getitem(0)
    prep = t.prepare(0)
    rows = prep["rows"]
    data, idx = (host(a) for a in t.gather(0, prep, rows - 2, 5))
    np.testing.assert_array_equal(bits(data[:2]), bits(want[0][rows - 2:]))
    np.testing.assert_array_equal(idx[:2], want[1][rows - 2:])
    assert not data[2:].any() and not idx[2:].any()
    assert ref.rng.randint(1 << 30) == t.rng.randint(1 << 30)


def ulps_apart(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def test_rotation_is_within_one_ulp_of_the_float64_product(W):
    """T:160-161: the reference rotates a float64 batch with np.dot (a dgemm, whose summation order is not specified) and
    stores float32.  A float64 rounding difference can only move a result that lies on a float32 rounding boundary, so the
    device's float64 x*cos - y*sin, rounded once, is at most one float32 ulp away; z and the remission are untouched."""
    n, P, B = 5000, 256, 4
    pts, rem = scan(51, n)
    pts = (pts * np.float32(3.7) - np.float32(40.0)).astype(np.float32)  # lidar-sized coordinates, both signs
    t = W.KittiWindowTester([pts], remissions=[rem], block_points=P, batch_size=B, min_block_points=64, block_size=37, stride=14.8,
                            rng=np.random.RandomState(5))
    prep = t.prepare(0)
    plain, idx0 = (host(a) for a in t.gather(0, prep, 0, B))
    angles = np.array([np.random.RandomState(6).uniform() * 2 * np.pi, 0.0, np.pi / 2, 5.1])
    data, idx = (host(a) for a in t.gather(0, prep, 0, B, angles=angles))
    want = R.rotate_z(plain[:, :, :3].astype(np.float64), angles)
    np.testing.assert_array_equal(idx, idx0)
    assert ulps_apart(data[:, :, :3], want).max() <= 1.0
    np.testing.assert_array_equal(bits(data[:, :, 2:]), bits(plain[:, :, 2:]))
    np.testing.assert_array_equal(bits(data[1]), bits(plain[1]))  # angle 0: cos 1, sin 0
    assert np.abs(data[0, :, :2] - plain[0, :, :2]).max() > 1.0


@pytest.mark.parametrize("accumulate,rotate", [(False, False), (True, False), (False, True)])
def test_run_end_to_end_against_restatement(W, accumulate, rotate):
    """T:108-231 over two scans and two votes, rows of 256 in batches of 3.  The forward is stand_in_forward_np's device twin
    with ties and NaN rows injected; its logits differ from numpy's by a few ulps, so the restatement is fed the device's own
    logits batch by batch -- after checking that it asks for exactly the batch the device was given (zero rows included;
    within one ulp where the batch was rotated) -- which leaves the loop, not the sine, under test."""
    sizes, P, B, votes = (5000, 6001), 256, 3, 2
    scans, rems = zip(*[scan(80 + i, n) for i, n in enumerate(sizes)])
    labs = [labels_of(80 + i, n) for i, n in enumerate(sizes)]
    labs[1][labs[1] == 13] = 2  # a class one scan does not hold
    kw = dict(num_classes=C, block_points=P, batch_size=B, min_block_points=64, accumulate_votes=accumulate, random_rotate=rotate)
    t = W.KittiWindowTester(list(scans), labels=labs, remissions=list(rems), rng=np.random.RandomState(6), **kw)
    ref = KittiWindowFlowRef(list(scans), labs, list(rems), rng=np.random.RandomState(6), **kw)
    wrng = np.random.default_rng(1)
    w, b = (wrng.standard_normal((3, C)) * 0.9).astype(np.float32), wrng.standard_normal(C).astype(np.float32)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    log = []

    def forward(x):
        assert x.shape == (B, P, 4)
        lg = torch.sin(x[:, :, :3] @ wt + bt) * 4.0
        k = len(log)
        if k % 3 == 0:
            lg[0, :100, 5] = 7.0
            lg[0, :100, 9] = 7.0        # ties: the first maximum
            lg[2, :50, 0] = 99.0        # class 0 is never predicted
        if k % 4 == 1:
            lg[1, 7, :] = float("nan")  # a NaN row: numpy's argmax takes the first NaN
            lg[1, 8, 11] = float("nan")
            lg[0, 9, 1:] = float("-inf")
        log.append((x.clone(), lg.clone()))
        return lg

    fed = t.run(forward, num_votes=votes)
    replay = iter(log)

    def forward_np(x):
        xd, lg = next(replay)
        if rotate:
            assert ulps_apart(x, host(xd)).max() <= 1.0
        else:
            np.testing.assert_array_equal(bits(x), bits(host(xd)))
        lg = host(lg)
        ok = np.isfinite(lg) & (lg != 7.0) & (lg != 99.0)
        # the sine's argument reaches 60 at these coordinates: six float32 roundings of up to half an ulp of 64 (3.8e-6) each
        # are 2.3e-5, times 4 and the sine's own last bits: under 2e-4
        assert np.abs(lg - stand_in_forward_np(host(xd)[:, :, :3], w, b))[ok].max() < 2e-4
        return lg

    ref.run(forward_np, num_votes=votes)
    assert next(replay, None) is None and fed > 2 * votes * 60 and any(x[B - 1].abs().max() == 0 for x, _ in log)
    for i in range(2):
        np.testing.assert_array_equal(host(t.pool(i)), ref.pools[i])
        per_vote = ref.pools[i].sum() / (votes if accumulate else 1)
        assert per_vote % P == 0 and per_vote > 3 * sizes[i]  # the pool holds one vote's rows, or both votes'
        np.testing.assert_array_equal(host(t.pred_label(i)), ref.pred[i])
        assert t.label_array(i).dtype == np.uint32
        np.testing.assert_array_equal(t.label_array(i), ref.pred[i])
        for a, c in zip(t.scan_counts(i), ref.counts[i]):
            np.testing.assert_array_equal(a, c)
        iou, mean = t.scan_iou(i)
        want_iou, want_mean = R.scan_iou(*ref.counts[i])
        np.testing.assert_array_equal(bits(iou), bits(want_iou))
        assert mean == want_mean
    for a, c in zip(t.totals(), ref.total):
        np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(bits(t.class_iou()), bits(np.array(ref.total[1][1:]) / (np.array(ref.total[2][1:], dtype=float) + 1e-6)))
    got, want = t.tenth_scan_figures(0), ref.logged[0]
    assert sorted(got) == sorted(want)
    for key in want:
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(want[key]))
    assert ref.rng.randint(1 << 30) == t.rng.randint(1 << 30)


@pytest.mark.parametrize("split,with_remission", [("valid", True), ("test", False)])
def test_dataset_class_is_the_drop_in(split, with_remission):
    """`__getitem__` alone: the reference's tuple, and the RNG advanced exactly as the restatement's"""
    from pointasnl_amd.SemanticKITTI.semantic_kitti_dataset import SemanticKittiDatasetSlidingWindow

    sizes = (5000, 5503)
    scans, rems = zip(*[scan(70 + i, n) for i, n in enumerate(sizes)])
    labs = [labels_of(70 + i, n) for i, n in enumerate(sizes)]
    ds = SemanticKittiDatasetSlidingWindow(list(scans), labels=labs if split == "valid" else None, remissions=list(rems), sample_points=256,
                                           stride=4, split=split, with_remission=with_remission, rng=np.random.RandomState(8),
                                           min_block_points=64)
    ref = KittiWindowFlowRef(list(scans), labs, list(rems) if with_remission else None, block_points=256, min_block_points=64,
                             rng=np.random.RandomState(8))
    assert len(ds) == 2
    for i in (1, 0, 1):
        got, want = ds[i], ref.getitem(i)
        assert len(got) == (4 if split == "valid" else 3)
        for a, b, dt in zip(got, want, (np.float32, np.int64)):
            assert a.dtype == b.dtype == dt and a.shape == b.shape
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(got[2]), bits(scans[i]))
        if split == "valid":
            assert got[3].dtype == np.int32 and np.array_equal(got[3], labs[i])
    assert ds.tester.rng.randint(1 << 30) == ref.rng.randint(1 << 30)


def test_error_paths(W):
    pts, rem = scan(1, 5000)
    lab = labels_of(1, 5000)
    with pytest.raises(ValueError):  # blocks of a few hundred points in rows of 8192: the make-up slice falls short
        W.KittiWindowTester([pts], block_points=8192, min_block_points=64, rng=np.random.RandomState(0)).blocks(0)
    with pytest.raises(ValueError):  # 100 points, under 4096 memberships: every block is small
        W.KittiWindowTester([pts[:100]], rng=np.random.RandomState(0)).blocks(0)
    flat = pts.copy()
    flat[:, 1] = 2.0
    with pytest.raises(ValueError):  # zero extent in y: no window at all
        W.KittiWindowTester([flat], block_points=256, min_block_points=10, rng=np.random.RandomState(0)).blocks(0)
    with pytest.raises(ValueError):
        W.KittiWindowTester([np.hstack([pts, pts])], labels=[lab])
    with pytest.raises(ValueError):
        W.KittiWindowTester([pts], labels=[lab + 30])
    with pytest.raises(ValueError):
        W.KittiWindowTester([pts], remissions=[rem[:10]])
    t = W.KittiWindowTester([pts], block_points=256, min_block_points=64, rng=np.random.RandomState(0))  # split 'test': no scores
    assert t.run(lambda x: torch.zeros((6, 256, C), device="cuda"), num_votes=1) > 60
    assert (t.label_array(0) == 1).all() and t.counts == {}
