"""CPU: the numpy restatement of the SemanticKITTI sliding-window whole-scan test loop (tests/kitti_window_flow_ref.py, the
yardstick of KittiWindowTester) pinned to the reference's own class `SemanticKittiDatasetSlidingWindow`
(SemanticKITTI/semantic_kitti_dataset.py, imported from the reference tree, built with __new__ over a stub scan object), the
batched merge to the literal loop, its vote, pool reset, final_preds, count, IoU and every-tenth-scan lines to the literal
reference expressions, and the committed golden run to the restatement."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

import kitti_window_flow_ref as R
from kitti_window_flow_ref import KittiWindowFlowRef, scan

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
REF_DIR = os.path.join(REF, "SemanticKITTI")
C = 20


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


class StubScan:
    """what the reference class reads of auxiliary.laserscan.SemLaserScan"""

    def __init__(self, points, remissions, labels):
        self._points, self._remissions, self._labels = points, remissions, labels

    def open_scan(self, name):
        self.points, self.remissions = self._points[int(name)], self._remissions[int(name)]

    def open_label(self, name):
        self.sem_label = self._labels[int(name)]


def reference_dataset(points, remissions, labels, split, with_remission, sample_points=8192, block_size=10, stride=4):
    if not os.path.exists(os.path.join(REF_DIR, "semantic_kitti_dataset.py")):
        pytest.skip("reference tree absent")
    sys.path.insert(0, REF_DIR)  # `from auxiliary import laserscan`
    try:
        spec = importlib.util.spec_from_file_location("_ref_semantic_kitti_dataset", os.path.join(REF_DIR, "semantic_kitti_dataset.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(REF_DIR)
    ds = mod.SemanticKittiDatasetSlidingWindow.__new__(mod.SemanticKittiDatasetSlidingWindow)
    ds.split, ds.stride, ds.block_size, ds.block_points, ds.should_map, ds.with_remission = split, stride, block_size, sample_points, False, with_remission
    ds.scan = StubScan(points, remissions, labels)
    ds.points_name = ds.label_name = [str(k) for k in range(len(points))]
    return ds


def labels_of(seed, n):
    return np.random.default_rng(seed).integers(0, C, n).astype(np.int32)


@pytest.mark.parametrize("split,with_remission", [("valid", False), ("valid", True), ("test", False), ("test", True)])
def test_restatement_equals_reference_class(split, with_remission):
    """60 000 points over 30 m x 30 m at stride 4: 8 x 8 windows, the inner ones above 4096 points, the outer ones merged"""
    seed, n = 5, 60000
    pts, rem = scan(seed, n, 30.0, 30.0, edge=0)
    lab = labels_of(seed, n)
    ds = reference_dataset([pts], [rem], [lab], split, with_remission)
    ref = KittiWindowFlowRef([pts], [lab], [rem] if with_remission else None, num_classes=C, rng=np.random.RandomState(seed))
    np.random.seed(seed)
    for vote in range(2):
        want = ds[0]
        got = ref.getitem(0)
        assert len(want) == (3 if split == "test" else 4)
        for a, b, dt in zip(got, want, (np.float32, np.int64)):
            assert a.dtype == b.dtype == dt and a.shape == b.shape
            np.testing.assert_array_equal(bits(a), bits(b))
        assert got[0].shape[1:] == (8192, 4 if with_remission else 3) and want[2] is pts
        sizes = [len(m) for m in ref.last["members"]]
        assert len(sizes) == 64 and len(ref.last["parts"]) < 64 and max(sizes) > 4096  # real merges into real blocks
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)  # the RNG streams are still in step


def lattice(nx, ny, stride, block, origin=(-77.29800415039062, 51.06399917602539)):
    return [(np.array([origin[0] + i * stride, origin[1] + j * stride]) + np.array([origin[0] + i * stride + block, origin[1] + j * stride + block])) / 2.0
            for i in range(nx) for j in range(ny)]


@pytest.mark.parametrize("kind", ["lattice", "lattice_3.3", "random"])
def test_batched_merge_equals_the_literal_loop(kind):
    """by final parts: the batched distance expression has the bits of the per-centre np.linalg.norm, so argsort sees the
    same array and breaks every tie the same way"""
    from pointasnl_amd.SemanticKITTI import window_tester as W

    rng = np.random.default_rng(3)
    if kind == "random":
        centers = [c for c in rng.random((400, 2)) * 160.0 - 80.0]
    else:
        centers = lattice(22, 19, 4 if kind == "lattice" else 3.3, 10)
    sizes = np.where(rng.random(len(centers)) < 0.6, 0, rng.integers(0, 9000, len(centers)))  # mostly empty, as a lidar scan's
    want = R.merge(sizes, centers, 4096)
    assert 1 < len(want) < len(centers) / 2  # most windows were merged away
    assert R.merge(sizes, centers, 4096, nearest=R.nearest_batched) == want
    assert W.merge_blocks(sizes, np.array(centers), 4096) == want
    assert W.merge_blocks(sizes, np.array(centers), 4096, nearest=W.nearest_block_literal) == want
    center = centers[7]
    d = np.array(centers) - center
    np.testing.assert_array_equal(bits(W.batched_norms(d)), bits(np.array([np.linalg.norm(c - center, ord=2) for c in centers])))
    assert W.batched_norm_agrees() and W.batched_norm_agrees(3.3)


def test_value_errors_fire_where_the_reference_crashes():
    seed, n = 9, 30000
    pts, rem = scan(seed, n, 16.0, 16.0, edge=0)
    lab = labels_of(seed, n)
    # (a) a block of about 12 000 points dealt out in rows of 32 768: the make-up slice is shorter than makeup_num, the
    # chunks are ragged and the reference's np.concatenate of the split data fails
    ds = reference_dataset([pts], [rem], [lab], "test", False, sample_points=32768)
    np.random.seed(seed)
    with pytest.raises(ValueError):
        ds[0]
    with pytest.raises(ValueError):
        KittiWindowFlowRef([pts], None, None, block_points=32768, rng=np.random.RandomState(seed)).getitem(0)
    with pytest.raises(ValueError):
        R.draw_rows(100, 256, np.random.RandomState(0))
    assert len(R.draw_rows(128, 256, np.random.RandomState(0))) == 256
    # (b) 300 points, fewer than 4096 memberships in all: the last block is popped too and the reference indexes an empty argsort
    ds = reference_dataset([pts[:300]], [rem[:300]], [lab[:300]], "test", False)
    with pytest.raises(IndexError):
        ds[0]
    with pytest.raises(ValueError):
        KittiWindowFlowRef([pts[:300]], None, None, rng=np.random.RandomState(seed)).getitem(0)
    with pytest.raises(ValueError):
        R.merge([10, 0, 30], lattice(3, 1, 4, 10), 4096)


def stand_in(batch, w, b):
    return (np.sin(batch[:, :, :3].astype(np.float32) @ w + b) * 4.0).astype(np.float32)


@pytest.mark.parametrize("accumulate", [False, True])
def test_vote_reset_final_preds_counts_and_logged_figures_are_the_reference_expressions(accumulate):
    """T:140-231 evaluated literally over the blocks the restatement dealt out (11 scans: the every-tenth-scan branch runs
    at scans 0 and 10, the second time on the labelweights T:224 renormalised the first time)"""
    S, P, B, votes = 11, 64, 3, 2
    scans = [scan(20 + k, 300 + 7 * k, 9.0, 9.0, edge=0)[0] for k in range(S)]
    labs = [labels_of(20 + k, len(s)) % (C - 2) for k, s in enumerate(scans)]  # two classes absent
    wrng = np.random.default_rng(1)
    w, b = (wrng.standard_normal((3, C)) * 0.9).astype(np.float32), wrng.standard_normal(C).astype(np.float32)
    items = []

    class Logged(KittiWindowFlowRef):
        def getitem(self, i):
            out = KittiWindowFlowRef.getitem(self, i)
            items.append(out)
            return out

    def forward(batch):
        lg = stand_in(batch, w, b)
        lg[0, :5, 0] = 99.0                 # class 0 is never predicted
        lg[1, :5, 3] = lg[1, :5, 7] = 50.0  # ties: the first maximum
        lg[2, 5, 4] = np.nan                # numpy's argmax takes the first NaN
        return lg

    ref = Logged(scans, labs, None, num_classes=C, block_points=P, batch_size=B, min_block_points=32, rng=np.random.RandomState(4),
                 accumulate_votes=accumulate)
    ref.run(forward, num_votes=votes)
    assert len(items) == S * votes

    def add_vote(vote_label_pool, point_idx, pred_label):  # T:99-105
        for bb in range(pred_label.shape[0]):
            for n in range(pred_label.shape[1]):
                vote_label_pool[int(point_idx[bb, n]), int(pred_label[bb, n])] += 1
        return vote_label_pool

    NUM_CLASSES, BATCH_SIZE, NUM_POINT = C, B, P
    total_correct, total_seen = 0, 0
    total_seen_class, total_correct_class, total_iou_deno_class = ([0 for _ in range(NUM_CLASSES)] for _ in range(3))
    labelweights = np.zeros(NUM_CLASSES)
    replay = iter(items)
    for batch_idx in range(S):
        t_seen_class, t_correct_class, t_iou_deno_class = ([0 for _ in range(NUM_CLASSES)] for _ in range(3))
        whole_scene_data, whole_scene_label = scans[batch_idx], labs[batch_idx]
        for vote_idx in range(votes):
            scene_data, scene_point_index = next(replay)
            num_blocks = scene_data.shape[0]
            s_batch_num = (num_blocks + BATCH_SIZE - 1) // BATCH_SIZE
            batch_data = np.zeros((BATCH_SIZE, NUM_POINT, 3))
            batch_point_index = np.zeros((BATCH_SIZE, NUM_POINT))
            for sbatch in range(s_batch_num):
                start_idx = sbatch * BATCH_SIZE
                end_idx = min((sbatch + 1) * BATCH_SIZE, num_blocks)
                real_batch_size = end_idx - start_idx
                batch_data[0:real_batch_size, ...] = scene_data[start_idx:end_idx, ...]
                batch_point_index[0:real_batch_size, ...] = scene_point_index[start_idx:end_idx, ...]
                pred_val = forward(batch_data)
                batch_pred_label = np.argmax(pred_val[:, :, 1:], 2) + 1
                if sbatch == 0 and (vote_idx == 0 or not accumulate):
                    vote_label_pool = np.zeros((whole_scene_data.shape[0], NUM_CLASSES))
                vote_label_pool = add_vote(vote_label_pool, batch_point_index[0:real_batch_size, ...], batch_pred_label[0:real_batch_size, ...])
        final_preds = np.argmax(vote_label_pool, axis=1)
        final_preds = final_preds.astype(np.uint32)
        np.testing.assert_array_equal(ref.pools[batch_idx], vote_label_pool)
        assert ref.pred[batch_idx].dtype == np.uint32
        np.testing.assert_array_equal(ref.pred[batch_idx], final_preds)
        correct = np.sum(final_preds == whole_scene_label)
        seen = len(whole_scene_label)
        total_correct += correct
        total_seen += seen
        tmp, _ = np.histogram(whole_scene_label, range(NUM_CLASSES + 1))
        labelweights += tmp
        for l in range(NUM_CLASSES):
            tem_seen = np.sum(whole_scene_label == l)
            t_seen_class[l] += tem_seen
            total_seen_class[l] += tem_seen
            temp_correct = np.sum((final_preds == l) & (whole_scene_label == l))
            temp_iou_deno_class = np.sum((final_preds == l) | (whole_scene_label == l))
            total_correct_class[l] += temp_correct
            t_correct_class[l] += temp_correct
            total_iou_deno_class[l] += temp_iou_deno_class
            t_iou_deno_class[l] += temp_iou_deno_class
        iou = np.array(t_correct_class[1:]) / (np.array(t_iou_deno_class[1:], dtype=float) + 1e-6)
        arr = np.array(t_seen_class[1:])
        mIoU = np.mean(iou[arr != 0])
        for got, want in zip(ref.counts[batch_idx], (t_seen_class, t_correct_class, t_iou_deno_class)):
            np.testing.assert_array_equal(got, np.array(want))
        g_iou, g_mean = R.scan_iou(*ref.counts[batch_idx])
        np.testing.assert_array_equal(bits(g_iou), bits(iou))
        assert g_mean == mIoU
        if batch_idx % 10 == 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                logged = ref.logged[batch_idx]
                assert logged["miou"] == np.mean(np.array(total_correct_class[1:]) / (np.array(total_iou_deno_class[1:], dtype=float) + 1e-6))
                assert logged["accuracy"] == total_correct / float(total_seen)
                assert logged["class_accuracy"] == np.mean(np.array(total_correct_class) / (np.array(total_seen_class, dtype=float) + 1e-6))
                labelweights = labelweights.astype(np.float32) / np.sum(labelweights.astype(np.float32))
                for l in range(1, NUM_CLASSES):
                    assert logged["labelweights"][l - 1] == labelweights[l - 1]
                    np.testing.assert_array_equal(logged["iou"][l - 1], total_correct_class[l] / float(total_iou_deno_class[l]))
    assert sorted(ref.logged) == [0, 10] and next(replay, None) is None
    assert ref.logged[10]["labelweights"].dtype == np.float32
    for got, want in zip(ref.total, (total_seen_class, total_correct_class, total_iou_deno_class)):
        np.testing.assert_array_equal(got, np.array(want))
    # the same counts from a confusion matrix (rows the truth), as the device derives them
    m = np.zeros((C, C), np.int64)
    np.add.at(m, (labs[3], ref.pred[3].astype(np.int64)), 1)
    np.testing.assert_array_equal(m.sum(1), ref.counts[3][0])
    np.testing.assert_array_equal(np.diagonal(m), ref.counts[3][1])
    np.testing.assert_array_equal(m.sum(0) + m.sum(1) - np.diagonal(m), ref.counts[3][2])


def test_rotation_is_the_providers_and_draws_one_uniform_per_row():
    if not os.path.exists(os.path.join(REF, "utils", "provider.py")):
        pytest.skip("reference tree absent")
    import types

    spec = importlib.util.spec_from_file_location("_ref_provider", os.path.join(REF, "utils", "provider.py"))
    provider = importlib.util.module_from_spec(spec)
    absent = importlib.util.find_spec("h5py") is None
    if absent:
        sys.modules["h5py"] = types.ModuleType("h5py")  # imported at the top of provider.py for its file readers only
    try:
        spec.loader.exec_module(provider)
    finally:
        if absent:
            del sys.modules["h5py"]
    batch = np.random.default_rng(0).standard_normal((4, 50, 3)) * 30.0
    np.random.seed(11)
    want = provider.rotate_point_cloud_z(batch)
    rng = np.random.RandomState(11)
    got = R.rotate_z(batch, [rng.uniform() * 2 * np.pi for _ in range(4)])
    assert want.dtype == got.dtype == np.float32
    np.testing.assert_array_equal(bits(got), bits(want))
    assert np.random.randint(1 << 30) == rng.randint(1 << 30)


def test_golden_kitti_window_flow_is_the_restatement():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_kitti_window_flow as M

    path = os.path.join(HERE, "golden", "kitti_window_flow.npz")
    gold = np.load(path)
    assert os.path.getsize(path) < 64 * 1024
    pts, rem = M.scan_points()
    ref = KittiWindowFlowRef([pts], [M.labels()], [rem], num_classes=M.NUM_CLASSES, block_points=M.BLOCK_POINTS, block_size=M.BLOCK_SIZE,
                             stride=M.STRIDE, min_block_points=M.MIN_BLOCK_POINTS, rng=np.random.RandomState(int(gold["seed"][0])))
    data, idx = ref.getitem(0)
    last = ref.last
    np.testing.assert_array_equal(bits(last["coordmin"]), bits(gold["coordmin"]))
    np.testing.assert_array_equal(bits(last["coordmax"]), bits(gold["coordmax"]))
    assert [last["nx"], last["ny"]] == gold["grid"].tolist()
    counts = np.array([len(m) for m in last["members"]])
    np.testing.assert_array_equal(counts, gold["counts"])
    np.testing.assert_array_equal(M.pack(last["members"], M.N), gold["members"])
    # the scan is built so that the merge's ties cannot end in a ragged chunk: small windows exist, and even all together
    # they stay a small block; every other window can be made up to block_points on its own
    small = counts[counts <= M.MIN_BLOCK_POINTS]
    assert 0 < small.sum() <= M.MIN_BLOCK_POINTS and counts[counts > M.MIN_BLOCK_POINTS].min() >= M.BLOCK_POINTS // 2
    assert len(last["parts"]) == np.count_nonzero(counts > M.MIN_BLOCK_POINTS) and data.shape[1:] == (M.BLOCK_POINTS, 4)
    assert np.bincount(idx.ravel(), minlength=M.N).min() >= 1  # every point is dealt out


def test_kitti_window_entries_are_declared_exported_and_importable():
    """the feature's surface: four C-ABI entries and the two Python modules"""
    from pointasnl_amd import _hip
    from pointasnl_amd.SemanticKITTI import semantic_kitti_dataset, window_tester

    names = ["pasnl_kwindow_hist_bytes", "pasnl_kwindow_count", "pasnl_kwindow_fill", "pasnl_kwindow_gather"]
    header = open(os.path.join(os.path.dirname(HERE), "include", "pasnl.h")).read()
    lib = _hip.lib()
    for name in names:
        assert name in _hip.SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert lib.pasnl_kwindow_hist_bytes(ctypes.c_long(120000), 73, 73) == 73 * 73 * 1875 * 4  # no limit of 64 per axis
    assert lib.pasnl_kwindow_hist_bytes(ctypes.c_long(120000), 50000, 50000) == 0                # positions past int32
    null, d = ctypes.c_void_p(0), ctypes.c_double
    assert lib.pasnl_kwindow_count(ctypes.c_long(100), null, null, 50000, 50000, d(10), d(4), null, null, null) == -5
    assert lib.pasnl_kwindow_count(ctypes.c_long(100), null, null, 73, 73, d(10), d(4), null, null, null) == -2    # NULL buffers
    assert lib.pasnl_kwindow_count(ctypes.c_long(100), null, null, 73, 73, d(10), d(0), null, null, null) == -1    # stride 0
    assert lib.pasnl_kwindow_fill(ctypes.c_long(100), null, null, 73, 73, d(10), d(4), null, null, ctypes.c_long(5), null, null) == -2
    assert lib.pasnl_kwindow_gather(0, 0, 8, null, ctypes.c_long(1), null, ctypes.c_long(5), null, null, 0, null, null, null, null) == 0
    assert lib.pasnl_kwindow_gather(1, 1, 8, null, ctypes.c_long(1), null, ctypes.c_long(5), null, null, 2, null, null, null, null) == -1
    assert semantic_kitti_dataset.SemanticKittiDatasetSlidingWindow.__name__ == "SemanticKittiDatasetSlidingWindow"
    assert window_tester.merge_blocks([7, 0, 9], np.array(lattice(3, 1, 4, 10)), 8) == [[2, 1, 0]]
    with pytest.raises(ValueError):
        window_tester.merge_blocks([10, 20, 30], np.array(lattice(3, 1, 4, 10)), 4096)
    with pytest.raises(ValueError):
        window_tester.draw_rows(100, 256, np.random.RandomState(0))
