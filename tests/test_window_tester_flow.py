"""CPU: the numpy restatement of the ScanNet sliding-window whole-scene test loop (tests/window_flow_ref.py, the yardstick
of WindowTester) pinned to the reference's own class `ScannetDatasetWholeSceneSlidingWindow` (ScanNet/scannet_dataset.py,
imported from the reference tree, built with __new__ over in-memory scenes), its vote, argmax, count, IoU and export lines
to the literal reference expressions, and the committed golden run to the restatement."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

import window_flow_ref as R
from window_flow_ref import WindowFlowRef, scene

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
REF_FILE = os.path.join(REF, "ScanNet", "scannet_dataset.py")
C = 21


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def scene6(seed, n):
    p, c = scene(seed, n)
    return np.ascontiguousarray(np.hstack([p, c]))


def reference_dataset(points, labels, block_points, with_rgb):
    if not os.path.exists(REF_FILE):
        pytest.skip("reference tree absent")
    spec = importlib.util.spec_from_file_location("_ref_scannet_dataset", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ds = mod.ScannetDatasetWholeSceneSlidingWindow.__new__(mod.ScannetDatasetWholeSceneSlidingWindow)
    ds.split, ds.stride, ds.with_rgb, ds.block_points = "test", 0.5, with_rgb, block_points
    ds.scene_points_list, ds.semantic_labels_list, ds.labelweights = points, labels, np.ones(C)
    return ds


@pytest.mark.parametrize("n,block_points,with_rgb", [(60000, 8192, True), (60000, 8192, False), (30000, 2048, True),
                                                      (30000, 2048, False)])
def test_restatement_equals_reference_class(n, block_points, with_rgb):
    seed = 5
    labels = [np.random.default_rng(seed).integers(0, C, n).astype(np.int64)]
    theirs, ours = [scene6(seed, n)], [scene6(seed, n)]
    ds = reference_dataset(theirs, labels, block_points, with_rgb)
    ref = WindowFlowRef(ours, labels, num_classes=C, block_points=block_points, with_rgb=with_rgb, rng=np.random.RandomState(seed))
    np.random.seed(seed)
    for vote in range(3):  # the scene moves for good: every vote starts from the last one's points
        want = ds[0]
        got = ref.getitem(0)
        assert len(ref.last["found"]) == int(np.count_nonzero(ref.last["counts"]))
        for a, b, dt in zip(got, want, (np.float32, np.int32, np.float64, np.int64)):
            assert a.dtype == b.dtype == dt and a.shape == b.shape
            np.testing.assert_array_equal(bits(a), bits(b))
        assert got[0].shape[1:] == (block_points, 6 if with_rgb else 3)
        np.testing.assert_array_equal(bits(ours[0]), bits(theirs[0]))
        assert 0.5 < np.count_nonzero(got[2]) / got[2].size < 0.8  # about 0.65 of the rows carry a weight
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)  # the RNG streams are still in step


@pytest.mark.parametrize("n", [1000, 200003])
def test_mean_is_the_sequential_float32_sum(n):
    """the fact the device's centroid relies on: np.mean over axis 0 of a float32 (N,3) view, strided or not, is per column
    one float32 sum in index order divided by float32(N)"""
    pts = scene6(3, n)
    pts[:, 0:3] += np.float32(3.25)
    want = np.cumsum(pts[:, 0:3], axis=0, dtype=np.float32)[-1] / np.float32(n)
    for view in (pts[:, 0:3], np.ascontiguousarray(pts[:, 0:3])):
        got = np.mean(view, axis=0, keepdims=True)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(bits(got[0]), bits(want))
    if n <= 1000:
        np.testing.assert_array_equal(bits(R.sequential_mean_f32(pts[:, 0:3])), bits(want))


def test_move_keeps_the_last_of_a_repeated_choice():
    rng = np.random.RandomState(2)
    xyz = scene(4, 500)[0]
    before = xyz.copy()
    state = rng.get_state()
    choices, centroid, max_length = R.move(xyz, rng, noise_ratio=3.0)  # 1500 draws over 500 points: many repeats
    assert len(choices) == 1500 and len(np.unique(choices)) < 500 and max_length.dtype == np.float32
    rng.set_state(state)
    rng.choice(500, 1500)
    shift = (rng.randn(1500, 3) - 0.5) / 0.5 * 0.002
    last = R.last_occurrence(choices, 500)
    assert last.sum() == len(np.unique(choices))
    want = before.copy()
    normalized = (before - centroid) / max_length
    for j in np.flatnonzero(last):  # the device's formula, draw by draw
        i = choices[j]
        want[i] = ((normalized[i].astype(np.float64) + shift[j]) * np.float64(max_length) + centroid[0].astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(bits(xyz), bits(want))


def test_merge_is_the_reference_loop_and_raises_where_it_crashes():
    centers = [np.array([x, 0.75]) for x in (0.75, 1.3, 1.75, 2.25, 2.8)]  # off the lattice: no equal distances
    # 100 goes to its nearest neighbour (4096 -> 4196, now large enough); 10 goes to the block left of it
    assert R.merge([5000, 100, 4096, 9000, 10], centers, 4096) == [[0], [2, 1], [3, 4]]
    assert R.merge([7, 9], centers[:2], 8) == [[1, 0]]
    with pytest.raises(ValueError):
        R.merge([], [], 4096)
    with pytest.raises(ValueError):
        R.merge([10], centers[:1], 4096)
    with pytest.raises(ValueError):
        R.merge([10, 20, 30], centers[:3], 4096)  # the last block left is itself small
    flat = scene6(1, 300)
    flat[:, 0] = 1.0  # zero extent in x
    with pytest.raises(ValueError):
        WindowFlowRef([flat], [np.zeros(300, np.int64)], block_points=64, min_block_points=8, rng=np.random.RandomState(0)).getitem(0)


def test_vote_count_iou_and_export_lines_are_the_reference_expressions():
    rng = np.random.default_rng(7)
    B, N, npts = 3, 50, 40
    pred_val = rng.standard_normal((B, N, C)).astype(np.float32)
    pred_val[0, :10, 0] = 99.0                    # class 0 is never predicted
    pred_val[1, :10, 3] = pred_val[1, :10, 7] = 50.0   # ties: the first maximum
    pred_val[2, 5, 4] = np.nan                    # numpy's argmax takes the first NaN
    pred_val[2, 6, 1:] = -np.inf
    point_idx = rng.integers(0, npts, (B, N))
    point_idx[0, :8] = 3                          # repeated points
    weight = (rng.random((B, N)) < 0.65).astype(np.float64)
    # T:159 and add_vote (T:96-103), literally
    batch_pred_label = np.argmax(pred_val[:, :, 1:], 2) + 1
    vote_label_pool = np.zeros((npts, C))
    for b in range(B):
        for n in range(N):
            if weight[b, n]:
                vote_label_pool[int(point_idx[b, n]), int(batch_pred_label[b, n])] += 1
    np.testing.assert_array_equal(R.predict(pred_val), batch_pred_label)
    assert batch_pred_label[2, 5] == 4 and batch_pred_label[2, 6] == 1 and batch_pred_label[1, 0] == 3
    pool = R.add_vote(np.zeros((npts, C)), point_idx, batch_pred_label, weight)
    np.testing.assert_array_equal(pool, vote_label_pool)
    # T:163-175, literally
    pred_label = np.argmax(vote_label_pool, 1)
    whole_scene_label = rng.integers(0, C - 2, npts)  # two classes absent
    seen, correct, deno = [0] * C, [0] * C, [0] * C
    for l in range(C):
        seen[l] += np.sum((whole_scene_label == l))
        correct[l] += np.sum((pred_label == l) & (whole_scene_label == l))
        deno[l] += np.sum(((pred_label == l) | (whole_scene_label == l)) & (whole_scene_label > 0))
    got = R.class_counts(whole_scene_label, pred_label, C)
    for a, b in zip(got, (seen, correct, deno)):
        np.testing.assert_array_equal(a, np.array(b))
    iou_map = np.array(correct) / (np.array(deno, dtype=float) + 1e-6)
    tmp_iou = np.mean(iou_map[np.array(seen) != 0])
    g_map, g_mean = R.scene_iou(*got)
    np.testing.assert_array_equal(bits(g_map), bits(iou_map))
    assert g_mean == tmp_iou
    np.testing.assert_array_equal(bits(R.class_iou(got[1], got[2])), bits(np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)))
    # the same counts from a confusion matrix (rows the truth), as the device derives them
    m = np.zeros((C, C), np.int64)
    np.add.at(m, (whole_scene_label, pred_label), 1)
    np.testing.assert_array_equal(m.sum(1), got[0])
    np.testing.assert_array_equal(np.diagonal(m), got[1])
    np.testing.assert_array_equal(m[1:].sum(0) + np.where(np.arange(C) > 0, m.sum(1) - np.diagonal(m), 0), got[2])
    # T:179-180, literally
    ids = rng.permutation(90)[:npts]
    whole_scene_data = np.zeros(90)
    whole_scene_data[ids] = R.TEST_CLASS[pred_label.astype(np.int32)]
    np.testing.assert_array_equal(R.export(pred_label, ids, 90), whole_scene_data)
    assert R.TEST_CLASS.shape == (21,) and R.TEST_CLASS[-1] == 39


def test_golden_window_flow_is_the_restatement():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_window_flow as M

    gold = np.load(os.path.join(HERE, "golden", "window_flow.npz"))
    assert os.path.getsize(os.path.join(HERE, "golden", "window_flow.npz")) < 400 * 1024
    pts = [M.scene_points()]
    ref = WindowFlowRef(pts, [M.labels()], num_classes=M.NUM_CLASSES, block_points=M.BLOCK_POINTS, stride=M.STRIDE,
                        rng=np.random.RandomState(int(gold["seed"][0])))
    ref.getitem(0)
    np.testing.assert_array_equal(bits(pts[0][:, 0:3]), bits(gold["moved1"]))
    ref.getitem(0)
    np.testing.assert_array_equal(bits(pts[0][:, 0:3]), bits(gold["moved2"]))
    last = ref.last
    np.testing.assert_array_equal(bits(last["coordmin"]), bits(gold["coordmin"]))
    np.testing.assert_array_equal(bits(last["coordmax"]), bits(gold["coordmax"]))
    assert [last["nx"], last["ny"]] == gold["grid"].tolist()
    np.testing.assert_array_equal(last["counts"], gold["counts"])
    assert np.count_nonzero(gold["counts"] > 4096) >= 1 and np.count_nonzero((gold["counts"] > 0) & (gold["counts"] <= 4096)) >= 1
    nwin = last["nx"] * last["ny"]
    np.testing.assert_array_equal(M.pack(last["found"], nwin, M.N, "members"), gold["members"])
    np.testing.assert_array_equal(M.pack(last["found"], nwin, M.N, "masks"), gold["masks"])


def test_window_entries_are_declared_exported_and_importable():
    """the feature's surface: eight C-ABI entries and the two Python modules"""
    from pointasnl_amd import _hip
    from pointasnl_amd.ScanNet import scannet_dataset, window_tester

    names = ["pasnl_window_noise", "pasnl_window_bounds", "pasnl_window_hist_bytes", "pasnl_window_count", "pasnl_window_fill",
             "pasnl_window_gather", "pasnl_window_vote", "pasnl_window_pool_labels"]
    lib = _hip.lib()
    for name in names:
        assert name in _hip.SYMBOLS and hasattr(lib, name)
    assert lib.pasnl_version() == 100
    assert lib.pasnl_window_hist_bytes(ctypes.c_long(200000), 13, 11) == 13 * 11 * 3125 * 4
    null = ctypes.c_void_p(0)
    assert lib.pasnl_window_hist_bytes(ctypes.c_long(120000), 73, 73) == 73 * 73 * 1875 * 4  # no limit of 64 per axis
    assert lib.pasnl_window_hist_bytes(ctypes.c_long(120000), 50000, 50000) == 0                # positions past int32
    assert lib.pasnl_window_count(ctypes.c_long(100), null, null, 50000, 50000, ctypes.c_double(0.5), null, null, null) == -5
    assert lib.pasnl_window_count(ctypes.c_long(100), null, null, 65, 3, ctypes.c_double(0.5), null, null, null) == -2  # > 64 per axis
    assert lib.pasnl_window_count(ctypes.c_long(100), null, null, 4, 3, ctypes.c_double(0.5), null, null, null) == -2
    assert lib.pasnl_window_vote(1, 8, 1, null, null, null, ctypes.c_long(5), null, null) == -1            # c < 2
    assert lib.pasnl_window_gather(0, 0, 8, null, ctypes.c_long(1), null, null, ctypes.c_long(5), null, null, 0, null, null, 1, null, null,
                                   null, null, null) == 0                                                  # no rows: a no-op
    assert np.array_equal(window_tester.TEST_CLASS, R.TEST_CLASS)
    assert scannet_dataset.ScannetDatasetWholeSceneSlidingWindow.__name__ == "ScannetDatasetWholeSceneSlidingWindow"
    assert window_tester.merge_blocks([7, 9], [np.array([0.75, 0.75]), np.array([1.25, 0.75])], 8) == [[1, 0]]
    with pytest.raises(ValueError):
        window_tester.merge_blocks([10, 20, 30], [np.array([x, 0.75]) for x in (0.75, 1.25, 1.75)], 4096)
