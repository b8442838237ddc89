"""CPU: the numpy restatement of the SemanticKITTI test loop (tests/scan_flow_ref.py, the yardstick of ScanTester) pinned to
the reference's own generator `get_batch_gen('test')` (SemanticKITTI/semantic_kitti_dataset_grid.py:192-245, imported from
the reference tree with stub tensorflow / cpp_wrappers modules and a patched get_data, over in-memory scans with sklearn
trees), its vote lines to the float16 formula the kernel implements, and the committed golden run to the restatement."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

from scan_flow_ref import ScanFlowRef, scan, softmax_f32

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
REF_KITTI = os.path.join(REF, "SemanticKITTI")


def import_reference_dataset(monkeypatch):
    if not os.path.exists(os.path.join(REF_KITTI, "semantic_kitti_dataset_grid.py")):
        pytest.skip("reference tree absent")
    pytest.importorskip("yaml")
    tf = types.ModuleType("tensorflow")
    tf.float32, tf.int32 = "float32", "int32"
    cw = types.ModuleType("cpp_wrappers")
    cs = types.ModuleType("cpp_wrappers.cpp_subsampling")
    gs = types.ModuleType("cpp_wrappers.cpp_subsampling.grid_subsampling")
    cw.cpp_subsampling, cs.grid_subsampling = cs, gs
    for name, mod in (("tensorflow", tf), ("cpp_wrappers", cw), ("cpp_wrappers.cpp_subsampling", cs),
                      ("cpp_wrappers.cpp_subsampling.grid_subsampling", gs)):
        monkeypatch.setitem(sys.modules, name, mod)
    monkeypatch.chdir(REF_KITTI)  # the module reads semantic-kitti.yaml from the working directory
    spec = importlib.util.spec_from_file_location("_ref_semantic_kitti_dataset_grid", os.path.join(REF_KITTI, "semantic_kitti_dataset_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_equals_reference_generator(monkeypatch, tmp_path):
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = import_reference_dataset(monkeypatch)
    scans = [scan(900 + i, n) for i, n in enumerate((700, 450, 900))]
    paths = []
    for i, s in enumerate(scans):
        d = tmp_path / "08" / "velodyne"
        d.mkdir(parents=True, exist_ok=True)
        paths.append(str(d / f"{i:06d}.npy"))
        np.save(paths[-1], s)
    trees = {p: KDTree(s) for p, s in zip(paths, scans)}

    ds = mod.SemanticKITTIDataset.__new__(mod.SemanticKITTIDataset)
    ds.args = types.SimpleNamespace(num_point=64, num_buffer=24, in_radius=0, batch_size=2)
    ds.test_list, ds.possibility, ds.min_possibility = paths, [], []
    ds.get_data = lambda path: (np.array(trees[path].data, copy=False), trees[path], np.zeros(len(trees[path].data), np.uint8))

    seed = 11
    np.random.seed(seed)
    gen_func, _, _ = ds.get_batch_gen("test")
    ref = ScanFlowRef(scans, num_point=64, num_buffer=24, batch_size=2, rng=np.random.RandomState(seed))
    for a, b in zip(ds.possibility, ref.possibility):
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
    assert ds.min_possibility == ref.min_possibility

    ncrops = 0
    while ncrops < 300:  # several epochs of int(3/2)*2*4 = 8 crops, the generator restarted per epoch as test_init_op does
        for sel_pc, _, _, sel_idx, cloud in gen_func():
            cloud_ind, pick_idx, selected_idx = ref.crop()
            assert cloud_ind == int(cloud[0])
            np.testing.assert_array_equal(selected_idx.astype(np.int32), sel_idx)
            np.testing.assert_array_equal(scans[cloud_ind][selected_idx], sel_pc)
            for a, b in zip(ds.possibility, ref.possibility):
                np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
            np.testing.assert_array_equal(np.asarray(ds.min_possibility, np.float64).view(np.int64),
                                          np.asarray(ref.min_possibility, np.float64).view(np.int64))
            ncrops += 1
    assert ncrops >= 300
    # the loop's RNG stream is still in step
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)


def vote_formula(table, probs, inds, smooth=0.98):
    """the kernel's arithmetic, row by row: fp16((float)fp16(fp16(smooth) * old) + float32(1 - smooth) * p); repeated
    indices: the last row wins (every row reads the value before the crop)"""
    h, f = np.float16(smooth), np.float32(1 - smooth)
    old = table.copy()
    for j, i in enumerate(inds):
        prod = np.float16(np.float32(h) * old[i].astype(np.float32))
        table[i] = (prod.astype(np.float32) + f * probs[j]).astype(np.float16)


@pytest.mark.parametrize("smooth", [0.98, 0.9, 0.5])
def test_vote_lines_are_the_float16_formula(smooth):
    rng = np.random.default_rng(3)
    n, c, npt = 50, 7, 40
    ref = ScanFlowRef([scan(1, 300), scan(2, 300)], num_classes=c, num_point=npt, num_buffer=4, batch_size=3, test_smooth=smooth,
                      rng=np.random.RandomState(0))
    ref.test_probs = [(rng.random((n, c)) * 0.7).astype(np.float16), (rng.random((n, c))).astype(np.float16)]
    # rows near float16 rounding boundaries: old values with an odd last bit, probabilities on half-ulp steps
    ref.test_probs[0][:5] = np.float16(0.5) + np.arange(5)[:, None].astype(np.float16) * np.float16(2 ** -11)
    want = [t.copy() for t in ref.test_probs]
    probs = softmax_f32(rng.standard_normal((3, npt, c)) * 3)
    probs[0, :4] = np.float32(2 ** -12)
    inds = rng.integers(0, n, (3, npt)).astype(np.int32)
    inds[0, 10:20] = 7                       # repeated index inside a crop
    clouds = np.array([[0], [1], [0]], np.int32)  # crops 0 and 2 hit the same scan
    inds[2, :5] = inds[0, :5]
    ref.vote(probs, inds, clouds)
    for j in range(3):
        vote_formula(want[clouds[j, 0]], probs[j], inds[j], smooth)
    for a, b in zip(ref.test_probs, want):
        np.testing.assert_array_equal(a.view(np.uint16), b.view(np.uint16))


def test_golden_scan_flow_is_the_restatement():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scan_flow as M

    gold = np.load(os.path.join(HERE, "golden", "scan_flow.npz"))
    got = M.record()
    assert sorted(got) == sorted(gold.files)
    for k in gold.files:
        np.testing.assert_array_equal(got[k], gold[k], err_msg=k)
