"""CPU: the numpy restatement of the ScanNet grid test and validation loops (tests/scene_flow_ref.py, the yardstick of
SceneTester) pinned to the reference's own generator `ScannetDataset.get_batch_gen` (ScanNet/scannet_dataset_grid.py:435-549,
imported from the reference tree with stub tensorflow / cpp_wrappers / ply_helper / mesh modules, over in-memory scenes
with sklearn trees), its vote, label, confusion and IoU lines to the literal reference expressions, and the committed
golden run to the restatement."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

import scene_flow_ref as R
from scene_flow_ref import SceneFlowRef, scene, softmax_f32

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
REF_SCANNET = os.path.join(REF, "ScanNet")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference_dataset(monkeypatch):
    if not os.path.exists(os.path.join(REF_SCANNET, "scannet_dataset_grid.py")):
        pytest.skip("reference tree absent")
    tf = types.ModuleType("tensorflow")
    tf.float32, tf.int32 = "float32", "int32"
    ply = types.ModuleType("ply_helper")
    ply.read_ply = ply.write_ply = None
    mesh = types.ModuleType("mesh")
    mesh.rasterize_mesh = None
    cw = types.ModuleType("cpp_wrappers")
    cs = types.ModuleType("cpp_wrappers.cpp_subsampling")
    gs = types.ModuleType("cpp_wrappers.cpp_subsampling.grid_subsampling")
    cw.cpp_subsampling, cs.grid_subsampling = cs, gs
    for name, mod in (("tensorflow", tf), ("ply_helper", ply), ("mesh", mesh), ("cpp_wrappers", cw),
                      ("cpp_wrappers.cpp_subsampling", cs), ("cpp_wrappers.cpp_subsampling.grid_subsampling", gs)):
        monkeypatch.setitem(sys.modules, name, mod)
    monkeypatch.setattr(sys, "path", list(sys.path))  # the module appends to sys.path
    return _load("_ref_scannet_dataset_grid", os.path.join(REF_SCANNET, "scannet_dataset_grid.py"))


SIZES, NPOINT, BUFFER, SEED = (700, 450, 900), 64, 24, 11
LABEL_VALUES = np.array([0, 1, 2, 4, 7, 9])


@pytest.mark.parametrize("split", ["test", "validation"])
def test_restatement_equals_reference_generator(monkeypatch, split):
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = import_reference_dataset(monkeypatch)
    pc = [scene(900 + i, n) for i, n in enumerate(SIZES)]
    scenes, colors = [p for p, _ in pc], [c for _, c in pc]
    lrng = np.random.default_rng(2)
    labels = [lrng.choice(LABEL_VALUES, n).astype(np.int32) for n in SIZES]
    kcap = NPOINT + BUFFER + BUFFER // 4 - 1
    assert all(n >= kcap for n in SIZES)  # no crop can fall under k: nothing is skipped

    ds = mod.ScannetDataset.__new__(mod.ScannetDataset)
    ds.npoint, ds.buffer = NPOINT, BUFFER
    ds.input_trees = {split: [KDTree(s, leaf_size=50) for s in scenes]}
    ds.input_colors = {split: colors}
    ds.input_labels = {split: labels}
    ds.label_values = LABEL_VALUES
    ds.label_to_idx = {l: i for i, l in enumerate(LABEL_VALUES)}
    config = types.SimpleNamespace(in_radius=0, batch_size=2, validation_size=5, epoch_steps=5)

    np.random.seed(SEED)
    gen_func, _, _ = ds.get_batch_gen(split, config)
    ref = SceneFlowRef(scenes, colors=colors, labels=labels, num_classes=len(LABEL_VALUES), num_point=NPOINT, num_buffer=BUFFER,
                       batch_size=2, split=split, validation_size=5, label_values=LABEL_VALUES, rng=np.random.RandomState(SEED))
    bits = lambda a: np.ascontiguousarray(a).view(np.int64 if np.asarray(a).dtype == np.float64 else np.int32)  # noqa: E731
    for a, b in zip(ds.potentials[split], ref.potentials):
        np.testing.assert_array_equal(bits(a), bits(b))
    assert ds.min_potentials[split] == ref.min_potentials

    ncrops = 0
    while ncrops < 300:  # epochs of validation_size * batch_size = 10 crops, the generator restarted per epoch as the init op does
        for pts, feats, lab, lens, inds, cloud, weights in gen_func():
            c = ref.crop()
            assert c["cloud_ind"] == int(cloud) and lens == [NPOINT]
            np.testing.assert_array_equal(c["input_inds"], inds)
            assert pts.dtype == np.float32 and c["input_points"].dtype == np.float32
            np.testing.assert_array_equal(bits(c["input_points"]), bits(pts))
            assert feats.shape == (NPOINT, 6) and feats.dtype == c["features"].dtype
            np.testing.assert_array_equal(bits(c["features"]), bits(feats))
            # what TF makes of the float64 feature columns: float32 -- the device's colour and abs_coords columns
            np.testing.assert_array_equal(bits(c["features"].astype(np.float32)), bits(feats.astype(np.float32)))
            np.testing.assert_array_equal(c["labels"], lab)
            for a, b in zip(ds.potentials[split], ref.potentials):
                np.testing.assert_array_equal(bits(a), bits(b))
            np.testing.assert_array_equal(bits(np.asarray(ds.min_potentials[split], np.float64)),
                                          bits(np.asarray(ref.min_potentials, np.float64)))
            ncrops += 1
    assert ncrops >= 300
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)  # the RNG streams are still in step


def vote_formula(table, probs, inds, smooth):
    """the kernel's arithmetic, row by row: f32(f32(smooth) * old) + f32(f32(1 - smooth) * p); repeated indices: the last
    row wins (every row reads the value before the crop)"""
    a, b = np.float32(smooth), np.float32(1 - smooth)
    old = table.copy()
    for j, i in enumerate(inds):
        table[i] = (a * old[i]).astype(np.float32) + (b * probs[j]).astype(np.float32)


@pytest.mark.parametrize("split", ["test", "validation"])
def test_vote_lines_are_the_float32_formula(split):
    rng = np.random.default_rng(3)
    n, c, npt = 50, 7, 40
    ref = SceneFlowRef([scene(1, 300)[0], scene(2, 300)[0]], num_classes=c, num_point=npt, num_buffer=4, batch_size=3, split=split,
                       label_values=np.arange(c), rng=np.random.RandomState(0))
    assert ref.test_smooth == (0.98 if split == "test" else 0.95)
    ref.test_probs = [(rng.random((n, c - 1)) * 0.7).astype(np.float32), rng.random((n, c - 1)).astype(np.float32)]
    want = [t.copy() for t in ref.test_probs]
    probs = softmax_f32(rng.standard_normal((3, npt, c)) * 3)[:, :, 1:].copy()
    inds = rng.integers(0, n, (3, npt)).astype(np.int32)
    inds[0, 10:20] = 7                              # a repeated index inside a crop
    clouds = np.array([0, 1, 0], np.int32)          # crops 0 and 2 hit the same scene
    inds[2, :5] = inds[0, :5]
    ref.vote(probs, inds, clouds)
    for j in range(3):
        vote_formula(want[clouds[j]], probs[j], inds[j], ref.test_smooth)
    for a, b in zip(ref.test_probs, want):
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("ignored", [(0,), (4,), (0, 7)])
def test_label_confusion_and_iou_lines_are_the_reference_expressions(ignored):
    sk = pytest.importorskip("sklearn.metrics")
    if not os.path.exists(os.path.join(REF, "utils", "metrics.py")):
        pytest.skip("reference tree absent")
    metrics = _load("_ref_metrics", os.path.join(REF, "utils", "metrics.py"))
    rng = np.random.default_rng(5)
    lv = LABEL_VALUES
    nc = len(lv) - len(ignored)
    n = 400
    pts = scene(3, n)[0]
    ref = SceneFlowRef([pts], num_classes=nc + 1, num_point=8, num_buffer=4, batch_size=1, label_values=lv, ignored_labels=ignored,
                       rng=np.random.RandomState(0))
    tab = rng.random((n, nc)).astype(np.float32)
    tab[:, 2] *= 0.01                      # a class that is (almost) never predicted
    tab[:20, 0] = tab[:20, 3] = 2.0        # ties: the first maximum
    tab[20:30] = 0                         # all-zero rows: the first column of the expanded row, an ignored one when it leads
    ref.test_probs[0] = tab
    proj = rng.integers(0, n, 900)
    proj[:50] = 17                         # a repeated index
    preds, pots, probs = ref.reproject(0, proj)
    # T:190-205, literally
    p0 = tab[proj, :]
    p2 = p0.copy()
    for l_ind, label_value in enumerate(lv):
        if label_value in ignored:
            p2 = np.insert(p2, l_ind, 0, axis=1)
    np.testing.assert_array_equal(preds, lv[np.argmax(p2, axis=1)].astype(np.int32))
    np.testing.assert_array_equal(pots, ref.potentials[0][proj])
    np.testing.assert_array_equal(probs, p0)
    assert preds.dtype == np.int32 and pots.dtype == np.float64 and probs.dtype == np.float32
    # targets: one class absent (lv[-1]), a label outside label_values (5)
    targets = rng.choice(np.append(lv[:-1], 5), 900).astype(np.int32)
    C = R.confusion(targets, preds, lv)
    np.testing.assert_array_equal(C, sk.confusion_matrix(targets, preds, labels=lv))
    assert C.sum() == np.count_nonzero(np.isin(targets, lv)) < 900
    Cd = R.drop_ignored(C, lv, ignored)
    assert Cd.shape == (nc, nc)
    want = metrics.IoU_from_confusions(Cd)
    np.testing.assert_array_equal(R.iou_from_confusions(Cd), want)
    assert Cd[-1].sum() == 0 and want[-1] > 0  # the absent class takes the mean of the present ones


def test_golden_scene_flow_is_the_restatement():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scene_flow as M

    gold = np.load(os.path.join(HERE, "golden", "scene_flow.npz"))
    got = M.record()
    assert sorted(got) == sorted(gold.files)
    for k in gold.files:
        np.testing.assert_array_equal(got[k], gold[k], err_msg=k)
    assert len(gold["test_checkpoints"]) >= 1 and len(gold["validation_checkpoints"]) >= 2  # both rules fire in the run
    kcap = M.NUM_POINT + M.NUM_BUFFER + M.NUM_BUFFER // 4 - 1
    assert all(n >= kcap for _, n in M.SCENES)
