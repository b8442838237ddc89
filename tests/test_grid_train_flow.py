"""CPU: the numpy restatement of the two grid training input loops (tests/grid_train_flow_ref.py, the yardstick of
SceneTrainer and ScanTrainer) pinned to the reference's own generators -- `ScannetDataset.get_batch_gen('training')`
(ScanNet/scannet_dataset_grid.py:435-549) and `SemanticKITTIDataset.get_batch_gen('training')`
(SemanticKITTI/semantic_kitti_dataset_grid.py:193-292), imported from the reference tree as tests/test_scene_tester_flow.py
and tests/test_scan_tester_flow.py do -- the committed golden epoch to the restatement, and the surface of the feature:
the three C-ABI entries, their host-side validation, the modules."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

import grid_train_flow_ref as R
import test_scan_tester_flow as TK
import test_scene_tester_flow as TS
from scan_flow_ref import scan
from scene_flow_ref import scene

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIZES, NPOINT, BUFFER, SEED = (700, 450, 900), 64, 24, 11
KCAP = NPOINT + BUFFER + BUFFER // 4 - 1
LABEL_VALUES = np.array([0, 1, 2, 4, 7, 9])
LOSS_TOL = 1e-5  # * max(1, |ref|), tests/block_train_checks.py: numpy's log and exp against themselves on another machine


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def test_scene_restatement_equals_reference_generator(monkeypatch):
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = TS.import_reference_dataset(monkeypatch)
    split = "training"
    pc = [scene(900 + i, n) for i, n in enumerate(SIZES)]
    scenes, colors = [p for p, _ in pc], [c for _, c in pc]
    lrng = np.random.default_rng(2)
    labels = [lrng.choice(LABEL_VALUES, n).astype(np.int32) for n in SIZES]
    label_weights = np.array([0.0, 1.3, 0.7, 2.1, 1.0, 1.9])
    assert all(n >= KCAP for n in SIZES)  # no crop can fall under k: nothing is skipped

    ds = mod.ScannetDataset.__new__(mod.ScannetDataset)
    ds.npoint, ds.buffer = NPOINT, BUFFER
    ds.input_trees = {split: [KDTree(s, leaf_size=50) for s in scenes]}
    ds.input_colors = {split: colors}
    ds.input_labels = {split: labels}
    ds.label_values = LABEL_VALUES
    ds.label_to_idx = {l: i for i, l in enumerate(LABEL_VALUES)}
    ds.label_weights = label_weights
    config = types.SimpleNamespace(in_radius=0, batch_size=2, validation_size=7, epoch_steps=5)

    np.random.seed(SEED)
    gen_func, gen_types, _ = ds.get_batch_gen(split, config)
    assert config.augment_symmetries == [True, False, False] and config.augment_rotation == "vertical"
    assert (config.augment_scale_min, config.augment_scale_max, config.augment_scale_anisotropic) == (0.9, 1.1, True)
    assert (config.augment_noise, config.augment_color) == (0.001, 1.0)  # philox_ref.DEFAULT, grid_augment.TRAINING
    ref = R.SceneTrainFlowRef(scenes, labels, colors=colors, label_weights=label_weights, num_classes=len(LABEL_VALUES),
                              num_point=NPOINT, num_buffer=BUFFER, batch_size=2, epoch_steps=5, label_values=LABEL_VALUES,
                              rng=np.random.RandomState(SEED))
    for a, b in zip(ds.potentials[split], ref.potentials):
        np.testing.assert_array_equal(bits(a), bits(b))

    ncrops = 0
    while ncrops < 300:  # epochs of epoch_steps * batch_size = 10 crops; the potentials persist from epoch to epoch
        per_epoch = 0
        for pts, feats, lab, lens, inds, cloud, weights in gen_func():
            c = ref.crop()
            assert c["cloud_ind"] == int(cloud) and lens == [NPOINT]
            np.testing.assert_array_equal(c["input_inds"], inds)
            np.testing.assert_array_equal(bits(c["input_points"]), bits(pts))
            np.testing.assert_array_equal(bits(c["features"][:, :3].astype(np.float32)), bits(feats[:, :3].astype(np.float32)))
            np.testing.assert_array_equal(c["labels"], lab)
            assert (np.asarray(lab) >= 0).all() and (np.asarray(lab) < len(LABEL_VALUES)).all()
            np.testing.assert_array_equal(bits(np.asarray(c["weights"]).astype(np.float32)), bits(np.asarray(weights).astype(np.float32)))
            for a, b in zip(ds.potentials[split], ref.potentials):
                np.testing.assert_array_equal(bits(a), bits(b))
            np.testing.assert_array_equal(bits(np.asarray(ds.min_potentials[split], np.float64)),
                                          bits(np.asarray(ref.min_potentials, np.float64)))
            ncrops += 1
            per_epoch += 1
        assert per_epoch == 10
    assert ncrops >= 300
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)  # the RNG streams are still in step


def test_scan_restatement_equals_reference_generator(monkeypatch, tmp_path):
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = TK.import_reference_dataset(monkeypatch)
    sizes = SIZES + (520, 610, 480)
    assert all(n >= KCAP for n in sizes)
    scans = [scan(900 + i, n) for i, n in enumerate(sizes)]
    lrng = np.random.default_rng(2)
    labels = [lrng.integers(0, 5, n).astype(np.int32) for n in sizes]
    labelweights = np.array([0.0, 1.3, 0.7, 2.1, 1.0])
    paths = [str(tmp_path / "00" / "velodyne" / f"{i:06d}.npy") for i in range(len(scans))]
    trees = {p: KDTree(s) for p, s in zip(paths, scans)}
    lab_of = dict(zip(paths, labels))

    ds = mod.SemanticKITTIDataset.__new__(mod.SemanticKITTIDataset)
    ds.args = types.SimpleNamespace(num_point=NPOINT, num_buffer=BUFFER, in_radius=0, batch_size=2)
    ds.train_list, ds.labelweights = paths, labelweights
    ds.get_data = lambda path: (np.array(trees[path].data, copy=False), trees[path], lab_of[path])

    np.random.seed(SEED)
    gen_func, _, _ = ds.get_batch_gen("training")
    assert ds.args.augment_symmetries == [True, False, False]
    ref = R.ScanTrainFlowRef(scans, labels, label_weights=labelweights, num_classes=5, num_point=NPOINT, num_buffer=BUFFER,
                             batch_size=2, rng=np.random.RandomState(SEED))
    draws = []

    class Spy:  # the three draws per item, by name and in order
        def __getattr__(self, name):
            fn = getattr(np.random, name)

            def call(*a, **k):
                draws.append(name)
                return fn(*a, **k)

            return call

    ncrops = 0
    while ncrops < 300:  # epochs of int(6/2)*2 = 6 items, in list order
        order = []
        for sel_pc, sel_lab, w, sel_idx, cloud in gen_func():
            i = int(cloud[0])
            order.append(i)
            c = ref.crop(i)
            np.testing.assert_array_equal(c["selected_idx"].astype(np.int32), sel_idx)
            np.testing.assert_array_equal(bits(scans[i][c["selected_idx"]]), bits(sel_pc))
            np.testing.assert_array_equal(bits(c["selected_pc"].astype(np.float32)), bits(sel_pc))
            np.testing.assert_array_equal(c["labels"].astype(np.int32), sel_lab)
            assert w.dtype == np.float32
            np.testing.assert_array_equal(bits(c["weights"].astype(np.float32)), bits(w))
            ncrops += 1
        assert order == list(range(6))
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)
    # one more item with every draw named: choice, randint, shuffle
    ref.rng = Spy()
    ref.crop(0)
    assert draws == ["choice", "randint", "shuffle"]


def test_golden_grid_train_flow_is_the_restatement():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_grid_train_flow as M

    gold = np.load(os.path.join(HERE, "golden", "grid_train_flow.npz"))
    got = M.record()
    assert sorted(got) == sorted(gold.files)
    for k in gold.files:
        if k.endswith("loss_sum"):
            assert abs(got[k][0] - gold[k][0]) <= LOSS_TOL * max(1.0, abs(gold[k][0])), k
        else:
            np.testing.assert_array_equal(got[k], gold[k], err_msg=k)
    kcap = M.NUM_POINT + M.NUM_BUFFER + M.NUM_BUFFER // 4 - 1
    assert all(n >= kcap for _, n in M.SCENES + M.SCANS)
    for name in ("scene", "scan"):
        c, s, d = (int(v) for v in gold[name + "/totals"])
        assert 0 < c < s and d == 2 * s - c
    assert int(gold["scene/totals"][1]) == M.EPOCH_STEPS * M.BATCH * M.NUM_POINT
    assert int(gold["scan/totals"][1]) == 3 * M.BATCH * M.NUM_POINT and gold["scan/clouds"].max() == 5  # S = 7: the last is never drawn
    assert os.path.getsize(os.path.join(HERE, "golden", "grid_train_flow.npz")) < (1 << 20)


def test_epoch_tallies_recount_and_lines():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_grid_train_flow as M

    ref = M.refs()["scan"]
    w, b = R.stand_in_weights(M.STEP_SEED, M.CLASSES["scan"])
    logits = []

    def step(x, y, s):
        logits.append(R.stand_in_forward_np(x, w, b))
        return logits[-1]

    out = R.train_epoch(ref, step, M.CLASSES["scan"], seed=M.AUG_SEED)
    assert (out["total_correct"], out["total_seen"], out["total_iou_deno"]) == R.recount(out["labels"], logits)
    lines = R.report(out)
    assert lines[1] == "Training Accuracy: %f" % (out["total_correct"] / float(out["total_seen"]) * 100)
    assert lines[0].startswith("Training Loss: ") and lines[2].startswith("Training IoU: ")
    # the augmentation moved the points, and by no more than scale, symmetry and noise allow
    ref2 = M.refs()["scan"]
    plain = R.train_epoch(ref2, step, M.CLASSES["scan"], seed=None)
    for a, p in zip(out["fed"], plain["fed"]):
        assert (bits(a) != bits(p)).any()
        ra, rp = np.linalg.norm(a[:, :, :2], axis=2), np.linalg.norm(p[:, :, :2], axis=2)
        assert (ra <= rp * 1.1 + 0.01).all() and (ra >= rp * 0.9 - 0.01).all()
    np.testing.assert_array_equal(np.stack(out["inds"]), np.stack(plain["inds"]))  # the augmentation draws nothing from numpy


def test_new_symbols_are_declared_exported_and_validated():
    """the feature's surface: the three entries in the header and in `_hip.SYMBOLS`, outside the scope tests/abi_cases.py
    counts, their validation before any launch, and the Python modules"""
    import abi_cases
    from pointasnl_amd import _hip

    lib = _hip.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pasnl.h")).read(), flags=re.S)
    new = ("pasnl_scan_pick_given", "pasnl_scan_train_labels", "pasnl_scan_augment")
    for s in new:
        assert s in _hip.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, header)
        assert s.startswith(abi_cases.EXCLUDED_PREFIXES)
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(256)
    EINVAL, ENULL = -1, -2
    clouds = (ctypes.c_int * 3)(0, 2, 1)
    pg = lib.pasnl_scan_pick_given
    assert pg(-1, 3, some, some, clouds, some, some, some, null) == EINVAL
    assert pg(3, 0, some, some, clouds, some, some, some, null) == EINVAL
    assert pg(3, 2, some, some, clouds, some, some, some, null) == EINVAL      # cloud 2 outside [0, 2)
    assert pg(3, 3, some, some, (ctypes.c_int * 3)(0, -1, 1), some, some, some, null) == EINVAL
    assert pg(0, 3, null, null, null, null, null, null, null) == 0
    for k in range(6):
        args = [some, some, clouds, some, some, some]
        args[k] = null
        assert pg(3, 3, *args, null) == ENULL
    tl = lib.pasnl_scan_train_labels
    assert tl(-1, 8, some, some, some, some, some, 4, some, some, null) == EINVAL
    assert tl(1, 0, some, some, some, some, some, 4, some, some, null) == EINVAL
    assert tl(1, 8, some, some, some, some, some, -1, some, some, null) == EINVAL
    assert tl(0, 8, null, null, null, null, null, 4, null, null, null) == 0
    for k in (0, 1, 2, 3, 5, 6):  # weights (4) may be NULL
        args = [some, some, some, some, some, some, some]
        nw = 4
        args[k] = null
        assert tl(1, 8, *args[:5], nw, *args[5:], null) == ENULL
    au = lib.pasnl_scan_augment
    f = ctypes.c_float
    cfg = lambda rot=1, lo=0.9, hi=1.1, noise=0.001, color=1.0: (rot, f(lo), f(hi), 1, 1, 0, 0, f(noise), f(color),  # noqa: E731
                                                                  ctypes.c_ulonglong(7))
    assert au(-1, 8, 3, some, some, *cfg(), some, null, null, null) == EINVAL
    assert au(1, 0, 3, some, some, *cfg(), some, null, null, null) == EINVAL
    assert au(1, 8, 2, some, some, *cfg(), some, null, null, null) == EINVAL        # a row holds xyz at least
    assert au(1, 8, 3, some, some, *cfg(rot=2), some, null, null, null) == EINVAL   # neither 'vertical' nor 'none'
    assert au(1, 8, 3, some, some, *cfg(lo=1.2), some, null, null, null) == EINVAL
    assert au(1, 8, 3, some, some, *cfg(noise=-1.0), some, null, null, null) == EINVAL
    assert au(1, 8, 3, some, some, *cfg(color=float("nan")), some, null, null, null) == EINVAL
    assert au(0, 8, 3, null, null, *cfg(), null, null, null, null) == 0
    assert au(1, 8, 3, null, some, *cfg(), some, null, null, null) == ENULL
    assert au(1, 8, 3, some, null, *cfg(), some, null, null, null) == ENULL
    assert au(1, 8, 3, some, some, *cfg(), null, null, null, null) == ENULL         # item0 is required
    from pointasnl_amd import grid_augment
    from pointasnl_amd.ScanNet.scene_tester import SceneCrops, SceneTester
    from pointasnl_amd.ScanNet.scene_trainer import SceneTrainer
    from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer

    assert issubclass(SceneTester, SceneCrops) and issubclass(SceneTrainer, SceneCrops) and not issubclass(SceneTrainer, SceneTester)
    for cls in (SceneTrainer, ScanTrainer):
        for name in ("next_batch", "run", "totals", "accuracy", "iou", "mean_loss", "report"):
            assert hasattr(cls, name)
    import philox_ref as P

    assert grid_augment.host_config(grid_augment.config_of()) == P.DEFAULT
    assert "Philox4x32-10" in grid_augment.__doc__ and "counter" in grid_augment.__doc__
    with pytest.raises(ValueError, match="Unknown rotation augmentation"):
        grid_augment.config_of(dict(augment_rotation="all"))
