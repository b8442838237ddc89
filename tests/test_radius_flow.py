"""CPU: the numpy restatement of the four grid flows in the radius form (tests/radius_flow_ref.py, the yardstick of
RadiusSceneTester, RadiusSceneTrainer, RadiusScanTester and RadiusScanTrainer) pinned to the reference's own generators run
with `in_radius > 0` (ScanNet/scannet_dataset_grid.py:435-549 and SemanticKITTI/semantic_kitti_dataset_grid.py:193-292, imported
as tests/test_scene_tester_flow.py and tests/test_scan_tester_flow.py import them) over sklearn trees whose `idx_array` is the
restatement's order; the committed golden run to the restatement; and the surface of the feature: the new entries in the
header, the symbol list and the library, their argument checks, the tree-order validation, and the four k-form classes that
still refuse `in_radius > 0`."""
import ctypes
import itertools
import os
import sys
import types

import numpy as np
import pytest

import radius_flow_ref as R
from scan_flow_ref import scan
from scene_flow_ref import scene
from test_scan_tester_flow import import_reference_dataset as import_kitti
from test_scene_tester_flow import import_reference_dataset as import_scannet

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES, NPOINT, SEED = (700, 450, 900), 64, 11
LABEL_VALUES = np.array([0, 1, 2, 4, 7, 9])
SCENE_WEIGHTS = np.array([0.0, 1.5, 0.5, 2.0, 1.0, 0.25])
SCAN_WEIGHTS = np.array([0.0, 1.3, 0.7, 2.1, 1.0])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def branches_ran(counts, zero):
    """no branch goes silently unrun: a sphere under num_point points, one with at least as many, and (zero) an empty one"""
    counts = np.asarray(counts)
    assert (counts[counts > 0] < NPOINT).any() and (counts >= NPOINT).any()
    assert (counts == 0).any() == zero


@pytest.mark.parametrize("radius", [0.8, 1.3])
@pytest.mark.parametrize("split", ["validation", "test", "training"])
def test_scannet_restatement_equals_reference_generator(monkeypatch, split, radius):
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = import_scannet(monkeypatch)
    pc = [scene(900 + i, n) for i, n in enumerate(SIZES)]
    scenes, colors = [p for p, _ in pc], [c for _, c in pc]
    lrng = np.random.default_rng(2)
    labels = [lrng.choice(LABEL_VALUES, n).astype(np.int32) for n in SIZES]
    trees = [KDTree(s, leaf_size=50) for s in scenes]  # D:324

    ds = mod.ScannetDataset.__new__(mod.ScannetDataset)
    ds.npoint, ds.buffer = NPOINT, 24
    ds.input_trees = {split: trees}
    ds.input_colors = {split: colors}
    ds.input_labels = {split: labels}
    ds.label_values = LABEL_VALUES
    ds.label_to_idx = {l: i for i, l in enumerate(LABEL_VALUES)}
    ds.label_weights = SCENE_WEIGHTS
    config = types.SimpleNamespace(in_radius=radius, batch_size=2, validation_size=5, epoch_steps=5)

    np.random.seed(SEED)
    gen_func, _, _ = ds.get_batch_gen(split, config)
    ref = R.SceneRadiusFlowRef(scenes, colors, labels, radius, orders=[np.asarray(t.idx_array) for t in trees], split=split,
                               num_point=NPOINT, batch_size=2, steps=5, label_values=LABEL_VALUES, label_weights=SCENE_WEIGHTS,
                               rng=np.random.RandomState(SEED))

    def same_state():
        for a, b in zip(ds.potentials[split], ref.potentials):
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(np.asarray(ds.min_potentials[split], np.float64)),
                                      bits(np.asarray(ref.min_potentials, np.float64)))

    same_state()
    ncrops = 0
    while ncrops < 300:  # epochs of 10 crops, or fewer: the generator restarted per epoch as the init op does
        for got, c in itertools.zip_longest(gen_func(), ref.epoch()):
            assert got is not None and c is not None  # the two epochs end together: no crop is skipped on either side
            pts, feats, lab, lens, inds, cloud, weights = got
            assert c["cloud_ind"] == int(cloud) and lens == [NPOINT]
            np.testing.assert_array_equal(c["input_inds"], inds)
            assert pts.dtype == np.float32 and pts.shape == (NPOINT, 3)
            np.testing.assert_array_equal(bits(c["input_points"]), bits(pts))
            assert feats.shape == (NPOINT, 6) and feats.dtype == c["features"].dtype
            np.testing.assert_array_equal(bits(c["features"]), bits(feats))
            np.testing.assert_array_equal(c["labels"], lab)
            np.testing.assert_array_equal(bits(np.asarray(c["weights"], np.float64)), bits(np.asarray(weights, np.float64)))
            same_state()
            ncrops += 1
        same_state()  # also after an epoch that an empty sphere ended: the potentials were drawn afresh on both sides
    assert ncrops >= 300 and ncrops == int(np.count_nonzero(np.asarray(ref.counts) > 0))
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)  # the two RNG streams are still in step
    branches_ran(ref.counts, zero=radius == 0.8)
    assert ref.ended == int(np.count_nonzero(np.asarray(ref.counts) == 0))
    assert ref.stats["margin"] > 1e-9  # no candidate within 1e-9 r^2 of the sphere: the membership is not a rounding matter


def kitti_dataset(monkeypatch, tmp_path, split, radius):
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = import_kitti(monkeypatch)
    scans = [scan(900 + i, n) for i, n in enumerate(SIZES)]
    lrng = np.random.default_rng(2)
    labels = [lrng.integers(0, 5, n).astype(np.int32) for n in SIZES]
    paths = [str(tmp_path / "08" / "velodyne" / f"{i:06d}.npy") for i in range(len(scans))]
    os.makedirs(os.path.dirname(paths[0]), exist_ok=True)
    for p, s in zip(paths, scans):
        np.save(p, s)
    trees = {p: KDTree(s) for p, s in zip(paths, scans)}  # K:159
    lab = dict(zip(paths, labels))
    ds = mod.SemanticKITTIDataset.__new__(mod.SemanticKITTIDataset)
    ds.args = types.SimpleNamespace(num_point=NPOINT, num_buffer=24, in_radius=radius, batch_size=2)
    ds.test_list = ds.train_list = paths
    ds.possibility, ds.min_possibility = [], []
    ds.labelweights = SCAN_WEIGHTS
    ds.get_data = lambda path: (np.array(trees[path].data, copy=False), trees[path], lab[path])
    np.random.seed(SEED)
    gen_func, _, _ = ds.get_batch_gen(split)
    ref = R.ScanRadiusFlowRef(scans, labels, radius, orders=[np.asarray(trees[p].idx_array) for p in paths], split=split,
                              num_point=NPOINT, batch_size=2, label_weights=SCAN_WEIGHTS, rng=np.random.RandomState(SEED))
    return ds, gen_func, ref


@pytest.mark.parametrize("split,radius,crops", [("test", 10.0, 80), ("training", 10.0, 80), ("test", 3.0, 16)])
def test_kitti_restatement_equals_reference_generator(monkeypatch, tmp_path, split, radius, crops):
    ds, gen_func, ref = kitti_dataset(monkeypatch, tmp_path, split, radius)

    def same_state():
        assert len(ds.possibility) == len(ref.possibility)
        for a, b in zip(ds.possibility, ref.possibility):
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(np.asarray(ds.min_possibility, np.float64)),
                                      bits(np.asarray(ref.min_possibility, np.float64)))

    same_state()
    ncrops = 0
    with np.errstate(invalid="ignore"):  # r = 3: the reference's own 0/0
        while ncrops < crops:
            for got, c in itertools.zip_longest(gen_func(), ref.epoch()):
                assert got is not None and c is not None
                sel_pc, sel_lab, weights, sel_idx, cloud = got
                assert c["cloud_ind"] == int(cloud[0])
                np.testing.assert_array_equal(c["idx"], sel_idx)
                assert sel_pc.shape == (NPOINT, 3)
                np.testing.assert_array_equal(bits(c["points"]), bits(sel_pc))
                np.testing.assert_array_equal(c["labels"], sel_lab)
                np.testing.assert_array_equal(bits(c["weights"]), bits(weights))
                same_state()
                ncrops += 1
    assert ncrops >= crops and ncrops == len(ref.counts)
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)
    assert ref.stats["margin"] > 1e-9
    if radius == 10.0:
        branches_ran(ref.counts, zero=False)
        assert not any(np.isnan(p).any() for p in ref.possibility)
    else:  # the degenerate run: a sphere that holds its centre alone makes the possibility NaN, and argmin picks it for ever
        counts = np.asarray(ref.counts)
        first = int(np.flatnonzero(counts == 1)[0])
        assert (counts[first:] == 1).all() and sum(int(np.isnan(p).sum()) for p in ref.possibility) == 1


def test_golden_radius_flow_is_the_restatement():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_radius_flow as M

    gold = np.load(os.path.join(HERE, "golden", "radius_flow.npz"))
    orders = M.load_orders(gold)
    got = M.record(orders)
    assert sorted(got) == sorted(gold.files)
    for k in gold.files:
        np.testing.assert_array_equal(bits(got[k]), bits(gold[k]), err_msg=k)
    for flow, (_, _, radius, passes) in M.FLOWS.items():
        counts = gold[f"{flow}/counts"]
        assert len(counts) >= passes and len(gold[f"{flow}/inds"]) == np.count_nonzero(counts)
        if radius == 0.8:  # the run crosses an epoch that an empty sphere ended
            assert (counts == 0).any() and counts[-1] > 0
        if radius != 3.0:
            assert (counts[counts > 0] < NPOINT).any() and (counts >= NPOINT).any()
    try:
        have = M.tree_orders()
    except ImportError:
        return
    for p in ("scene", "scan"):  # the committed orders are sklearn's idx_array of the reference's trees
        for a, b in zip(have[p], orders[p]):
            np.testing.assert_array_equal(a, b)


# ---- the surface
NEW_ENTRIES = ("pasnl_scan_radius_workspace_bytes", "pasnl_scan_radius_members", "pasnl_scene_radius_members",
               "pasnl_scan_radius_gather", "pasnl_scene_radius_gather")


def test_new_entries_are_declared_listed_and_exported():
    from pointasnl_amd import _hip

    header = open(os.path.join(os.path.dirname(HERE), "include", "pasnl.h")).read()
    lib = _hip.lib()
    for name in NEW_ENTRIES:
        assert name + "(" in header and name in _hip.SYMBOLS and hasattr(lib, name)
        assert name.startswith(("pasnl_scan_", "pasnl_scene_"))
    assert int(lib.pasnl_scan_radius_workspace_bytes(3, ctypes.c_long(4097))) == 3 * 65 * 4
    assert int(lib.pasnl_scan_radius_workspace_bytes(0, ctypes.c_long(10))) == 0


def test_bad_arguments_are_answered_before_any_launch():
    """no device is needed: every answer comes from the argument checks"""
    from pointasnl_amd import _hip

    lib = _hip.lib()
    one = ctypes.c_void_p(256)  # a non-null pointer that is never followed
    null = ctypes.c_void_p(0)
    L, D, Z = ctypes.c_long, ctypes.c_double, ctypes.c_size_t
    for entry in (lib.pasnl_scan_radius_members, lib.pasnl_scene_radius_members):
        ok = dict(b=1, nmax=L(100), points=one, desc=one, radius=D(1.0), order=null, members=one, stride=L(100), count=one, ws=one,
                  ws_bytes=Z(8))
        call = lambda **kw: entry(*dict(ok, **kw).values(), null)  # noqa: E731
        for bad in (dict(radius=D(0.0)), dict(radius=D(-1.0)), dict(radius=D(float("nan"))), dict(b=0), dict(nmax=L(0)),
                    dict(stride=L(99)), dict(nmax=L(1 << 31), stride=L(1 << 31))):
            assert call(**bad) == -1, bad
        for k in ("points", "desc", "members", "count", "ws"):
            assert call(**{k: null}) == -2, k
        assert call(ws_bytes=Z(7)) == -3
    gather = dict(b=1, desc=one, points=one, members=one, stride=L(100), count=one, perm=one, num_point=64, select=one, out=one)
    call = lambda **kw: lib.pasnl_scan_radius_gather(*dict(gather, **kw).values(), null)  # noqa: E731
    assert call(num_point=0) == -1 and call(b=-1) == -1 and call(stride=L(0)) == -1 and call(b=0) == 0
    for k in ("desc", "points", "members", "count", "perm", "select", "out"):
        assert call(**{k: null}) == -2, k
    sgather = dict(b=1, desc=one, points=one, colors=one, nfeat=3, members=one, stride=L(100), count=one, perm=one, num_point=64,
                   abs_coords=0, select=one, out=one)
    call = lambda **kw: lib.pasnl_scene_radius_gather(*dict(sgather, **kw).values(), null)  # noqa: E731
    assert call(num_point=0) == -1 and call(nfeat=-1) == -1 and call(b=0) == 0
    for k in ("desc", "points", "colors", "members", "count", "perm", "select", "out"):
        assert call(**{k: null}) == -2, k


def test_tree_orders_must_be_permutations():
    from pointasnl_amd.radius_crop import flat_tree_orders

    sizes = [5, 3]
    assert flat_tree_orders(None, sizes) is None
    flat = flat_tree_orders([np.array([4, 0, 2, 1, 3]), np.array([2, 1, 0], np.int64)], sizes)
    assert flat.dtype == np.int32 and flat.tolist() == [4, 0, 2, 1, 3, 2, 1, 0]
    for bad in ([np.arange(5)], [np.arange(5), np.arange(4)], [np.array([0, 1, 2, 3, 3]), np.arange(3)],
                [np.arange(5), np.array([0, 1, 3])], [np.arange(5) * 1.0, np.arange(3)], [np.arange(1, 6), np.arange(3)]):
        with pytest.raises(ValueError):
            flat_tree_orders(bad, sizes)


def test_draw_perm_is_the_reference_lines():
    from pointasnl_amd.radius_crop import draw_perm

    for count in (1, 5, 63, 64, 65, 300):
        a, b = np.random.RandomState(3), np.random.RandomState(3)
        got = draw_perm(a, count, NPOINT)
        x = np.arange(count) * 7  # crop_pc's lines on a list of `count` members (K:274-281)
        idx = np.arange(len(x))
        b.shuffle(idx)
        sel = x[idx][:NPOINT]
        if len(sel) < NPOINT:
            num_in = len(sel)
            dup = b.choice(num_in, NPOINT - num_in)
            sel = sel[list(range(num_in)) + list(dup)]
        np.testing.assert_array_equal(x[got], sel)
        assert got.dtype == np.int32 and a.randint(1 << 30) == b.randint(1 << 30)
        assert len(set(got[:min(count, NPOINT)].tolist())) == min(count, NPOINT)


def test_the_k_form_classes_still_refuse_a_radius():
    from pointasnl_amd.ScanNet.scene_tester import SceneTester
    from pointasnl_amd.ScanNet.scene_trainer import SceneTrainer
    from pointasnl_amd.SemanticKITTI.scan_tester import ScanTester
    from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer

    pts = [np.zeros((10, 3), np.float32)]
    lab = [np.zeros(10, np.int32)]
    for make, name in ((lambda: SceneTester(pts, in_radius=2.0), "RadiusSceneTester"),
                       (lambda: SceneTrainer(pts, lab, in_radius=2.0), "RadiusSceneTrainer"),
                       (lambda: ScanTester(pts, in_radius=2.0), "RadiusScanTester"),
                       (lambda: ScanTrainer(pts, lab, in_radius=2.0), "RadiusScanTrainer")):
        with pytest.raises(NotImplementedError, match=name):
            make()
    import pointasnl_amd.ScanNet.scene_radius as SR
    import pointasnl_amd.SemanticKITTI.scan_radius as KR

    for cls in (SR.RadiusSceneTester, KR.RadiusScanTester):
        with pytest.raises(TypeError):  # in_radius is required
            cls(pts)
        with pytest.raises(ValueError):
            cls(pts, in_radius=0.0)
