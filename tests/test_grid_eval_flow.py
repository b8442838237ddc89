"""CPU: the numpy restatement of the two grid pipelines' per-epoch evaluation (tests/grid_eval_flow_ref.py, the yardstick of
SceneEvaluator and ScanEvaluator) pinned to the reference's own `eval_one_epoch` functions -- cut out of
ScanNet/train_scannet_grid.py:304-434 and SemanticKITTI/train_semantic_kitti_grid.py:265-330 with `ast` (the scripts parse
arguments at import) and run under small stand-ins for tf, sess, FLAGS, tqdm and log_string over the reference's own
generators -- the committed golden epochs to the restatement, and the surface of the feature: the three C-ABI entries,
their host-side validation, the modules and the constructors' checks."""
import ast
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

import grid_eval_flow_ref as R
import test_scan_tester_flow as TK
import test_scene_tester_flow as TS
from scan_flow_ref import softmax_f32

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_grid_eval_flow as M  # noqa: E402


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


# ---- the stand-ins the reference's functions run under
class OutOfRangeError(Exception):
    pass


class Sym:
    """a graph tensor: only its slicing is used (`pred[:, :, 1:]`)"""

    def __init__(self, name):
        self.name = name

    def __getitem__(self, key):
        assert key == (slice(None), slice(None), slice(1, None))
        return Sym(self.name + "[:, :, 1:]")


def make_tf():
    tf = types.SimpleNamespace()
    tf.nn = types.SimpleNamespace(softmax=lambda x: Sym("softmax(%s)" % x.name))
    tf.errors = types.SimpleNamespace(OutOfRangeError=OutOfRangeError)
    return tf


class Tqdm:
    """tqdm(iterable, total=) and `with tqdm(total=) as pbar`"""

    def __init__(self, iterable=None, total=None):
        self.iterable = iterable

    def __iter__(self):
        return iter(self.iterable)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def update(self, n):
        pass


INIT = "val_init_op"
INPUTS = dict(is_training_pl="is_training_pl", labels="labels", point_inds="point_inds", cloud_inds="cloud_inds")


class Sess:
    """sess.run(val_init_op) restarts the generator; sess.run((prob_logits, labels, point_inds, cloud_inds), feed) batches B
    items of it (drop_remainder), feeds the stand-in model and takes the float32 softmax of logits[..., 1:]"""

    def __init__(self, gen_func, B, batch_of):
        self.gen_func, self.B, self.batch_of, self.it = gen_func, B, batch_of, None

    def run(self, ops, feed=None):
        if ops == INIT:
            self.it = self.gen_func()
            return None
        assert feed == {"is_training_pl": False} and ops[0].name == "softmax(pred[:, :, 1:])" and ops[1:] == ("labels", "point_inds", "cloud_inds")
        items = []
        for _ in range(self.B):
            try:
                items.append(next(self.it))
            except StopIteration:
                raise OutOfRangeError()
        return self.batch_of(items)


def cut(path, name):
    """the function `name` of the script at `path`, compiled on its own"""
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(fn) == 1
    return compile(ast.Module(body=fn, type_ignores=[]), path, "exec")


def positional(sk):
    """the reference passes `labels` by position; current sklearn takes it by keyword only"""
    return lambda truth, preds, labels: sk.confusion_matrix(truth, preds, labels=labels)


def reference_metrics():
    return TS._load("_ref_metrics", os.path.join(REF, "utils", "metrics.py"))


def test_scene_restatement_equals_reference_eval_one_epoch(monkeypatch):
    sk = pytest.importorskip("sklearn.metrics")
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = TS.import_reference_dataset(monkeypatch)
    script = os.path.join(REF, "ScanNet", "train_scannet_grid.py")
    if not os.path.exists(script):
        pytest.skip("reference tree absent")
    scenes, colors, labels, vlab, proj = M.scenes()
    split = "validation"
    ds = mod.ScannetDataset.__new__(mod.ScannetDataset)
    ds.npoint, ds.buffer = M.NUM_POINT, M.NUM_BUFFER
    ds.input_trees = {split: [KDTree(s, leaf_size=50) for s in scenes]}
    ds.input_colors = {split: colors}
    ds.input_labels = {split: labels}
    ds.label_values = M.LABEL_VALUES
    ds.label_to_idx = {l: i for i, l in enumerate(M.LABEL_VALUES)}
    ds.ignored_labels = np.sort(list(M.IGNORED))
    ds.num_classes = len(M.LABEL_VALUES)
    ds.validation_split, ds.all_splits = 1, [1] * len(scenes)
    ds.train_files = ["scene%d.ply" % i for i in range(len(scenes))]
    ds.validation_labels, ds.validation_proj = vlab, proj
    config = types.SimpleNamespace(in_radius=0, batch_size=M.BATCH, validation_size=M.VALIDATION_SIZE, epoch_steps=5)
    np.random.seed(M.SEED["scene"])
    gen_func, _, _ = ds.get_batch_gen(split, config)
    assert config.augment_symmetries == [False, False, False]  # grid_eval_flow_ref.VALIDATION, the evaluators' config

    model = M.model("scene")

    def batch_of(items):
        pts, feats, lab, lens, inds, cloud, w = zip(*items)
        assert all(not np.asarray(x).any() for x in w)  # D:528-529: the validation split's weights are zero
        x = np.concatenate([np.stack(pts), np.stack(feats)[:, :, :3].astype(np.float32)], axis=-1).astype(np.float32)
        return softmax_f32(model(x)[:, :, 1:]), np.stack(lab).astype(np.int32), np.stack(inds).astype(np.int32), np.array(cloud, np.int32)

    log = []
    ns = dict(np=np, tf=make_tf(), tqdm=Tqdm, log_string=log.append, confusion_matrix=positional(sk),
              IoU_from_confusions=reference_metrics().IoU_from_confusions, NUM_CLASSES=len(M.LABEL_VALUES),
              FLAGS=types.SimpleNamespace(validation_size=M.VALIDATION_SIZE), validation_probs=None, val_proportions=None,
              seg_label_to_cat=M.CATS)
    exec(cut(script, "eval_one_epoch"), ns)
    sess = Sess(gen_func, M.BATCH, batch_of)
    ref = M.scene_ref()
    voted = 0
    for e in range(M.EPOCHS):
        del log[:]
        got = ns["eval_one_epoch"](Sym("pred"), INPUTS, sess, INIT, ds, M.VOTE[e])
        want = ref.eval_one_epoch(model, vote=M.VOTE[e], seg_label_to_cat=M.CATS)
        assert log == want["log"]
        for g, w in zip(got, (want["mIoU"], want["mIoU_vote"])):
            assert type(g) is type(w) and g == w
        assert isinstance(got[0], np.float32) and got[0] > 0
        if M.VOTE[e]:
            voted += 1
            assert isinstance(got[1], np.float64) and got[1] > 0
        else:
            assert got[1] == 0
        for a, b in zip(ns["validation_probs"], ref.validation_probs):
            assert a.dtype == np.float64
            np.testing.assert_array_equal(bits(a), bits(b))
        np.testing.assert_array_equal(bits(ns["val_proportions"]), bits(ref.val_proportions))
        for a, b in zip(ds.potentials[split], ref.gen.potentials):
            np.testing.assert_array_equal(bits(a), bits(b))
    assert voted == 2
    assert np.random.randint(1 << 30) == ref.gen.rng.randint(1 << 30)  # the RNG streams are still in step
    # the dtype rule the kernel mirrors: a float32 product widened into a float64 sum
    p = np.float32(0.3) * np.ones(2, np.float32)
    assert ((1 - 0.95) * p).dtype == np.float32 and (0.95 * np.zeros(2) + (1 - 0.95) * p).dtype == np.float64


def test_scan_restatement_equals_reference_eval_one_epoch(monkeypatch, tmp_path):
    sk = pytest.importorskip("sklearn.metrics")
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    mod = TK.import_reference_dataset(monkeypatch)
    script = os.path.join(REF, "SemanticKITTI", "train_semantic_kitti_grid.py")
    if not os.path.exists(script):
        pytest.skip("reference tree absent")
    scans, labels = M.scans()
    C = M.CLASSES["scan"]
    paths = [str(tmp_path / "08" / "velodyne" / f"{i:06d}.npy") for i in range(len(scans))]
    trees = {p: KDTree(s) for p, s in zip(paths, scans)}
    lab_of = dict(zip(paths, labels))
    ds = mod.SemanticKITTIDataset.__new__(mod.SemanticKITTIDataset)
    ds.args = types.SimpleNamespace(num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER, in_radius=0, batch_size=M.BATCH)
    ds.val_list, ds.labelweights = paths, np.ones(C)
    ds.get_data = lambda path: (np.array(trees[path].data, copy=False), trees[path], lab_of[path])
    ds.label_values, ds.ignored_labels = np.arange(C), np.sort([0])
    np.random.seed(M.SEED["scan"])
    gen_func, _, _ = ds.get_batch_gen("validation")
    assert ds.args.augment_symmetries == [False, False, False] and ds.args.val_steps == len(scans) // M.BATCH

    model = M.model("scan")

    def batch_of(items):
        pts, lab, w, inds, cloud = zip(*items)
        x = np.stack(pts).astype(np.float32)
        return softmax_f32(model(x)[:, :, 1:]), np.stack(lab), np.stack(inds), np.concatenate(cloud)

    log = []
    ns = dict(np=np, tf=make_tf(), tqdm=Tqdm, log_string=log.append, confusion_matrix=positional(sk),
              IoU_from_confusions=reference_metrics().IoU_from_confusions, NUM_CLASSES=C,
              FLAGS=types.SimpleNamespace(epoch_steps_eval=len(scans) // M.BATCH, debug=False), seg_label_to_cat=M.CATS)
    exec(cut(script, "eval_one_epoch"), ns)
    sess = Sess(gen_func, M.BATCH, batch_of)
    ref = M.scan_ref()
    for e in range(M.EPOCHS):
        del log[:]
        got = ns["eval_one_epoch"](Sym("pred"), INPUTS, sess, INIT, ds)
        want = ref.eval_one_epoch(model, M.CATS)
        assert log == want["log"]
        assert isinstance(got, np.float32) and type(want["mIoU"]) is np.float32 and got == want["mIoU"] and got > 0
    assert np.random.randint(1 << 30) == ref.gen.rng.randint(1 << 30)


def test_golden_grid_eval_flow_is_the_restatement():
    path = os.path.join(HERE, "golden", "grid_eval_flow.npz")
    gold = np.load(path)
    got = M.record()
    assert sorted(got) == sorted(gold.files)
    for k in gold.files:
        if got[k].dtype.kind == "f":
            np.testing.assert_array_equal(bits(got[k]), bits(gold[k]), err_msg=k)
        else:
            np.testing.assert_array_equal(got[k], gold[k], err_msg=k)
    assert os.path.getsize(path) < (1 << 20)
    kcap = M.NUM_POINT + M.NUM_BUFFER + M.NUM_BUFFER // 4 - 1
    assert all(n >= kcap for _, n in M.SCENES + M.SCANS)
    for e in range(M.EPOCHS):
        C = gold["scene/%d/confusion" % e]
        assert C.sum() == M.VALIDATION_SIZE * M.BATCH * M.NUM_POINT and C[:, 0].sum() == 0  # every label is listed; 0 is never predicted
        assert (gold["scene/%d/miou" % e][1] > 0) == M.VOTE[e] and ("scene/%d/confusion_vote" % e in gold.files) == M.VOTE[e]
        assert len(gold["scene/%d/log" % e]) == (5 if M.VOTE[e] else 2)
        assert gold["scan/%d/confusion" % e].sum() == 3 * M.BATCH * M.NUM_POINT and gold["scan/%d/clouds" % e].max() == 5
    Cv = gold["scene/0/confusion_vote"]
    assert Cv.sum() < len(M.SCENES) * M.MESH  # the label outside label_values was dropped
    t0, t2 = gold["scene/0/table"], gold["scene/2/table"]
    assert t0.dtype == np.float64 and t0.shape == (sum(n for _, n in M.SCENES), M.CLASSES["scene"] - 1)
    assert (t0.sum(1) == 0).any() and (bits(t0) != bits(t2)).any()  # points no crop visited stay zero; the table persists and moves


def test_stand_in_model_keeps_its_gap():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 500, 6)).astype(np.float32)
    for C in (5, 6, 21):
        lg = R.gap_logits(x, C)
        assert lg.shape == (3, 500, C) and lg.dtype == np.float32 and (lg == np.round(lg)).all()
        assert R.top_two_gap(lg) >= 2
        assert len(np.unique(np.argmax(lg[:, :, 1:], -1))) == C - 1  # every class is predicted somewhere


def test_new_symbols_are_declared_exported_and_validated():
    """the feature's surface: the three entries in the header and in `_hip.SYMBOLS`, outside the scope tests/abi_cases.py
    counts, and their validation before any launch"""
    import abi_cases
    from pointasnl_amd import _hip

    lib = _hip.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pasnl.h")).read(), flags=re.S)
    new = ("pasnl_scan_eval_confusion", "pasnl_scene_eval_vote", "pasnl_scene_eval_vote_confusion")
    for s in new:
        assert s in _hip.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, header)
        assert s.startswith(abi_cases.EXCLUDED_PREFIXES) and not abi_cases.in_scope(s)
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(256)
    EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5
    L = ctypes.c_long
    ig = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    ig6 = ig(1, 0, 0, 0, 0, 0)
    ec = lib.pasnl_scan_eval_confusion
    assert ec(-1, 8, 5, some, 1, some, ig6, 6, some, null) == EINVAL
    assert ec(65536, 8, 5, some, 1, some, ig6, 6, some, null) == EINVAL
    assert ec(1, 0, 5, some, 1, some, ig6, 6, some, null) == EINVAL
    assert ec(1, 8, 0, some, 1, some, ig6, 6, some, null) == EINVAL
    assert ec(1, 8, 5, some, 1, some, ig6, 0, some, null) == EINVAL
    assert ec(1, 8, 64, some, 1, some, ig(*([1] + [0] * 64)), 65, some, null) == EUNSUPPORTED
    assert ec(1, 8, 4, some, 1, some, ig6, 6, some, null) == EINVAL          # 4 + 1 ignored != 6
    assert ec(1, 8, 5, some, 1, some, ig(0, 0, 0, 0, 0, 0), 6, some, null) == EINVAL
    assert ec(0, 8, 5, null, 1, null, null, 6, null, null) == 0
    for k in range(4):
        args = [some, some, ig6, some]
        args[k] = null
        assert ec(1, 8, 5, args[0], 1, args[1], args[2], 6, args[3], null) == ENULL
    ev = lib.pasnl_scene_eval_vote
    so, sn = ctypes.c_double(0.95), ctypes.c_float(0.05)
    assert ev(-1, 8, 5, some, 1, some, some, some, so, sn, some, some, null) == EINVAL
    assert ev(1, 0, 5, some, 1, some, some, some, so, sn, some, some, null) == EINVAL
    assert ev(1, 8, 0, some, 1, some, some, some, so, sn, some, some, null) == EINVAL
    assert ev(1, 8, 65, some, 1, some, some, some, so, sn, some, some, null) == EUNSUPPORTED
    assert ev(0, 8, 5, null, 1, null, null, null, so, sn, null, null, null) == 0
    for k in range(6):
        args = [some] * 6
        args[k] = null
        assert ev(1, 8, 5, args[0], 1, args[1], args[2], args[3], so, sn, args[4], args[5], null) == ENULL
    vc = lib.pasnl_scene_eval_vote_confusion
    assert vc(L(-1), some, 5, L(4), null, some, some, ig6, 6, some, some, null) == EINVAL
    assert vc(L(8), some, 5, L(-1), null, some, some, ig6, 6, some, some, null) == EINVAL
    assert vc(L(8), some, 0, L(4), null, some, some, ig6, 6, some, some, null) == EINVAL
    assert vc(L(8), some, 5, L(4), null, some, some, ig6, 0, some, some, null) == EINVAL
    assert vc(L(8), some, 64, L(4), null, some, some, ig(*([1] + [0] * 64)), 65, some, some, null) == EUNSUPPORTED
    assert vc(L(8), some, 4, L(4), null, some, some, ig6, 6, some, some, null) == EINVAL
    assert vc(L(0), null, 5, L(4), null, null, null, null, 6, null, null, null) == 0
    for k in (0, 2, 3, 4, 5, 6):  # proj (1) may be NULL
        args = [some, null, some, some, ig6, some, some]
        args[k] = null
        assert vc(L(8), args[0], 5, L(4), *args[1:5], 6, *args[5:], null) == ENULL


def test_modules_and_constructor_checks():
    from pointasnl_amd import grid_augment
    from pointasnl_amd.ScanNet.scene_evaluator import SceneEvaluator
    from pointasnl_amd.ScanNet.scene_tester import SceneCrops, SceneTester, iou_from_confusions
    from pointasnl_amd.SemanticKITTI.scan_evaluator import ScanEvaluator
    from pointasnl_amd.grid_eval_loop import GridEvalLoop

    assert issubclass(SceneEvaluator, SceneCrops) and issubclass(SceneEvaluator, GridEvalLoop) and issubclass(ScanEvaluator, GridEvalLoop)
    assert not issubclass(SceneEvaluator, SceneTester)
    for cls in (SceneEvaluator, ScanEvaluator):
        for name in ("run", "report", "score", "confusion", "drop_ignored", "iou_from_confusions", "enqueue_batch"):
            assert hasattr(cls, name)
    assert hasattr(SceneEvaluator, "validation_probs") and hasattr(SceneEvaluator, "vote_confusion")
    assert GridEvalLoop.drop_ignored is SceneTester.drop_ignored and GridEvalLoop.iou_from_confusions(np.eye(3)).shape == (3,)
    np.testing.assert_array_equal(GridEvalLoop.iou_from_confusions(np.eye(3)), iou_from_confusions(np.eye(3)))
    assert grid_augment.host_config(grid_augment.config_of(augment_symmetries=(False, False, False))) == R.VALIDATION
    lines = GridEvalLoop.class_lines(np.array([0.5, 0.25]), M.CATS, 3)
    assert lines == R.class_lines(np.array([0.5, 0.25]), M.CATS, 3) == "------- IoU --------\nclass wall           IoU: 50.000 \nclass floor          IoU: 25.000 \n"
    # the constructors' checks that need no device
    pts, cols, labels, vlab, proj = M.scenes()
    kw = dict(colors=cols, validation_labels=vlab, validation_proj=proj, num_classes=6, num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER,
              batch_size=M.BATCH, validation_size=M.VALIDATION_SIZE, label_values=M.LABEL_VALUES)
    with pytest.raises(NotImplementedError, match="radius form"):
        SceneEvaluator(pts, labels, in_radius=1.0, **kw)
    with pytest.raises(ValueError, match="ignored labels"):
        SceneEvaluator(pts, labels, **dict(kw, num_classes=5))
    with pytest.raises(ValueError, match="distinct"):
        SceneEvaluator(pts, labels, **dict(kw, label_values=[0, 1, 2, 4, 7, 7]))
    with pytest.raises(KeyError):
        SceneEvaluator(pts, [np.full_like(l, 3) for l in labels], **kw)
    with pytest.raises(ValueError, match="one label array per scene"):
        SceneEvaluator(pts, labels[:2], **kw)
    with pytest.raises(ValueError, match="one validation_labels array per scene"):
        SceneEvaluator(pts, labels, **dict(kw, validation_labels=vlab[:2]))
    with pytest.raises(ValueError, match="identity"):
        SceneEvaluator(pts, labels, **dict(kw, validation_proj=None))  # 800 labels for 700 points
    with pytest.raises(ValueError, match="outside"):
        SceneEvaluator(pts, labels, **dict(kw, validation_proj=[p + 10000 for p in proj]))
    sc, sl = M.scans()
    with pytest.raises(NotImplementedError, match="radius form"):
        ScanEvaluator(sc, sl, num_classes=5, in_radius=2.0)
    with pytest.raises(ValueError, match="batch_size"):
        ScanEvaluator(sc[:1], sl[:1], num_classes=5, num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER, batch_size=2)
    with pytest.raises(ValueError, match="ignored labels"):
        ScanEvaluator(sc, sl, num_classes=5, ignored_labels=())
