"""CPU: the restatement tests/block_train_flow_ref.py of the two segmentation training input loops against the reference's
own run of one epoch per dataset (tests/golden/block_train_flow.npz, recorded by tests/golden/make_block_train_flow.py), and
the surface of the feature: the two C-ABI entries, their host-side validation, the two trainer classes."""
import ctypes
import os
import re

import numpy as np
import pytest

import block_train_flow_ref as R
from block_flow_ref import fixture_scenes
from kitti_block_flow_ref import fixture_scans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLASSES = dict(scannet=21, kitti=20)
LINE = dict(scannet="Training accuracy: %f", kitti="Trainingaccuracy: %f")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "block_train_flow.npz"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def state_of(rng):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def replay(gold, name, items=None, batch=None):
    """the recorded epoch through the restatement -> (its results, the RandomState after it, the logits of every step)"""
    B, P = int(gold["batch"][0]) if batch is None else batch, int(gold["block_points"][0])
    w, b = R.stand_in_weights(int(gold["step_seed"][0]), CLASSES[name])
    rng = np.random.RandomState(int(gold[name + "/seed"][0]))
    logits = []

    def step(fed, label, smpw):
        logits.append(R.stand_in_forward_np(fed, w, b))
        return logits[-1]

    with np.errstate(divide="ignore", invalid="ignore"):
        if name == "scannet":
            scenes = fixture_scenes() if items is None else items
            out = R.train_epoch(lambda i: R.chopped_item(*scenes[i], gold["scannet/labelweights"], P, rng)[:3], len(scenes), B, P, 6,
                                R.train_batch, step, CLASSES[name], rng)
        else:
            scans = fixture_scans() if items is None else items
            out = R.train_epoch(lambda i: R.kitti_chopped_item(*scans[i], gold["kitti/lut"], P, rng)[:3], len(scans), B, P, 4,
                                R.kitti_train_batch, step, CLASSES[name], rng)
    return out, rng, logits


@pytest.mark.parametrize("name", ["scannet", "kitti"])
def test_restatement_equals_the_reference_epoch_bit_for_bit(gold, name):
    """the shuffled order, every fed batch (no differing float32 element: the rotation's explicit sums equal numpy's
    product on this epoch), labels, smpw, the three totals, and the RNG state after the epoch"""
    out, rng, logits = replay(gold, name)
    np.testing.assert_array_equal(out["order"], gold[name + "/order"])
    assert out["num_batches"] == 2 == len(out["fed"])
    for n in range(2):
        assert out["fed"][n].dtype == np.float32 and np.isfinite(out["fed"][n]).all()
        np.testing.assert_array_equal(bits(out["fed"][n]), bits(gold["%s/%d/fed" % (name, n)]))
        np.testing.assert_array_equal(out["labels"][n], gold["%s/%d/labels" % (name, n)])
        np.testing.assert_array_equal(bits(out["smpw"][n]), bits(gold["%s/%d/smpw" % (name, n)]))
    totals = [out[k] for k in ("total_correct", "total_seen", "total_iou_deno")]
    assert totals == list(gold[name + "/totals"]) and 0 < totals[0] < totals[1]
    np.testing.assert_array_equal(state_of(rng), gold[name + "/rng"])
    assert tuple(totals) == R.recount(out["labels"], logits)
    lines = R.report(out, LINE[name])
    assert lines[1] == LINE[name] % (totals[0] / float(totals[1])) and lines[2] == "Training IoU: %f" % (totals[0] / float(totals[2]))
    assert lines[0].startswith("Training loss: ") and np.isfinite(out["loss_sum"])


def test_the_remainder_of_the_shuffled_order_is_never_drawn(gold):
    """S = 5, B = 2 (the SemanticKITTI fixture): two batches, the fifth shuffled index draws no item; the ScanNet fixture with
    a fifth scene appended behaves the same"""
    out, _, _ = replay(gold, "kitti")
    assert len(out["order"]) == 5 and out["num_batches"] == 2 and out["total_seen"] == 2 * 2 * 64
    for name, items in (("kitti", fixture_scans()), ("scannet", fixture_scenes() + fixture_scenes()[:1])):
        drawn = []

        class Spy(list):
            def __getitem__(self, i):
                drawn.append(i)
                return list.__getitem__(self, i)

        out, _, _ = replay(gold, name, items=Spy(items))
        assert len(items) == 5 and out["num_batches"] == 2 and len(out["fed"]) == 2
        assert drawn == [int(i) for i in out["order"][:4]] and int(out["order"][4]) not in drawn
        assert out["total_seen"] == 2 * 2 * 64


def test_training_order_and_validation_order_differ_on_the_fixture(gold):
    """rotate -> float32 -> normalize (T:253-254) against normalize -> rotate (T:301-302) on the recorded epoch's own
    blocks and angles: at least one float32 bit differs, so the order is under test"""
    P = int(gold["block_points"][0])
    rng = np.random.RandomState(int(gold["scannet/seed"][0]))
    scenes = fixture_scenes()
    order = np.arange(0, 4)
    rng.shuffle(order)
    raw = np.zeros((2, P, 6))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(2):
            raw[k] = R.chopped_item(*scenes[int(order[k])], gold["scannet/labelweights"], P, rng)[0]
    angles = [rng.uniform() * 2 * np.pi for _ in range(2)]
    train, evalo = R.train_batch(raw, angles), R.eval_order_batch(raw, angles)
    np.testing.assert_array_equal(bits(train), bits(gold["scannet/0/fed"]))
    differing = int((bits(train[:, :, :3]) != bits(evalo[:, :, :3])).sum())
    print("%d of %d coordinates differ between the two orders" % (differing, train[:, :, :3].size))
    assert differing >= 1 and np.abs(train - evalo).max() < 1e-6
    np.testing.assert_array_equal(bits(train[:, :, 3:]), bits(evalo[:, :, 3:]))
    # and the explicit sums are the reference's np.dot on these blocks
    np.testing.assert_array_equal(bits(R.rotate_z_sums(raw[:, :, :3], angles)), bits(R.rotate_z(raw[:, :, :3], angles)))


@pytest.mark.parametrize("name", ["scannet", "kitti"])
def test_tally_identity(gold, name):
    """an entry adds 1 to the denominator when prediction and label agree and 2 when they do not"""
    c, s, d = (int(v) for v in gold[name + "/totals"])
    assert d == 2 * s - c
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((3, 70, 7)).astype(np.float32)
    logits[0, :5, 2] = logits[0, :5, 4] = 9.0  # ties: the first maximum
    logits[1, :5, 3] = np.nan                  # the first NaN
    label = rng.integers(0, 7, (3, 70)).astype(np.int32)
    out = R.new_totals()
    R.train_score(out, logits, label, np.ones((3, 70), np.float32), 7)
    assert out["total_iou_deno"] == 2 * out["total_seen"] - out["total_correct"] and out["total_seen"] == 210
    assert (out["total_correct"], out["total_seen"], out["total_iou_deno"]) == R.recount([label], [logits])


def test_new_symbols_are_declared_exported_and_validated():
    """the feature's surface: both entries in the header and in `_hip.SYMBOLS`, their validation before any launch, and the
    Python classes"""
    from pointasnl_amd import _hip

    lib = _hip.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pasnl.h")).read(), flags=re.S)
    for s in ("pasnl_block_train_batch", "pasnl_block_train_score"):
        assert s in _hip.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, header)
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(256)
    EINVAL, ENULL, EUNSUPPORTED = -1, -2, -5
    tb = lib.pasnl_block_train_batch
    assert tb(-1, 8, 3, some, some, some, null) == EINVAL
    assert tb(1, 0, 3, some, some, some, null) == EINVAL
    assert tb(1, 8, 2, some, some, some, null) == EINVAL
    assert tb(0, 8, 3, null, null, null, null) == 0
    assert tb(1, 8, 3, null, some, some, null) == ENULL
    assert tb(1, 8, 3, some, null, some, null) == ENULL  # rot is required here
    assert tb(1, 8, 3, some, some, null, null) == ENULL
    ts = lib.pasnl_block_train_score
    assert ts(-1, 8, 5, *[some] * 6, null) == EINVAL
    assert ts(1, 0, 5, *[some] * 6, null) == EINVAL
    assert ts(1, 8, 0, *[some] * 6, null) == EINVAL
    assert ts(1, 8, 257, *[some] * 6, null) == EUNSUPPORTED
    assert ts(0, 8, 5, *[null] * 6, null) == 0
    for k in range(6):
        args = [some] * 6
        args[k] = null
        assert ts(1, 8, 5, *args, null) == ENULL
    from pointasnl_amd.ScanNet.block_trainer import BlockTrainer
    from pointasnl_amd.SemanticKITTI.block_trainer import KittiBlockTrainer
    from pointasnl_amd.ScanNet.scannet_dataset import ScannetDataset
    from pointasnl_amd.SemanticKITTI.semantic_kitti_dataset import SemanticKittiDataset

    for cls in (BlockTrainer, KittiBlockTrainer):
        for name in ("run", "run_train", "totals", "accuracy", "iou", "mean_loss", "report", "train_batch"):
            assert hasattr(cls, name)
    assert KittiBlockTrainer.ACCURACY_LINE == LINE["kitti"] and BlockTrainer.ACCURACY_LINE == LINE["scannet"]
    assert isinstance(ScannetDataset.trainer, property) and isinstance(SemanticKittiDataset.trainer, property)
