"""GPU: the SemanticKITTI grid loops in the radius form (pointasnl_amd.SemanticKITTI.scan_radius: pasnl_scan_pick or
pasnl_scan_pick_given, pasnl_scan_radius_members, one read-back, pasnl_scan_radius_gather, pasnl_scan_possibility_update)
against the committed golden run tests/golden/radius_flow.npz (the restatement tests/radius_flow_ref.py over sklearn's tree
orders, which tests/test_radius_flow.py pins to the reference's generator), crop for crop -- the degenerate run of a sphere
that holds its centre alone included -- and with tree_orders=None against the restatement run live with the identity order."""
import os
import sys

import numpy as np
import pytest

from grid_train_checks import bits, host

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_radius_flow as M  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "radius_flow.npz"))


@pytest.fixture(scope="module")
def data():
    return M.scans()


def count_readbacks(t):
    calls = []
    inner = t.read_count
    t.read_count = lambda: calls.append(1) or inner()
    return calls


def make_tester(data, radius, orders):
    from pointasnl_amd.SemanticKITTI.scan_radius import RadiusScanTester

    return RadiusScanTester(data[0], num_classes=M.SCAN_CLASSES, num_point=M.NUM_POINT, batch_size=M.BATCH,
                            rng=np.random.RandomState(M.SEED), in_radius=radius, tree_orders=orders)


def make_trainer(data, radius, orders, **kw):
    from pointasnl_amd.SemanticKITTI.scan_radius import RadiusScanTrainer

    return RadiusScanTrainer(data[0], data[1], num_classes=M.SCAN_CLASSES, num_point=M.NUM_POINT, batch_size=M.BATCH,
                             label_weights=M.SCAN_WEIGHTS, rng=np.random.RandomState(M.SEED), in_radius=radius, tree_orders=orders, **kw)


@pytest.mark.parametrize("flow", ["scan_test_10", "scan_test_3"])
def test_tester_crops_equal_the_golden_run(gold, data, flow):
    radius = M.FLOWS[flow][2]
    t = make_tester(data, radius, M.load_orders(gold)["scan"])
    calls = count_readbacks(t)
    n = len(gold[f"{flow}/counts"])
    assert t.crops_per_epoch == 8 and n % M.BATCH == 0
    for i in range(n // M.BATCH):
        pts, inds, clouds = (host(a) for a in t.next_batch())
        crops = slice(i * M.BATCH, (i + 1) * M.BATCH)
        np.testing.assert_array_equal(inds, gold[f"{flow}/inds"][crops])
        np.testing.assert_array_equal(clouds, gold[f"{flow}/clouds"][crops])
        np.testing.assert_array_equal(bits(pts), bits(gold[f"{flow}/inputs"][crops]))
    assert len(calls) == n == t.readbacks  # exactly one read-back per crop
    state = host(t.possibility)
    want = gold[f"{flow}/state"]
    # by bits, but a NaN for a NaN (r = 3): the sign of the 0/0 NaN is the processor's choice, x86 sets it, the GPU does not
    np.testing.assert_array_equal(np.isnan(state), np.isnan(want))
    np.testing.assert_array_equal(bits(np.nan_to_num(state, nan=-1.0)), bits(np.nan_to_num(want, nan=-1.0)))
    assert t.rng.randint(1 << 30) == int(gold[f"{flow}/next_draw"])
    assert int(np.isnan(state).sum()) == (1 if radius == 3.0 else 0)
    assert int(np.isnan(t.min_possibility()).sum()) == (1 if radius == 3.0 else 0)
    with pytest.raises(TypeError):
        t.enqueue()


def test_trainer_crops_equal_the_golden_run(gold, data):
    flow = "scan_training_10"
    t = make_trainer(data, 10.0, M.load_orders(gold)["scan"], augment=False)
    calls = count_readbacks(t)
    n = len(gold[f"{flow}/counts"])
    assert t.steps_per_epoch == 1
    for i in range(n // M.BATCH):
        pts, lab, wts, inds, clouds = (host(a) for a in t.next_batch())
        crops = slice(i * M.BATCH, (i + 1) * M.BATCH)
        assert clouds.tolist() == [0, 1]  # int(3 / 2) * 2 items per epoch: the third scan is never drawn (K:195)
        np.testing.assert_array_equal(clouds, gold[f"{flow}/clouds"][crops])
        np.testing.assert_array_equal(inds, gold[f"{flow}/inds"][crops])
        np.testing.assert_array_equal(bits(pts), bits(gold[f"{flow}/inputs"][crops]))
        np.testing.assert_array_equal(lab, gold[f"{flow}/labels"][crops])
        np.testing.assert_array_equal(bits(wts), bits(gold[f"{flow}/weights"][crops]))
    assert len(calls) == n == t.readbacks
    assert t.rng.randint(1 << 30) == int(gold[f"{flow}/next_draw"])
    counts = gold[f"{flow}/counts"]
    assert (counts < M.NUM_POINT).any() and (counts >= M.NUM_POINT).any()


def test_device_scan_with_a_tree_order_gives_the_reference_crop(gold, data):
    """crop_pc(in_radius > 0) over DeviceScan(points, tree_order): the restatement's crop_pc under the same draws, for a sphere
    under and one over num_point; without an order the members come by ascending index, as before"""
    from pointasnl_amd.SemanticKITTI.semantic_kitti_dataset_grid import DeviceScan, crop_pc

    scans, labels = data
    orders = M.load_orders(gold)["scan"]
    ref = M.make_ref("scan_training_10", orders, np.random.RandomState(0))
    seen = set()
    for cloud, pick in ((0, 5), (0, 17), (1, 4), (2, 11)):  # spheres of 142, 30, 38 and 429 points
        tree = DeviceScan(scans[cloud], tree_order=orders[cloud])
        a, b = np.random.RandomState(pick), np.random.RandomState(pick)
        ref.rng = b
        want = ref.crop_pc(ref.pc[cloud], labels[cloud], cloud, np.array([pick]))
        got = crop_pc(scans[cloud], labels[cloud], tree, np.array([pick]), M.NUM_POINT, in_radius=10.0, rng=a)
        np.testing.assert_array_equal(got[2], want[2])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(bits(got[0]), bits(want[0].astype(np.float32)))
        assert a.randint(1 << 30) == b.randint(1 << 30)
        seen.add(ref.counts[-1] < M.NUM_POINT)
        plain = DeviceScan(scans[cloud]).query_radius(scans[cloud][pick].reshape(1, 3), 10.0)[0]
        members = tree.query_radius(scans[cloud][pick].reshape(1, 3), 10.0)[0]
        assert plain.tolist() == sorted(members.tolist()) and members.dtype == np.int64
    assert seen == {True, False}
    with pytest.raises(ValueError):
        DeviceScan(scans[0], tree_order=orders[1])


def test_identity_order_is_the_restatement(data):
    """tree_orders=None: members by ascending index, the restatement with orders=None; the trainer augmented, so only
    indices, labels and weights are compared, and one epoch of `run`"""
    t = make_tester(data, 10.0, None)
    ref = M.make_ref("scan_test_10", None, np.random.RandomState(M.SEED))
    for _ in range(10):
        pts, inds, clouds = (host(a) for a in t.next_batch())
        want = [ref.crop() for _ in range(M.BATCH)]
        np.testing.assert_array_equal(inds, np.stack([c["idx"] for c in want]))
        np.testing.assert_array_equal(bits(pts), bits(np.stack([c["points"] for c in want])))
        assert clouds.tolist() == [c["cloud_ind"] for c in want]
    np.testing.assert_array_equal(bits(host(t.possibility)), bits(np.concatenate(ref.possibility)))
    assert t.rng.randint(1 << 30) == ref.rng.randint(1 << 30)

    tr = make_trainer(data, 10.0, None, augment=True, seed=5)
    ref = M.make_ref("scan_training_10", None, np.random.RandomState(M.SEED))
    seen = []

    def step(x, y, w):
        import torch

        seen.append((host(x), host(y), host(w)))
        return torch.zeros((M.BATCH, M.NUM_POINT, M.SCAN_CLASSES), dtype=torch.float32, device="cuda")

    tr.run(step)
    want = list(ref.epoch())
    assert len(seen) == 1 == tr.num_batches and tr.item == M.BATCH and tr.readbacks == 2
    np.testing.assert_array_equal(seen[0][1], np.stack([c["labels"] for c in want]))
    np.testing.assert_array_equal(bits(seen[0][2]), bits(np.stack([c["weights"] for c in want])))
    assert (bits(seen[0][0]) != bits(np.stack([c["points"] for c in want]))).any()  # augmented
    assert tr.rng.randint(1 << 30) == ref.rng.randint(1 << 30)
