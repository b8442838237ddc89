"""GPU: the ScanNet grid loops in the radius form (pointasnl_amd.ScanNet.scene_radius: pasnl_scene_pick,
pasnl_scene_radius_members, one read-back, pasnl_scene_radius_gather, pasnl_scene_potential_update) against the committed
golden run tests/golden/radius_flow.npz (the restatement tests/radius_flow_ref.py over sklearn's tree orders, which
tests/test_radius_flow.py pins to the reference's generator), crop for crop and across an epoch that an empty sphere ends;
and with tree_orders=None against the restatement run live with the identity order."""
import os
import sys

import numpy as np
import pytest

import grid_train_flow_ref as T
from grid_train_checks import bits, host, same_epoch, stand_in_step

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_radius_flow as M  # noqa: E402

PER_EPOCH = M.STEPS * M.BATCH


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "radius_flow.npz"))


@pytest.fixture(scope="module")
def data():
    return M.scenes()


def epochs_of(counts):
    """the passes of the generator's loop -> [(crop numbers of the epoch, ended by an empty sphere)]"""
    out, epoch, crop = [], [], 0
    for c in counts:
        if c == 0:
            out.append((epoch, True))
            epoch = []
            continue
        epoch.append(crop)
        crop += 1
        if len(epoch) == PER_EPOCH:
            out.append((epoch, False))
            epoch = []
    assert not epoch
    return out


def count_readbacks(t):
    calls = []
    inner = t.read_count
    t.read_count = lambda: calls.append(1) or inner()
    return calls


def walk(t, gold, flow, check):
    """every batch of the golden run from the class, the epochs' early ends included; check(got, crop numbers)"""
    from pointasnl_amd.radius_crop import EpochEnded

    counts = gold[f"{flow}/counts"]
    calls = count_readbacks(t)
    ended = 0
    for epoch, early in epochs_of(counts):
        for i in range(len(epoch) // M.BATCH):
            check(t.next_batch(), epoch[i * M.BATCH:(i + 1) * M.BATCH])
        if early:  # the crops of the unfinished batch are dropped, the potentials drawn afresh
            with pytest.raises(EpochEnded):
                t.next_batch()
            assert float(t.potentials.max()) < 1e-3 and (host(t.min_pots) == [float(host(t.potentials_of(i)).min()) for i in range(3)]).all()
            ended += 1
    assert len(calls) == len(counts) == t.readbacks  # exactly one read-back per pass of the generator's loop
    np.testing.assert_array_equal(bits(host(t.potentials)), bits(gold[f"{flow}/state"]))
    assert t.rng.randint(1 << 30) == int(gold[f"{flow}/next_draw"])  # the RNG is in step, across the early end too
    return ended


@pytest.mark.parametrize("flow,abs_coords", [("scene_validation_08", True), ("scene_test_13", False)])
def test_tester_crops_equal_the_golden_run(gold, data, flow, abs_coords):
    from pointasnl_amd.ScanNet.scene_radius import RadiusSceneTester

    scenes, colors, _ = data
    _, split, radius, _ = M.FLOWS[flow]
    t = RadiusSceneTester(scenes, colors=colors, num_classes=len(M.LABEL_VALUES), num_point=M.NUM_POINT, batch_size=M.BATCH, split=split,
                          validation_size=M.STEPS, label_values=M.LABEL_VALUES, rng=np.random.RandomState(M.SEED), abs_coords=abs_coords,
                          in_radius=radius, tree_orders=M.load_orders(gold)["scene"])
    width = 9 if abs_coords else 6

    def check(got, crops):
        inputs, inds, clouds = (host(a) for a in got)
        assert inputs.shape == (M.BATCH, M.NUM_POINT, width) and inputs.dtype == np.float32
        np.testing.assert_array_equal(inds, gold[f"{flow}/inds"][crops])
        np.testing.assert_array_equal(clouds, gold[f"{flow}/clouds"][crops])
        np.testing.assert_array_equal(bits(inputs), bits(gold[f"{flow}/inputs"][crops][:, :, :width]))

    assert walk(t, gold, flow, check) == (1 if radius == 0.8 else 0)
    with pytest.raises(TypeError):
        t.enqueue()


def test_tester_run_goes_on_after_an_early_end(data):
    """`run` over eight epochs with the identity order: the seventh ends after 7 crops (three batches voted), the eighth
    starts from the re-drawn potentials"""
    import torch

    from pointasnl_amd.ScanNet.scene_radius import RadiusSceneTester

    scenes, colors, _ = data
    C = len(M.LABEL_VALUES)
    t = RadiusSceneTester(scenes, colors=colors, num_classes=C, num_point=M.NUM_POINT, batch_size=M.BATCH, split="validation",
                          validation_size=M.STEPS, label_values=M.LABEL_VALUES, rng=np.random.RandomState(M.SEED), in_radius=0.8)
    ref = M.make_ref("scene_validation_08", None, np.random.RandomState(M.SEED))
    batches = []

    def forward(x):
        batches.append(host(x))
        return torch.zeros((M.BATCH, M.NUM_POINT, C), dtype=torch.float32, device="cuda")

    assert t.run(forward, num_votes=100, max_epochs=8) == 8
    want = [b for _ in range(8) for b in ref.batches()]
    assert len(batches) == len(want) == 38 and t.readbacks == len(ref.counts)
    for x, crops in zip(batches, want):
        np.testing.assert_array_equal(bits(x[:, :, :3]), bits(np.stack([c["input_points"] for c in crops])))
    np.testing.assert_array_equal(bits(host(t.potentials)), bits(np.concatenate(ref.potentials)))
    assert float(host(t.test_probs(0)).max()) > 0  # the votes went in


def test_trainer_crops_equal_the_golden_run(gold, data):
    from pointasnl_amd.ScanNet.scene_radius import RadiusSceneTrainer

    flow = "scene_training_08"
    scenes, colors, labels = data
    t = RadiusSceneTrainer(scenes, labels, colors=colors, num_classes=len(M.LABEL_VALUES), num_point=M.NUM_POINT, batch_size=M.BATCH,
                           epoch_steps=M.STEPS, label_values=M.LABEL_VALUES, label_weights=M.SCENE_WEIGHTS,
                           rng=np.random.RandomState(M.SEED), augment=False, in_radius=0.8, tree_orders=M.load_orders(gold)["scene"])

    def check(got, crops):
        inputs, lab, wts, inds, clouds = (host(a) for a in got)
        np.testing.assert_array_equal(inds, gold[f"{flow}/inds"][crops])
        np.testing.assert_array_equal(clouds, gold[f"{flow}/clouds"][crops])
        np.testing.assert_array_equal(lab, gold[f"{flow}/labels"][crops])
        np.testing.assert_array_equal(bits(wts), bits(gold[f"{flow}/weights"][crops]))
        np.testing.assert_array_equal(bits(inputs), bits(gold[f"{flow}/inputs"][crops][:, :, :6]))

    assert walk(t, gold, flow, check) == 1
    assert (gold[f"{flow}/counts"] < M.NUM_POINT).any() and (gold[f"{flow}/weights"] > 0).any()


def test_identity_order_and_an_epoch_that_ends_early(data):
    """tree_orders=None is the restatement with the identity order; its seventh epoch ends after 7 crops: three batches are
    scored, the seventh crop is dropped, and mean_loss divides by three (train_scannet_grid.py:294-300)"""
    from pointasnl_amd.ScanNet.scene_radius import RadiusSceneTrainer

    scenes, colors, labels = data
    C = len(M.LABEL_VALUES)
    t = RadiusSceneTrainer(scenes, labels, colors=colors, num_classes=C, num_point=M.NUM_POINT, batch_size=M.BATCH, epoch_steps=M.STEPS,
                           label_values=M.LABEL_VALUES, label_weights=M.SCENE_WEIGHTS, rng=np.random.RandomState(M.SEED),
                           augment=False, in_radius=0.8)
    ref = M.make_ref("scene_training_08", None, np.random.RandomState(M.SEED))
    w, b = T.stand_in_weights(7, C)
    done = []
    for _ in range(8):
        log = []
        acc = t.run(stand_in_step(w, b, log))
        want = list(ref.batches())
        assert len(log) == len(want) == t.num_batches
        same_epoch(t, acc, log, C)
        for (x, y, wt, _), crops in zip(log, want):
            np.testing.assert_array_equal(bits(x), bits(np.stack([np.hstack((c["input_points"], c["features"][:, :3])).astype(np.float32)
                                                                    for c in crops])))
            np.testing.assert_array_equal(y, np.stack([c["labels"] for c in crops]))
            np.testing.assert_array_equal(bits(wt), bits(np.stack([c["weights"] for c in crops]).astype(np.float32)))
        done.append(len(log))
    assert done == [5, 5, 5, 5, 5, 5, 3, 5] and ref.ended == 1
    for a, p in zip(ref.potentials, range(3)):
        np.testing.assert_array_equal(bits(host(t.potentials_of(p))), bits(a))
    assert t.rng.randint(1 << 30) == ref.rng.randint(1 << 30)
