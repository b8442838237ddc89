"""CPU: tests/block_flow_ref.py, the numpy restatement of ScanNet's two training-time validation loops, against the
reference's own run of `ScannetDataset` and `ScannetDatasetWholeScene` recorded in tests/golden/block_flow.npz
(tests/golden/make_block_flow.py) -- arrays bit for bit, the RNG state included -- and the restated loops' counters against a
recount entry by entry."""
import os

import numpy as np
import pytest

import block_flow_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = [("chopped", True, "val"), ("chopped", False, "val"), ("chopped", True, "train"),
        ("whole", True, "val"), ("whole", False, "val"), ("whole", True, "train")]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "block_flow.npz"))


def scenes_of(gold):
    k, out = 0, []
    while "scene%d/points" % k in gold.files:
        out.append((gold["scene%d/points" % k], gold["scene%d/labels" % k]))
        k += 1
    return out


def state_of(rng):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def test_fixture_scenes_are_the_recorded_inputs(gold):
    for (p, l), (gp, gl) in zip(R.fixture_scenes(), scenes_of(gold)):
        np.testing.assert_array_equal(bits(p), bits(gp))
        np.testing.assert_array_equal(l, gl)
    assert len(scenes_of(gold)) == 4


@pytest.mark.parametrize("kind,rgb,split", RUNS)
def test_restatement_equals_the_reference_run(gold, kind, rgb, split):
    """every item of every run: data, labels and weights bit for bit, dtypes, and the RNG state after each call"""
    scenes = scenes_of(gold)
    tag = "%s/%s/%s" % (kind, "rgb" if rgb else "xyz", split)
    P = int(gold["block_points"][0])
    weights = np.ones(21) if split == "val" else R.train_weights([l for _, l in scenes], whole=kind == "whole")
    np.testing.assert_array_equal(bits(weights), bits(gold[tag + "/labelweights"]))
    assert int(gold[tag + "/len"][0]) == len(scenes)
    rng = np.random.RandomState(int(gold["seed"][0]))
    item = R.chopped_item if kind == "chopped" else R.whole_item
    for visit in range(2 * len(scenes)):
        p, l = scenes[visit % len(scenes)]
        data, seg, smpw, _ = item(p, l, weights, P, rng, with_rgb=rgb)
        for got, name in ((data, "data"), (seg, "seg"), (smpw, "smpw")):
            want = gold["%s/%d/%s" % (tag, visit, name)]
            assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype)
            np.testing.assert_array_equal(bits(got), bits(want))
        np.testing.assert_array_equal(state_of(rng), gold["%s/%d/rng" % (tag, visit)])


def test_fixture_covers_the_rejection_loop_and_an_empty_column(gold):
    """what the GPU tests rely on: tries that pass first, pass late and never pass; a 3 x 2 grid with an empty column"""
    scenes = scenes_of(gold)
    seen = set()
    for seed in range(12):
        for k in (1, 3):
            info = R.chopped_item(*scenes[k], np.ones(21), 64, np.random.RandomState(seed))[3]
            n = len(info["tries"])
            seen.add("first" if n == 1 else ("never" if not info["tries"][-1]["valid"] else "late"))
    assert seen == {"first", "late", "never"}
    shape, counts, found = R.columns(scenes[2][0][:, 0:3])
    assert shape == (3, 2) and (counts == 0).sum() == 1 and len(found) == 5


def test_voxel_key_is_a_key_not_a_triple():
    """distinct voxel triples share a key where vy * 62 + vz wraps: (vx, vy, vz) = (0, 1, 0) and (0, 0, 62)"""
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([1.5, 1.5, 3.0])
    pts = np.array([[0.0, 1.5 / 31 * 0.5, 0.0], [0.0, 0.0, 3.0]], np.float32)
    keys = R.voxel_keys(pts, lo, hi)
    assert keys[0] == keys[1] == 62.0


def canned(w, b):
    return lambda fed: R.stand_in_forward_np(fed, w, b)


@pytest.mark.parametrize("whole", [False, True])
def test_loop_counters_equal_a_recount(gold, whole):
    scenes = scenes_of(gold)
    C, P, B = 5, 32, 3
    w, b = R.stand_in_weights(3, C)
    order = [0, 1, 2, 3, 1, 2, 0]
    rng = np.random.RandomState(4)
    weights = np.array([1.0, 0.5, 2.0, 1.25, 3.0])
    logits = []

    def forward(fed):
        logits.append(R.stand_in_forward_np(fed, w, b))
        return logits[-1]

    if whole:
        out = R.eval_whole(lambda i: R.whole_item(*scenes[order[i]], weights, P, rng)[:3], len(order), B, forward, C, extra=0.25)
        assert out["num_batches"] == len(order) and len(out["fed"]) <= len(order)
    else:
        out = R.eval_chopped(lambda i: R.chopped_item(*scenes[order[i]], weights, P, rng)[:3], len(order), B, P, 6, forward, C, rng,
                             extra=0.25)
        assert out["num_batches"] == len(order) // B == len(out["fed"])
    tc, ts, seen, correct, deno, hist = R.recount(out["labels"], out["smpw"], logits, C)
    assert (tc, ts) == (out["total_correct"], out["total_seen"]) and ts > 0
    for got, want in ((seen, out["seen"]), (correct, out["correct"]), (deno, out["deno"]), (hist, out["hist"])):
        np.testing.assert_array_equal(got, want)
    assert out["mean_loss"] == pytest.approx((sum(out["losses"]) + 0.25 * len(out["losses"])) / out["num_batches"])
    lines = R.report(out, ["c%d" % k for k in range(C)], whole)
    assert lines[0].startswith("Eval whole scene mean loss" if whole else "Eval mean loss") and len(lines) == (5 if whole else 4)
