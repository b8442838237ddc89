"""Generates tests/golden/grid_train_flow.npz: one short epoch of each grid training input loop from the numpy restatement
(tests/grid_train_flow_ref.py, which tests/test_grid_train_flow.py pins to the reference's generators) with the stand-in
forward and the augmentation under the kernel's generator (tests/philox_ref.py), for the tests that cannot read the
reference tree.

  python tests/golden/make_grid_train_flow.py

Scenes, scans and labels are regenerated from seeds; the file holds, per trainer, the selected indices and clouds of every
crop, the labels and weights, the three tallies and the loss sum (replayed under a tolerance); the fed points are not
stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SCENES = ((961, 700), (962, 450), (963, 900))                                    # (seed, n)
SCANS = ((971, 700), (972, 450), (973, 900), (974, 520), (975, 610), (976, 480), (977, 455))  # S = 7, B = 2: the seventh is never drawn
NUM_POINT, NUM_BUFFER, BATCH, EPOCH_STEPS = 64, 24, 2, 4
LABEL_VALUES = np.array([0, 1, 2, 4, 7, 9])
CLASSES = dict(scene=len(LABEL_VALUES), scan=5)
SEED = dict(scene=21, scan=22)       # the numpy RandomState of each loop
AUG_SEED, STEP_SEED = 0x5EED0123456789AB, 3


def scenes():
    from scene_flow_ref import scene

    pc = [scene(s, n) for s, n in SCENES]
    rng = np.random.default_rng(4)
    return [p for p, _ in pc], [c for _, c in pc], [rng.choice(LABEL_VALUES, n).astype(np.int32) for _, n in SCENES]


def scans():
    from scan_flow_ref import scan

    rng = np.random.default_rng(6)
    return [scan(s, n) for s, n in SCANS], [rng.integers(0, CLASSES["scan"], n).astype(np.int32) for _, n in SCANS]


def weights(name):
    return (1.0 + np.arange(CLASSES[name]) / 4.0) * (np.arange(CLASSES[name]) > 0)  # float64, class 0 weighs nothing (K:80)


def refs():
    import grid_train_flow_ref as R

    pts, cols, labs = scenes()
    sc, sl = scans()
    return dict(scene=R.SceneTrainFlowRef(pts, labs, colors=cols, label_weights=weights("scene"), num_classes=CLASSES["scene"],
                                          num_point=NUM_POINT, num_buffer=NUM_BUFFER, batch_size=BATCH, epoch_steps=EPOCH_STEPS,
                                          label_values=LABEL_VALUES, rng=np.random.RandomState(SEED["scene"])),
                scan=R.ScanTrainFlowRef(sc, sl, label_weights=weights("scan"), num_classes=CLASSES["scan"], num_point=NUM_POINT,
                                        num_buffer=NUM_BUFFER, batch_size=BATCH, rng=np.random.RandomState(SEED["scan"])))


def record():
    import grid_train_flow_ref as R

    out = {}
    for name, ref in refs().items():
        w, b = R.stand_in_weights(STEP_SEED, CLASSES[name])
        ep = R.train_epoch(ref, lambda x, y, s: R.stand_in_forward_np(x, w, b), CLASSES[name], seed=AUG_SEED)
        out[name + "/inds"] = np.stack(ep["inds"]).astype(np.int32)
        out[name + "/clouds"] = np.stack(ep["clouds"]).astype(np.int32)
        out[name + "/labels"] = np.stack(ep["labels"]).astype(np.int32)
        out[name + "/weights"] = np.stack(ep["smpw"]).astype(np.float32)
        out[name + "/totals"] = np.array([ep["total_correct"], ep["total_seen"], ep["total_iou_deno"]], np.int64)
        out[name + "/loss_sum"] = np.array([ep["loss_sum"]], np.float64)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "grid_train_flow.npz"), **record())
