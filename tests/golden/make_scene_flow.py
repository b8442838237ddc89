"""Generates tests/golden/scene_flow.npz: a small run of the ScanNet grid test loop (the numpy restatement
tests/scene_flow_ref.py, which tests/test_scene_tester_flow.py pins to the reference's generator), for the GPU tests that
cannot read the reference tree.

  python tests/golden/make_scene_flow.py

Scenes are regenerated from seeds (tests/scene_flow_ref.scene); for each split the file holds the crop sequence -- cloud,
point and the selected indices of every crop -- the float64 potentials and minima after every epoch, the checkpoints
fired, the final float32 vote tables and the sub-cloud confusion matrix against seeded labels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SCENES = ((961, 200), (962, 260), (963, 230))  # (seed, n)
NUM_CLASSES, NUM_POINT, NUM_BUFFER, BATCH, VALIDATION_SIZE, SEED, EPOCHS = 6, 128, 32, 2, 4, 7, 8
LABEL_VALUES, IGNORED = np.array([0, 2, 3, 5, 8, 9]), (0,)
NUM_VOTES = 100  # never reached: max_epochs ends the runs


def scenes():
    from scene_flow_ref import scene

    pc = [scene(s, n) for s, n in SCENES]
    return [p for p, _ in pc], [c for _, c in pc]


def labels():
    """seeded ground truth per scene: values of LABEL_VALUES and one value (7) outside them"""
    rng = np.random.default_rng(SEED)
    return [rng.choice(np.append(LABEL_VALUES, 7), n).astype(np.int32) for _, n in SCENES]


def forward_weights():
    rng = np.random.default_rng(SEED + 1)
    return (rng.standard_normal((3, NUM_CLASSES)) * 0.9).astype(np.float32), rng.standard_normal(NUM_CLASSES).astype(np.float32)


def make_ref(split):
    from scene_flow_ref import SceneFlowRef

    pts, cols = scenes()
    return SceneFlowRef(pts, colors=cols, labels=[np.where(l == 7, 0, l) for l in labels()], num_classes=NUM_CLASSES, num_point=NUM_POINT, num_buffer=NUM_BUFFER,
                        batch_size=BATCH, split=split, validation_size=VALIDATION_SIZE, label_values=LABEL_VALUES,
                        ignored_labels=IGNORED, rng=np.random.RandomState(SEED))


def record():
    from scan_flow_ref import stand_in_forward_np
    from scene_flow_ref import softmax_f32

    w, b = forward_weights()
    out = {}
    for split in ("test", "validation"):
        ref = make_ref(split)
        log, pots, mins = [], [], []

        def forward(x):
            return stand_in_forward_np(x[:, :, :3], w, b)
        epochs = 0
        while epochs < EPOCHS:  # epoch by epoch, to record the potentials after each
            for _ in range(VALIDATION_SIZE):
                inputs, inds, clouds, crops = ref.batch()
                log.extend(crops)
                ref.vote(softmax_f32(forward(inputs)[:, :, 1:]), inds, clouds)
            pots.append(np.concatenate(ref.potentials))
            mins.append(np.asarray(ref.min_potentials, np.float64))
            epochs += 1
        # the checkpoints of the same run, by run() itself on a fresh restatement
        again = make_ref(split)
        ran = again.run(forward, num_votes=NUM_VOTES, max_epochs=EPOCHS)
        p = split + "_"
        out[p + "cloud"] = np.asarray([c["cloud_ind"] for c in log], np.int32)
        out[p + "point"] = np.asarray([c["point_ind"] for c in log], np.int32)
        out[p + "selected"] = np.stack([c["input_inds"] for c in log]).astype(np.int32)
        out[p + "potentials"] = np.stack(pots)
        out[p + "min_potentials"] = np.stack(mins)
        out[p + "epochs"] = np.asarray([ran], np.int32)
        out[p + "checkpoints"] = np.asarray(again.checkpoints, np.float64).reshape(-1, 2)
        out[p + "test_probs"] = np.concatenate(ref.test_probs)
        out[p + "confusion"] = ref.confusion(labels())
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "scene_flow.npz"), **record())
