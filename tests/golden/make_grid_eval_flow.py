"""Generates tests/golden/grid_eval_flow.npz: three epochs of each grid pipeline's per-epoch evaluation from the numpy
restatement (tests/grid_eval_flow_ref.py, which tests/test_grid_eval_flow.py pins to the reference's own `eval_one_epoch`
functions) with the integer-logit stand-in model, unaugmented, for the tests that cannot read the reference tree.

  python tests/golden/make_grid_eval_flow.py

Scenes, scans, labels and projections are regenerated from seeds; the file holds, per epoch, the selected clouds and
indices, the summed confusions, mIoU (and mIoU_vote: epochs 0 and 2 vote), the log lines, and ScanNet's float64 tables."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SCENES = ((900, 700), (901, 450), (902, 900))                                    # (seed, n)
SCANS = ((900, 700), (901, 450), (902, 900), (903, 520), (904, 610), (905, 480), (906, 455))  # S = 7, B = 2: the seventh is never drawn
MESH = 800                                                                       # evaluation points per scene
NUM_POINT, NUM_BUFFER, BATCH, VALIDATION_SIZE, EPOCHS = 64, 24, 2, 7, 3
LABEL_VALUES = np.array([0, 1, 2, 4, 7, 9])
IGNORED = (0,)
CLASSES = dict(scene=len(LABEL_VALUES), scan=5)
SEED = dict(scene=11, scan=12)       # the numpy RandomState of each loop
VOTE = (True, False, True)
CATS = {0: 'unannotated', 1: 'wall', 2: 'floor', 3: 'chair', 4: 'tabel', 5: 'desk'}


def scenes():
    """-> points, colors, labels (values of LABEL_VALUES), validation_labels (one value outside them), validation_proj"""
    from scan_flow_ref import proj_brute
    from scene_flow_ref import scene

    pc = [scene(s, n) for s, n in SCENES]
    rng = np.random.default_rng(2)
    labels = [rng.choice(LABEL_VALUES, n).astype(np.int32) for _, n in SCENES]
    raw = [scene(970 + i, MESH)[0] for i in range(len(SCENES))]
    proj = [proj_brute(pc[i][0], raw[i]).astype(np.int32) for i in range(len(SCENES))]
    vlab = [rng.choice(np.append(LABEL_VALUES, 5), MESH).astype(np.int32) for _ in SCENES]
    return [p for p, _ in pc], [c for _, c in pc], labels, vlab, proj


def scans():
    from scan_flow_ref import scan

    rng = np.random.default_rng(6)
    return [scan(s, n) for s, n in SCANS], [rng.integers(0, CLASSES["scan"], n).astype(np.int32) for _, n in SCANS]


def scene_ref(**kw):
    import grid_eval_flow_ref as R

    pts, cols, labels, vlab, proj = scenes()
    return R.SceneEvalFlowRef(pts, labels, colors=cols, validation_labels=vlab, validation_proj=proj, num_classes=CLASSES["scene"],
                              num_point=NUM_POINT, num_buffer=NUM_BUFFER, batch_size=BATCH, validation_size=VALIDATION_SIZE,
                              label_values=LABEL_VALUES, ignored_labels=IGNORED, rng=np.random.RandomState(SEED["scene"]), **kw)


def scan_ref():
    import grid_eval_flow_ref as R

    sc, sl = scans()
    return R.ScanEvalFlowRef(sc, sl, num_classes=CLASSES["scan"], num_point=NUM_POINT, num_buffer=NUM_BUFFER, batch_size=BATCH,
                             ignored_labels=IGNORED, rng=np.random.RandomState(SEED["scan"]))


def model(name):
    import grid_eval_flow_ref as R

    return lambda x: R.gap_logits(x, CLASSES[name])


def record():
    out = {}
    ref = scene_ref()
    for e in range(EPOCHS):
        ep = ref.eval_one_epoch(model("scene"), vote=VOTE[e], seg_label_to_cat=CATS)
        k = "scene/%d/" % e
        out[k + "clouds"] = np.stack(ep["clouds"]).astype(np.int32)
        out[k + "inds"] = np.stack(ep["inds"]).astype(np.int32)
        out[k + "confusion"] = ep["Confs"].astype(np.int64)
        out[k + "miou"] = np.array([ep["mIoU"], ep["mIoU_vote"]], np.float64)
        out[k + "log"] = np.array(ep["log"])
        out[k + "table"] = np.concatenate(ref.validation_probs)
        if VOTE[e]:
            out[k + "confusion_vote"] = ep["Confs_vote"].astype(np.int64)
    ref = scan_ref()
    for e in range(EPOCHS):
        ep = ref.eval_one_epoch(model("scan"), CATS)
        k = "scan/%d/" % e
        out[k + "clouds"] = np.stack(ep["clouds"]).astype(np.int32)
        out[k + "inds"] = np.stack(ep["inds"]).astype(np.int32)
        out[k + "confusion"] = ep["Confs"].astype(np.int64)
        out[k + "miou"] = np.array([ep["mIoU"]], np.float64)
        out[k + "log"] = np.array(ep["log"])
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "grid_eval_flow.npz"), **record())
