"""Generates tests/golden/radius_flow.npz: short runs of the four grid flows in the radius form (the numpy restatement
tests/radius_flow_ref.py, which tests/test_radius_flow.py pins to the reference's generators), for the GPU tests that cannot
read the reference tree.

  python tests/golden/make_radius_flow.py        (needs sklearn: the tree orders are its KDTree.idx_array)

Scenes and scans are regenerated from seeds (tests/scene_flow_ref.scene, tests/scan_flow_ref.scan).  The file holds the tree
orders (`orders/<pipeline>/<i>`) and per flow the crops of CROPS passes of the generator -- inputs, indices, clouds, labels,
weights, the sphere's count of every pass (0: the epoch ended there) -- the potentials after the last pass and the next draw
of the RNG."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SIZES, NUM_POINT, BATCH, SEED, STEPS = (700, 450, 900), 64, 2, 11, 5
LABEL_VALUES = np.array([0, 1, 2, 4, 7, 9])
SCENE_WEIGHTS = np.array([0.0, 1.5, 0.5, 2.0, 1.0, 0.25])
SCAN_CLASSES = 5
SCAN_WEIGHTS = np.array([0.0, 1.3, 0.7, 2.1, 1.0])
# flow -> (pipeline, split, radius, passes of the generator's loop)
FLOWS = {
    "scene_validation_08": ("scene", "validation", 0.8, 80),
    "scene_training_08": ("scene", "training", 0.8, 80),
    "scene_test_13": ("scene", "test", 1.3, 40),
    "scan_test_10": ("scan", "test", 10.0, 40),
    "scan_training_10": ("scan", "training", 10.0, 40),
    "scan_test_3": ("scan", "test", 3.0, 16),
}


def scenes():
    from scene_flow_ref import scene

    pc = [scene(900 + i, n) for i, n in enumerate(SIZES)]
    lrng = np.random.default_rng(2)
    return [p for p, _ in pc], [c for _, c in pc], [lrng.choice(LABEL_VALUES, n).astype(np.int32) for n in SIZES]


def scans():
    from scan_flow_ref import scan

    lrng = np.random.default_rng(2)
    return [scan(900 + i, n) for i, n in enumerate(SIZES)], [lrng.integers(0, SCAN_CLASSES, n).astype(np.int32) for n in SIZES]


def tree_orders():
    """sklearn's idx_array of the reference's trees: leaf_size=50 for ScanNet (D:324), the default for SemanticKITTI (K:159)"""
    from sklearn.neighbors import KDTree

    return dict(scene=[np.asarray(KDTree(s, leaf_size=50).idx_array).astype(np.int32) for s in scenes()[0]],
                scan=[np.asarray(KDTree(s).idx_array).astype(np.int32) for s in scans()[0]])


def make_ref(flow, orders, rng):
    import radius_flow_ref as R

    pipeline, split, radius, _ = FLOWS[flow]
    if pipeline == "scene":
        pts, cols, labs = scenes()
        return R.SceneRadiusFlowRef(pts, cols, labs, radius, orders=orders, split=split, num_point=NUM_POINT, batch_size=BATCH,
                                    steps=STEPS, label_values=LABEL_VALUES, label_weights=SCENE_WEIGHTS, rng=rng)
    pts, labs = scans()
    return R.ScanRadiusFlowRef(pts, labs, radius, orders=orders, split=split, num_point=NUM_POINT, batch_size=BATCH,
                               label_weights=SCAN_WEIGHTS, rng=rng)


def record_flow(flow, orders):
    """-> dict of arrays: the passes of the generator's loop, epoch after epoch, until FLOWS[flow] passes are done"""
    pipeline, split, radius, passes = FLOWS[flow]
    ref = make_ref(flow, orders, np.random.RandomState(SEED))
    out = dict(inputs=[], inds=[], clouds=[], labels=[], weights=[])
    while len(ref.counts) < passes:
        for c in ref.epoch():
            if pipeline == "scene":  # the model input with abs_coords: xyz, colours, float32(xyz + pick)
                out["inputs"].append(np.hstack((c["input_points"], c["features"])).astype(np.float32))
                out["inds"].append(c["input_inds"].astype(np.int32))
            else:
                out["inputs"].append(c["points"])
                out["inds"].append(c["idx"])
            out["clouds"].append(c["cloud_ind"])
            out["labels"].append(np.asarray(c["labels"]).astype(np.int32))
            out["weights"].append(np.asarray(c["weights"]).astype(np.float32))
    res = {k: np.stack(v) if k != "clouds" else np.asarray(v, np.int32) for k, v in out.items()}
    res["counts"] = np.asarray(ref.counts, np.int32)
    state = ref.potentials if pipeline == "scene" else ref.possibility
    res["state"] = np.concatenate(state) if len(state) else np.zeros(0)
    res["next_draw"] = np.asarray(ref.rng.randint(1 << 30), np.int64)
    return res


def record(orders):
    out = {}
    for pipeline in ("scene", "scan"):
        for i, o in enumerate(orders[pipeline]):
            out[f"orders/{pipeline}/{i}"] = np.asarray(o, np.int32)
    for flow, (pipeline, _, _, _) in FLOWS.items():
        for k, v in record_flow(flow, orders[pipeline]).items():
            out[f"{flow}/{k}"] = v
    return out


def load_orders(gold):
    return {p: [gold[f"orders/{p}/{i}"] for i in range(len(SIZES))] for p in ("scene", "scan")}


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "radius_flow.npz"), **record(tree_orders()))
