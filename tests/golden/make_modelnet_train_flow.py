"""Generates tests/golden/modelnet_train_flow.npz from the REFERENCE's own run of its augmentation functions
(utils/provider.py, imported from the reference tree named by PASNL_REFERENCE), for the tests that cannot read that tree.

  PASNL_REFERENCE=/path/to/PointASNL python tests/golden/make_modelnet_train_flow.py

A seeded batch of BATCH prepared clouds of NPOINTS points (tests/modelnet_flow_ref.shape through pc_normalize, float32
values in a float64 array as `next_batch` returns them) goes through the chain exactly as train.py:226-237 applies it --
[rotate_point_cloud(_with_normal), rotate_perturbation_point_cloud(_with_normal)], random_scale_point_cloud,
shift_point_cloud, shuffle_points, random_point_dropout -- under np.random.seed(seed), for the four combinations of
{normals, no normals} x {rotation, no rotation} and every seed of GOLDEN_SEEDS.  The file holds data only: the seeds, the
generator's parameters, the four outputs per seed (float32 with rotation, float64 without) and one draw after each run,
which pins the position of the RNG stream."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SHAPE_SEED, BATCH, NPOINTS, N_RAW = 5200, 5, 67, 90
GOLDEN_SEEDS = (0, 7, 19)
COMBOS = ((True, False), (True, True), (False, False), (False, True))  # (normals, rotation)


def tag(normals, rotation):
    return ("normal" if normals else "xyz") + ("_rot" if rotation else "_plain")


def batch(normals):
    """what next_batch returns: (BATCH, NPOINTS, 3|6) float64 holding float32 values"""
    from modelnet_flow_ref import pc_normalize, shape

    out = np.zeros((BATCH, NPOINTS, 6 if normals else 3))
    for i in range(BATCH):
        point_set = shape(SHAPE_SEED + i, N_RAW, ("blob", "lattice", "dup")[i % 3])[0:NPOINTS, :]
        point_set[:, 0:3] = pc_normalize(point_set[:, 0:3])
        out[i] = point_set if normals else point_set[:, 0:3]
    return out


def reference_module():
    ref = os.environ.get("PASNL_REFERENCE", "/root/reference")
    spec = importlib.util.spec_from_file_location("_ref_provider", os.path.join(ref, "utils", "provider.py"))
    provider = importlib.util.module_from_spec(spec)
    absent = importlib.util.find_spec("h5py") is None
    if absent:
        sys.modules["h5py"] = types.ModuleType("h5py")  # imported at the top of provider.py for its file readers only
    path = list(sys.path)
    try:
        spec.loader.exec_module(provider)  # the module appends to sys.path
    finally:
        sys.path[:] = path
        if absent:
            del sys.modules["h5py"]
    return provider


def reference_chain(provider, normals, rotation, seed):
    """train.py:226-237 under np.random.seed(seed) -> (the augmented batch, a draw after it)"""
    np.random.seed(seed)
    batch_data = batch(normals)
    if rotation:
        if normals:
            batch_data = provider.rotate_point_cloud_with_normal(batch_data)
            batch_data = provider.rotate_perturbation_point_cloud_with_normal(batch_data)
        else:
            batch_data = provider.rotate_point_cloud(batch_data)
            batch_data = provider.rotate_perturbation_point_cloud(batch_data)
    batch_data[:, :, 0:3] = provider.random_scale_point_cloud(batch_data[:, :, 0:3])
    batch_data[:, :, 0:3] = provider.shift_point_cloud(batch_data[:, :, 0:3])
    batch_data = provider.shuffle_points(batch_data)
    batch_data = provider.random_point_dropout(batch_data)
    return batch_data, np.random.randint(1 << 30)


def record():
    provider = reference_module()
    rec = dict(seeds=np.asarray(GOLDEN_SEEDS, np.int64), params=np.asarray([SHAPE_SEED, BATCH, NPOINTS, N_RAW], np.int64))
    for normals, rotation in COMBOS:
        for seed in GOLDEN_SEEDS:
            out, after = reference_chain(provider, normals, rotation, seed)
            assert out.dtype == (np.float32 if rotation else np.float64)
            rec["%s/%d/out" % (tag(normals, rotation), seed)] = out
            rec["%s/%d/after" % (tag(normals, rotation), seed)] = np.asarray([after], np.int64)
    return rec


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "modelnet_train_flow.npz"), **record())
