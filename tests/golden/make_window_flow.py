"""Generates tests/golden/window_flow.npz from the REFERENCE's own run of the sliding-window dataset
(ScanNet/scannet_dataset.py, `ScannetDatasetWholeSceneSlidingWindow.__getitem__`, imported from the reference tree named by
PASNL_REFERENCE), for the tests that cannot read that tree.

  PASNL_REFERENCE=/path/to/PointASNL python tests/golden/make_window_flow.py

The scene is regenerated from a seed (tests/scene_flow_ref.scene, halved so that a window holds more than the reference's
4096 points at this size).  The file holds what does not depend on numpy's argsort tie in the merge: the RNG seed, the
scene's xyz after the reference's first and second call, and -- cut from those twice-moved points with the reference's
window expressions (tests/window_flow_ref.windows, which tests/test_window_tester_flow.py pins to the reference's blocks)
-- the second call's bounds, per-window counts, and every window's member list and 0.001-margin mask as packed bit rows."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SCENE_SEED, N, SCALE, SEED, BLOCK_POINTS, NUM_CLASSES, STRIDE = 971, 10000, 0.5, 13, 2048, 21, 0.5


def scene_points():
    """-> (N,6) float32: xyz (halved) and rgb"""
    from scene_flow_ref import scene

    p, c = scene(SCENE_SEED, N)
    return np.ascontiguousarray(np.hstack([(p * np.float32(SCALE)).astype(np.float32), c]))


def labels():
    return np.random.default_rng(SCENE_SEED).integers(0, NUM_CLASSES, N).astype(np.int64)


def pack(found, nwin, n, which):
    bits = np.zeros((nwin, n), bool)
    for w, members, mask, _ in found:
        bits[w, members if which == "members" else members[mask]] = True
    return np.packbits(bits, axis=1)


def record():
    from window_flow_ref import windows

    ref = os.environ.get("PASNL_REFERENCE", "/root/reference")
    spec = importlib.util.spec_from_file_location("_ref_scannet_dataset", os.path.join(ref, "ScanNet", "scannet_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ds = mod.ScannetDatasetWholeSceneSlidingWindow.__new__(mod.ScannetDatasetWholeSceneSlidingWindow)
    ds.split, ds.stride, ds.with_rgb, ds.block_points = "test", STRIDE, True, BLOCK_POINTS
    ds.scene_points_list, ds.semantic_labels_list, ds.labelweights = [scene_points()], [labels()], np.ones(NUM_CLASSES)
    np.random.seed(SEED)
    ds[0]
    moved1 = ds.scene_points_list[0][:, 0:3].copy()
    ds[0]
    moved2 = ds.scene_points_list[0][:, 0:3].copy()
    coordmin, coordmax, (nx, ny), counts, found = windows(moved2, STRIDE)
    return dict(seed=np.asarray([SEED], np.int64), moved1=moved1, moved2=moved2, coordmin=coordmin, coordmax=coordmax,
                grid=np.asarray([nx, ny], np.int32), counts=counts, members=pack(found, nx * ny, N, "members"),
                masks=pack(found, nx * ny, N, "masks"))


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "window_flow.npz"), **record())
