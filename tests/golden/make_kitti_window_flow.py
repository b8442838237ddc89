"""Generates tests/golden/kitti_window_flow.npz: a small recorded run of the SemanticKITTI sliding-window dataset flow, data
only, for the tests that cannot read the reference tree.

  python tests/golden/make_kitti_window_flow.py

The reference class hard-codes 4096 points as its merge threshold, far above what a committed fixture can hold, so the run is
recorded with the restatement tests/kitti_window_flow_ref.py (which tests/test_kitti_window_tester_flow.py pins to the
reference class bit for bit) at its parameter min_block_points=64.  The scan is regenerated from a seed.  The file holds what
does not depend on numpy's argsort tie in the merge: the bounds, the grid, and every window's count (empty windows and
windows at or under min_block_points among them) and member list as packed bit rows."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SCAN_SEED, N, SEED, BLOCK_POINTS, NUM_CLASSES, BLOCK_SIZE, STRIDE, MIN_BLOCK_POINTS = 311, 5000, 17, 256, 20, 10, 4, 64


def scan_points():
    """-> (N,3) float32 xyz, (N,) float32 remissions"""
    from kitti_window_flow_ref import scan

    return scan(SCAN_SEED, N)


def labels():
    return np.random.default_rng(SCAN_SEED).integers(0, NUM_CLASSES, N).astype(np.int32)


def pack(members, n):
    bits = np.zeros((len(members), n), bool)
    for w, m in enumerate(members):
        bits[w, m] = True
    return np.packbits(bits, axis=1)


def record():
    from kitti_window_flow_ref import KittiWindowFlowRef

    pts, rem = scan_points()
    ref = KittiWindowFlowRef([pts], [labels()], [rem], num_classes=NUM_CLASSES, block_points=BLOCK_POINTS, block_size=BLOCK_SIZE,
                             stride=STRIDE, min_block_points=MIN_BLOCK_POINTS, rng=np.random.RandomState(SEED))
    ref.getitem(0)
    last = ref.last
    counts = np.asarray([len(m) for m in last["members"]], np.int64)
    return dict(seed=np.asarray([SEED], np.int64), coordmin=last["coordmin"], coordmax=last["coordmax"],
                grid=np.asarray([last["nx"], last["ny"]], np.int32), counts=counts, members=pack(last["members"], N))


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "kitti_window_flow.npz"), **record())
