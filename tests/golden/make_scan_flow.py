"""Generates tests/golden/scan_flow.npz: a small run of the SemanticKITTI test loop's crop sequence (the numpy restatement
tests/scan_flow_ref.py, which tests/test_scan_tester_flow.py pins to the reference's generator), for the GPU tests that
cannot read the reference tree.

  python tests/golden/make_scan_flow.py

Scans are regenerated from seeds (tests/scan_flow_ref.scan); the file holds the crop sequence -- cloud, pick and the
selected indices of every crop -- and the float64 possibility and min_possibility after every epoch."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SCANS = ((951, 1500), (952, 1800), (953, 1200))  # (seed, n)
NUM_POINT, NUM_BUFFER, BATCH, SEED, EPOCHS = 256, 64, 2, 5, 3


def scans():
    from scan_flow_ref import scan

    return [scan(s, n) for s, n in SCANS]


def record():
    from scan_flow_ref import ScanFlowRef

    ref = ScanFlowRef(scans(), num_point=NUM_POINT, num_buffer=NUM_BUFFER, batch_size=BATCH, rng=np.random.RandomState(SEED))
    per_epoch = int(len(SCANS) / BATCH) * BATCH * 4
    cloud, pick, sel, poss, mins = [], [], [], [], []
    for _ in range(EPOCHS):
        for _ in range(per_epoch):
            c, p, s = ref.crop()
            cloud.append(c)
            pick.append(p)
            sel.append(s)
        poss.append(np.concatenate(ref.possibility))
        mins.append(np.asarray(ref.min_possibility, np.float64))
    return dict(cloud=np.asarray(cloud, np.int32), pick=np.asarray(pick, np.int32), selected=np.stack(sel).astype(np.int32),
                possibility=np.stack(poss), min_possibility=np.stack(mins))


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "scan_flow.npz"), **record())
