"""Generates tests/golden/kitti_block_flow.npz from the REFERENCE's own run of SemanticKITTI's two validation datasets
(SemanticKITTI/semantic_kitti_dataset.py, `SemanticKittiDataset` and `SemanticKittiDataset_whole`, imported from the reference
tree named by PASNL_REFERENCE), for the tests that cannot read that tree.

  PASNL_REFERENCE=/path/to/PointASNL python tests/golden/make_kitti_block_flow.py

The classes are built with __new__ over a stub scan object (the real SemLaserScan reads files, and needs np.float); the
weight table is the restatement's (tests/kitti_block_flow_ref.label_weights_lut) of the module's `mapped_content`, which is
recorded as data.  Per run -- class x with_remission -- the file holds the seed, every scan's three arrays on two visits and the state
of numpy's global RNG after each call; and the scans themselves.  What the tests rely on is asserted here: the columns per
scan, an empty column, tries that pass first, pass late and never pass."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SEED, SAMPLE_POINTS, BLOCK_SIZE, PADDING = 21, 64, 10, 0.01
RUNS = [("chopped", False), ("chopped", True), ("whole", False), ("whole", True)]


class StubScan:
    """what the reference classes read of auxiliary.laserscan.SemLaserScan"""

    def __init__(self, scans):
        self._scans = scans

    def open_scan(self, name):
        self.points, self.remissions = self._scans[int(name)][0], self._scans[int(name)][1]

    def open_label(self, name):
        self.sem_label = self._scans[int(name)][2]


def reference_module(ref=None):
    ref_dir = os.path.join(ref or os.environ.get("PASNL_REFERENCE", "/root/reference"), "SemanticKITTI")
    sys.path.insert(0, ref_dir)  # `from auxiliary import laserscan`
    try:
        spec = importlib.util.spec_from_file_location("_ref_semantic_kitti_dataset", os.path.join(ref_dir, "semantic_kitti_dataset.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(ref_dir)
    return mod


def reference_dataset(mod, kind, scans, with_remission, sample_points=SAMPLE_POINTS, block_size=BLOCK_SIZE, padding=PADDING):
    from kitti_block_flow_ref import label_weights_lut

    cls = mod.SemanticKittiDataset if kind == "chopped" else mod.SemanticKittiDataset_whole
    ds = cls.__new__(cls)
    ds.padding, ds.block_size, ds.sample_points, ds.with_remission, ds.should_map = padding, block_size, sample_points, with_remission, False
    ds.scan = StubScan(scans)
    ds.points_name = ds.label_name = [str(k) for k in range(len(scans))]
    ds.label_weights_lut = label_weights_lut(mod.mapped_content)  # (the constructor's table, D:54-58)
    return ds


def rng_state(rng=np.random):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.uint32), np.asarray([st[2]], np.uint32)])


def record():
    import kitti_block_flow_ref as R

    mod = reference_module()
    scans = R.fixture_scans()
    content = mod.mapped_content
    out = dict(seed=np.asarray([SEED], np.int64), sample_points=np.asarray([SAMPLE_POINTS], np.int64),
               block_size=np.asarray([BLOCK_SIZE], np.int64), padding=np.asarray([PADDING], np.float64),
               content_keys=np.asarray(list(content.keys()), np.int64), content_values=np.asarray(list(content.values()), np.float64))
    for k, (p, r, l) in enumerate(scans):
        out["scan%d/points" % k], out["scan%d/remissions" % k], out["scan%d/labels" % k] = p, r, l
    grids = [R.columns(p, BLOCK_SIZE, PADDING) for p, _, _ in scans]
    assert [len(f) for _, _, f in grids] == [1, 12, 5, 9, 5], [len(f) for _, _, f in grids]
    assert grids[4][0] == (3, 2) and (grids[4][1] == 0).sum() == 1  # an empty column
    assert all((c > 0).all() for _, c, _ in grids[:4])
    for kind, rem in RUNS:
        ds = reference_dataset(mod, kind, scans, rem)
        tag = "%s/%s" % (kind, "rem" if rem else "xyz")
        out[tag + "/len"] = np.asarray([len(ds)], np.int64)
        out[tag + "/lut"] = np.asarray(ds.label_weights_lut)
        assert ds.label_weights_lut.dtype == np.float32
        np.random.seed(SEED)
        mirror = np.random.RandomState(SEED)
        tries = []
        for visit in range(2 * len(ds)):  # every scan twice: the stream moves on between the visits
            data, seg, smpw = ds[visit % len(ds)]
            out["%s/%d/data" % (tag, visit)], out["%s/%d/seg" % (tag, visit)] = data, seg
            out["%s/%d/smpw" % (tag, visit)], out["%s/%d/rng" % (tag, visit)] = smpw, rng_state()
            p, r, l = scans[visit % len(ds)]
            item = (R.chopped_item if kind == "chopped" else R.whole_item)(p, r if rem else None, l, ds.label_weights_lut, SAMPLE_POINTS,
                                                                           mirror, BLOCK_SIZE, PADDING)
            assert np.array_equal(item[0], data) and np.array_equal(rng_state(mirror), rng_state())
            if kind == "chopped":
                tries.append((len(item[3]["tries"]), item[3]["tries"][-1]["valid"]))
        if kind == "chopped":  # tries that pass first, pass late, and never pass (the tenth crop is used)
            assert (1, True) in tries and any(1 < t < 10 and v for t, v in tries) and (10, False) in tries, tries
            assert tries[3] == (10, False) and tries[8] == (10, False)
            out[tag + "/tries"] = np.asarray([t for t, _ in tries], np.int64)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "kitti_block_flow.npz"), **record())
