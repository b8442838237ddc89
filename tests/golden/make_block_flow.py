"""Generates tests/golden/block_flow.npz from the REFERENCE's own run of ScanNet's two validation datasets
(ScanNet/scannet_dataset.py, `ScannetDataset` and `ScannetDatasetWholeScene`, imported from the reference tree named by
PASNL_REFERENCE), for the tests that cannot read that tree.

  PASNL_REFERENCE=/path/to/PointASNL python tests/golden/make_block_flow.py

The scenes (tests/block_flow_ref.fixture_scenes) are written as the reference's pickle into a temporary directory and read
back by the reference's constructors.  Per run -- class x with_rgb x split -- the file holds the seed, every item's three
arrays and the state of numpy's global RNG after each call; and the scenes themselves, and the 'train' label weights."""
import importlib.util
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SEED, BLOCK_POINTS = 29, 64
RUNS = [("chopped", True, "val"), ("chopped", False, "val"), ("chopped", True, "train"),
        ("whole", True, "val"), ("whole", False, "val"), ("whole", True, "train")]


def rng_state():
    st = np.random.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def record():
    from block_flow_ref import fixture_scenes

    ref = os.environ.get("PASNL_REFERENCE", "/root/reference")
    spec = importlib.util.spec_from_file_location("_ref_scannet_dataset", os.path.join(ref, "ScanNet", "scannet_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scenes = fixture_scenes()
    out = dict(seed=np.asarray([SEED], np.int64), block_points=np.asarray([BLOCK_POINTS], np.int64))
    for k, (p, l) in enumerate(scenes):
        out["scene%d/points" % k], out["scene%d/labels" % k] = p, l
    with tempfile.TemporaryDirectory() as root, np.errstate(divide="ignore", invalid="ignore"):
        for split in ("val", "train"):
            with open(os.path.join(root, "scannet_%s_rgb21c_pointid.pickle" % split), "wb") as fp:
                pickle.dump([p.copy() for p, _ in scenes], fp)
                pickle.dump([l.copy() for _, l in scenes], fp)
                pickle.dump([np.arange(len(l)) for _, l in scenes], fp)
                pickle.dump([len(l) for _, l in scenes], fp)
        for kind, rgb, split in RUNS:
            cls = mod.ScannetDataset if kind == "chopped" else mod.ScannetDatasetWholeScene
            ds = cls(root, block_points=BLOCK_POINTS, split=split, with_rgb=rgb)
            tag = "%s/%s/%s" % (kind, "rgb" if rgb else "xyz", split)
            out[tag + "/len"] = np.asarray([len(ds)], np.int64)
            out[tag + "/labelweights"] = np.asarray(ds.labelweights)
            np.random.seed(SEED)
            for visit in range(2 * len(ds)):  # every scene twice: the stream moves on between the visits
                data, seg, smpw = ds[visit % len(ds)]
                out["%s/%d/data" % (tag, visit)], out["%s/%d/seg" % (tag, visit)] = data, seg
                out["%s/%d/smpw" % (tag, visit)], out["%s/%d/rng" % (tag, visit)] = smpw, rng_state()
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "block_flow.npz"), **record())
