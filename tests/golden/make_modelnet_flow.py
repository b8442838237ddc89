"""Generates tests/golden/modelnet_flow.npz from the REFERENCE's own run of its dataset class (modelnet_dataset.py,
`ModelNetDataset`, imported from the reference tree named by PASNL_REFERENCE), for the tests that cannot read that tree.

  PASNL_REFERENCE=/path/to/PointASNL python tests/golden/make_modelnet_flow.py

A seeded synthetic dataset root is written into a temporary directory -- the shape-name list, the two split lists and a
few comma-separated .txt shapes (tests/modelnet_flow_ref.shape, printed with nine significant digits: float32 survives the
round trip through np.loadtxt) -- and the reference's class runs one epoch of the 'test' split over it with `uniform` false
and true under a fixed np.random.seed.  The file holds data only: the seed, the generator's parameters, the batches
`next_batch` returned (they are float32 values in float64 arrays; kept as float32) and one draw after the epoch, which pins
the position of the RNG stream."""
import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SHAPE_SEED, SHAPES, N_RAW, NPOINTS, BATCH, SEED = 4100, 10, 300, 64, 4, 23
CLASS_NAMES = ["chair", "night_stand", "lamp", "sofa"]
KINDS = ["blob", "blob", "lattice", "blob", "dup", "blob", "blob", "lattice", "blob", "blob"]


def shapes():
    from modelnet_flow_ref import shape

    return [shape(SHAPE_SEED + i, N_RAW, KINDS[i]) for i in range(SHAPES)]


def labels():
    return np.random.default_rng(SHAPE_SEED).integers(0, len(CLASS_NAMES), SHAPES).astype(np.int32)


def write_root(root):
    """the dataset root as the reference reads it; the 'test' split lists the shapes in order"""
    lab, ids = labels(), []
    with open(os.path.join(root, "modelnet40_shape_names.txt"), "w") as f:
        f.write("".join(name + "\n" for name in CLASS_NAMES))
    for i, s in enumerate(shapes()):
        name = CLASS_NAMES[lab[i]]
        ids.append("%s_%04d" % (name, i + 1))
        os.makedirs(os.path.join(root, name), exist_ok=True)
        np.savetxt(os.path.join(root, name, ids[-1] + ".txt"), s, fmt="%.9g", delimiter=",")
    for split in ("train", "test"):
        with open(os.path.join(root, "modelnet40_%s.txt" % split), "w") as f:
            f.write("".join(i + "\n" for i in ids))


def reference_module():
    ref = os.environ.get("PASNL_REFERENCE", "/root/reference")
    spec = importlib.util.spec_from_file_location("_ref_modelnet_dataset", os.path.join(ref, "modelnet_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)  # the module appends to sys.path
    finally:
        sys.path[:] = path
    return mod


def reference_epoch(mod, root, uniform, normal_channel=True, shuffle=None, batch=BATCH):
    """one epoch of the reference's class under np.random.seed(SEED) -> (list of (data f64, label i32), a draw after it)"""
    np.random.seed(SEED)
    ds = mod.ModelNetDataset(root=root, batch_size=batch, npoints=NPOINTS, split="test", normal_channel=normal_channel, uniform=uniform,
                             shuffle=shuffle)
    out = []
    while ds.has_next_batch():
        out.append(ds.next_batch())
    return out, np.random.randint(1 << 30)


def record():
    mod = reference_module()
    rec = dict(seed=np.asarray([SEED], np.int64),
               params=np.asarray([SHAPE_SEED, SHAPES, N_RAW, NPOINTS, BATCH], np.int64))
    with tempfile.TemporaryDirectory() as root:
        write_root(root)
        for uniform in (False, True):
            batches, after = reference_epoch(mod, root, uniform)
            data = np.concatenate([d for d, _ in batches])
            assert data.dtype == np.float64 and np.array_equal(data.astype(np.float32).astype(np.float64), data)
            tag = "uniform" if uniform else "first"
            rec[tag + "/data"] = data.astype(np.float32)
            rec[tag + "/label"] = np.concatenate([l for _, l in batches])
            rec[tag + "/bsizes"] = np.asarray([d.shape[0] for d, _ in batches], np.int32)
            rec[tag + "/after"] = np.asarray([after], np.int64)
    return rec


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "modelnet_flow.npz"), **record())
