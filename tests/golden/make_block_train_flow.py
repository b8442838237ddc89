"""Generates tests/golden/block_train_flow.npz from the REFERENCE's own functions (imported from the reference tree named by
PASNL_REFERENCE), for the tests that cannot read that tree: one short training epoch per dataset.

  PASNL_REFERENCE=/path/to/PointASNL python tests/golden/make_block_train_flow.py

The epoch is `train_one_epoch` round the reference's `ScannetDataset.__getitem__` / `SemanticKittiDataset.__getitem__`,
`provider.rotate_point_cloud_z` and -- for ScanNet -- `provider.normalize_data`, under numpy's global RNG as the reference
uses it: the shuffle, per batch B items and then the transform's B angles.  The training scripts import TensorFlow and
cannot be imported, so the loop round those functions and its three tallies (every entry counts: the matches, B * P, and per
class the entries whose prediction or label is that class) are written out here; the step is the stand-in
tests/block_flow_ref.stand_in_forward_np on the fed float32 batch.  The datasets are the fixtures of
tests/block_flow_ref.fixture_scenes (4 scenes, with rgb, split='train' weights) and
tests/kitti_block_flow_ref.fixture_scans (5 scans, with remission; the fifth shuffled index is dropped), at B = 2 and 64
points per block.  Per dataset the file holds the seed, the shuffled order, every fed batch with its labels and smpw, the
three totals and the RNG state after the epoch: arrays only.

numpy's dgemm fixes no summation order, so `rotate_point_cloud_z` may differ from the explicit sums of
tests/block_train_flow_ref.py by one float32 ulp, which would move a whole normalized block.  The seeds are chosen so that
it does not: `record` asserts ZERO differing float32 elements between the restatement and the reference's run over every
fed element -- 2 batches x 2 x 64 x 6 = 1536 for ScanNet and 2 x 2 x 64 x 4 = 1024 for SemanticKITTI, 2560 in all, of
which 1536 are rotated coordinates -- and prints the counts."""
import importlib.util
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

BATCH, BLOCK_POINTS, STEP_SEED = 2, 64, 6
SEEDS = dict(scannet=41, kitti=43)
CLASSES = dict(scannet=21, kitti=20)


def rng_state(rng=np.random):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def epoch(ds, width, transforms, num_classes, w, b):
    """one training epoch round the reference's dataset and transforms (each assigned back into the float64 batch, as the
    loop does), under numpy's global RNG"""
    from block_flow_ref import stand_in_forward_np

    idxs = np.arange(0, len(ds))
    np.random.shuffle(idxs)
    rec = dict(order=idxs.astype(np.int64))
    correct = seen = deno = 0
    for n in range(len(ds) // BATCH):
        data = np.zeros((BATCH, BLOCK_POINTS, width))
        label = np.zeros((BATCH, BLOCK_POINTS), dtype=np.int32)
        smpw = np.zeros((BATCH, BLOCK_POINTS), dtype=np.float32)
        for k in range(BATCH):
            data[k, ...], label[k, :], smpw[k, :] = ds[idxs[n * BATCH + k]]
        for transform in transforms:
            data[:, :, :3] = transform(data[:, :, :3])
        fed = data.astype(np.float32)
        pred = stand_in_forward_np(fed, w, b).argmax(axis=2)
        correct += int((pred == label).sum())
        seen += BATCH * BLOCK_POINTS
        deno += sum(int(np.logical_or(pred == c, label == c).sum()) for c in range(num_classes))
        rec["%d/fed" % n], rec["%d/labels" % n], rec["%d/smpw" % n] = fed, label, smpw
    rec["totals"] = np.asarray([correct, seen, deno], np.int64)
    rec["rng"] = rng_state()
    return rec


def scannet_epoch(w, b):
    import make_modelnet_train_flow as M
    from block_flow_ref import fixture_scenes

    ref = os.environ.get("PASNL_REFERENCE", "/root/reference")
    spec = importlib.util.spec_from_file_location("_ref_scannet_dataset", os.path.join(ref, "ScanNet", "scannet_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    provider = M.reference_module()
    scenes = fixture_scenes()
    with tempfile.TemporaryDirectory() as root, np.errstate(divide="ignore", invalid="ignore"):
        with open(os.path.join(root, "scannet_train_rgb21c_pointid.pickle"), "wb") as fp:
            pickle.dump([p.copy() for p, _ in scenes], fp)
            pickle.dump([l.copy() for _, l in scenes], fp)
            pickle.dump([np.arange(len(l)) for _, l in scenes], fp)
            pickle.dump([len(l) for _, l in scenes], fp)
        ds = mod.ScannetDataset(root, block_points=BLOCK_POINTS, split="train", with_rgb=True)
        np.random.seed(SEEDS["scannet"])
        rec = epoch(ds, 6, (provider.rotate_point_cloud_z, provider.normalize_data), CLASSES["scannet"], w, b)
    rec["labelweights"] = np.asarray(ds.labelweights)
    return rec


def kitti_epoch(w, b):
    import make_kitti_block_flow as K
    import make_modelnet_train_flow as M
    from kitti_block_flow_ref import fixture_scans

    provider = M.reference_module()
    ds = K.reference_dataset(K.reference_module(), "chopped", fixture_scans(), True, sample_points=BLOCK_POINTS)
    np.random.seed(SEEDS["kitti"])
    rec = epoch(ds, 4, (provider.rotate_point_cloud_z,), CLASSES["kitti"], w, b)
    rec["lut"] = np.asarray(ds.label_weights_lut)
    return rec


def restated(name, rec, w, b):
    """the same epoch through tests/block_train_flow_ref.py"""
    import block_train_flow_ref as R
    from block_flow_ref import fixture_scenes
    from kitti_block_flow_ref import fixture_scans

    rng = np.random.RandomState(SEEDS[name])
    if name == "scannet":
        scenes = fixture_scenes()
        return R.train_epoch(lambda i: R.chopped_item(*scenes[i], rec["labelweights"], BLOCK_POINTS, rng)[:3], len(scenes), BATCH,
                             BLOCK_POINTS, 6, R.train_batch, lambda x, l, s: R.stand_in_forward_np(x, w, b), CLASSES[name], rng), rng
    scans = fixture_scans()
    return R.train_epoch(lambda i: R.kitti_chopped_item(*scans[i], rec["lut"], BLOCK_POINTS, rng)[:3], len(scans), BATCH, BLOCK_POINTS, 4,
                         R.kitti_train_batch, lambda x, l, s: R.stand_in_forward_np(x, w, b), CLASSES[name], rng), rng


def record():
    from block_flow_ref import stand_in_weights

    out = dict(batch=np.asarray([BATCH], np.int64), block_points=np.asarray([BLOCK_POINTS], np.int64),
               step_seed=np.asarray([STEP_SEED], np.int64))
    compared = 0
    for name, run in (("scannet", scannet_epoch), ("kitti", kitti_epoch)):
        w, b = stand_in_weights(STEP_SEED, CLASSES[name])
        rec = run(w, b)
        mine, rng = restated(name, rec, w, b)
        assert np.array_equal(mine["order"], rec["order"]) and np.array_equal(rng_state(rng), rec["rng"])
        differing = elements = 0
        for n, fed in enumerate(mine["fed"]):
            differing += int((fed.view(np.int32) != rec["%d/fed" % n].view(np.int32)).sum())
            elements += fed.size
        assert elements > 0 and len(mine["fed"]) == 2
        print("%s: %d of %d fed float32 elements differ between the restatement and the reference" % (name, differing, elements))
        assert differing == 0, "choose another seed: numpy's product differs from the explicit sums by an ulp in this epoch"
        assert [mine[k] for k in ("total_correct", "total_seen", "total_iou_deno")] == list(rec["totals"])
        compared += elements
        out[name + "/seed"] = np.asarray([SEEDS[name]], np.int64)
        for k, v in rec.items():
            out[name + "/" + k] = v
    print("%d elements compared in all" % compared)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "block_train_flow.npz"), **record())
