"""The ModelNet40 training input loop, host numpy chain plus upload vs ModelNetTrainer, around a no-op step, over a synthetic
training split of the real size: 9843 prepared shapes of 1024 points, 6 channels, 40 classes, at batch 16 (the reference's
default) and batch 64, with and without --rotation's two rotations.

  (a) host: train.py's loop as written -- the float64 batch assembled in numpy from the prepared shapes, the augmentation
      chain of utils/provider.py in numpy (rotation about y and perturbation through np.dot, scale, shift, one shuffle of
      the points, dropout), the copy into the persistent float64 batch, the cast to float32 and the upload, per batch;
  (b) ModelNetTrainer.run: one staged copy of the draws and pasnl_modelnet_augment per batch, the vote and the tally on the
      device, one readback per epoch.

The step is a no-op that returns fixed logits on the device, so the figures are the input side alone; (b) also pays for the
vote and the tally, (a) does not bring any logits down.  Both use uniform=False (the first 1024 rows), so neither pays for
sampling inside the timed epoch.

Prints one JSON line: clouds per second of both loops (medians over --repeats epochs) for each batch size and rotation
setting, and their ratio.

  python tools/modelnet_train_bench.py [--shapes 9843] [--warmup 1] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median(xs):
    return float(np.median(np.asarray(xs)))


def host_chain(batch_data, rotation, rng, mt):
    """train.py:226-237 on a float64 (bsize, N, 6) batch, numpy as the reference's provider functions use it"""
    bsize, npoint, _ = batch_data.shape
    if rotation:
        for k in range(bsize):
            m = mt.rotation_about_y(rng.uniform())
            batch_data[k, :, 0:3] = np.dot(batch_data[k, :, 0:3], m)
            batch_data[k, :, 3:6] = np.dot(batch_data[k, :, 3:6], m)
        rotated = np.zeros(batch_data.shape, dtype=np.float32)
        for k in range(bsize):
            m = mt.perturbation(rng.randn(3))
            rotated[k, :, 0:3] = np.dot(batch_data[k, :, 0:3], m)
            rotated[k, :, 3:6] = np.dot(batch_data[k, :, 3:6], m)
        batch_data = rotated
    scales = rng.uniform(0.8, 1.25, bsize)
    for k in range(bsize):
        batch_data[k, :, 0:3] *= scales[k]
    shifts = rng.uniform(-0.1, 0.1, (bsize, 3))
    for k in range(bsize):
        batch_data[k, :, 0:3] += shifts[k, :]
    idx = np.arange(npoint)
    rng.shuffle(idx)
    batch_data = batch_data[:, idx, :]
    for k in range(bsize):
        ratio = rng.random() * 0.875
        drop_idx = np.where(rng.random((npoint)) <= ratio)[0]
        if len(drop_idx) > 0:
            batch_data[k, drop_idx, :] = batch_data[k, 0, :]
    return batch_data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=9843)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    import modelnet_flow_ref as R
    from pointasnl_amd import modelnet_trainer as MT

    torch.cuda.set_device(0)
    S, N, C = args.shapes, 1024, 40
    rng = np.random.default_rng(1)
    raw = rng.standard_normal((S, N, 6), dtype=np.float32) * np.float32(0.4)
    labels = rng.integers(0, C, S)
    raw_dev = torch.from_numpy(raw).cuda()
    shapes_dev = [raw_dev[i] for i in range(S)]

    def timed(step):
        for _ in range(args.warmup):
            step()
        secs = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs

    out = dict(metric="modelnet_train_input_loop", shapes=S, points=N, channels=6, step="no-op", repeats=args.repeats)
    for B in (16, 64):
        logits = torch.zeros((B, C), dtype=torch.float32, device="cuda")
        ds = R.ModelNetFlowRef([raw[i] for i in range(S)], labels, batch_size=B, npoints=N, normal_channel=True, shuffle=True,
                               rng=np.random.RandomState(0))
        while ds.has_next_batch():  # fills the reference's cache: the timed epochs assemble batches from prepared shapes
            ds.next_batch()
        ds.reset()
        for rotation in (False, True):
            host_rng = np.random.RandomState(0)

            def host_epoch():
                cur = np.zeros((B, N, 6))
                while ds.has_next_batch():
                    data, label = ds.next_batch()
                    data = host_chain(data, rotation, host_rng, MT)
                    cur[0:data.shape[0], ...] = data
                    fed = torch.from_numpy(cur.astype(np.float32)).cuda()
                    lab = torch.from_numpy(label).cuda()
                    del fed, lab
                ds.reset()

            host_s = timed(host_epoch)
            trainer = MT.ModelNetTrainer(shapes_dev, labels, num_point=N, batch_size=B, normal_channel=True, rotation=rotation,
                                         rng=np.random.RandomState(0))
            dev_s = timed(lambda: trainer.run(lambda x, y: logits))
            host_cps, dev_cps = S / median(host_s), S / median(dev_s)
            out["b%d_%s" % (B, "rotation" if rotation else "plain")] = dict(
                host_clouds_per_s=round(host_cps, 1), modelnettrainer_clouds_per_s=round(dev_cps, 1), ratio=round(dev_cps / host_cps, 3),
                host_s_per_epoch=round(median(host_s), 4), modelnettrainer_s_per_epoch=round(median(dev_s), 4),
                modelnettrainer_s_per_epoch_runs=[round(s, 4) for s in dev_s])
            del trainer
        del ds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
