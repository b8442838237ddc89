"""The two segmentation training input loops, host chain vs BlockTrainer / KittiBlockTrainer, around the same stand-in step
(sin(x[:, :, :3] @ w + b) * 4 on the device) at the reference's shape -- block_points 8192, batch 8 -- over the synthetic
scenes of tools/block_test_bench.py (indoor scenes of --points points with colours, 21 classes) and the synthetic scans of
tools/kitti_block_test_bench.py (a ground disc of --kitti-points points, 20 classes, no remission).  Input side and tallies
only: the step is a stand-in on both sides and neither trains anything.

  (a) host: `train_one_epoch` as written (tests/block_train_flow_ref.py, the restatement pinned to the reference's run) --
      the shuffle, every item in numpy, rotate_point_cloud_z and (ScanNet) normalize_data in numpy, the batch, its labels
      and its weights uploaded, the logits brought down, argmax, the three tallies and the loss in numpy;
  (b) BlockTrainer.run / KittiBlockTrainer.run: items, transform and tallies on the device, one read-back per try of the
      rejection loop and one per epoch.

Prints one JSON line: blocks of block_points points per second of both, for both datasets (medians over --repeats epochs),
and their ratios.

  python tools/block_train_bench.py [--points 150000] [--kitti-points 120000] [--radius 50] [--scenes 16] [--warmup 1]
                                    [--repeats 5] [--device-epochs 20]

A device epoch of two batches lasts a few milliseconds, so one timed device sample is --device-epochs epochs in a row.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--kitti-points", type=int, default=120000)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device-epochs", type=int, default=20)
    args = ap.parse_args()

    import block_flow_ref as F
    import block_train_flow_ref as R
    from kitti_window_test_bench import lidar_scan  # (tools/ is the script's directory)
    from pointasnl_amd.ScanNet.block_trainer import BlockTrainer
    from pointasnl_amd.SemanticKITTI.block_trainer import KittiBlockTrainer

    torch.cuda.set_device(0)
    P, B, S = 8192, 8, args.scenes

    def labels_of(k, n, c, dtype):
        lab = np.random.default_rng(5 + k).integers(1, c, n)
        lab[np.random.default_rng(50 + k).random(n) < 0.1] = 0
        return lab.astype(dtype)

    def timed(epoch):
        for _ in range(args.warmup):
            epoch()
        secs = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs

    out = dict(metric="block_train_loops", scenes=S, block_points=P, batch=B, repeats=args.repeats, device_epochs_per_sample=args.device_epochs,
               step="stand-in")
    for name in ("scannet", "kitti"):
        if name == "scannet":
            C, width, points = 21, 6, args.points
            clouds = [np.ascontiguousarray(np.hstack(F.scene(5 + k, points))) for k in range(S)]
            labels = [labels_of(k, points, C, np.int64) for k in range(S)]
            weights = np.ones(C)
            trainer = BlockTrainer(clouds, labels, num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0))
            transform = R.train_batch
        else:
            C, width, points = 20, 3, args.kitti_points
            clouds = [lidar_scan(5 + k, points, args.radius) for k in range(S)]
            labels = [labels_of(k, points, C, np.int32) for k in range(S)]
            weights = np.ones(C, np.float32)
            trainer = KittiBlockTrainer(clouds, labels, num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0))
            transform = R.kitti_train_batch
        w, b = R.stand_in_weights(1, C)
        wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

        def step(x, labels_dev, smpw_dev):
            return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

        def host_step(fed, label, smpw):
            return step(torch.from_numpy(fed).cuda(), torch.from_numpy(label).cuda(), torch.from_numpy(smpw).cuda()).cpu().numpy()

        rng = np.random.RandomState(0)
        if name == "scannet":
            def getitem(i):
                return R.chopped_item(clouds[i], labels[i], weights, P, rng)[:3]
        else:
            def getitem(i):
                return R.kitti_chopped_item(clouds[i], None, labels[i], weights, P, rng)[:3]

        host_s = timed(lambda: R.train_epoch(getitem, S, B, P, width, transform, host_step, C, rng))
        dev_s = [s / args.device_epochs for s in timed(lambda: [trainer.run(step) for _ in range(args.device_epochs)])]
        blocks = int(S / B) * B
        host_bps, dev_bps = blocks / median(host_s), blocks / median(dev_s)
        out[name] = dict(points=points, blocks_per_epoch=blocks, host_blocks_per_s=round(host_bps, 2),
                         trainer_blocks_per_s=round(dev_bps, 2), ratio=round(dev_bps / host_bps, 3),
                         host_s_per_epoch=round(median(host_s), 3), trainer_s_per_epoch=round(median(dev_s), 4),
                         host_s_per_epoch_runs=[round(s, 3) for s in host_s], trainer_s_per_epoch_runs=[round(s, 4) for s in dev_s])
        del trainer
    print(json.dumps(out))


if __name__ == "__main__":
    main()
