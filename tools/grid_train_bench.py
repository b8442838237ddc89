"""The two grid training input loops, host chain vs SceneTrainer / ScanTrainer, around the same stand-in step
(sin(x[:, :, :3] @ w + b) * 4 on the device) at the reference's shapes -- ScanNet: num_point 8192, num_buffer 1024, batch 4,
colours, 21 classes; SemanticKITTI: num_point 10240, num_buffer 1024, batch 4, 20 classes -- over the synthetic scenes of
tools/block_test_bench.py and the synthetic scans of tools/kitti_window_test_bench.py.  Input side and tallies only: the step
is a stand-in on both sides and neither trains anything.

  (a) host: the generator as written (tests/grid_train_flow_ref.py, the restatement pinned to the reference's generators) with
      its search answered by a prebuilt sklearn KDTree per cloud, as the reference's is; the numpy restatement of the
      augmentation (tests/philox_ref.py: the kernel's generator and formula on the host); the batch, its labels and its
      weights uploaded, the logits brought down, argmax, the three tallies and the loss in numpy;
  (b) SceneTrainer.run / ScanTrainer.run: crops, labels, augmentation and tallies on the device, one read-back per epoch.

Prints one JSON line: crops per second of both, for both datasets (medians over --repeats epochs).

  python tools/grid_train_bench.py [--points 150000] [--kitti-points 120000] [--radius 50] [--scenes 8] [--steps 4]
                                   [--warmup 1] [--repeats 3] [--device-epochs 5]

One timed device sample is --device-epochs epochs in a row.

--in-radius R (R > 0): the radius form instead -- RadiusSceneTrainer / RadiusScanTrainer against the host chain (sklearn
query_radius + numpy) and against SceneTrainer / ScanTrainer at the same num_point, unaugmented (tools/radius_bench.py);
--kitti-in-radius is the SemanticKITTI radius (default: 5 R).
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


def radius_form(args):
    import block_flow_ref as F
    import radius_bench  # (tools/ is the script's directory)
    from kitti_window_test_bench import lidar_scan

    torch.cuda.set_device(0)
    S, B = args.scenes, 4

    def labels_of(k, n, c):
        return np.random.default_rng(5 + k).integers(0, c, n).astype(np.int32)

    pc = [F.scene(5 + k, args.points) for k in range(S)]
    out = dict(metric="grid_train_loops_radius")
    out["scannet"] = radius_bench.run("scene", "training", [p for p, _ in pc], [c for _, c in pc],
                                      [labels_of(k, args.points, 21) for k in range(S)], args.in_radius, 8192, B, args.steps, 0,
                                      args.warmup, args.repeats, 21)
    scans = [lidar_scan(5 + k, args.kitti_points, args.radius) for k in range(S)]
    out["kitti"] = radius_bench.run("scan", "training", scans, None, [labels_of(k, args.kitti_points, 20) for k in range(S)],
                                    args.kitti_in_radius or 5 * args.in_radius, 10240, B, 0, 0, args.warmup, args.repeats, 20)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--kitti-points", type=int, default=120000)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=4, help="ScanNet: batches per epoch (epoch_steps)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device-epochs", type=int, default=5)
    ap.add_argument("--in-radius", type=float, default=0.0)
    ap.add_argument("--kitti-in-radius", type=float, default=0.0)
    args = ap.parse_args()
    if args.in_radius > 0:
        return radius_form(args)

    from sklearn.neighbors import KDTree

    import block_flow_ref as F
    import grid_train_flow_ref as R
    import scene_flow_ref
    from kitti_window_test_bench import lidar_scan  # (tools/ is the script's directory)
    from pointasnl_amd.ScanNet.scene_trainer import SceneTrainer
    from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer

    torch.cuda.set_device(0)
    S, B, SEED = args.scenes, 4, 0x5EED
    trees = {}

    def tree_first(pc64, centre, k):
        """the restatement's search, answered by the cloud's prebuilt tree (input_trees[...].query, search_tree.query)"""
        return trees[id(pc64)].query(np.asarray(centre).reshape(1, -1), k=k)[1][0], None

    R.nearest_first = scene_flow_ref.nearest_first = tree_first

    def labels_of(k, n, c):
        lab = np.random.default_rng(5 + k).integers(1, c, n)
        lab[np.random.default_rng(50 + k).random(n) < 0.1] = 0
        return lab.astype(np.int32)

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

    out = dict(metric="grid_train_loops", clouds=S, batch=B, repeats=args.repeats, device_epochs_per_sample=args.device_epochs,
               step="stand-in")
    for name in ("scannet", "kitti"):
        if name == "scannet":
            C, P, points = 21, 8192, args.points
            pc = [F.scene(5 + k, points) for k in range(S)]
            clouds, colors = [p for p, _ in pc], [c for _, c in pc]
            labels = [labels_of(k, points, C) for k in range(S)]
            trainer = SceneTrainer(clouds, labels, colors=colors, num_classes=C, num_point=P, num_buffer=1024, batch_size=B,
                                   epoch_steps=args.steps, rng=np.random.RandomState(0), seed=SEED)
            ref = R.SceneTrainFlowRef(clouds, labels, colors=colors, num_classes=C, num_point=P, num_buffer=1024, batch_size=B,
                                      epoch_steps=args.steps, rng=np.random.RandomState(0))
        else:
            C, P, points = 20, 10240, args.kitti_points
            clouds = [lidar_scan(5 + k, points, args.radius) for k in range(S)]
            labels = [labels_of(k, points, C) for k in range(S)]
            trainer = ScanTrainer(clouds, labels, num_classes=C, num_point=P, num_buffer=1024, batch_size=B,
                                  rng=np.random.RandomState(0), seed=SEED)
            ref = R.ScanTrainFlowRef(clouds, labels, num_classes=C, num_point=P, num_buffer=1024, batch_size=B,
                                     rng=np.random.RandomState(0))
        trees.clear()
        for p64 in ref.pc:
            trees[id(p64)] = KDTree(p64, leaf_size=50)
        w, b = R.stand_in_weights(1, C)
        wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

        def step(x, labels_dev, weights_dev):
            return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

        def host_step(fed, label, smpw):
            return step(torch.from_numpy(fed).cuda(), torch.from_numpy(label).cuda(), torch.from_numpy(smpw).cuda()).cpu().numpy()

        host_s = timed(lambda: R.train_epoch(ref, host_step, C, seed=SEED))
        dev_s = [s / args.device_epochs for s in timed(lambda: [trainer.run(step) for _ in range(args.device_epochs)])]
        crops = trainer.steps_per_epoch * B
        host_cps, dev_cps = crops / median(host_s), crops / median(dev_s)
        out[name] = dict(points=points, num_point=P, crops_per_epoch=crops, host_crops_per_s=round(host_cps, 2),
                         trainer_crops_per_s=round(dev_cps, 2), ratio=round(dev_cps / host_cps, 3),
                         host_s_per_epoch=round(median(host_s), 3), trainer_s_per_epoch=round(median(dev_s), 4),
                         host_s_per_epoch_runs=[round(s, 3) for s in host_s], trainer_s_per_epoch_runs=[round(s, 4) for s in dev_s])
        del trainer
    print(json.dumps(out))


if __name__ == "__main__":
    main()
