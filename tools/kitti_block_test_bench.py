"""SemanticKITTI's two training-time validation loops, host bookkeeping vs KittiBlockTester, around the same stand-in forward
(sin(x[:, :, :3] @ w + b) * 4 on the device) over synthetic lidar-sized scans of --points points (the scans of
tools/kitti_window_test_bench.py: a ground disc with 1/r density out to --radius metres) at the reference's defaults
(block_points 8192, batch 8, block_size 10, 20 classes, no remission).  Bookkeeping only: the forward is a stand-in on both
sides.

  (a) host: the numpy flow of D:68-109 / D:164-211 and T:267-328 / T:331-418 (tests/kitti_block_flow_ref.py, the restatement
      pinned to the reference classes), every batch uploaded, the logits brought down, argmax, counters and loss on the host;
  (b) KittiBlockTester.run_chopped / run_whole: crops, rows, rotation and score on the device.

Prints one JSON line -- blocks of block_points points per second of both, for both loops (medians over --repeats epochs), and
their ratios -- and writes it to --out (default profiles/kitti_block_test_bench.json; '' writes nothing).

  python tools/kitti_block_test_bench.py [--points 120000] [--radius 50] [--scans 8] [--warmup 1] [--repeats 3] [--out PATH]
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
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_block_test_bench.json"))
    args = ap.parse_args()

    import kitti_block_flow_ref as R
    from kitti_window_test_bench import lidar_scan  # (tools/ is the script's directory)
    from pointasnl_amd.SemanticKITTI import block_tester as T

    torch.cuda.set_device(0)
    C, P, B, S = 20, 8192, 8, args.scans
    scans, labels = [], []
    for k in range(S):
        scans.append(lidar_scan(5 + k, args.points, args.radius))
        lab = np.random.default_rng(5 + k).integers(1, C, args.points)
        lab[np.random.default_rng(50 + k).random(args.points) < 0.1] = 0
        labels.append(lab.astype(np.int32))
    w, b = R.stand_in_weights(1, C)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    lut = np.ones(C, np.float32)

    def forward(x):
        return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

    def host_forward(fed):
        return forward(torch.from_numpy(fed).cuda()).cpu().numpy()

    rng = np.random.RandomState(0)

    def host_chopped():
        out = R.eval_chopped(lambda i: R.chopped_item(scans[i], None, labels[i], lut, P, rng)[:3], S, B, P, 3, host_forward, C, rng)
        return len(out["fed"]) * B

    def host_whole():
        out = R.eval_whole(lambda i: R.whole_item(scans[i], None, labels[i], lut, P, rng)[:3], S, B, host_forward, C)
        return len(out["fed"]) * B

    tester = T.KittiBlockTester(scans, labels, num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0))

    def dev_chopped():
        tester.run_chopped(forward)
        return tester.forwards * B

    def dev_whole():
        tester.run_whole(forward)
        return tester.forwards * B

    def timed(step):
        for _ in range(args.warmup):
            step()
        secs, rows = [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows.append(step())
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs, rows

    out = dict(metric="kitti_block_test_loops", points=args.points, radius=args.radius, scans=S, block_points=P, batch=B,
               repeats=args.repeats)
    for name, host_step, dev_step in (("chopped", host_chopped, dev_chopped), ("whole", host_whole, dev_whole)):
        hs, hr = timed(host_step)
        ds, dr = timed(dev_step)
        host_bps, dev_bps = median([r / s for r, s in zip(hr, hs)]), median([r / s for r, s in zip(dr, ds)])
        out.update({name + "_blocks_per_epoch": dr, name + "_host_blocks_per_s": round(host_bps, 2),
                    name + "_kittiblocktester_blocks_per_s": round(dev_bps, 2), name + "_ratio": round(dev_bps / host_bps, 3),
                    name + "_host_s_per_epoch": round(median(hs), 3), name + "_kittiblocktester_s_per_epoch": round(median(ds), 4),
                    name + "_kittiblocktester_s_per_epoch_runs": [round(s, 4) for s in ds]})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
