"""ScanNet's two training-time validation loops, host bookkeeping vs BlockTester, around the same stand-in forward
(sin(x[:, :, :3] @ w + b) * 4 on the device) over synthetic indoor scenes of --points points at the reference's defaults
(block_points 8192, batch 8, 21 classes, with rgb).

  (a) host: the numpy flow of D:31-64 / D:92-129 and T:279-329 / T:333-420 (tests/block_flow_ref.py, the restatement pinned
      to the reference classes), every batch uploaded, the logits brought down, argmax, counters and loss on the host;
  (b) BlockTester.run_chopped / run_whole: crops, rows, normalisation, rotation and score on the device.

Prints one JSON line: blocks of block_points points per second of both, for both loops (medians over --repeats epochs), and
their ratios.

  python tools/block_test_bench.py [--points 150000] [--scenes 8] [--warmup 1] [--repeats 3]
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
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import block_flow_ref as R
    from pointasnl_amd.ScanNet import block_tester as T

    torch.cuda.set_device(0)
    C, P, B, S = 21, 8192, 8, args.scenes
    scenes, labels = [], []
    for k in range(S):
        p, c = R.scene(5 + k, args.points)
        scenes.append(np.ascontiguousarray(np.hstack([p, c])))
        lab = np.random.default_rng(5 + k).integers(1, C, args.points)
        lab[np.random.default_rng(50 + k).random(args.points) < 0.1] = 0
        labels.append(lab.astype(np.int64))
    w, b = R.stand_in_weights(1, C)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    weights = np.ones(C)

    def forward(x):
        return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

    def host_forward(fed):
        return forward(torch.from_numpy(fed).cuda()).cpu().numpy()

    rng = np.random.RandomState(0)

    def host_chopped():
        out = R.eval_chopped(lambda i: R.chopped_item(scenes[i], labels[i], weights, P, rng)[:3], S, B, P, 6, host_forward, C, rng)
        return len(out["fed"]) * B

    def host_whole():
        out = R.eval_whole(lambda i: R.whole_item(scenes[i], labels[i], weights, P, rng)[:3], S, B, host_forward, C)
        return len(out["fed"]) * B

    tester = T.BlockTester(scenes, labels, num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0))

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

    out = dict(metric="block_test_loops", points=args.points, scenes=S, block_points=P, batch=B, repeats=args.repeats)
    for name, host_step, dev_step in (("chopped", host_chopped, dev_chopped), ("whole", host_whole, dev_whole)):
        hs, hr = timed(host_step)
        ds, dr = timed(dev_step)
        host_bps, dev_bps = median([r / s for r, s in zip(hr, hs)]), median([r / s for r, s in zip(dr, ds)])
        out.update({name + "_blocks_per_epoch": dr, name + "_host_blocks_per_s": round(host_bps, 2),
                    name + "_blocktester_blocks_per_s": round(dev_bps, 2), name + "_ratio": round(dev_bps / host_bps, 3),
                    name + "_host_s_per_epoch": round(median(hs), 3), name + "_blocktester_s_per_epoch": round(median(ds), 4),
                    name + "_blocktester_s_per_epoch_runs": [round(s, 4) for s in ds]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
