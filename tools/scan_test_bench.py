"""The SemanticKITTI test loop, host bookkeeping vs ScanTester, around the same pointasnl_sem_seg_res forward (seeded
VariableStore, B = 8, num_point = 10240) over synthetic lidar-like scans of ~1e5 sub-sampled points.

  (a) host: the reference's numpy flow (D:224-234, T:147-154) per crop, DeviceScan + crop_pc for the search, the batch
      uploaded, the votes on the host in float16;
  (b) ScanTester: next_batch() / vote() on the device, one readback per epoch.

Prints one JSON line: crops/s of both, their ratio, the device chain's us per crop (HIP events around next_batch alone)
and the reprojection's us per 120k-point raw scan.

  python tools/scan_test_bench.py [--scans 8] [--points 100000] [--batches 6] [--warmup 2] [--batch 8] [--num-point 10240]

--in-radius R (R > 0): the radius form instead -- RadiusScanTester against the host chain (sklearn query_radius + numpy) and
against ScanTester at the same num_point, input side only (tools/radius_bench.py); medians of three timed blocks.
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


def lidar(seed, n):
    rng = np.random.default_rng(seed)
    r = 2.0 + 48.0 * rng.random(n) ** 2
    th = rng.random(n) * 2 * np.pi
    p = np.stack([r * np.cos(th), r * np.sin(th), rng.standard_normal(n) * 0.05 - 1.7], 1)
    w = n // 5
    p[:w, 2] = rng.random(w) * 3.0 - 1.7
    return p.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--num-point", type=int, default=10240)
    ap.add_argument("--in-radius", type=float, default=0.0)
    args = ap.parse_args()
    if args.in_radius > 0:
        import radius_bench  # (tools/ is the script's directory)

        torch.cuda.set_device(0)
        scans = [lidar(1000 + i, args.points + 997 * i) for i in range(args.scans)]
        labels = [np.zeros(len(s), np.int32) for s in scans]
        print(json.dumps(radius_bench.run("scan", "test", scans, None, labels, args.in_radius, args.num_point, args.batch, 0,
                                          args.batches, args.warmup, 3, 20)))
        return

    from pointasnl_amd.models import pointasnl_sem_seg_res
    from pointasnl_amd.SemanticKITTI import scan_tester as T
    from pointasnl_amd.SemanticKITTI import semantic_kitti_dataset_grid as G
    from pointasnl_amd.utils import tf_util

    torch.cuda.set_device(0)
    B, NP, NB, C = args.batch, args.num_point, 1024, 20
    scans = [lidar(1000 + i, args.points + 997 * i) for i in range(args.scans)]
    tf_util.set_store(tf_util.VariableStore(seed=5))

    def forward(x):
        with torch.no_grad():
            out = pointasnl_sem_seg_res.get_model(x, False, C, feature_channel=0)
        return (out[0] if isinstance(out, (tuple, list)) else out).float()

    # (a) the host loop
    rng = np.random.RandomState(0)
    trees = [G.DeviceScan(s) for s in scans]
    pcs = [s.astype(np.float64) for s in scans]
    possibility = [rng.rand(len(s)) * 1e-3 for s in scans]
    min_possibility = [float(np.min(p)) for p in possibility]
    test_probs = [np.zeros((len(s), C), np.float16) for s in scans]
    labels = [np.zeros(len(s), np.uint8) for s in scans]

    def host_batch():
        pts, inds, clouds = [], [], []
        for _ in range(B):
            cloud_ind = int(np.argmin(min_possibility))
            pick_idx = np.argmin(possibility[cloud_ind])
            pc = pcs[cloud_ind]
            sel_pc, _, sel_idx = G.crop_pc(pc, labels[cloud_ind], trees[cloud_ind], pick_idx, NP, NB, 0.0, rng=rng)
            dists = np.sum(np.square((sel_pc - pc[pick_idx]).astype(np.float32)), axis=1)
            delta = np.square(1 - dists / np.max(dists))
            possibility[cloud_ind][sel_idx] += delta
            min_possibility[cloud_ind] = np.min(possibility[cloud_ind])
            pts.append(sel_pc.astype(np.float32))
            inds.append(sel_idx)
            clouds.append(cloud_ind)
        return np.stack(pts), np.stack(inds), clouds

    def host_step():
        pts, inds, clouds = host_batch()
        logits = forward(torch.from_numpy(pts).cuda())
        probs = torch.softmax(logits, -1).cpu().numpy()
        for j in range(B):
            c_i = clouds[j]
            test_probs[c_i][inds[j]] = 0.98 * test_probs[c_i][inds[j]] + (1 - 0.98) * probs[j]

    for _ in range(args.warmup):
        host_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.batches):
        host_step()
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    th0 = time.perf_counter()
    for _ in range(args.batches):
        host_batch()
    host_book_s = time.perf_counter() - th0

    # (b) ScanTester
    tester = T.ScanTester(scans, num_classes=C, num_point=NP, num_buffer=NB, batch_size=B, rng=np.random.RandomState(0))

    def dev_step():
        pts, inds, clouds = tester.next_batch()
        tester.vote(forward(pts), inds, clouds)

    for _ in range(args.warmup):
        dev_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.batches):
        dev_step()
    torch.cuda.synchronize()
    dev_s = time.perf_counter() - t0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.batches):
        tester.next_batch()
    e1.record()
    torch.cuda.synchronize()
    chain_us = e0.elapsed_time(e1) * 1e3 / (args.batches * B)

    # reprojection of one 120k-point raw scan onto scan 0
    raw = torch.from_numpy(lidar(7, 120000)).cuda()
    tester.reproject(0, raw_points=raw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        tester.reproject(0, raw_points=raw)
    torch.cuda.synchronize()
    rep_us = (time.perf_counter() - t0) * 1e6 / reps
    p0 = T.project(tester.scan_points(0), raw)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        T.project(tester.scan_points(0), raw)
    e1.record()
    torch.cuda.synchronize()

    crops = args.batches * B
    print(json.dumps(dict(metric="scan_test_loop", scans=args.scans, points=args.points, batch=B, num_point=NP, batches=args.batches,
                          host_crops_per_s=round(crops / host_s, 2), scantester_crops_per_s=round(crops / dev_s, 2),
                          ratio=round(host_s / dev_s, 3), host_bookkeeping_ms_per_crop=round(host_book_s * 1e3 / crops, 3),
                          chain_us_per_crop=round(chain_us, 1), reproject_us_per_120k_scan=round(rep_us, 1),
                          project_only_us=round(e0.elapsed_time(e1) * 1e3 / reps, 1), proj_checksum=int(p0.sum().item()))))


if __name__ == "__main__":
    main()
