"""The ScanNet grid test loop, host bookkeeping vs SceneTester, around the same pointasnl_sem_seg forward (seeded
VariableStore, B = 4, num_point = 8192, feature_channel = 3) over synthetic indoor scenes of ~1e5 sub-sampled points.

  (a) host: the reference's numpy flow (D:482-541, T:141-149) per crop -- sklearn KDTree.query around the noisy pick, the
      batch uploaded, the float32 votes on the host;
  (b) SceneTester: next_batch() / vote() on the device, one readback per epoch.

Prints one JSON line: crops/s of both (medians over --repeats timed blocks), their ratio, the device chain's us per crop
(HIP events around next_batch alone), its launches per crop, and the confusion kernel's time for a 1e5-point scene.

  python tools/scene_test_bench.py [--scenes 6] [--points 100000] [--batches 6] [--warmup 2] [--repeats 3]

--in-radius R (R > 0): the radius form instead -- RadiusSceneTester against the host chain (sklearn query_radius + numpy) and
against SceneTester at the same num_point, input side only (tools/radius_bench.py).
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


def indoor(seed, n):
    """a 7 x 6 m room: floor, two walls, boxes of furniture; colours in [0, 1)"""
    rng = np.random.default_rng(seed)
    a, b = n // 2, n // 2 + n // 4
    p = np.empty((n, 3))
    p[:a] = np.stack([rng.random(a) * 7, rng.random(a) * 6, rng.standard_normal(a) * 0.01], 1)
    w = b - a
    side = rng.random(w) < 0.5
    p[a:b] = np.stack([np.where(side, rng.random(w) * 7, 0.0), np.where(side, 0.0, rng.random(w) * 6), rng.random(w) * 2.6], 1)
    m = n - b
    box = rng.integers(0, 8, m)
    corner = rng.random((8, 2)) * np.array([6.0, 5.0])
    p[b:] = np.stack([corner[box, 0] + rng.random(m), corner[box, 1] + rng.random(m), rng.random(m) * 0.9], 1)
    return p.astype(np.float32), rng.random((n, 3)).astype(np.float32)


def median(xs):
    return float(np.median(np.asarray(xs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=6)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--in-radius", type=float, default=0.0)
    args = ap.parse_args()
    if args.in_radius > 0:
        import radius_bench  # (tools/ is the script's directory)

        torch.cuda.set_device(0)
        pc = [indoor(2000 + i, args.points + 997 * i) for i in range(args.scenes)]
        labels = [np.zeros(len(p), np.int32) for p, _ in pc]
        print(json.dumps(radius_bench.run("scene", "test", [p for p, _ in pc], [c for _, c in pc], labels, args.in_radius, 8192,
                                          args.batch, args.batches, args.batches, args.warmup, args.repeats, 21)))
        return

    from sklearn.neighbors import KDTree

    from pointasnl_amd import _hip
    from pointasnl_amd.models import pointasnl_sem_seg
    from pointasnl_amd.ScanNet import scene_tester as T
    from pointasnl_amd.utils import tf_util

    torch.cuda.set_device(0)
    B, NP, NB, C = args.batch, 8192, 1024, 21
    pc = [indoor(2000 + i, args.points + 997 * i) for i in range(args.scenes)]
    scenes, colors = [p for p, _ in pc], [c for _, c in pc]
    tf_util.set_store(tf_util.VariableStore(seed=5))

    def forward(x):
        with torch.no_grad():
            out = pointasnl_sem_seg.get_model(x, False, C, feature_channel=3)
        return (out[0] if isinstance(out, (tuple, list)) else out).float()

    # (a) the host loop
    rng = np.random.RandomState(0)
    trees = [KDTree(s, leaf_size=50) for s in scenes]
    potentials = [rng.rand(len(s)) * 1e-3 for s in scenes]
    min_potentials = [float(np.min(p)) for p in potentials]
    test_probs = [np.zeros((len(s), C - 1), np.float32) for s in scenes]

    def host_batch():
        xs, inds, clouds = [], [], []
        for _ in range(B):
            cloud_ind = int(np.argmin(min_potentials))
            point_ind = np.argmin(potentials[cloud_ind])
            points = np.array(trees[cloud_ind].data, copy=False)
            center_point = points[point_ind, :].reshape(1, -1)
            pick_point = center_point + rng.normal(scale=0.35, size=center_point.shape)
            k = NP + NB + rng.randint(0, NB // 4)
            input_inds = trees[cloud_ind].query(pick_point, k=k)[1][0]
            idx = np.arange(k)
            rng.shuffle(idx)
            input_inds = input_inds[idx][:NP]
            dists = np.sum(np.square((points[input_inds] - pick_point).astype(np.float32)), axis=1)
            potentials[cloud_ind][input_inds] += np.square(1 - dists / np.max(dists))
            min_potentials[cloud_ind] = float(np.min(potentials[cloud_ind]))
            input_points = (points[input_inds] - pick_point).astype(np.float32)
            xs.append(np.hstack((input_points, colors[cloud_ind][input_inds])))
            inds.append(input_inds)
            clouds.append(cloud_ind)
        return np.stack(xs), np.stack(inds), clouds

    def host_step():
        x, inds, clouds = host_batch()
        logits = forward(torch.from_numpy(x).cuda())
        probs = torch.softmax(logits[:, :, 1:], -1).cpu().numpy()
        for j in range(B):
            c_i = clouds[j]
            test_probs[c_i][inds[j]] = 0.98 * test_probs[c_i][inds[j]] + (1 - 0.98) * probs[j]

    def timed(step):
        for _ in range(args.warmup):
            step()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                step()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    crops = args.batches * B
    host_s = timed(host_step)
    book = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.batches):
            host_batch()
        book.append(time.perf_counter() - t0)

    # (b) SceneTester
    tester = T.SceneTester(scenes, colors=colors, num_classes=C, num_point=NP, num_buffer=NB, batch_size=B,
                           label_values=np.arange(C), rng=np.random.RandomState(0))

    def dev_step():
        x, inds, clouds = tester.next_batch()
        tester.vote(forward(x), inds, clouds)

    dev_s = timed(dev_step)
    chain = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.repeats):
        e0.record()
        for _ in range(args.batches):
            tester.next_batch()
        e1.record()
        torch.cuda.synchronize()
        chain.append(e0.elapsed_time(e1) * 1e3 / crops)
    # kernels per crop: every C-ABI call of one batch's chain, by the number of kernels it starts (include/pasnl.h)
    per_call = {"pasnl_scene_pick_crop": 8, "pasnl_scene_order_gather": 1, "pasnl_scene_potential_update": 1}
    _hip.PROFILE = []
    tester.enqueue()
    torch.cuda.synchronize()
    launches = sum(per_call[sym] for sym, *_ in _hip.PROFILE) / B
    _hip.PROFILE = None

    # the confusion matrix of one 1e5-point scene, 21 label values
    lrng = np.random.default_rng(1)
    lv = torch.arange(C, dtype=torch.int32, device="cuda")
    t = torch.from_numpy(lrng.integers(0, C, 100000).astype(np.int32)).cuda()
    p = torch.from_numpy(lrng.integers(0, C, 100000).astype(np.int32)).cuda()
    out = torch.zeros((C, C), dtype=torch.int64, device="cuda")
    import ctypes

    def cm():
        _hip.launch("pasnl_confusion_matrix", "bench", ctypes.c_long(100000), _hip.ptr(t), _hip.ptr(p), _hip.ptr(lv), C, _hip.ptr(out))
    for _ in range(5):
        cm()
    cms = []
    for _ in range(args.repeats):
        e0.record()
        for _ in range(20):
            cm()
        e1.record()
        torch.cuda.synchronize()
        cms.append(e0.elapsed_time(e1) * 1e3 / 20)

    print(json.dumps(dict(metric="scene_test_loop", scenes=args.scenes, points=args.points, batch=B, num_point=NP,
                          batches=args.batches, repeats=args.repeats,
                          host_crops_per_s=round(crops / median(host_s), 2), scenetester_crops_per_s=round(crops / median(dev_s), 2),
                          ratio=round(median(host_s) / median(dev_s), 3),
                          host_bookkeeping_ms_per_crop=round(median(book) * 1e3 / crops, 3),
                          chain_us_per_crop=round(median(chain), 1), chain_us_per_crop_runs=[round(c, 1) for c in chain],
                          launches_per_crop=launches, confusion_us_per_100k=round(median(cms), 1),
                          confusion_total=int(out.sum().item()))))


if __name__ == "__main__":
    main()
