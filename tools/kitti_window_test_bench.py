"""The SemanticKITTI sliding-window whole-scan test loop, host bookkeeping vs KittiWindowTester, around the same stand-in
forward (sin(x[:, :, :3] @ w + b) * 4 on the device) over one synthetic lidar-like scan of --points points (1/r density out
to --radius metres, so about 2 * radius across) at the reference's test settings (block_points 8192, batch 6, block_size 10,
stride 4, 20 classes, no remission).

  (a) host: the numpy flow of D:278-355 per vote (tests/kitti_window_flow_ref.py, the restatement pinned to the reference
      class; its merge is given the batched distance expression, the reference's per-centre loop is timed on one step and
      extrapolated), every batch uploaded, the logits brought down, argmax and the vote on the host with np.add.at;
  (b) KittiWindowTester.run: windows, gather and vote on the device, two small readbacks per vote.

Prints one JSON line: rows of block_points points per second of both (medians over --repeats votes), their ratio, and per
vote the seconds of the merge (host, both sides), of the membership kernels (pasnl_window_bounds, pasnl_kwindow_count,
pasnl_kwindow_fill, by HIP events) and of gather plus vote (by HIP events, forward excluded).

  python tools/kitti_window_test_bench.py [--points 120000] [--radius 80] [--warmup 1] [--repeats 3]
"""
import argparse
import ctypes
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


def lidar_scan(seed, n, radius):
    """ground disc with 1/r density out to `radius`, a sixth of the points on vertical structures, in ring order"""
    rng = np.random.default_rng(seed)
    r = 2.0 + (radius - 2.0) * rng.random(n)
    th = np.sort(rng.random(n) * 2 * np.pi)
    p = np.stack([r * np.cos(th), r * np.sin(th), rng.standard_normal(n) * 0.03 - 1.7], 1)
    p[: n // 6, 2] += rng.random(n // 6) * 2.5
    return p.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--radius", type=float, default=80.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import kitti_window_flow_ref as R
    from pointasnl_amd import _hip
    from pointasnl_amd.SemanticKITTI import window_tester as W

    torch.cuda.set_device(0)
    C, P, B = 20, 8192, 6
    pts = lidar_scan(5, args.points, args.radius)
    labels = np.random.default_rng(5).integers(0, C, args.points).astype(np.int32)
    wrng = np.random.default_rng(1)
    w, b = (wrng.standard_normal((3, C)) * 0.9).astype(np.float32), wrng.standard_normal(C).astype(np.float32)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

    def forward(x):
        return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

    # (a) the host loop, vote by vote
    ref = R.KittiWindowFlowRef([pts], [labels], None, num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0),
                               nearest=R.nearest_batched)
    pool = np.zeros((args.points, C))

    def host_vote():
        data, idx = ref.getitem(0)
        for start in range(0, data.shape[0], B):
            real = min(B, data.shape[0] - start)
            batch = np.zeros((B, P, 3), np.float32)
            batch[:real] = data[start:start + real]
            logits = forward(torch.from_numpy(batch).cuda()).cpu().numpy()
            R.add_vote(pool, idx[start:start + real], R.predict(logits)[:real])
        return data.shape[0]

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

    host_s, host_rows = timed(host_vote)
    votes = args.warmup + args.repeats
    host_windows_s, host_merge_s = ref.seconds["windows"] / votes, ref.seconds["merge"] / votes
    centers = ref.last["centers"]
    t0 = time.perf_counter()  # one step of the reference's merge as written (D:271-276) over all the centres
    R.nearest(centers[0], centers[1:])
    literal_step_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.nearest_batched(centers[0], centers[1:])
    batched_step_s = time.perf_counter() - t0

    # (b) KittiWindowTester
    tester = W.KittiWindowTester([pts], labels=[labels], num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0))
    dev_s, dev_rows = timed(lambda: tester.run(forward, num_votes=1))

    # the steps alone: the merge on the host, the device steps by HIP events (after a warm-up)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def events(fn, reps=5):
        fn()
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3)
        return median(out)

    n = args.points
    coordmin, coordmax, nx, ny = tester.grid(0)
    hist, counts = tester.count(0, nx, ny)
    t0 = time.perf_counter()
    parts = W.merge_blocks(counts, tester.centers(coordmin, coordmax, nx, ny), tester.min_block_points, tester.nearest)
    dev_merge_s = time.perf_counter() - t0
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    cnt = torch.empty((nx * ny,), dtype=torch.int32, device="cuda")
    woff = torch.from_numpy(np.where(counts > 0, np.cumsum(counts) - counts, -1).astype(np.int32)).cuda()
    cap = int(counts.sum())
    ci = torch.empty((cap,), dtype=torch.int32, device="cuda")
    blk, strd = ctypes.c_double(tester.block_size), ctypes.c_double(tester.stride)

    def membership():
        _hip.launch("pasnl_window_bounds", "bench", ctypes.c_long(n), ptr(tester.xyz[0]), ptr(tester.bounds))
        _hip.launch("pasnl_kwindow_count", "bench", ctypes.c_long(n), ptr(tester.xyz[0]), ptr(tester.bounds), nx, ny, blk, strd, ptr(hist),
                    ptr(cnt))
        _hip.launch("pasnl_kwindow_fill", "bench", ctypes.c_long(n), ptr(tester.xyz[0]), ptr(tester.bounds), nx, ny, blk, strd, ptr(hist),
                    ptr(woff), ctypes.c_long(cap), ptr(ci))

    membership_s = events(membership)
    prep = tester.prepare(0)
    tester.pools[0] = torch.zeros((n, C), dtype=torch.int32, device="cuda")
    logits = torch.zeros((B, P, C), dtype=torch.float32, device="cuda")
    out = (torch.empty((B, P, 3), dtype=torch.float32, device="cuda"), torch.empty((B, P), dtype=torch.int32, device="cuda"))

    def gather_vote():
        for start in range(0, prep["rows"], B):
            _, idx = tester.gather(0, prep, start, B, out)
            tester.vote(0, logits, idx, min(B, prep["rows"] - start))

    gather_vote_s = events(gather_vote, reps=3)

    host_rps = [r / s for r, s in zip(host_rows, host_s)]
    dev_rps = [r / s for r, s in zip(dev_rows, dev_s)]
    print(json.dumps(dict(metric="kitti_window_test_loop", points=n, block_points=P, batch=B, repeats=args.repeats, rows_per_vote=dev_rows,
                          windows=[nx, ny], empty_windows=int(np.count_nonzero(counts == 0)), final_blocks=len(parts), memberships=cap,
                          host_rows_per_s=round(median(host_rps), 2), kittiwindowtester_rows_per_s=round(median(dev_rps), 2),
                          ratio=round(median(dev_rps) / median(host_rps), 3), host_s_per_vote=round(median(host_s), 3),
                          kittiwindowtester_s_per_vote=round(median(dev_s), 3),
                          kittiwindowtester_s_per_vote_runs=[round(s, 3) for s in dev_s],
                          host_windows_s_per_vote=round(host_windows_s, 3), host_merge_batched_s_per_vote=round(host_merge_s, 3),
                          merge_s_per_vote=round(dev_merge_s, 3), merge_step_literal_s=round(literal_step_s, 6),
                          merge_step_batched_s=round(batched_step_s, 6), membership_kernels_s_per_vote=round(membership_s, 6),
                          gather_plus_vote_s_per_vote=round(gather_vote_s, 6))))


if __name__ == "__main__":
    main()
