"""The ScanNet sliding-window whole-scene test loop, host bookkeeping vs WindowTester, around the same stand-in forward
(sin(x[:, :, :3] @ w + b) * 4 on the device) over one synthetic indoor scene of --points points at the reference's defaults
(block_points 8192, batch 6, stride 0.5, 21 classes, with rgb).

  (a) host: the numpy flow of D:183-300 per vote (tests/window_flow_ref.py, the restatement pinned to the reference class),
      every batch uploaded, the logits brought down, argmax and the vote on the host -- vectorised with np.add.at, which is
      far faster than the reference's Python double loop (also timed, on one batch);
  (b) WindowTester.run: noise step, windows, gather and vote on the device, two small readbacks per vote.

Prints one JSON line: rows of block_points points (crops) per second of both (medians over --repeats votes), their ratio,
and, by HIP events, the noise step alone (pasnl_window_noise: the sequential centroid and the move), the bounds, the
window count and the fill.

  python tools/window_test_bench.py [--points 200000] [--warmup 1] [--repeats 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import window_flow_ref as R
    from pointasnl_amd import _hip
    from pointasnl_amd.ScanNet import window_tester as W

    torch.cuda.set_device(0)
    C, P, B = 21, 8192, 6
    p, c = R.scene(5, args.points)
    pts = np.ascontiguousarray(np.hstack([p, c]))
    labels = np.random.default_rng(5).integers(0, C, args.points).astype(np.int64)
    wrng = np.random.default_rng(1)
    w, b = (wrng.standard_normal((3, C)) * 0.9).astype(np.float32), wrng.standard_normal(C).astype(np.float32)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

    def forward(x):
        return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

    # (a) the host loop, vote by vote
    ref = R.WindowFlowRef([pts.copy()], [labels], num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0))
    pool = np.zeros((args.points, C))
    last = {}

    def host_vote():
        data, _, wgt, idx = ref.getitem(0)
        for start in range(0, data.shape[0], B):
            real = min(B, data.shape[0] - start)
            batch = np.zeros((B, P, 6), np.float32)
            batch[:real] = data[start:start + real]
            logits = forward(torch.from_numpy(batch).cuda()).cpu().numpy()
            pred = R.predict(logits)
            R.add_vote(pool, idx[start:start + real], pred[:real], wgt[start:start + real])
            last.update(idx=idx[start:start + real], pred=pred[:real], wgt=wgt[start:start + real])
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
    t0 = time.perf_counter()  # the reference's add_vote as written (T:96-103), one batch
    scratch = np.zeros((args.points, C))
    for bb in range(last["pred"].shape[0]):
        for n in range(P):
            if last["wgt"][bb, n]:
                scratch[int(last["idx"][bb, n]), int(last["pred"][bb, n])] += 1
    loop_vote_s = (time.perf_counter() - t0) * B / last["pred"].shape[0]

    # (b) WindowTester
    tester = W.WindowTester([pts.copy()], labels=[labels], num_classes=C, block_points=P, batch_size=B, rng=np.random.RandomState(0))
    dev_s, dev_rows = timed(lambda: tester.run(forward, num_votes=1))

    # the device steps alone, by HIP events (each launch sequence timed on its own, after a warm-up)
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
            out.append(e0.elapsed_time(e1) * 1e3)
        return round(median(out), 1)

    n = args.points
    m = int(np.ceil(0.2 * n))
    crng = np.random.RandomState(1)
    choices = crng.choice(n, m)
    slot = np.full(n, -1, np.int64)
    slot[choices] = np.arange(m)
    ch = torch.from_numpy(choices.astype(np.int32)).cuda()
    sh = torch.from_numpy((crng.randn(m, 3) - 0.5) / 0.5 * 0.002).cuda()
    la = torch.from_numpy((slot[choices] == np.arange(m)).astype(np.uint8)).cuda()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    xyz, stamp, stats, bounds = tester.xyz[0], tester.stamp[0], tester.stats, tester.bounds
    noise_us = events(lambda: _hip.launch("pasnl_window_noise", "bench", ctypes.c_long(n), ptr(xyz), m, ptr(ch), ptr(sh), ptr(la), 1 << 30,
                                          ptr(stamp), ptr(stats)))
    centroid_us = events(lambda: _hip.launch("pasnl_window_noise", "bench", ctypes.c_long(n), ptr(xyz), 0, None, None, None, 1 << 30,
                                             ptr(stamp), ptr(stats)))
    bounds_us = events(lambda: _hip.launch("pasnl_window_bounds", "bench", ctypes.c_long(n), ptr(xyz), ptr(bounds)))
    coordmin, coordmax, nx, ny = tester.grid(0)
    hist = torch.empty((int(_hip.lib().pasnl_window_hist_bytes(ctypes.c_long(n), nx, ny)) // 4,), dtype=torch.int32, device="cuda")
    cnt = torch.empty((nx * ny,), dtype=torch.int32, device="cuda")
    count_us = events(lambda: _hip.launch("pasnl_window_count", "bench", ctypes.c_long(n), ptr(xyz), ptr(bounds), nx, ny,
                                          ctypes.c_double(0.5), ptr(hist), ptr(cnt)))
    counts = cnt.cpu().numpy().astype(np.int64)
    woff = torch.from_numpy((np.cumsum(counts) - counts).astype(np.int32)).cuda()
    cap = int(counts.sum())
    ci, cm = torch.empty((cap,), dtype=torch.int32, device="cuda"), torch.empty((cap,), dtype=torch.uint8, device="cuda")
    fill_us = events(lambda: _hip.launch("pasnl_window_fill", "bench", ctypes.c_long(n), ptr(xyz), ptr(bounds), nx, ny, ctypes.c_double(0.5),
                                         ptr(hist), ptr(woff), ctypes.c_long(cap), ptr(ci), ptr(cm)))

    host_cps = [r / s for r, s in zip(host_rows, host_s)]
    dev_cps = [r / s for r, s in zip(dev_rows, dev_s)]
    print(json.dumps(dict(metric="window_test_loop", points=n, block_points=P, batch=B, repeats=args.repeats, rows_per_vote=dev_rows,
                          host_crops_per_s=round(median(host_cps), 2), windowtester_crops_per_s=round(median(dev_cps), 2),
                          ratio=round(median(dev_cps) / median(host_cps), 3), host_s_per_vote=round(median(host_s), 3),
                          windowtester_s_per_vote=round(median(dev_s), 3), windowtester_s_per_vote_runs=[round(s, 3) for s in dev_s],
                          reference_add_vote_loop_s_per_batch=round(loop_vote_s, 4), noise_step_us=noise_us,
                          centroid_and_extent_us=centroid_us, bounds_us=bounds_us, window_count_us=count_us, window_fill_us=fill_us,
                          windows=[nx, ny], memberships=cap)))


if __name__ == "__main__":
    main()
