"""Forward + backward of training-mode batch norm (tf_util.batch_norm_train: pasnl_cls_bn_train / pasnl_cls_bn_train_grad of
csrc/bn_train.hip, ReLU fused) against torch.nn.functional.batch_norm(training=True) + ReLU under autograd, and against the
library's own torch route (tf_util.BN_TRAIN_FUSED = False), on (rows, c) matrices of the models:
cls layer 1 (64*512*32, 32), cls layer 2 (64*128*32, 128), the after_conv outputs (64*512, 128), the head (64, 512) and ScanNet
layer 1 (16*1024*32, 32).

Per shape, the median of three runs; a run is the median of --repeats steps between HIP events after --warmup steps, in
microseconds.  A step is one forward and one backward to x, gamma and beta, moving statistics updated:
  fused_step_us / functional_step_us / torch_route_step_us
  fwd_us / bwd_us            the two entries alone, through the C ABI into preallocated buffers
  fwd_gbps / bwd_gbps        their minimum traffic (forward 2 reads + 1 write of the matrix; backward x, y, grad_y twice and
                             grad_x once: 7 passes) over the time, and as a share of the 8.0 TB/s HBM3E peak (hbm_peak_share)
plus the largest |difference| of the fused and the functional gradients relative to their scale (grad_rel_diff) and of each
against the same formula in float64 on the device (fused_err64 / functional_err64).  One JSON line per shape.  --cls: one more line, the classifier's whole training step (forward + backward at B = 16 x 1024) on
the fused route against the torch route.

  python tools/bn_train_bench.py [--warmup 3] [--repeats 11] [--shapes rows,c ...] [--cls]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64 * 512 * 32, 32), (64 * 128 * 32, 128), (64 * 512, 128), (64, 512), (16 * 1024 * 32, 32)]
RUNS = 3
HBM_PEAK = 8.0e12  # bytes/s, HBM3E specification of MI355X


def timed(fn, warmup, repeats):
    """median over RUNS runs of the median time of fn() in microseconds by HIP events"""
    runs = []
    for _ in range(RUNS):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        runs.append(float(np.median(times)))
    return float(np.median(runs))


def rounded(rec):
    return {k: (round(v, 3) if isinstance(v, float) and v > 1e-3 else v) for k, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--shapes", nargs="*", default=None, help="rows,c ...")
    ap.add_argument("--cls", action="store_true", help="also the classifier's training step, fused route against torch route")
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in s.split(",")) for s in args.shapes]

    from pointasnl_amd import _hip
    from pointasnl_amd.utils import tf_util as T

    _hip.require_device()
    torch.cuda.set_device(0)
    lib = _hip.lib()
    P = _hip.ptr
    for rows, c in shapes:
        gen = torch.Generator(device="cuda").manual_seed(rows * 31 + c)
        x = (torch.randn((rows, c), device="cuda", generator=gen) * 1.5 + 0.3).requires_grad_()
        gamma = (torch.rand((c,), device="cuda", generator=gen) + 0.5).requires_grad_()
        beta = (torch.rand((c,), device="cuda", generator=gen) - 0.5).requires_grad_()
        mm, mv = torch.zeros((c,), device="cuda"), torch.ones((c,), device="cuda")
        gy = torch.randn((rows, c), device="cuda", generator=gen)
        leaves = [x, gamma, beta]

        def fused():
            return T.batch_norm_train(x, gamma, beta, mm, mv, 0.9, activation="relu")

        def functional():
            return torch.relu(torch.nn.functional.batch_norm(x, mm, mv, gamma, beta, training=True, momentum=0.1, eps=T.BN_EPS))

        def torch_route():
            return T.batch_norm_train_torch(x, gamma, beta, mm, mv, 0.9, activation="relu")

        step = lambda route: torch.autograd.grad(route(), leaves, gy)
        rec = {"rows": rows, "c": c}
        for name, route in (("fused", fused), ("functional", functional), ("torch_route", torch_route)):
            rec[name + "_step_us"] = timed(lambda: step(route), args.warmup, args.repeats)
        rec["functional_over_fused"] = rec["functional_step_us"] / rec["fused_step_us"]
        rec["torch_route_over_fused"] = rec["torch_route_step_us"] / rec["fused_step_us"]
        fg, cg = step(fused), step(functional)
        rec["grad_rel_diff"] = max(float((a - b_).abs().max() / b_.abs().max()) for a, b_ in zip(fg, cg))
        # both against the same formula in float64 on the device: which route a difference belongs to
        l64 = [t.detach().double().requires_grad_() for t in leaves]
        xh = (l64[0] - l64[0].mean(dim=0)) / torch.sqrt(l64[0].var(dim=0, unbiased=False) + T.BN_EPS)
        g64 = torch.autograd.grad(torch.relu(xh * l64[1] + l64[2]), l64, gy.double())
        rel = lambda got: max(float((a.double() - r).abs().max() / r.abs().max()) for a, r in zip(got, g64))
        rec["fused_err64"], rec["functional_err64"] = rel(fg), rel(cg)
        del l64, xh, g64

        # the two entries alone, through the C ABI
        with torch.no_grad():
            y, mean, rstd = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
            gx, gg, gb = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        nbytes = int(lib.pasnl_cls_bn_train_workspace_bytes(rows, c))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
        fwd = lambda: _hip.launch("pasnl_cls_bn_train", "bn_train", rows, c, P(x), P(gamma), P(beta), T.BN_EPS, 0.9, 1, 1, P(mm), P(mv),
                                  P(y), P(mean), P(rstd), P(ws), nbytes)
        bwd = lambda: _hip.launch("pasnl_cls_bn_train_grad", "bn_train_grad", rows, c, P(x), P(y), P(gamma), P(mean), P(rstd), 1, P(gy),
                                  P(gx), P(gg), P(gb), P(ws), nbytes)
        rec["fwd_us"], rec["bwd_us"] = timed(fwd, args.warmup, args.repeats), timed(bwd, args.warmup, args.repeats)
        matrix = rows * c * 4
        rec["fwd_gbps"], rec["bwd_gbps"] = 3 * matrix / rec["fwd_us"] * 1e-3, 7 * matrix / rec["bwd_us"] * 1e-3
        rec["fwd_hbm_peak_share"], rec["bwd_hbm_peak_share"] = rec["fwd_gbps"] * 1e9 / HBM_PEAK, rec["bwd_gbps"] * 1e9 / HBM_PEAK
        rec["workspace_bytes"] = nbytes
        print(json.dumps(rounded(rec)), flush=True)
        del x, gy, y, gx, fg, cg, leaves
        torch.cuda.empty_cache()

    if args.cls:
        from pointasnl_amd.models import pointasnl_cls

        st = T.set_store(T.VariableStore(seed=1))
        gen = torch.Generator(device="cuda").manual_seed(5)
        pc = torch.rand((16, 1024, 3), device="cuda", generator=gen) * 2 - 1
        label = torch.arange(16, device="cuda") % 40
        with torch.no_grad():
            pointasnl_cls.get_model(pc, is_training=True)
        params = list(st.trainable().values())

        def train_step():
            logits, _ = pointasnl_cls.get_model(pc, is_training=True, bn_decay=0.9)
            torch.autograd.grad(torch.nn.functional.cross_entropy(logits, label), params, allow_unused=True)

        rec = {"cls_step": [16, 1024]}
        for name, flag in (("fused", True), ("torch_route", False)):
            T.BN_TRAIN_FUSED = flag
            try:
                rec[name + "_step_us"] = timed(train_step, args.warmup, args.repeats)
            finally:
                T.BN_TRAIN_FUSED = True
        rec["torch_route_over_fused"] = rec["torch_route_step_us"] / rec["fused_step_us"]
        print(json.dumps(rounded(rec)), flush=True)


if __name__ == "__main__":
    main()
