"""Forward + backward of the differentiable set-abstraction grouping and local cell (sa_group -> sa_local_cell_w; the backward
kernels of csrc/sa_grad.hip) against torch autograd of the op-by-op chain (gathers, cat, amax, matmul, relu, matmul, relu, the
weight net, transpose, batched matmul) on the same device, at three layers (b, n, p, k, c, c1):
cls layer 1 (64, 1024, 512, 32, 3, 64), sem_seg 16 x 8192 layer 1 (16, 8192, 1024, 32, 3, 32) and layer 2's width at 64 feature
channels (16, 1024, 256, 32, 64, 64) -- (b*p, k, c, c1) = (64*512, 32, 3, 64), (16*1024, 32, 3, 32), (16*256, 32, 64, 64).

Per shape, the median of three runs; a run is the median of --repeats calls between HIP events after --warmup calls (time, in
microseconds), or one step under torch.cuda.max_memory_allocated (peak, in MiB above what the inputs occupy):
  fused_step_us / chain_step_us     one forward + backward to xyz, feature, new_xyz and the six weight tensors
  fused_peak_mib / chain_peak_mib   the peak of one such step
  cell_us / cell_grad_us            pasnl_sa_local_cell and pasnl_cls_sa_local_cell_grad (all seven gradients) through the C ABI
  group_us / group_grad_us          pasnl_sa_group and pasnl_cls_sa_group_grad
plus the largest |difference| of the two routes' gradients relative to their scale (grad_rel_diff) and of each route against the
same chain in float64 on the device (fused_err64 / chain_err64 over all nine gradients, *_x over xyz, feature and new_xyz).  One
JSON line per shape.

  python tools/sa_cell_grad_bench.py [--warmup 3] [--repeats 11] [--shapes b,n,p,k,c,c1 ...]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 1024, 512, 32, 3, 64), (16, 8192, 1024, 32, 3, 32), (16, 1024, 256, 32, 64, 64)]
RUNS = 3


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


def peak_mib(step):
    """median over RUNS runs of max_memory_allocated over step() above what is allocated before it"""
    runs = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        runs.append((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20)
    return float(np.median(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--shapes", nargs="*", default=None, help="b,n,p,k,c,c1 ...")
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in s.split(",")) for s in args.shapes]

    from pointasnl_amd import _hip
    from pointasnl_amd.utils import pointasnl_util as U

    _hip.require_device()
    torch.cuda.set_device(0)
    lib = _hip.lib()
    for b, n, p, k, c, c1 in shapes:
        w = 6 + c
        g = b * p
        gen = torch.Generator(device="cuda").manual_seed(b * 1000003 + n * 1009 + p * 31 + c)
        rnd = lambda *s, scale=1.0: (torch.randn(s, device="cuda", generator=gen) * scale)
        xyz, feature, new_xyz = rnd(b, n, 3).requires_grad_(), rnd(b, n, c).requires_grad_(), rnd(b, p, 3).requires_grad_()
        idx = torch.randint(0, n, (b, p, k), device="cuda", generator=gen, dtype=torch.int32)
        wts = [rnd(w, c1, scale=w ** -0.5), rnd(c1, scale=0.3), rnd(c1, c1, scale=c1 ** -0.5), rnd(c1, scale=0.3),
               rnd(3, 32, scale=3 ** -0.5), rnd(32, scale=0.3)]
        for t in wts:
            t.requires_grad_()
        leaves = [xyz, feature, new_xyz] + wts
        g_out, g_skip = rnd(b, p, c1, 32), rnd(b, p, w)

        def fused():
            new_point, skip = U.sa_group(xyz, feature, idx, new_xyz)
            return U.sa_local_cell_w(new_point, *wts), skip

        take = idx.reshape(b, p * k).long()

        def chain():
            rows = lambda t: torch.gather(t, 1, take[:, :, None].expand(-1, -1, t.shape[-1])).reshape(b, p, k, t.shape[-1])
            gx = rows(xyz)
            new_point = torch.cat([gx - new_xyz[:, :, None, :], gx, rows(feature)], dim=-1)
            h2 = torch.relu(torch.relu(new_point @ wts[0] + wts[1]) @ wts[2] + wts[3])
            weight = torch.relu(new_point[..., 0:3] @ wts[4] + wts[5])
            return h2.transpose(2, 3) @ weight, new_point.amax(dim=2)

        step = lambda route: torch.autograd.grad(route(), leaves, (g_out, g_skip))
        rec = {"shape": [b, n, p, k, c, c1], "g_k_c_c1": [g, k, c, c1]}
        rec["fused_step_us"] = timed(lambda: step(fused), args.warmup, args.repeats)
        rec["chain_step_us"] = timed(lambda: step(chain), args.warmup, args.repeats)
        rec["chain_over_fused"] = rec["chain_step_us"] / rec["fused_step_us"]
        fg, cg = step(fused), step(chain)
        rec["grad_rel_diff"] = max(float((a - b_).abs().max() / b_.abs().max()) for a, b_ in zip(fg, cg))
        # both routes against the same chain in float64 on the device (float32 rounding flips ReLUs whose argument is nearly zero,
        # each flip a finite step in one row's gradient: the float64 chain says which route is nearer)
        leaves32, (o32, s32) = leaves, (g_out, g_skip)
        leaves = [t.detach().double().requires_grad_() for t in leaves32]
        xyz, feature, new_xyz, wts = leaves[0], leaves[1], leaves[2], leaves[3:]
        g64 = torch.autograd.grad(chain(), leaves, (o32.double(), s32.double()))
        leaves = leaves32
        xyz, feature, new_xyz, wts = leaves[0], leaves[1], leaves[2], leaves[3:]
        rel = lambda got: [float((a.double() - r).abs().max() / r.abs().max()) for a, r in zip(got, g64)]
        rec["fused_err64"], rec["chain_err64"] = max(rel(fg)), max(rel(cg))
        rec["fused_err64_x"], rec["chain_err64_x"] = max(rel(fg)[:3]), max(rel(cg)[:3])
        del fg, cg, g64
        rec["fused_peak_mib"] = peak_mib(lambda: step(fused))
        rec["chain_peak_mib"] = peak_mib(lambda: step(chain))

        # each new entry point next to its forward, through the C ABI into preallocated buffers
        with torch.no_grad():
            new_point, skip = U.sa_group(xyz, feature, idx, new_xyz)
            out = U.sa_local_cell_w(new_point, *wts)
        g_np = torch.randn_like(new_point)
        d_x = torch.empty_like(new_point)
        d_w = [torch.empty_like(t) for t in wts]
        d_xyz, d_feat, d_new = torch.empty_like(xyz), torch.empty_like(feature), torch.empty_like(new_xyz)
        cell_bytes = int(lib.pasnl_cls_sa_local_cell_grad_workspace_bytes(g, w, c1, c1))
        group_bytes = int(lib.pasnl_cls_sa_group_grad_workspace_bytes(b, n, c, p, k))
        ws = torch.empty((max(cell_bytes, group_bytes),), dtype=torch.uint8, device="cuda")
        P = _hip.ptr
        wp = [P(t) for t in wts]
        pairs = {
            "group": lambda: _hip.launch("pasnl_sa_group", "sa_group", b, n, c, p, k, P(xyz), P(feature), P(idx), P(new_xyz),
                                         P(new_point), P(skip)),
            "cell": lambda: _hip.launch("pasnl_sa_local_cell", "sa_local_cell", g, k, w, c1, c1, P(new_point), *wp, P(out)),
            "cell_grad": lambda: _hip.launch("pasnl_cls_sa_local_cell_grad", "sa_local_cell_grad", g, k, w, c1, c1, P(new_point), *wp,
                                             P(g_out), P(d_x), *[P(t) for t in d_w], P(ws), ctypes.c_size_t(cell_bytes)),
            "group_grad": lambda: _hip.launch("pasnl_cls_sa_group_grad", "sa_group_grad", b, n, c, p, k, P(xyz), P(feature), P(idx),
                                              P(new_xyz), P(g_np), P(g_skip), P(d_xyz), P(d_feat), P(d_new), P(ws),
                                              ctypes.c_size_t(group_bytes)),
        }
        for name in ("group", "cell", "cell_grad", "group_grad"):
            rec[name + "_us"] = timed(pairs[name], args.warmup, args.repeats)
        rec["cell_grad_workspace_bytes"], rec["group_grad_workspace_bytes"] = cell_bytes, group_bytes
        print(json.dumps({k_: (round(v, 3) if isinstance(v, float) and v > 1e-3 else v) for k_, v in rec.items()}), flush=True)
        del xyz, feature, new_xyz, idx, wts, leaves, new_point, skip, out, g_np, d_x, d_w, d_xyz, d_feat, d_new, ws, take
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
