"""Forward + backward of the differentiable AdaptiveSampling cell (as_gather -> one GEMM to [K | V | Q] -> as_attention_qkv ->
mlp2 -> as_reweight_x; the backward kernels of csrc/as_grad.hip) against torch autograd of the op-by-op chain (gathers, bmm,
softmax, bmm, mlp2, softmax(dim=2), sums) on the same device, at the four AS layers (b, n, m, k, as, c):
cls layer 1 (64, 1024, 512, 32, 12, 3) and 2 (64, 512, 128, 32, 12, 128), sem_seg 16 x 8192 layer 1 (16, 8192, 1024, 32, 8, 3)
and 2 (16, 1024, 256, 32, 4, 64) -- (g, as, c, cb) = (64*512, 12, 3, 32), (64*128, 12, 128, 65), (16*1024, 8, 3, 32),
(16*256, 4, 64, 33).

Per shape, HIP events around each call, --warmup calls first, the median of --repeats (>= 20) calls, in microseconds:
  fused_step_us / chain_step_us     one forward + backward to xyz, feature and the eight weight tensors
  fused_peak_mib / chain_peak_mib   torch.cuda.max_memory_allocated over one such step above what the inputs occupy
  attention_us / attention_grad_us  pasnl_as_attention_qkv and pasnl_cls_as_attention_qkv_grad through the C ABI
  reweight_us / reweight_grad_us    pasnl_as_reweight_x and pasnl_cls_as_reweight_x_grad
  gather_us / gather_grad_us        pasnl_as_gather and pasnl_cls_as_gather_grad
plus the largest |difference| of the two routes' gradients relative to their scale.  One JSON line per shape.

  python tools/as_grad_bench.py [--warmup 3] [--repeats 21] [--shapes b,n,m,k,as,c ...]
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

SHAPES = [(64, 1024, 512, 32, 12, 3), (64, 512, 128, 32, 12, 128), (16, 8192, 1024, 32, 8, 3), (16, 1024, 256, 32, 4, 64)]


def timed(fn, warmup, repeats):
    """median time of fn() in microseconds by HIP events"""
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
    return float(np.median(times))


def peak_mib(step):
    """max_memory_allocated over step() above what is allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--shapes", nargs="*", default=None, help="b,n,m,k,as,c ...")
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats must be at least 20")
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in s.split(",")) for s in args.shapes]

    from pointasnl_amd import _hip
    from pointasnl_amd.utils import pointasnl_util as U

    _hip.require_device()
    torch.cuda.set_device(0)
    lib = _hip.lib()
    for b, n, m, k, as_, c in shapes:
        ch = 3 + c
        cb = max(32, ch // 2)
        g = b * m
        gen = torch.Generator(device="cuda").manual_seed(b * 1000003 + n * 1009 + m * 31 + c)
        rnd = lambda *s, scale=1.0: (torch.randn(s, device="cuda", generator=gen) * scale)
        xyz, feature = rnd(b, n, 3).requires_grad_(), rnd(b, n, c).requires_grad_()
        idx = torch.randint(0, n, (b, m, k), device="cuda", generator=gen, dtype=torch.int32)
        w = [rnd(6 + c, 3 * cb, scale=(6 + c) ** -0.5), rnd(3 * cb, scale=0.1), rnd(cb, 32, scale=cb ** -0.5), rnd(32, scale=0.1),
             rnd(32, 1 + ch, scale=32 ** -0.5), rnd(1 + ch, scale=0.1)]
        for t in w:
            t.requires_grad_()
        leaves = [xyz, feature] + w
        gxyz, gfeat = rnd(b, m, 3), rnd(b, m, ch)

        def fused():
            x = U.as_gather(xyz, feature, idx, as_)
            kvq = torch.addmm(w[1], x.reshape(-1, 6 + c), w[0]).reshape(b, m, as_, 3 * cb)
            att = U.as_attention_qkv(kvq, cb)
            logits = torch.addmm(w[5], torch.relu(torch.addmm(w[3], att.reshape(-1, cb), w[2])), w[4]).reshape(b, m, as_, 1 + ch)
            return U.as_reweight_x(logits, x)

        take = idx[:, :, :as_].reshape(b, m * as_).long()

        def chain():
            rows = lambda t: torch.gather(t, 1, take[:, :, None].expand(-1, -1, t.shape[-1])).reshape(b, m, as_, t.shape[-1])
            p, f = rows(xyz), rows(feature)
            x = torch.cat([p - p[:, :, :1], p, f], dim=-1)
            kvq = torch.addmm(w[1], x.reshape(-1, 6 + c), w[0]).reshape(g, as_, 3 * cb)
            att = torch.softmax(torch.bmm(kvq[..., 2 * cb:], kvq[..., :cb].transpose(1, 2)) / (float(cb) ** 0.5), dim=-1)
            att = torch.bmm(att, kvq[..., cb:2 * cb])
            logits = torch.addmm(w[5], torch.relu(torch.addmm(w[3], att.reshape(-1, cb), w[2])), w[4]).reshape(b, m, as_, 1 + ch)
            wts = torch.softmax(logits, dim=2)
            return (wts[..., :1] * x[..., 3:6]).sum(dim=2), (wts[..., 1:] * x[..., 3:]).sum(dim=2)

        step = lambda route: torch.autograd.grad(route(), leaves, (gxyz, gfeat))
        rec = {"shape": [b, n, m, k, as_, c], "g_as_c_cb": [g, as_, c, cb]}
        rec["fused_step_us"] = timed(lambda: step(fused), args.warmup, args.repeats)
        rec["chain_step_us"] = timed(lambda: step(chain), args.warmup, args.repeats)
        rec["chain_over_fused"] = rec["chain_step_us"] / rec["fused_step_us"]
        fg, cg = step(fused), step(chain)
        # (without the last bias: the softmax over the neighbours ignores it, its gradient is rounding noise around zero)
        rec["grad_rel_diff"] = max(float((a - b_).abs().max() / b_.abs().max()) for a, b_ in list(zip(fg, cg))[:-1])
        del fg, cg
        torch.cuda.empty_cache()
        rec["fused_peak_mib"] = peak_mib(lambda: step(fused))
        rec["chain_peak_mib"] = peak_mib(lambda: step(chain))

        # each new kernel next to its forward, through the C ABI into preallocated buffers
        with torch.no_grad():
            x = U.as_gather(xyz, feature, idx, as_)
            kvq = torch.addmm(w[1], x.reshape(-1, 6 + c), w[0])
            att = U.as_attention_qkv(kvq.reshape(b, m, as_, 3 * cb), cb)
            logits = torch.addmm(w[5], torch.relu(torch.addmm(w[3], att.reshape(-1, cb), w[2])), w[4])
        gatt, gkvq, glogits, gx = torch.randn_like(att), torch.empty_like(kvq), torch.empty_like(logits), torch.randn_like(x)
        nxyz, nfeat = torch.empty_like(gxyz), torch.empty_like(gfeat)
        dxyz, dfeat = torch.empty_like(xyz), torch.empty_like(feature)
        nbytes = int(lib.pasnl_cls_as_gather_grad_workspace_bytes(b, n, c, m, as_))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        P = _hip.ptr
        pairs = {
            "attention": lambda: _hip.launch("pasnl_as_attention_qkv", "as_attention", g, as_, cb, P(kvq), P(att)),
            "attention_grad": lambda: _hip.launch("pasnl_cls_as_attention_qkv_grad", "as_attention_grad", g, as_, cb, P(kvq), P(gatt), P(gkvq)),
            "reweight": lambda: _hip.launch("pasnl_as_reweight_x", "as_reweight", g, as_, ch, P(logits), P(x), P(nxyz), P(nfeat)),
            "reweight_grad": lambda: _hip.launch("pasnl_cls_as_reweight_x_grad", "as_reweight_grad", g, as_, ch, P(logits), P(x), P(gxyz),
                                                 P(gfeat), P(glogits), P(gx)),
            "gather": lambda: _hip.launch("pasnl_as_gather", "as_gather", b, n, c, m, k, as_, P(xyz), P(feature), P(idx), P(x)),
            "gather_grad": lambda: _hip.launch("pasnl_cls_as_gather_grad", "as_gather_grad", b, n, c, m, k, as_, P(gx), P(idx), P(dxyz),
                                               P(dfeat), P(ws), ctypes.c_size_t(nbytes)),
        }
        for name in ("gather", "attention", "reweight", "gather_grad", "attention_grad", "reweight_grad"):
            rec[name + "_us"] = timed(pairs[name], args.warmup, args.repeats)
        rec["gather_grad_workspace_bytes"] = nbytes
        print(json.dumps({k_: (round(v, 3) if isinstance(v, float) and v > 1e-3 else v) for k_, v in rec.items()}), flush=True)
        del xyz, feature, idx, w, leaves, x, kvq, att, logits, gatt, gkvq, glogits, gx, ws, dxyz, dfeat, take
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
