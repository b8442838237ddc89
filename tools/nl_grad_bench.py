"""The fused backward of the non-local attention core (pasnl_cls_nl_attention_grad) against torch autograd's backward of the
op-by-op chain (matmul -> / sqrt(cb) -> softmax -> matmul) on the same device, at cls layer 1 (64, 512, 1024, 32), cls layer 2
(64, 128, 512, 64), ScanNet layer 1 (16, 1024, 8192, 32) and the cb = 128 form (8, 40, 80, 128).

Per shape, HIP events around each call, --warmup calls first, the median of --repeats (>= 20) calls, in microseconds:
  forward_us          U.nl_attention without gradients (the forward kernel)
  fused_backward_us   pasnl_cls_nl_attention_grad through the C ABI into preallocated buffers (both gradients)
  fused_autograd_us   torch.autograd.grad through _NLAttention (the same launches + torch's allocations of gradients and workspace)
  chain_autograd_us   torch.autograd.grad through the chain's graph (the (B,P,N) map and its softmax are saved tensors)
and torch.cuda.max_memory_allocated over one forward + backward above what the inputs occupy, for both (fused_peak_mib,
chain_peak_mib), plus the largest |difference| of the two sets of gradients relative to their scale.  One JSON line per shape.

  python tools/nl_grad_bench.py [--warmup 3] [--repeats 21] [--shapes b,p,n,cb ...]
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

SHAPES = [(64, 512, 1024, 32), (64, 128, 512, 64), (16, 1024, 8192, 32), (8, 40, 80, 128)]


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


def chain(q, kv):
    cb = q.shape[-1]
    att = torch.matmul(q, kv[..., :cb].transpose(1, 2))
    att = torch.softmax(att / (float(cb) ** 0.5), dim=-1)
    return torch.matmul(att, kv[..., cb:])


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
    ap.add_argument("--shapes", nargs="*", default=None, help="b,p,n,cb ...")
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats must be at least 20")
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in s.split(",")) for s in args.shapes]

    from pointasnl_amd import _hip
    from pointasnl_amd.utils import pointasnl_util as U

    _hip.require_device()
    torch.cuda.set_device(0)
    lib = _hip.lib()
    for b, p, n, cb in shapes:
        gen = torch.Generator(device="cuda").manual_seed(b * 1000003 + p * 1009 + n * 31 + cb)
        q = torch.randn((b, p, cb), device="cuda", generator=gen).requires_grad_()
        kv = torch.randn((b, n, 2 * cb), device="cuda", generator=gen).requires_grad_()
        g = torch.randn((b, p, cb), device="cuda", generator=gen)

        def forward():
            with torch.no_grad():
                return U.nl_attention(q, kv)

        out = forward()
        nbytes = int(lib.pasnl_cls_nl_attention_grad_workspace_bytes(b, p, n, cb))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        gq, gkv = torch.empty_like(q), torch.empty_like(kv)

        def fused_abi():
            _hip.launch("pasnl_cls_nl_attention_grad", "nl_attention_grad", b, p, n, cb, _hip.ptr(q), _hip.ptr(kv), _hip.ptr(out),
                        _hip.ptr(g), _hip.ptr(gq), _hip.ptr(gkv), _hip.ptr(ws), ctypes.c_size_t(nbytes))

        rec = {"shape": [b, p, n, cb], "workspace_bytes": nbytes}
        rec["forward_us"] = timed(forward, args.warmup, args.repeats)
        rec["fused_backward_us"] = timed(fused_abi, args.warmup, args.repeats)
        tracked = U.nl_attention(q, kv)
        rec["fused_autograd_us"] = timed(lambda: torch.autograd.grad(tracked, (q, kv), g, retain_graph=True), args.warmup, args.repeats)
        fq, fkv = torch.autograd.grad(tracked, (q, kv), g)
        del tracked
        chained = chain(q, kv)
        rec["chain_autograd_us"] = timed(lambda: torch.autograd.grad(chained, (q, kv), g, retain_graph=True), args.warmup, args.repeats)
        cq, ckv = torch.autograd.grad(chained, (q, kv), g)
        del chained
        rec["backward_over_forward"] = rec["fused_backward_us"] / rec["forward_us"]
        rec["chain_over_fused"] = rec["chain_autograd_us"] / rec["fused_autograd_us"]
        rec["grad_q_rel_diff"] = float((fq - cq).abs().max() / cq.abs().max())
        rec["grad_kv_rel_diff"] = float((fkv - ckv).abs().max() / ckv.abs().max())
        del fq, fkv, cq, ckv
        torch.cuda.empty_cache()
        rec["fused_peak_mib"] = peak_mib(lambda: torch.autograd.grad(U.nl_attention(q, kv), (q, kv), g))
        rec["chain_peak_mib"] = peak_mib(lambda: torch.autograd.grad(chain(q, kv), (q, kv), g))
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) and v > 1e-3 else v) for k, v in rec.items()}), flush=True)
        del q, kv, g, out, ws, gq, gkv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
