"""The fused backward of the input-space non-local cell (pasnl_cls_nl_cell_input_grad) against the two other ways to the same
six gradients on the same device, at the three models' first levels -- classifier (64, 512, 1024, 3, 3, 32), ScanNet
(16, 1024, 8192, 3, 3, 32), SemanticKITTI (8, 1280, 10240, 3, 3, 32) -- and a generic-width shape (8, 256, 2048, 8, 8, 128).

Per shape (b, p, n, c, cz, cb), HIP events around each call, --warmup calls first, the median of --repeats (>= 20) calls, in
microseconds:
  forward_us            U.nl_cell_input without gradients (the forward kernel)
  fused_backward_us     pasnl_cls_nl_cell_input_grad through the C ABI into preallocated buffers, all six gradients
  fused_weights_us      the same with grad_feature = grad_new_point = NULL (training on coordinates: no key-major launch)
  fused_autograd_us     torch.autograd.grad through nl_cell_input (the same launches + torch's allocations)
  projected_autograd_us torch.autograd.grad through torch matmul projections into U.nl_attention with its fused backward
                        (csrc/nl_grad.hip): [K | V] (b,n,2cb) and Q (b,p,cb) exist, the (b,p,n) map does not
  chain_autograd_us     torch.autograd.grad through the op-by-op chain: projections, matmul, / sqrt(cb), softmax, matmul
and torch.cuda.max_memory_allocated over one forward + backward above what the inputs occupy for the three routes
(*_peak_mib), plus the largest |difference| of the fused gradients from the chain's relative to their scale.  One JSON line per
shape.

  python tools/nl_cell_input_grad_bench.py [--warmup 3] [--repeats 21] [--shapes b,p,n,c,cz,cb ...]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from nl_grad_bench import peak_mib, timed  # noqa: E402

SHAPES = [(64, 512, 1024, 3, 3, 32), (16, 1024, 8192, 3, 3, 32), (8, 1280, 10240, 3, 3, 32), (8, 256, 2048, 8, 8, 128)]
NAMES = ("feature", "new_point", "wkv", "bkv", "wq", "bq")


def projections(t):
    return torch.matmul(t["feature"], t["wkv"]) + t["bkv"], torch.matmul(t["new_point"], t["wq"]) + t["bq"]


def chain(t):
    kv, q = projections(t)
    cb = q.shape[-1]
    att = torch.matmul(q, kv[..., :cb].transpose(1, 2))
    att = torch.softmax(att / (float(cb) ** 0.5), dim=-1)
    return torch.matmul(att, kv[..., cb:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--shapes", nargs="*", default=None, help="b,p,n,c,cz,cb ...")
    args = ap.parse_args()
    if args.repeats < 20:
        ap.error("--repeats must be at least 20")
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in s.split(",")) for s in args.shapes]

    from pointasnl_amd import _hip
    from pointasnl_amd.utils import pointasnl_util as U

    _hip.require_device()
    torch.cuda.set_device(0)
    lib = _hip.lib()
    for b, p, n, c, cz, cb in shapes:
        gen = torch.Generator(device="cuda").manual_seed(b * 1000003 + p * 1009 + n * 31 + c * 7 + cb)
        rand = lambda *sh: torch.randn(sh, device="cuda", generator=gen)
        # inputs and biases standard normal, weights / sqrt(fan-in): scores of a few units (tests/nl_cell_input_ref.py)
        t = dict(feature=rand(b, n, c), new_point=rand(b, p, cz), wkv=rand(c, 2 * cb) / c ** 0.5, bkv=rand(2 * cb),
                 wq=rand(cz, cb) / cz ** 0.5, bq=rand(cb))
        for v in t.values():
            v.requires_grad_()
        ins = tuple(t[k] for k in NAMES)
        g = rand(b, p, cb)

        def forward():
            with torch.no_grad():
                return U.nl_cell_input(*ins)

        def projected():
            kv, q = projections(t)
            return U.nl_attention(q, kv)

        nbytes = int(lib.pasnl_cls_nl_cell_input_grad_workspace_bytes(b, p, n, c, cz, cb))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        grads = [torch.empty_like(v) for v in ins]

        def fused_abi(outs):
            _hip.launch("pasnl_cls_nl_cell_input_grad", "nl_cell_input_grad", b, p, n, c, cz, cb, *(_hip.ptr(v) for v in ins),
                        _hip.ptr(g), *(_hip.ptr(o) for o in outs), _hip.ptr(ws), ctypes.c_size_t(nbytes))

        rec = {"shape": [b, p, n, c, cz, cb], "workspace_bytes": nbytes}
        rec["forward_us"] = timed(forward, args.warmup, args.repeats)
        rec["fused_backward_us"] = timed(lambda: fused_abi(grads), args.warmup, args.repeats)
        rec["fused_weights_us"] = timed(lambda: fused_abi([None, None] + grads[2:]), args.warmup, args.repeats)
        routes = (("fused", lambda: U.nl_cell_input(*ins)), ("projected", projected), ("chain", lambda: chain(t)))
        got = {}
        for name, route in routes:
            out = route()
            rec[f"{name}_autograd_us"] = timed(lambda: torch.autograd.grad(out, ins, g, retain_graph=True), args.warmup, args.repeats)
            if name != "projected":
                got[name] = torch.autograd.grad(out, ins, g)
            del out
        rec["backward_over_forward"] = rec["fused_backward_us"] / rec["forward_us"]
        rec["projected_over_fused"] = rec["projected_autograd_us"] / rec["fused_autograd_us"]
        rec["chain_over_fused"] = rec["chain_autograd_us"] / rec["fused_autograd_us"]
        for k, a, r in zip(NAMES, got["fused"], got["chain"]):
            rec[f"grad_{k}_rel_diff"] = float((a - r).abs().max() / r.abs().max())
        del got
        torch.cuda.empty_cache()
        for name, route in routes:
            rec[f"{name}_peak_mib"] = peak_mib(lambda: torch.autograd.grad(route(), ins, g))
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) and v > 1e-3 else v) for k, v in rec.items()}), flush=True)
        del t, ins, g, ws, grads
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
