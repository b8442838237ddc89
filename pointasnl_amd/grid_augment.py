"""`tf_augment_input` and the colour drop of the grid pipelines as one kernel -- reference ScanNet/scannet_dataset_grid.py
(D) :551-645 and SemanticKITTI/semantic_kitti_dataset_grid.py (K) :294-354 -- csrc/grid_train.hip `pasnl_scan_augment`.

TF's generator cannot be reproduced; the random numbers here are Philox4x32-10 words, addressed and never stored, so a
caller can restate any crop's draws (tests/philox_ref.py does):

  key      (seed & 0xffffffff, seed >> 32)
  counter  (j, item & 0xffffffff, item >> 32, stream)        item = item0 + c for crop c of the call
  uniform  u = (w >> 8) * 2^-24, exact in float32, in [0, 1)

  stream 0, per crop    j = 0: u_theta, u_sx, u_sy, u_sz      j = 1: u_symx, u_symy, u_symz, u_colour
      theta = u_theta * f32(2 pi); cos, sin: float32 of the float64 cosine and sine of theta
      s_i   = scale_min + u_si * (scale_max - scale_min), every operation rounded to float32 (u_sx serves the three axes
              unless anisotropic), times (u_symi > 0.5 ? 1 : -1) where the axis' symmetry is on
      keep  = u_colour < color
  stream 1, per point   j = the point's index in its crop: Box-Muller in float32, (x, y) normals from words (0, 1), the z
      normal from words (2, 3) (its second value is dropped): r = sqrt(-2 log(((wa >> 8) + 1) * 2^-24)),
      (r cos, r sin) of 2 pi * (wb >> 8) * 2^-24

  x' = (x*c) + (y*s),  y' = (y*c) - (x*s),  z' = z        the row vector times [[c,-s,0],[s,c,0],[0,0,1]]; 'none': x, y, z
  out_i = x'_i * s_i + f32(noise * normal_i)              float32, no contraction
  columns 3..5 are multiplied by keep when the rows hold at least 6; further columns are carried over

Deviations: the generator is Philox, not TF's; the summation order of TF's matmul is not promised (the sums above are the
kernel's); `augment_rotation` other than 'vertical' and 'none' raises as the reference does.
"""
import ctypes

import torch

from pointasnl_amd import _hip

_p = _hip.ptr

# what both get_batch_gen's write into their config (D:443-451, K:84-89, 197): the training split
TRAINING = dict(augment_rotation="vertical", augment_scale_min=0.9, augment_scale_max=1.1, augment_scale_anisotropic=True,
                augment_symmetries=(True, False, False), augment_noise=0.001, augment_color=1.0)
FIELDS = tuple(TRAINING)


def config_of(config=None, **overrides):
    """-> a dict of the seven augment_* fields from a dict or an object with those attributes (missing ones: the training
    split's values), then `overrides`"""
    out = dict(TRAINING)
    if config is not None:
        for f in FIELDS:
            if isinstance(config, dict):
                if f in config:
                    out[f] = config[f]
            elif hasattr(config, f):
                out[f] = getattr(config, f)
    out.update(overrides)
    if out["augment_rotation"] not in ("vertical", "none"):
        raise ValueError("Unknown rotation augmentation : " + str(out["augment_rotation"]))  # D:614
    sym = tuple(bool(v) for v in out["augment_symmetries"])
    if len(sym) != 3:
        raise ValueError("augment_symmetries holds one flag per axis")
    out["augment_symmetries"] = sym
    return out


def launch(b, num_point, width, src, dst, cfg, seed, item0, out_params=None, out_noise=None, what="augment_input"):
    """pasnl_scan_augment on device tensors; item0: a (1,) int64 device tensor (read as unsigned)"""
    _hip.launch("pasnl_scan_augment", what, int(b), int(num_point), int(width), _p(src), _p(dst),
                1 if cfg["augment_rotation"] == "vertical" else 0, ctypes.c_float(cfg["augment_scale_min"]),
                ctypes.c_float(cfg["augment_scale_max"]), 1 if cfg["augment_scale_anisotropic"] else 0,
                *(1 if v else 0 for v in cfg["augment_symmetries"]), ctypes.c_float(cfg["augment_noise"]),
                ctypes.c_float(cfg["augment_color"]), ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), _p(item0),
                _p(out_params), _p(out_noise))


def item_tensor(item0, device):
    """the running crop number as the (1,) int64 device tensor the kernel reads (its 64 bits, unsigned)"""
    v = int(item0) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v], dtype=torch.int64, device=device)


def augment_input(points, config=None, seed=0, item0=0, return_params=False, out=None):
    """tf_augment_input (and the colour drop, where the rows hold colours) of B crops: points (B,N,W) float32 on the device,
    W >= 3; config: a dict or an object with the reference's augment_* fields (default: the training split's); crop c draws
    under (seed, item0 + c) as the module docstring lays out; item0: an int, or a (1,) int64 device tensor (so a captured
    call replays with the number staged into it).  out: the destination (`points` itself: in place).
    -> the augmented (B,N,W) tensor; with return_params also params (B,8) f32 = theta, cos, sin, s0, s1, s2, keep, 0 (the
    reference returns its scales and rotations, D:645) and the unit normals (B,N,3) f32."""
    pts = _hip.as_dev(points, torch.float32)
    if pts.dim() != 3 or pts.shape[2] < 3 or pts.shape[1] < 1:
        raise ValueError("points must be (B, N, W) with N >= 1 and W >= 3")
    B, N, W = (int(v) for v in pts.shape)
    cfg = config_of(config)
    if out is None:
        out = torch.empty_like(pts)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, N, W) or not out.is_contiguous() or out.device != pts.device:
        raise ValueError("out must be a contiguous float32 tensor of the shape and device of points")
    item = item0 if isinstance(item0, torch.Tensor) else item_tensor(item0, pts.device)
    if item.dtype != torch.int64 or item.numel() != 1 or item.device != pts.device:
        raise ValueError("item0: an int or a (1,) int64 tensor on the device of points")
    params = torch.empty((B, 8), dtype=torch.float32, device=pts.device) if return_params else None
    noise = torch.empty((B, N, 3), dtype=torch.float32, device=pts.device) if return_params else None
    if B > 0:
        launch(B, N, W, pts, out, cfg, seed, item, params, noise)
    return (out, params, noise) if return_params else out


def host_config(cfg):
    """the field names tests/philox_ref.py uses, for restating a call on the host"""
    return dict(rotation=cfg["augment_rotation"], scale_min=cfg["augment_scale_min"], scale_max=cfg["augment_scale_max"],
                anisotropic=cfg["augment_scale_anisotropic"], symmetries=cfg["augment_symmetries"], noise=cfg["augment_noise"],
                color=cfg["augment_color"])


__all__ = ["augment_input", "config_of", "TRAINING", "host_config", "item_tensor", "launch"]
