"""Pure numpy Philox4x32-10 (Salmon et al., SC'11) and the draw layout of pasnl_scan_augment (include/pasnl.h,
pointasnl_amd/grid_augment.py): the host restatement of every random number the augmentation kernel uses, and of its float32
arithmetic.  Key (seed lo, seed hi); counter (j, item lo, item hi, stream); stream 0 holds a crop's draws (j = 0: u_theta,
u_sx, u_sy, u_sz; j = 1: u_symx, u_symy, u_symz, u_colour), stream 1 the noise words of point j."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI_F32 = np.float32(2 * np.pi)

DEFAULT = dict(rotation="vertical", scale_min=0.9, scale_max=1.1, anisotropic=True, symmetries=(True, False, False), noise=0.001,
               color=1.0)  # D:443-451, K:84-89, 197


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32 words, key: (2,) uint32 words -> (..., 4) uint32"""
    c = [np.asarray(counter, np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def words(seed, item, j, stream):
    """the four words at counter (j, item lo, item hi, stream) under `seed`; j may be an array"""
    j = np.asarray(j, np.uint32)
    item = int(item) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty(j.shape + (4,), np.uint32)
    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = j, item & 0xFFFFFFFF, item >> 32, stream
    return philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))


def uniform(w):
    """(w >> 8) * 2^-24: exact in float32, in [0, 1)"""
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def symmetry(u):
    """(u > 0.5 ? 1 : -1): tf.round(u) * 2 - 1 under round-half-to-even"""
    return np.where(np.asarray(u, np.float32) > np.float32(0.5), np.float32(1), np.float32(-1)).astype(np.float32)


def crop_params(seed, item, cfg=DEFAULT):
    """-> dict(theta f32, scales (3,) f32 with the symmetry's sign, keep f32 0|1) of crop number `item`"""
    a, s = uniform(words(seed, item, 0, 0)), uniform(words(seed, item, 1, 0))
    theta = np.float32(a[0] * TWO_PI_F32) if cfg["rotation"] == "vertical" else np.float32(0)
    lo, hi = np.float32(cfg["scale_min"]), np.float32(cfg["scale_max"])
    span = np.float32(hi - lo)
    u = a[1:4] if cfg["anisotropic"] else a[[1, 1, 1]]
    scales = (lo + (u * span).astype(np.float32)).astype(np.float32)
    for i in range(3):
        if cfg["symmetries"][i]:
            scales[i] = scales[i] * symmetry(s[i])
    keep = np.float32(1 if s[3] < np.float32(cfg["color"]) else 0)
    return dict(theta=theta, scales=scales, keep=keep)


def noise_words(seed, item, num_point):
    return words(seed, item, np.arange(num_point), 1)


def box_muller64(wa, wb):
    """float64 Box-Muller of two words: radius from ((wa >> 8) + 1) * 2^-24 in (0, 1], angle 2 pi (wb >> 8) * 2^-24"""
    u1 = ((np.asarray(wa, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(wb, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)


def normals64(seed, item, num_point):
    """the (num_point, 3) unit normals of crop `item` in float64: (x, y) from words (0, 1), z from words (2, 3)"""
    w = noise_words(seed, item, num_point)
    x, y = box_muller64(w[:, 0], w[:, 1])
    z, _ = box_muller64(w[:, 2], w[:, 3])
    return np.stack([x, y, z], 1)


def apply(points, cos, sin, scales, keep, normals, cfg=DEFAULT):
    """the kernel's float32 formula on one crop (num_point, width) from the emitted cos, sin, signed scales, keep and the
    float32 unit normals: x' = (x*c) + (y*s), y' = (y*c) - (x*s); out = x' * s_i + f32(noise * normal_i); columns 3..5 times
    keep when width >= 6; further columns copied"""
    p = np.asarray(points, np.float32)
    out = p.copy()
    c, s, sc, nrm = np.float32(cos), np.float32(sin), np.asarray(scales, np.float32), np.asarray(normals, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if cfg["rotation"] == "vertical":
        rx = ((x * c).astype(np.float32) + (y * s).astype(np.float32)).astype(np.float32)
        ry = ((y * c).astype(np.float32) - (x * s).astype(np.float32)).astype(np.float32)
    else:
        rx, ry = x, y
    sd = np.float32(cfg["noise"])
    for i, v in enumerate((rx, ry, z)):
        out[:, i] = ((v * sc[i]).astype(np.float32) + (sd * nrm[:, i]).astype(np.float32)).astype(np.float32)
    if p.shape[1] >= 6:
        out[:, 3:6] = (p[:, 3:6] * np.float32(keep)).astype(np.float32)
    return out


def augment(points, seed, item0, cfg=DEFAULT):
    """the whole augmentation of (b, num_point, width) crops on the host, normals in float64 rounded to float32: what the
    kernel computes up to its float32 Box-Muller and its cosine and sine (the host chain of tools/grid_train_bench.py)"""
    p = np.asarray(points, np.float32)
    out = np.empty_like(p)
    for c in range(p.shape[0]):
        q = crop_params(seed, item0 + c, cfg)
        th = np.float64(q["theta"])
        out[c] = apply(p[c], np.float32(np.cos(th)), np.float32(np.sin(th)), q["scales"], q["keep"],
                       normals64(seed, item0 + c, p.shape[1]).astype(np.float32), cfg)
    return out
