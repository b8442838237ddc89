"""GPU: pasnl_scan_augment (csrc/grid_train.hip) and `pointasnl_amd.grid_augment.augment_input` against the host restatement
tests/philox_ref.py.  The per-crop draws (theta, scales, keep) are compared by bits; cos and sin within one float32 ulp of
numpy's float64 values rounded; the output points by bits against the float32 formula evaluated in numpy from the emitted
cos, sin, scales and unit normals; the unit normals against float64 Box-Muller of the same Philox words under NOISE_TOL.
Every call writes into guarded views of exactly the sizes include/pasnl.h states, twice over different stale bytes."""
import ctypes

import numpy as np
import pytest
import torch

import philox_ref as P
from guarded import ALT_BYTE, NAN_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

B = 3
NUM_POINTS = (1, 63, 70, 257)   # a single point; ragged against the wave (64) and the workgroup (256)
WIDTHS = (3, 6, 9)
SEED = 0x0123456789ABCDEF

# Largest |out_noise - float64 Box-Muller| measured over every call of this file on one MI355X: 3.624e-7 (EXPERIMENTS.md,
# "Grid training input loops"); the bound is 4 x that.  The estimate was a few float32 ulps of a value of magnitude <= 5.8,
# about 2e-6; a measurement above 1e-5 would be a defect in the transform.
NOISE_MEASURED = 3.624e-7
NOISE_TOL = 4 * NOISE_MEASURED

CONFIGS = {
    "training": P.DEFAULT,
    "rotation_none": dict(P.DEFAULT, rotation="none"),
    "isotropic": dict(P.DEFAULT, anisotropic=False),
    "all_symmetries": dict(P.DEFAULT, symmetries=(True, True, True)),
    "color_half": dict(P.DEFAULT, color=0.5),
    "noise_zero": dict(P.DEFAULT, noise=0.0),
}
worst = {"noise": 0.0}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def product_config(cfg):
    return dict(augment_rotation=cfg["rotation"], augment_scale_min=cfg["scale_min"], augment_scale_max=cfg["scale_max"],
                augment_scale_anisotropic=cfg["anisotropic"], augment_symmetries=cfg["symmetries"], augment_noise=cfg["noise"],
                augment_color=cfg["color"])


def crops(num_point, width, seed=0):
    rng = np.random.default_rng(1000 * num_point + width + seed)
    pts = (rng.standard_normal((B, num_point, width)) * 3).astype(np.float32)
    pts[:, :, 3:] = rng.random((B, num_point, width - 3)).astype(np.float32)
    return pts


def run_guarded(pts, cfg, seed, item0, in_place, fill):
    """one call through the C ABI into guarded views -> (dst, params, noise) host arrays"""
    from pointasnl_amd import _hip, grid_augment

    b, n, w = pts.shape
    dst = Guarded(pts.nbytes, fill, output_guard(w * 4))
    par = Guarded(b * 8 * 4, fill, output_guard(32))
    noi = Guarded(b * n * 3 * 4, fill, output_guard(12))
    src_t = torch.from_numpy(pts).cuda()
    if in_place:
        dst.inside().copy_(src_t.reshape(-1).view(torch.uint8))
        src_ptr = dst.ptr
    else:
        src_ptr = src_t.data_ptr()
    item = grid_augment.item_tensor(item0, src_t.device)
    pc = product_config(cfg)
    f = ctypes.c_float
    _hip.launch("pasnl_scan_augment", "test", b, n, w, ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst.ptr),
                1 if pc["augment_rotation"] == "vertical" else 0, f(pc["augment_scale_min"]), f(pc["augment_scale_max"]),
                1 if pc["augment_scale_anisotropic"] else 0, *(int(v) for v in pc["augment_symmetries"]), f(pc["augment_noise"]),
                f(pc["augment_color"]), ctypes.c_ulonglong(seed), _hip.ptr(item), ctypes.c_void_p(par.ptr), ctypes.c_void_p(noi.ptr))
    torch.cuda.synchronize()
    assert dst.guards_intact() and par.guards_intact() and noi.guards_intact()
    if not in_place:
        np.testing.assert_array_equal(bits(src_t.cpu().numpy()), bits(pts))  # the source is read only
    return dst.floats((b, n, w)), par.floats((b, 8)), noi.floats((b, n, 3))


def ulp32(x):
    return np.spacing(np.abs(np.float32(x)))


def check(num_point, width, in_place, cfg, item0=5):
    pts = crops(num_point, width)
    out, par, noise = run_guarded(pts, cfg, SEED, item0, in_place, NAN_BYTE)
    out2, par2, noise2 = run_guarded(pts, cfg, SEED, item0, in_place, ALT_BYTE)
    for a, b in ((out, out2), (par, par2), (noise, noise2)):  # every element is written: nothing of the stale bytes is left
        np.testing.assert_array_equal(bits(a), bits(b))
    for c in range(B):
        q = P.crop_params(SEED, item0 + c, cfg)
        theta, cs, sn = par[c, 0], par[c, 1], par[c, 2]
        assert bits(theta) == bits(q["theta"])
        np.testing.assert_array_equal(bits(par[c, 3:6]), bits(q["scales"]))
        assert par[c, 6] == q["keep"] and par[c, 7] == 0
        if cfg["rotation"] == "vertical":
            for got, ref in ((cs, np.float32(np.cos(np.float64(theta)))), (sn, np.float32(np.sin(np.float64(theta))))):
                assert abs(np.float64(got) - np.float64(ref)) <= ulp32(ref)
        else:
            assert (theta, cs, sn) == (0, 1, 0)
        want64 = P.normals64(SEED, item0 + c, num_point)
        diff = float(np.abs(noise[c].astype(np.float64) - want64).max())
        worst["noise"] = max(worst["noise"], diff)
        assert diff <= NOISE_TOL, diff
        want = P.apply(pts[c], cs, sn, par[c, 3:6], par[c, 6], noise[c], cfg)
        np.testing.assert_array_equal(bits(out[c]), bits(want))
        if width >= 6:
            np.testing.assert_array_equal(bits(out[c][:, 3:6]), bits((pts[c][:, 3:6] * par[c, 6]).astype(np.float32)))
        np.testing.assert_array_equal(bits(out[c][:, (6 if width >= 6 else 3):]), bits(pts[c][:, (6 if width >= 6 else 3):]))
    return out, par, noise


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("num_point", NUM_POINTS)
def test_training_config(num_point, width, in_place):
    check(num_point, width, in_place, P.DEFAULT)


@pytest.mark.parametrize("name", [k for k in CONFIGS if k != "training"])
def test_every_switch(name):
    cfg = CONFIGS[name]
    seen_keep, seen_flip = set(), set()
    for num_point in NUM_POINTS:
        for width in WIDTHS:
            for in_place in (False, True):
                out, par, noise = check(num_point, width, in_place, cfg, item0=11 * num_point)
                seen_keep |= set(par[:, 6].tolist())
                seen_flip |= set(np.sign(par[:, 3:6]).reshape(-1).tolist())
                if name == "isotropic":
                    assert (np.abs(par[:, 3]) == par[:, 4]).all() and (par[:, 4] == par[:, 5]).all()
                if name == "noise_zero" and num_point > 1:
                    assert np.abs(noise).max() > 0.1  # the normals are still emitted; they are multiplied by zero
    if name == "color_half":
        assert seen_keep == {0.0, 1.0}  # both branches of the colour drop ran
    else:
        assert seen_keep == {1.0}
    if name == "all_symmetries":
        assert seen_flip == {-1.0, 1.0}


def test_normals_are_unit_normal_reproducible_and_disjoint():
    """over the 3 * 3 * 257 normals of one call: mean and variance; the same (seed, item0) twice; item0 + b"""
    n = 257
    pts = crops(n, 3)
    _, _, noise = run_guarded(pts, P.DEFAULT, SEED, 40, False, NAN_BYTE)
    _, _, again = run_guarded(pts, P.DEFAULT, SEED, 40, True, ALT_BYTE)
    np.testing.assert_array_equal(bits(noise), bits(again))
    _, _, after = run_guarded(pts, P.DEFAULT, SEED, 40 + B, False, NAN_BYTE)
    rows = lambda a: {r.tobytes() for r in a.reshape(-1, 3)}  # noqa: E731
    assert len(rows(noise)) == B * n and not (rows(noise) & rows(after))
    # a sample of m unit normals: the mean has standard error 1 / sqrt(m), the variance sqrt(2 / (m - 1)); four standard
    # errors are passed by a true normal sample once in 16 000 draws, and this sample is fixed by (SEED, 40)
    m = noise.size
    assert m == 3 * 3 * 257
    v = noise.astype(np.float64)
    assert abs(v.mean()) <= 4.0 / np.sqrt(m)
    assert abs(v.var(ddof=1) - 1.0) <= 4.0 * np.sqrt(2.0 / (m - 1))
    assert np.abs(v).max() <= np.sqrt(2 * 24 * np.log(2.0)) * (1 + 1e-6)  # the radius at u1 = 2^-24: 5.77
    _, _, other = run_guarded(pts, P.DEFAULT, SEED + 1, 40, False, NAN_BYTE)
    assert not (rows(noise) & rows(other))  # the seed is part of the address


def test_public_form_and_item_staging():
    from pointasnl_amd import grid_augment

    pts = crops(70, 6)
    dev = torch.from_numpy(pts).cuda()
    want, par, noise = run_guarded(pts, P.DEFAULT, 9, 123, False, NAN_BYTE)
    out, params, normals = grid_augment.augment_input(dev, None, 9, 123, return_params=True)
    assert out.data_ptr() != dev.data_ptr() and tuple(params.shape) == (B, 8) and tuple(normals.shape) == (B, 70, 3)
    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(want))
    np.testing.assert_array_equal(bits(params.cpu().numpy()), bits(par))
    np.testing.assert_array_equal(bits(normals.cpu().numpy()), bits(noise))
    item = grid_augment.item_tensor(0, dev.device)
    item.fill_(123)  # staged on the device: the same call, another number
    same = grid_augment.augment_input(dev, grid_augment.TRAINING, 9, item, out=dev)
    assert same.data_ptr() == dev.data_ptr()
    np.testing.assert_array_equal(bits(dev.cpu().numpy()), bits(want))
    big, bpar, bnoise = (t.cpu().numpy() for t in grid_augment.augment_input(torch.from_numpy(pts).cuda(), types_config(), 9,
                                                                             (1 << 64) - 2, return_params=True))
    for c in range(B):  # the item number is an unsigned 64-bit counter and wraps
        q = P.crop_params(9, ((1 << 64) - 2 + c) % (1 << 64))
        assert bits(bpar[c, 0]) == bits(q["theta"])
        np.testing.assert_array_equal(bits(bpar[c, 3:6]), bits(q["scales"]))
        np.testing.assert_array_equal(bits(big[c]), bits(P.apply(pts[c], bpar[c, 1], bpar[c, 2], bpar[c, 3:6], bpar[c, 6], bnoise[c])))
    with pytest.raises(ValueError):
        grid_augment.augment_input(dev[:, :, :2], None, 0, 0)
    with pytest.raises(ValueError, match="Unknown rotation"):
        grid_augment.augment_input(dev, dict(augment_rotation="all"), 0, 0)


def types_config():
    import types

    return types.SimpleNamespace(**product_config(P.DEFAULT))


def test_zz_report_worst_noise_error():
    print("box-muller: largest |float32 kernel - float64 restatement| over this file's words: %.3e (bound %.3e)"
          % (worst["noise"], NOISE_TOL))
    assert worst["noise"] <= NOISE_TOL
