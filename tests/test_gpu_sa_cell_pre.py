"""The pre-projected local cell (pasnl_sa_project + pasnl_sa_cell_pre / pasnl_sa_cell_pre_centre0): conv0 split at its linear part,
[xyz | feature] . W0[3:] + b0 once per source point and (xyz - centre) . W0[0:3] per neighbour.  Against the fp64 restatement of
pointasnl_util.py:63-74,248-249,264-274 (1e-5 of the output scale), its skip maxima bit-equal to the gathered maximum, its two
centre forms bit-equal to each other, and within fp32 rounding of the plain cell (pasnl_sa_cell)."""
import numpy as np
import pytest
import torch

from conftest import clouds
from oracle import cells

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _store(seed):
    from pointasnl_amd.utils import tf_util

    return tf_util.set_store(tf_util.VariableStore(seed=seed, randomize_bn=True))


@pytest.mark.parametrize("b,n,c,m,k,c1", [
    (64, 512, 128, 128, 64, 128),  # cls layer2 at the benchmark's batch
    (2, 512, 128, 128, 64, 128), (1, 256, 64, 37, 32, 32),                   # the models' shapes (8-step tail)
    (19, 96, 24, 33, 32, 32),      # row width 32: no partial chunk; 19 clouds: the XCD map with a ragged last round
    (17, 64, 56, 16, 32, 64),      # row width 64: two full chunks, no partial chunk
    (2, 128, 16, 40, 64, 64),      # partial chunk with 16 live steps
    (1, 100, 28, 5, 96, 64),       # three tiles per group
    (1, 50, 4, 1, 32, 128)])       # one group, one chunk: fewer groups than waves
def test_pre_projected_cell(b, n, c, m, k, c1):
    from pointasnl_amd.utils import pointasnl_util as U

    st = _store(b * 11 + c)
    rng = np.random.default_rng(n + c)
    xyz = clouds(5, b, n)
    feat = rng.standard_normal((b, n, c)).astype(np.float32)
    idx = rng.integers(0, n, (b, m, k)).astype(np.int32)
    centres = xyz[np.arange(b)[:, None], idx[:, :, 0]]
    mlp = [c1, c1, 2 * c1]
    with st.scope("L"):
        got, skip = U.sa_cell_pre(dev(xyz), dev(feat), dev(idx), dev(centres), mlp, False, None, None, True)
        got0, skip0, cen, nf = U.sa_cell_pre(dev(xyz), dev(feat), dev(idx), None, mlp, False, None, None, True)
        plain, plain_skip = U.sa_cell(dev(xyz), dev(feat), dev(idx), dev(centres), mlp, False, None, None, True)
    # the centre0 form reads the same centres from its own tiles: the same bits, and pasnl_take_neighbor0's outputs
    assert torch.equal(got, got0) and torch.equal(skip, skip0)
    np.testing.assert_array_equal(cen.cpu().numpy(), centres)
    np.testing.assert_array_equal(nf.cpu().numpy(), np.concatenate([centres, feat[np.arange(b)[:, None], idx[:, :, 0]]], axis=-1))
    bi = np.arange(b)[:, None, None]
    gx = xyz[bi, idx]
    x = np.concatenate([gx - centres[:, :, None, :], gx, feat[bi, idx]], axis=-1)  # (b,m,k,6+c) float32, exact
    np.testing.assert_array_equal(skip.cpu().numpy(), x.max(axis=2))
    np.testing.assert_array_equal(skip.cpu().numpy(), plain_skip.cpu().numpy())
    p = st.export_numpy()
    x64 = x.astype(np.float64)
    h = cells._layer(cells._layer(x64, p["L/conv0"], "relu"), p["L/conv1"], "relu")
    wn = cells._layer(x64[..., :3], p["L/weight_net/wconv0"], "relu")
    want = np.swapaxes(h, 2, 3) @ wn  # (b,m,c1,32)
    scale = np.abs(want).max()
    g = got.cpu().numpy()
    assert np.abs(g - want).max() / scale < 1e-5
    np.testing.assert_allclose(g, plain.cpu().numpy(), rtol=1e-5, atol=1e-6 * scale)


def test_projection_table():
    """pasnl_sa_project alone: [xyz | feature] . W0[3:] + b0 per point, ragged last tile (n not a multiple of 32)"""
    from pointasnl_amd import _hip

    rng = np.random.default_rng(3)
    b, n, c, c1 = 3, 77, 36, 64
    xyz = clouds(7, b, n)
    feat = rng.standard_normal((b, n, c)).astype(np.float32)
    w0 = rng.standard_normal((6 + c, c1)).astype(np.float32)
    b0 = rng.standard_normal(c1).astype(np.float32)
    proj = torch.full((b, n, c1), np.nan, dtype=torch.float32, device="cuda")
    x, f, w, bb = dev(xyz), dev(feat), dev(w0), dev(b0)
    _hip.launch("pasnl_sa_project", "sa_project", b, n, c, c1, _hip.ptr(x), _hip.ptr(f), _hip.ptr(w), _hip.ptr(bb), _hip.ptr(proj))
    torch.cuda.synchronize()
    want = np.concatenate([xyz, feat], axis=-1).astype(np.float64) @ w0[3:].astype(np.float64) + b0
    got = proj.cpu().numpy()
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-6


def test_classifier_with_and_without_the_table(monkeypatch):
    """A classifier forward with SA_CELL_PREPROJECT on and off: layer2 takes the table (and only it does), the argmax agrees and
    the logits agree within 1e-5 of their scale"""
    from pointasnl_amd.models import pointasnl_cls
    from pointasnl_amd.utils import pointasnl_util as U

    rng = np.random.default_rng(11)
    pc = rng.standard_normal((4, 1024, 3)).astype(np.float32)
    pc /= np.abs(pc).max()
    calls = []
    real = U.sa_cell_pre

    def counted(*a, **kw):
        calls.append(a[1].shape)
        return real(*a, **kw)

    monkeypatch.setattr(U, "sa_cell_pre", counted)
    out = {}
    for flag in (True, False):
        monkeypatch.setattr(U, "SA_CELL_PREPROJECT", flag)
        _store(5)
        with torch.no_grad():
            logits, _ = pointasnl_cls.get_model(dev(pc), is_training=False)
        torch.cuda.synchronize()
        out[flag] = logits.cpu().numpy()
    assert calls == [(4, 512, 128)]
    scale = np.abs(out[False]).max()
    assert (out[True].argmax(1) == out[False].argmax(1)).all()
    assert np.abs(out[True] - out[False]).max() / scale < 1e-5
