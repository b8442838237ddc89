"""pasnl_cls_tail_mlp2 (csrc/mlp_pool.hip): the classifier's layer 2 tail and the first two convolutions of its layer3_2 group-all
module in one launch.

Kernel level: `out` against pasnl_sa_tail_packed -- the same bits --, H2 = relu(relu([xyz | out] W0 + b0) W1 + b1) against the
fp64 restatement within 1e-5 of its scale, every element (ReLU is continuous: none excluded), on clouds of three whole tiles of
32 rows, a ragged last tile, exactly one tile, a single row and four whole tiles.  Buffers: outputs in guarded buffers
(tests/guarded.py), two stale fills, an H2 buffer one byte short, unsupported widths, null pointers, an empty batch.
Model level: pointasnl_cls with the switch on against off (the logits follow another summation order in two of their
convolutions: argmax equal, 1e-4 of their scale -- the bound test_cls_forward_matches_oracle holds the model to), eager and
replayed from a captured graph."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
from conftest import clouds
from oracle import cells

pytestmark = pytest.mark.gpu

W, CB, C, C1, C2 = 134, 64, 256, 256, 512
SHAPES = [(3, 96), (2, 40), (1, 32), (1, 1), (2, 128)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pack(entry, size_fn, w):
    from pointasnl_amd import _hip
    m = dev(w)
    pk = torch.empty(int(getattr(_hip.lib(), size_fn)(m.shape[0], m.shape[1])) // 4, device="cuda")
    _hip.launch(entry, "pack", m.shape[0], m.shape[1], _hip.ptr(m), _hip.ptr(pk))
    return pk


_PROBLEMS = {}


def problem(b, n):
    """inputs, packed weights, the separate tail's `out` and the fp64 results of one shape -- computed once, shared, never changed"""
    if (b, n) in _PROBLEMS:
        return _PROBLEMS[(b, n)]
    from pointasnl_amd import _hip
    rng = np.random.default_rng(2000 * b + n)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    rows = b * n
    h = dict(after=np.maximum(f(rows, C), 0), skip=f(rows, W), att=f(rows, CB), xyz=f(rows, 3),
             ws=f(W, C) / np.float32(np.sqrt(W)), bs=f(C), wb=f(CB, C) / np.float32(np.sqrt(CB)), bb=f(C),
             wagg=f(C, C) / np.float32(np.sqrt(C)), bagg=f(C),
             w0=f(3 + C, C1) / np.float32(np.sqrt(3 + C)), b0=f(C1), w1=f(C1, C2) / np.float32(np.sqrt(C1)), b1=f(C2))
    d = {k: dev(v) for k, v in h.items()}
    for k in ("ws", "wb", "wagg"):
        d[k + "_pk"] = _pack("pasnl_sa_tail_pack_weights", "pasnl_sa_tail_packed_weights_bytes", h[k])
    d["w0_pk"] = _pack("pasnl_mlp3_pack_weights", "pasnl_mlp3_packed_weights_bytes",
                       np.concatenate([np.zeros((1, C1), np.float32), h["w0"]]))  # a zero row for the rows' zero column
    d["w1_pk"] = _pack("pasnl_mlp3_pack_weights", "pasnl_mlp3_packed_weights_bytes", h["w1"])
    # ---- the separate tail
    out = torch.full((rows, C), float("nan"), device="cuda")
    _hip.launch("pasnl_sa_tail_packed", "sa_tail", rows, W, CB, C, _hip.ptr(d["after"]), _hip.ptr(d["skip"]), _hip.ptr(d["att"]),
                _hip.ptr(d["ws_pk"]), _hip.ptr(d["bs"]), _hip.ptr(d["wb_pk"]), _hip.ptr(d["bb"]), _hip.ptr(d["wagg_pk"]),
                _hip.ptr(d["bagg"]), _hip.ptr(None), _hip.ptr(None), _hip.ptr(None), _hip.ptr(out))
    tail_out = out.cpu().numpy()
    # ---- fp64
    g = {k: v.astype(np.float64) for k, v in h.items()}
    o64 = g["after"] + np.maximum(g["skip"] @ g["ws"] + g["bs"], 0) + np.maximum(g["att"] @ g["wb"] + g["bb"], 0)
    o64 = np.maximum(o64 @ g["wagg"] + g["bagg"], 0)
    x = np.concatenate([g["xyz"], o64], axis=1)
    for i in range(2):
        x = cells._layer(x, {"w": g[f"w{i}"], "b": g[f"b{i}"]}, "relu")
    _PROBLEMS[(b, n)] = (d, tail_out, (o64, x))
    return _PROBLEMS[(b, n)]


def fused_args(b, n, d, out_ptr, h2_ptr, h2_bytes, override={}):
    """the entry's arguments in order (without the stream); override: name -> value"""
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    a = dict(b=b, n=n, w=W, cb=CB, c=C, after=p(d["after"]), skip=p(d["skip"]), att=p(d["att"]), ws=p(d["ws_pk"]), bs=p(d["bs"]),
             wb=p(d["wb_pk"]), bb=p(d["bb"]), wagg=p(d["wagg_pk"]), bagg=p(d["bagg"]), xyz=p(d["xyz"]), c1=C1, c2=C2,
             w0=p(d["w0_pk"]), b0=p(d["b0"]), w1=p(d["w1_pk"]), b1=p(d["b1"]),
             out=ctypes.c_void_p(out_ptr), h2=ctypes.c_void_p(h2_ptr), h2_bytes=ctypes.c_size_t(h2_bytes))
    assert not set(override) - set(a)
    a.update(override)
    return list(a.values())


def run_guarded(b, n, out_fill, h2_fill, short=0, override={}):
    """one call with both outputs in guarded buffers -> (status, out, h2)"""
    from pointasnl_amd import _hip
    d, _, _ = problem(b, n)
    out = guarded.Guarded(b * n * C * 4, out_fill, guarded.output_guard(C * 4))
    h2 = guarded.Guarded(b * n * C2 * 4, h2_fill, guarded.output_guard(C2 * 4))
    rc = _hip.lib().pasnl_cls_tail_mlp2(*fused_args(b, n, d, out.ptr, h2.ptr, b * n * C2 * 4 - short, override), _hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, h2


@pytest.mark.parametrize("b,n", SHAPES)
def test_fused_launch_gives_the_tails_bits_and_h2_and_stays_inside_its_buffers(b, n):
    _, tail_out, (out64, h2_64) = problem(b, n)
    runs = []
    for out_fill, h2_fill in ((guarded.NAN_BYTE, guarded.WS_BYTE), (guarded.ALT_BYTE, guarded.ALT_WS_BYTE)):
        rc, out, h2 = run_guarded(b, n, out_fill, h2_fill)
        assert rc == 0
        assert out.guards_intact() and h2.guards_intact()
        runs.append((out.floats((b * n, C)), h2.floats((b * n, C2))))
    got_out, got_h2 = runs[0]
    # whatever the buffers held before: the same bits
    np.testing.assert_array_equal(got_out.view(np.uint32), runs[1][0].view(np.uint32))
    np.testing.assert_array_equal(got_h2.view(np.uint32), runs[1][1].view(np.uint32))
    # the separate tail: the same bits
    assert torch.equal(torch.from_numpy(got_out), torch.from_numpy(tail_out))
    # fp64: 1e-5 of the scale, every element
    scale = np.abs(h2_64).max()
    err = np.abs(got_h2 - h2_64).max() / scale
    # (for the record, not a bound: the two vendor GEMMs the launch replaces, on the same rows)
    d = problem(b, n)[0]
    x = torch.cat([d["xyz"], torch.from_numpy(tail_out).cuda()], dim=1)
    vendor = torch.relu(torch.addmm(d["b1"], torch.relu(torch.addmm(d["b0"], x, d["w0"])), d["w1"])).cpu().numpy()
    print(f"h2 (b={b}, n={n}): max abs err / scale = {err:.3e} (vendor GEMM chain: {np.abs(vendor - h2_64).max() / scale:.3e}); "
          f"out: {np.abs(got_out - out64).max() / np.abs(out64).max():.3e}")
    assert err <= 1e-5


def test_one_byte_less_h2_is_refused_and_nothing_is_touched():
    rc, out, h2 = run_guarded(3, 96, guarded.NAN_BYTE, guarded.WS_BYTE, short=1)
    assert rc == -3
    assert out.untouched() and h2.untouched()


@pytest.mark.parametrize("override,status", [
    (dict(w=133), -5), (dict(w=135), -5), (dict(cb=32), -5), (dict(c=128), -5), (dict(c=288), -5), (dict(c1=128), -5), (dict(c2=256), -5),
    (dict(c2=1024), -5), (dict(n=0), -1), (dict(b=-1), -1),
] + [({k: ctypes.c_void_p(0)}, -2) for k in ("after", "skip", "att", "ws", "bs", "wb", "bb", "wagg", "bagg", "xyz", "w0", "b0", "w1", "b1",
                                              "out", "h2")])
def test_unsupported_shapes_and_null_pointers_are_refused_before_any_launch(override, status):
    rc, out, h2 = run_guarded(2, 40, guarded.NAN_BYTE, guarded.WS_BYTE, override=override)
    assert rc == status
    assert out.untouched() and h2.untouched()


def test_an_empty_batch_is_a_successful_no_op():
    rc, out, h2 = run_guarded(2, 40, guarded.NAN_BYTE, guarded.WS_BYTE, override=dict(b=0))
    assert rc == 0
    assert out.untouched() and h2.untouched()


# ---------------------------------------------------------------------------------------------------------------- the model
def _store(seed):
    from pointasnl_amd.utils import tf_util
    return tf_util.set_store(tf_util.VariableStore(seed=seed, randomize_bn=True))


def _forward(x, adaptive, switch, monkeypatch):
    """(logits, l1_points, l2_points, launched entry points) of pointasnl_cls with the switch set"""
    from pointasnl_amd import _hip
    from pointasnl_amd.models import pointasnl_cls
    from pointasnl_amd.utils import pointasnl_util as U

    monkeypatch.setattr(U, "SA_TAIL_MLP2", switch)
    # 16 clouds are 2048 rows at layer 2: the row count from which a layer's tail is one kernel at all
    _store(23)
    _hip.PROFILE = []
    try:
        with torch.no_grad():
            logits, ep = pointasnl_cls.get_model(x, is_training=False, adaptive_sample=adaptive)
        launched = [sym for sym, _, _, _ in _hip.PROFILE]
    finally:
        _hip.PROFILE = None
    torch.cuda.synchronize()
    return logits.clone(), ep["l1_points"].clone(), ep["l2_points"].clone(), launched


@pytest.mark.parametrize("adaptive", [False, True])
def test_classifier_with_and_without_the_fused_launch(adaptive, monkeypatch):
    x = dev(clouds(43, 16, 1024))
    off = _forward(x, adaptive, False, monkeypatch)
    on = _forward(x, adaptive, "always" if adaptive else True, monkeypatch)
    assert "pasnl_cls_tail_mlp2" in on[3] and "pasnl_cls_tail_mlp2" not in off[3]
    assert on[3].count("pasnl_sa_tail_packed") == off[3].count("pasnl_sa_tail_packed") - 1
    assert torch.equal(on[1], off[1]), "l1_points"
    assert torch.equal(on[2], off[2]), "l2_points"
    a, b = on[0].cpu().numpy().astype(np.float64), off[0].cpu().numpy().astype(np.float64)
    dev_ = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    print(f"logits on against off (adaptive={adaptive}): max abs deviation / scale = {dev_:.3e}")
    assert (a.argmax(1) == b.argmax(1)).all()
    assert dev_ < 1e-4


def test_fused_forward_replayed_from_a_captured_graph_gives_the_eager_bits(monkeypatch):
    from pointasnl_amd.models import pointasnl_cls

    x = dev(clouds(43, 16, 1024))
    eager = _forward(x, False, True, monkeypatch)  # (also packs the weights: no launch of a packing kernel is captured)
    assert "pasnl_cls_tail_mlp2" in eager[3]

    def fwd():
        with torch.no_grad():
            logits, ep = pointasnl_cls.get_model(x, is_training=False, adaptive_sample=False)
        return logits, ep["l1_points"], ep["l2_points"]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fwd()  # the stream's own workspace, allocated outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        gout = fwd()
    torch.cuda.current_stream().wait_stream(s)
    for i in range(2):
        for t in gout:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("logits", "l1_points", "l2_points"), gout, eager):
            assert torch.equal(a, b), f"replay {i}: {name}"
