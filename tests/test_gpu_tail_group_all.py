"""pasnl_cls_tail_group_all (csrc/mlp_pool.hip): the classifier's layer 1 tail and its layer3_1 group-all module in one launch.

Kernel level: against the two launches it replaces (pasnl_sa_tail_packed writing the [0 | xyz | out] table, pasnl_mlp3_max_pool
reading it) -- the same bits -- and against the fp64 restatement of both (rtol 1e-4 / atol 1e-5 of the output scale, the bound
tests/test_gpu_cells.py holds the group-all module to), on clouds of one tile, less than a tile, and one and a half tiles.
Buffers: outputs and workspace in guarded buffers (tests/guarded.py), two fill patterns, a short workspace, unsupported widths and
null pointers.  Model level: pointasnl_cls with the switch on against off, eager and replayed from a captured graph."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
from conftest import clouds
from oracle import cells

pytestmark = pytest.mark.gpu

W, CB, C, MLP = 9, 32, 128, (128, 256, 512)
SHAPES = [(3, 96), (2, 40), (1, 64)]  # (clouds, points): a full and a half 64-row tile; less than a tile; exactly one tile
POOLED_STRIDE = MLP[2] + 8            # the pooled vectors are rows of a wider table: the columns between them are not written


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
    """inputs, packed weights, the two-launch result and the fp64 result of one shape -- computed once, shared, never changed"""
    if (b, n) in _PROBLEMS:
        return _PROBLEMS[(b, n)]
    from pointasnl_amd import _hip
    rng = np.random.default_rng(1000 * b + n)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    rows = b * n
    h = dict(after=np.maximum(f(rows, C), 0), skip=f(rows, W), att=f(rows, CB), xyz=clouds(7, b, n).reshape(rows, 3),
             ws=f(W, C) / np.float32(3), bs=f(C), wb=f(CB, C) / np.float32(np.sqrt(CB)), bb=f(C),
             wagg=f(C, C) / np.float32(np.sqrt(C)), bagg=f(C),
             w0=f(3 + C, MLP[0]) / np.float32(np.sqrt(3 + C)), b0=f(MLP[0]), w1=f(MLP[0], MLP[1]) / np.float32(np.sqrt(MLP[0])),
             b1=f(MLP[1]), w2=f(MLP[1], MLP[2]) / np.float32(np.sqrt(MLP[1])), b2=f(MLP[2]))
    d = {k: dev(v) for k, v in h.items()}
    for k in ("ws", "wb", "wagg"):
        d[k + "_pk"] = _pack("pasnl_sa_tail_pack_weights", "pasnl_sa_tail_packed_weights_bytes", h[k])
    d["w0_pk"] = _pack("pasnl_mlp3_pack_weights", "pasnl_mlp3_packed_weights_bytes",
                       np.concatenate([np.zeros((1, MLP[0]), np.float32), h["w0"]]))  # a zero row for the table's zero column
    d["w1_pk"] = _pack("pasnl_mlp3_pack_weights", "pasnl_mlp3_packed_weights_bytes", h["w1"])
    d["w2_pk"] = _pack("pasnl_mlp3_pack_weights", "pasnl_mlp3_packed_weights_bytes", h["w2"])
    # ---- the two launches
    out = torch.full((rows, C), float("nan"), device="cuda")
    cat = torch.full((rows, C + 4), float("nan"), device="cuda")
    pooled = torch.full((b, MLP[2]), float("nan"), device="cuda")
    nbytes = int(_hip.lib().pasnl_mlp3_max_pool_workspace_bytes(b, n, MLP[2]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _hip.launch("pasnl_sa_tail_packed", "sa_tail", rows, W, CB, C, _hip.ptr(d["after"]), _hip.ptr(d["skip"]), _hip.ptr(d["att"]),
                _hip.ptr(d["ws_pk"]), _hip.ptr(d["bs"]), _hip.ptr(d["wb_pk"]), _hip.ptr(d["bb"]), _hip.ptr(d["wagg_pk"]),
                _hip.ptr(d["bagg"]), _hip.ptr(None), _hip.ptr(d["xyz"]), _hip.ptr(cat), _hip.ptr(out))
    _hip.launch("pasnl_mlp3_max_pool", "mlp3_max_pool", b, n, C + 4, *MLP, _hip.ptr(cat), _hip.ptr(d["w0_pk"]), _hip.ptr(d["b0"]),
                _hip.ptr(d["w1_pk"]), _hip.ptr(d["b1"]), _hip.ptr(d["w2_pk"]), _hip.ptr(d["b2"]), _hip.ptr(pooled),
                ctypes.c_long(MLP[2]), _hip.ptr(ws), ctypes.c_size_t(nbytes))
    two = (out.cpu().numpy(), pooled.cpu().numpy())
    # ---- fp64
    g = {k: v.astype(np.float64) for k, v in h.items()}
    o64 = g["after"] + np.maximum(g["skip"] @ g["ws"] + g["bs"], 0) + np.maximum(g["att"] @ g["wb"] + g["bb"], 0)
    o64 = np.maximum(o64 @ g["wagg"] + g["bagg"], 0)
    x = np.concatenate([g["xyz"], o64], axis=1).reshape(b, n, 3 + C)
    for i in range(3):
        x = cells._layer(x, {"w": g[f"w{i}"], "b": g[f"b{i}"]}, "relu")
    _PROBLEMS[(b, n)] = (d, nbytes, two, (o64, x.max(axis=1)))
    return _PROBLEMS[(b, n)]


def fused_args(b, n, d, out_ptr, pooled_ptr, ws_ptr, ws_bytes, override={}):
    """the entry's arguments in order (without the stream); override: name -> value"""
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    a = dict(b=b, n=n, w=W, cb=CB, c=C, after=p(d["after"]), skip=p(d["skip"]), att=p(d["att"]), ws=p(d["ws_pk"]), bs=p(d["bs"]),
             wb=p(d["wb_pk"]), bb=p(d["bb"]), wagg=p(d["wagg_pk"]), bagg=p(d["bagg"]), xyz=p(d["xyz"]), c1=MLP[0], c2=MLP[1],
             c3=MLP[2], w0=p(d["w0_pk"]), b0=p(d["b0"]), w1=p(d["w1_pk"]), b1=p(d["b1"]), w2=p(d["w2_pk"]), b2=p(d["b2"]),
             out=ctypes.c_void_p(out_ptr), pooled=ctypes.c_void_p(pooled_ptr), stride=ctypes.c_long(POOLED_STRIDE),
             workspace=ctypes.c_void_p(ws_ptr), workspace_bytes=ctypes.c_size_t(ws_bytes))
    assert not set(override) - set(a)
    a.update(override)
    return list(a.values())


def run_guarded(b, n, out_fill, ws_fill, short=0, override={}):
    """one call with every output and the workspace in guarded buffers -> (status, out, pooled, workspace)"""
    from pointasnl_amd import _hip
    d, nbytes, _, _ = problem(b, n)
    out = guarded.Guarded(b * n * C * 4, out_fill, guarded.output_guard(C * 4))
    pooled = guarded.Guarded(((b - 1) * POOLED_STRIDE + MLP[2]) * 4, out_fill, guarded.output_guard(POOLED_STRIDE * 4))
    ws = guarded.Guarded(nbytes, ws_fill)
    rc = _hip.lib().pasnl_cls_tail_group_all(*fused_args(b, n, d, out.ptr, pooled.ptr, ws.ptr, nbytes - short, override),
                                             _hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, out, pooled, ws


def pooled_rows(pooled, b):
    """(vectors (b, c3), the bytes of the table between them) of the strided pooled buffer"""
    flat = np.concatenate([pooled.array((-1,), np.uint32), np.zeros(POOLED_STRIDE - MLP[2], np.uint32)]).reshape(b, POOLED_STRIDE)
    return flat[:, :MLP[2]].view(np.float32), flat[:-1, MLP[2]:]


@pytest.mark.parametrize("b,n", SHAPES)
def test_fused_launch_gives_the_two_launches_bits_and_stays_inside_its_buffers(b, n):
    _, _, (two_out, two_pooled), (out64, pooled64) = problem(b, n)
    runs = []
    for out_fill, ws_fill in ((guarded.NAN_BYTE, guarded.WS_BYTE), (guarded.ALT_BYTE, guarded.ALT_WS_BYTE)):
        rc, out, pooled, ws = run_guarded(b, n, out_fill, ws_fill)
        assert rc == 0
        assert out.guards_intact() and pooled.guards_intact() and ws.guards_intact()
        vec, between = pooled_rows(pooled, b)
        assert (between == np.uint32(out_fill * 0x01010101)).all(), "columns of the pooled table beside the vectors were written"
        runs.append((out.floats((b * n, C)), vec.copy()))
    got_out, got_pooled = runs[0]
    # whatever the buffers held before: the same bits
    np.testing.assert_array_equal(got_out.view(np.uint32), runs[1][0].view(np.uint32))
    np.testing.assert_array_equal(got_pooled.view(np.uint32), runs[1][1].view(np.uint32))
    # the two launches it replaces: the same bits
    assert torch.equal(torch.from_numpy(got_out), torch.from_numpy(two_out))
    assert torch.equal(torch.from_numpy(got_pooled), torch.from_numpy(two_pooled))
    # fp64
    for name, got, want in (("out", got_out, out64), ("pooled", got_pooled, pooled64), ("two-launch pooled", two_pooled, pooled64)):
        scale = np.abs(want).max()
        print(f"{name} (b={b}, n={n}): max abs err / scale = {np.abs(got - want).max() / scale:.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * scale, err_msg=name)


def test_one_byte_less_workspace_is_refused_and_nothing_is_touched():
    rc, out, pooled, ws = run_guarded(3, 96, guarded.NAN_BYTE, guarded.WS_BYTE, short=1)
    assert rc == -3
    assert out.untouched() and pooled.untouched() and ws.untouched()


@pytest.mark.parametrize("override,status", [
    (dict(w=10), -5), (dict(w=8), -5), (dict(cb=64), -5), (dict(c=256), -5), (dict(c=96), -5), (dict(c1=256), -5), (dict(c2=512), -5),
    (dict(c3=1024), -5),
    (dict(n=0), -1), (dict(b=-1), -1), (dict(stride=ctypes.c_long(MLP[2] - 1)), -1),
] + [({k: ctypes.c_void_p(0)}, -2) for k in ("after", "skip", "att", "ws", "bs", "wb", "bb", "wagg", "bagg", "xyz", "w0", "b0", "w1", "b1",
                                              "w2", "b2", "out", "pooled", "workspace")])
def test_unsupported_shapes_and_null_pointers_are_refused_before_any_launch(override, status):
    if override.get("c3") == 1024:  # (the workspace check comes first and scales with c3: give it room, the shape is still refused)
        from pointasnl_amd import _hip
        d, nbytes, _, _ = problem(2, 40)
        out = guarded.Guarded(2 * 40 * C * 4, guarded.NAN_BYTE)
        pooled = guarded.Guarded(4 * 1024 * 4, guarded.NAN_BYTE)
        ws = guarded.Guarded(2 * nbytes, guarded.WS_BYTE)
        args = fused_args(2, 40, d, out.ptr, pooled.ptr, ws.ptr, 2 * nbytes, dict(override, stride=ctypes.c_long(1024)))
        rc = _hip.lib().pasnl_cls_tail_group_all(*args, _hip.stream_ptr())
        torch.cuda.synchronize()
    else:
        rc, out, pooled, ws = run_guarded(2, 40, guarded.NAN_BYTE, guarded.WS_BYTE, override=override)
    assert rc == status
    assert out.untouched() and pooled.untouched() and ws.untouched()


def test_an_empty_batch_is_a_successful_no_op():
    rc, out, pooled, ws = run_guarded(2, 40, guarded.NAN_BYTE, guarded.WS_BYTE, override=dict(b=0))
    assert rc == 0
    assert out.untouched() and pooled.untouched() and ws.untouched()


# ---------------------------------------------------------------------------------------------------------------- the model
def _store(seed):
    from pointasnl_amd.utils import tf_util
    return tf_util.set_store(tf_util.VariableStore(seed=seed, randomize_bn=True))


def _forward(x, adaptive, switch, monkeypatch):
    """(logits, l1_points, l2_points, launched entry points) of pointasnl_cls with the switch set"""
    from pointasnl_amd import _hip
    from pointasnl_amd.models import pointasnl_cls
    from pointasnl_amd.utils import pointasnl_util as U

    monkeypatch.setattr(U, "SA_TAIL_GROUP_ALL", switch)
    # two clouds are 1024 rows at layer 1: below the row count from which a layer's tail is one kernel at all (the three small
    # GEMMs win on few rows).  Lowered for both sides, so that the two-launch path and the fused launch are what is compared
    monkeypatch.setattr(U, "SA_TAIL_MIN_ROWS", 1024)
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
def test_classifier_is_the_same_with_and_without_the_fused_launch(adaptive, monkeypatch):
    x = dev(clouds(41, 2, 1024))
    off = _forward(x, adaptive, False, monkeypatch)
    # (with adaptive sampling the model takes the fused launch only when told to: it measured slower there)
    on = _forward(x, adaptive, "always" if adaptive else True, monkeypatch)
    assert "pasnl_cls_tail_group_all" in on[3] and on[3].count("pasnl_mlp3_max_pool") == off[3].count("pasnl_mlp3_max_pool") - 1
    assert "pasnl_cls_tail_group_all" not in off[3]
    for name, a, b in zip(("logits", "l1_points", "l2_points"), on, off):
        assert torch.equal(a, b), name


def test_fused_forward_replayed_from_a_captured_graph_gives_the_eager_bits(monkeypatch):
    from pointasnl_amd.models import pointasnl_cls

    x = dev(clouds(41, 2, 1024))
    eager = _forward(x, False, True, monkeypatch)  # (also packs the weights: no launch of a packing kernel is captured)

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
