"""pasnl_cls_nl_cell_input (csrc/nl_input.hip): the non-local cell of a narrow level, attended in input space.

Kernel level: against the fp64 restatement of the cb-wide cell (tests/nl_cell_input_ref.py) at DESIGN 5's atol = rtol = 1e-5,
on shapes that take every path -- a ragged query tile, fewer keys than a block / than waves, uneven key ranges, the generic
width, 4 / 8 / 16 waves per workgroup, more than one staged chunk per wave --, a key that dominates the softmax, guarded
output with poisoned rows behind the inputs, refusals before any launch.  Path level: PointNonLocalCell with NL_INPUT_SPACE
on against off.  Model level: pointasnl_cls on against off, and eager against replayed from a captured graph."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import nl_cell_input_ref as R
from conftest import clouds

pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 70, 45, 3, 6, 32),     # p not a multiple of 64, fewer keys than one wave's block
    (1, 1, 1, 3, 6, 32),
    (3, 130, 333, 3, 6, 32),   # three query tiles, uneven key ranges
    (1, 64, 3, 3, 6, 32),      # fewer keys than waves
    (2, 33, 77, 6, 9, 64),
    (1, 40, 200, 8, 16, 128),
    (1, 64, 600, 3, 6, 32),    # 8 waves per workgroup
    (1, 70, 4500, 3, 6, 32),   # 16 waves, a second (ragged) chunk per wave
    (512, 1, 1100, 3, 6, 32),  # 4 waves, a second chunk per wave
    (1, 10, 2100, 5, 7, 64),   # the generic width: 8 waves at the most, a second chunk per wave
]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared problems are read-only)


def call(shape, d, out_ptr, override={}):
    """one call of the entry point -> status; d: name -> device tensor; override: name -> value"""
    from pointasnl_amd import _hip
    b, p, n, c, cz, cb = shape
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    a = dict(b=b, p=p, n=n, c=c, cz=cz, cb=cb, feature=ptr(d["feature"]), new_point=ptr(d["new_point"]), wkv=ptr(d["wkv"]),
             bkv=ptr(d["bkv"]), wq=ptr(d["wq"]), bq=ptr(d["bq"]), out=ctypes.c_void_p(out_ptr))
    assert not set(override) - set(a)
    a.update(override)
    rc = _hip.lib().pasnl_cls_nl_cell_input(*a.values(), _hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def run(shape, h):
    b, p, n, c, cz, cb = shape
    out = torch.full((b, p, cb), float("nan"), device="cuda")
    assert call(shape, {k: dev(v) for k, v in h.items()}, out.data_ptr()) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_the_fp64_cell(shape):
    h = R.problem(*shape)
    want = R.restated(h, shape[5])
    got = run(shape, h)
    print(f"{shape}: {R.split_of(shape[0], shape[1], shape[2], shape[3])} waves, worst error / bound = {R.worst_ratio(got, want):.4f}, "
          f"mirror {R.worst_ratio(R.mirror(h, shape[5], R.split_of(shape[0], shape[1], shape[2], shape[3])), want):.4f}")
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)


def test_one_key_dominates_the_softmax():
    # as tests/test_gpu_cells.py::test_nl_attention_spike: a late key whose score leads every other by > 80 in log2 units
    shape = (1, 64, 300, 3, 6, 32)
    b, p, n, c, cz, cb = shape
    h = {k: v.copy() for k, v in R.problem(*shape, seed=5).items()}
    h["feature"] *= np.float32(0.1)
    g = {k: v.astype(np.float64) for k, v in h.items()}
    u = (g["new_point"][0, 3] @ g["wq"] + g["bq"]) @ g["wkv"][:, :cb].T  # query 3's direction in input space
    h["feature"][0, 250] = (u / (u @ u) * (120.0 * np.sqrt(cb) / np.log2(np.e))).astype(np.float32)  # 120 log2 units
    x = h["feature"][0].astype(np.float64)
    score = (x @ u) * np.log2(np.e) / np.sqrt(cb)
    assert score[250] - np.delete(score, 250).max() > 80
    got = run(shape, h)
    assert np.isfinite(got).all()
    v250 = x[250] @ g["wkv"][:, cb:] + g["bkv"][cb:]
    np.testing.assert_allclose(got[0, 3], v250, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(2, 70, 45, 3, 6, 32), (3, 130, 333, 3, 6, 32), (2, 33, 77, 6, 9, 64), (1, 70, 4500, 3, 6, 32)])
def test_output_stays_inside_its_buffer_and_rows_behind_the_inputs_are_not_read(shape):
    b, p, n, c, cz, cb = shape
    h = R.problem(*shape)
    d = {k: dev(v) for k, v in h.items()}
    nan = lambda rows, w: torch.full((rows, w), float("nan"), device="cuda")
    d["feature"] = torch.cat([d["feature"].reshape(b * n, c), nan(80, c)])      # poisoned rows behind the last cloud
    d["new_point"] = torch.cat([d["new_point"].reshape(b * p, cz), nan(80, cz)])
    runs = []
    for fill in (guarded.NAN_BYTE, guarded.ALT_BYTE):
        out = guarded.Guarded(b * p * cb * 4, fill, guarded.output_guard(cb * 4))
        assert call(shape, d, out.ptr) == 0
        assert out.guards_intact()
        runs.append(out.floats((b, p, cb)))
    assert np.isfinite(runs[0]).all()
    np.testing.assert_array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    np.testing.assert_array_equal(runs[0].view(np.uint32), run(shape, h).view(np.uint32))  # a pure function of its inputs
    np.testing.assert_allclose(runs[0], R.restated(h, cb), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("override,status", [
    (dict(c=9), -5), (dict(cz=17), -5), (dict(cb=48), -5), (dict(n=0), -1), (dict(c=0), -1), (dict(cz=0), -1), (dict(b=-1), -1),
    (dict(p=-1), -1),
] + [({k: ctypes.c_void_p(0)}, -2) for k in ("feature", "new_point", "wkv", "bkv", "wq", "bq", "out")])
def test_unsupported_shapes_and_null_pointers_are_refused_before_any_launch(override, status):
    shape = (2, 70, 45, 3, 6, 32)
    d = {k: dev(v) for k, v in R.problem(*shape).items()}
    out = guarded.Guarded(2 * 70 * 32 * 4, guarded.NAN_BYTE, guarded.output_guard(32 * 4))
    assert call(shape, d, out.ptr, override) == status
    assert out.untouched()


@pytest.mark.parametrize("override", [dict(b=0), dict(p=0)])
def test_an_empty_batch_is_a_successful_no_op(override):
    shape = (2, 70, 45, 3, 6, 32)
    d = {k: dev(v) for k, v in R.problem(*shape).items()}
    out = guarded.Guarded(2 * 70 * 32 * 4, guarded.NAN_BYTE, guarded.output_guard(32 * 4))
    assert call(shape, d, out.ptr, override) == 0
    assert out.untouched()


# ------------------------------------------------------------------------------------------------------------- the Python path
def _store(seed):
    from pointasnl_amd.utils import tf_util
    return tf_util.set_store(tf_util.VariableStore(seed=seed, randomize_bn=True))


def _launched(fn):
    from pointasnl_amd import _hip
    _hip.PROFILE = []
    try:
        with torch.no_grad():
            out = fn()
        launched = [sym for sym, _, _, _ in _hip.PROFILE]
    finally:
        _hip.PROFILE = None
    torch.cuda.synchronize()
    return out, launched


@pytest.mark.parametrize("project", [False, True])
def test_point_non_local_cell_with_and_without_the_input_space_kernel(project, monkeypatch):
    from pointasnl_amd.utils import pointasnl_util as U
    rng = np.random.default_rng(11)
    feature = dev(rng.standard_normal((2, 200, 3)).astype(np.float32))
    new_point = dev(rng.standard_normal((2, 1, 96, 6)).astype(np.float32))  # (B,1,P,C): the layers' call
    outs = {}
    for flag in (True, False):
        monkeypatch.setattr(U, "NL_INPUT_SPACE", flag)
        _store(21)
        outs[flag] = _launched(lambda: U.PointNonLocalCell(feature, new_point, [32, 128], False, None, None, 'layer1', bn=True,
                                                           project=project))
    assert "pasnl_cls_nl_cell_input" in outs[True][1] and "pasnl_narrow_project2" not in outs[True][1]
    assert "pasnl_cls_nl_cell_input" not in outs[False][1] and "pasnl_narrow_project2" in outs[False][1]
    assert outs[True][0].shape == ((2, 96, 128) if project else (2, 96, 32))
    assert torch.allclose(outs[True][0], outs[False][0], rtol=1e-5, atol=1e-5)


def test_a_width_the_kernel_does_not_cover_takes_the_projected_path(monkeypatch):
    from pointasnl_amd.utils import pointasnl_util as U
    rng = np.random.default_rng(12)
    feature = dev(rng.standard_normal((2, 100, 9)).astype(np.float32))
    new_point = dev(rng.standard_normal((2, 1, 40, 12)).astype(np.float32))
    _store(21)
    out, launched = _launched(lambda: U.PointNonLocalCell(feature, new_point, [32, 64], False, None, None, 'layer1', bn=True))
    assert "pasnl_cls_nl_cell_input" not in launched and "pasnl_narrow_project2" in launched
    assert out.shape == (2, 40, 64)


# ------------------------------------------------------------------------------------------------------------------ the model
def _forward(x, adaptive, flag, monkeypatch):
    from pointasnl_amd.models import pointasnl_cls
    from pointasnl_amd.utils import pointasnl_util as U
    monkeypatch.setattr(U, "NL_INPUT_SPACE", flag)
    _store(23)
    (logits, _), launched = _launched(lambda: pointasnl_cls.get_model(x, is_training=False, adaptive_sample=adaptive))
    return logits.clone(), launched


@pytest.mark.parametrize("adaptive", [False, True])
def test_classifier_with_and_without_the_input_space_kernel(adaptive, monkeypatch):
    x = dev(clouds(41, 2, 1024))
    # (with adaptive sampling the model takes the kernel only when told to: the step measured slower there)
    on, launched_on = _forward(x, adaptive, "always" if adaptive else True, monkeypatch)
    off, launched_off = _forward(x, adaptive, False, monkeypatch)
    assert launched_on.count("pasnl_cls_nl_cell_input") == 1 and "pasnl_cls_nl_cell_input" not in launched_off
    assert launched_on.count("pasnl_narrow_project2") == launched_off.count("pasnl_narrow_project2") - 1
    scale = float(off.abs().max())
    print(f"adaptive={adaptive}: max |on - off| / scale = {float((on - off).abs().max()) / scale:.3e}")
    assert float((on - off).abs().max()) <= 1e-4 * scale
    assert torch.equal(on.argmax(dim=1), off.argmax(dim=1))
    if adaptive:  # the model's own default there: the cb-wide kernels
        default, launched_default = _forward(x, adaptive, True, monkeypatch)
        assert "pasnl_cls_nl_cell_input" not in launched_default and torch.equal(default, off)


def test_forward_replayed_from_a_captured_graph_gives_the_eager_bits(monkeypatch):
    from pointasnl_amd.models import pointasnl_cls
    x = dev(clouds(41, 2, 1024))
    eager, launched = _forward(x, False, True, monkeypatch)  # (also folds and packs the weights: nothing of that is captured)
    assert "pasnl_cls_nl_cell_input" in launched

    def fwd():
        with torch.no_grad():
            return pointasnl_cls.get_model(x, is_training=False, adaptive_sample=False)[0]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fwd()  # the stream's own workspaces, allocated outside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        gout = fwd()
    torch.cuda.current_stream().wait_stream(s)
    for i in range(2):
        gout.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, eager), f"replay {i}"
