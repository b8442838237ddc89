"""is_training=True through tf_util's wrappers, the layers and the models (csrc/bn_train.hip behind every GEMM).

Wrappers: against a float64 torch restatement of GEMM, bias, batch norm, activation on the CPU; yardstick the same chain in
float32 on the CPU; allowed err <= max(4 * err_chain, 1e-5) (tests/test_gpu_bn_train.py's rule).  The gradient of a bias in
front of a batch norm is zero in exact arithmetic (the mean takes it out again): it is held to the size of the terms that cancel.

Layers and models: the fused route (tf_util.BN_TRAIN_FUSED = True) against the torch route (False) from the same variables,
moving statistics and dropout address.  The tolerance is the torch route's own float32 noise: the False route with its
statistics taken in float32 against the same route with them taken in float64 (tf_util.BN_TRAIN_TORCH_DTYPE); the fused route is
allowed 4 x that per quantity, and never less than 1e-5.  Figures of the classifier at B = 8, N = 1024 (err fused / noise) are
printed by the test and recorded in EXPERIMENTS.md ("Training mode")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# entries that take BN-folded weights: none of them may be launched with is_training=True
FOLDED = ("pasnl_sa_local_cell", "pasnl_sa_cell", "pasnl_sa_project", "pasnl_sa_tail", "pasnl_cls_tail", "pasnl_decode_cell",
          "pasnl_mlp3_max_pool", "pasnl_dense_", "pasnl_narrow_project2", "pasnl_as_attention_proj", "pasnl_as_cell",
          "pasnl_cls_nl_cell_input", "pasnl_fp_interpolate_cat", "pasnl_mlp3_pack", "pasnl_sa_tail_pack", "pasnl_bf16x3")


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd.utils import tf_util

    return tf_util


@pytest.fixture()
def launches(monkeypatch):
    from pointasnl_amd import _hip

    seen = []
    inner = _hip._launch

    def counting(symbol, what, *args):
        seen.append(symbol)
        return inner(symbol, what, *args)

    monkeypatch.setattr(_hip, "_launch", counting)
    return seen


def folded_launches(seen):
    return sorted({s for s in seen if s.startswith(FOLDED)})


def err(got, want, scale=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / (max(np.abs(want).max(), 1e-300) if scale is None else scale))


def allowed(chain_err):
    return max(4 * chain_err, 1e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# the wrappers
# ---------------------------------------------------------------------------------------------------------------------------
def restate(x, v, activation, bn, unbiased, decay, dtype):
    """GEMM, bias, batch norm with the batch's statistics, activation on the CPU in `dtype`, differentiated by torch
    -> (y, {name: gradient}, moving_mean, moving_variance)"""
    t = {k: torch.tensor(a, dtype=dtype, requires_grad=k not in ("moving_mean", "moving_variance")) for k, a in v.items()}
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    z = xt.reshape(-1, x.shape[-1]) @ t["weights"] + t["biases"]
    rows = z.shape[0]
    mm = mv = None
    if bn:
        mean = z.mean(dim=0)
        var = ((z - mean) ** 2).mean(dim=0)
        z.retain_grad()
        pre = z
        z = (z - mean) / torch.sqrt(var + 1e-3) * t["gamma"] + t["beta"]
        keep = 1 - float(np.float32(decay))
        mm = t["moving_mean"] - (t["moving_mean"] - mean) * keep
        mv = t["moving_variance"] - (t["moving_variance"] - var * (rows / max(rows - 1, 1) if unbiased else 1.0)) * keep
    y = {"relu": torch.relu, "sigmoid": torch.sigmoid, None: lambda a: a}[activation](z)
    return xt, t, y, (pre if bn else None), mm, mv


WRAPPERS = [("conv2d", (2, 37, 5, 9), 33, "relu", True), ("conv2d", (2, 40, 1, 16), 64, None, True),
            ("conv1d", (3, 211, 12), 20, "relu", True), ("fully_connected", (64, 40), 32, "relu", True),
            ("fully_connected", (9, 24), 7, "sigmoid", True), ("conv1d", (2, 50, 8), 5, "relu", False)]


@pytest.mark.parametrize("kind,shape,cout,activation,bn", WRAPPERS)
def test_wrapper_in_training_mode(T, launches, kind, shape, cout, activation, bn):
    rng = np.random.default_rng([len(shape), cout])
    x = rng.standard_normal(shape).astype(np.float32)
    gy = rng.standard_normal(shape[:-1] + (cout,)).astype(np.float32)
    decay = 0.25
    st = T.set_store(T.VariableStore(seed=5, randomize_bn=True))

    def call(inp, is_training):
        kw = dict(scope="lay", bn=bn, bn_decay=decay, is_training=is_training, activation_fn=activation)
        if kind == "conv2d":
            return T.conv2d(inp, cout, [1, 1], padding='VALID', stride=[1, 1], **kw)
        if kind == "conv1d":
            return T.conv1d(inp, cout, 1, padding='VALID', **kw)
        return T.fully_connected(inp, cout, **kw)

    with torch.no_grad():
        call(torch.from_numpy(x).cuda(), False)  # creates the variables
    v = {n.split("lay/")[1].replace("bn/", ""): t.cpu().numpy().copy() for n, t in st.vars.items()}
    tr = st.trainable()
    assert set(n.split("/")[-1] for n in tr) == ({"weights", "biases", "gamma", "beta"} if bn else {"weights", "biases"})
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    del launches[:]
    y = call(xd, True)
    y.backward(torch.from_numpy(gy).cuda())
    if bn:
        assert "pasnl_cls_bn_train" in launches and "pasnl_cls_bn_train_grad" in launches
    assert not folded_launches(launches)
    unbiased = T._bn_unbiased(len(shape))
    assert unbiased == (kind != "conv1d")
    ref = {}
    for dtype in (torch.float64, torch.float32):
        xt, t, yy, pre, mm, mv = restate(x, v, activation, bn, unbiased, decay, dtype)
        yy.backward(torch.tensor(gy, dtype=dtype).reshape(yy.shape))
        ref[dtype] = dict(y=yy.detach().numpy().reshape(gy.shape), x=xt.grad.numpy(), mm=None if mm is None else mm.detach().numpy(),
                          mv=None if mv is None else mv.detach().numpy(), cancel=None if pre is None else pre.grad.abs().sum(0).numpy(),
                          **{k: a.grad.numpy() for k, a in t.items() if a.grad is not None})
    r64, r32 = ref[torch.float64], ref[torch.float32]
    got = dict(y=y.detach().cpu().numpy(), x=xd.grad.cpu().numpy(), **{n.split("/")[-1]: p.grad.cpu().numpy() for n, p in tr.items()})
    if bn:
        got["mm"], got["mv"] = st.vars["lay/bn/moving_mean"].cpu().numpy(), st.vars["lay/bn/moving_variance"].cpu().numpy()
    for name in got:
        scale = float(r64["cancel"].max()) if (bn and name == "biases") else None
        e, ec = err(got[name], r64[name], scale), err(r32[name], r64[name], scale)
        print(f"{kind} {name}: err {e:.3g} (chain {ec:.3g})")
        assert np.isfinite(got[name]).all() and e <= allowed(ec), name
    if bn:  # the rank rule is visible: the other choice of `unbiased` misses the moving variance
        other = restate(x, v, activation, bn, not unbiased, decay, torch.float64)[5].detach().numpy()
        assert err(got["mv"], other) > 10 * allowed(err(r32["mv"], r64["mv"]))

    # ---- the stale-cache test: an in-place SGD step, then the same wrapper at inference folds the NEW variables and statistics
    with torch.no_grad():
        for p in tr.values():
            p.sub_(0.5 * p.grad)
        out = call(torch.from_numpy(x).cuda(), False).cpu().numpy()
    n = {k.split("lay/")[1].replace("bn/", ""): t.detach().double().cpu() for k, t in st.vars.items()}
    w, b = n["weights"], n["biases"]
    if bn:
        s = n["gamma"] / torch.sqrt(n["moving_variance"] + 1e-3)
        w, b = w * s, (b - n["moving_mean"]) * s + n["beta"]
    z = torch.from_numpy(x).double().reshape(-1, shape[-1]) @ w + b
    want = {"relu": torch.relu, "sigmoid": torch.sigmoid, None: lambda a: a}[activation](z).numpy().reshape(out.shape)
    assert err(out, want) <= 1e-5
    assert err(out, got["y"]) > 1e-3  # (and that is not what the layer computed before)


def test_is_training_as_a_tensor_is_a_type_error(T):
    T.set_store(T.VariableStore(seed=5))
    x = torch.zeros((4, 8), device="cuda")
    for flag in (torch.tensor(True), torch.tensor(True).cuda()):
        with pytest.raises(TypeError):
            T.fully_connected(x, 4, scope="fc", bn=True, is_training=flag)
        with pytest.raises(TypeError):
            T.conv1d(x[None], 4, 1, scope="c1", bn=True, is_training=flag)
        with pytest.raises(TypeError):
            T.conv2d(x[None, None], 4, [1, 1], scope="c2", bn=True, is_training=flag)
    with pytest.raises(NotImplementedError):
        T.dropout(x, True, "dp", noise_shape=[4, 1])


# ---------------------------------------------------------------------------------------------------------------------------
# layers and models: fused route against the torch route
# ---------------------------------------------------------------------------------------------------------------------------
def three_routes(T, st, run):
    """run() -> (outputs dict, loss) is called under: the fused route; the torch route in float32; the torch route with float64
    statistics -- each from the same variables, moving statistics and dropout address -> {route: {name: numpy}}"""
    moving0 = {n: t.clone() for n, t in st.vars.items() if "moving_" in n}
    tr = st.trainable()
    res = {}
    for route, fused, dtype in (("fused", True, None), ("torch", False, None), ("torch64", False, torch.float64)):
        with torch.no_grad():
            for n, t in moving0.items():
                st.vars[n].copy_(t)
        for p in tr.values():
            p.grad = None
        st.dropout_calls = 0
        T.BN_TRAIN_FUSED, T.BN_TRAIN_TORCH_DTYPE = fused, dtype
        try:
            outs, loss = run()
            loss.backward()
        finally:
            T.BN_TRAIN_FUSED, T.BN_TRAIN_TORCH_DTYPE = True, None
        torch.cuda.synchronize()
        r = {"out/" + k: v.detach().cpu().numpy() for k, v in outs.items()}
        r.update({"grad/" + n: (None if p.grad is None else p.grad.cpu().numpy()) for n, p in tr.items()})
        r.update({"stat/" + n: st.vars[n].cpu().numpy() for n in moving0})
        res[route] = r
    return res, moving0


def compare_routes(res, what):
    """the fused route within 4 x the torch route's own float32 noise, per quantity (outputs; the gradients of weights / gamma /
    beta; the gradients of biases, relative to their layer's beta gradient; the moving statistics); -> the figures"""
    # a gradient that is zero in exact arithmetic -- a bias in front of a batch norm, or a beta whose shift a later batch norm
    # removes again (the non-local cell's keys|values, a group_all module's last layer in front of fc1) -- is rounding residue in
    # every route: it is measured against 1e-4 of the model's largest gradient, never against itself
    floor = 1e-4 * max(np.abs(v).max() for n, v in res["torch64"].items() if n.startswith("grad/") and v is not None)

    def scale_of(name):
        if not name.startswith("grad/"):
            return None
        scale = np.abs(res["torch64"][name]).max()
        if name.endswith("/biases"):
            beta = name[:-len("biases")] + "bn/beta"
            if res["torch64"].get(beta) is not None:
                scale = np.abs(res["torch64"][beta]).max()
        return max(scale, floor)

    figures = {}
    for name, want in res["torch64"].items():
        if want is None:
            assert res["fused"][name] is None, name
            continue
        kind = name.split("/")[0] + ("/biases" if name.endswith("/biases") else "")
        e = err(res["fused"][name], want, scale_of(name))
        noise = err(res["torch"][name], want, scale_of(name))
        assert np.isfinite(res["fused"][name]).all(), name
        f = figures.setdefault(kind, [0.0, 0.0])
        if e > 2e-3 or noise > 2e-3:
            print(f"    {name}: fused {e:.3g}, noise {noise:.3g}, scale {np.abs(want).max():.3g}")
        f[0], f[1] = max(f[0], e), max(f[1], noise)
    for kind, (e, noise) in figures.items():
        print(f"{what} {kind}: fused {e:.3g}, torch-route noise {noise:.3g}")
    for kind, (e, noise) in figures.items():
        assert e <= max(4 * noise, 1e-5), (what, kind, e, noise)
    return figures


def cloud(b, n, seed=0):
    rng = np.random.default_rng(seed)
    pc = rng.standard_normal((b, n, 3)).astype(np.float32)
    return torch.from_numpy(pc / np.abs(pc).max()).cuda()


def test_cls_model_in_training_mode(T, launches):
    """Figures at B = 8, N = 1024 on MI355X (err of the fused route / the torch route's own float32 noise, both against the torch
    route with float64 statistics): logits 3.0e-6 / 4.2e-6, moving statistics 1.8e-6 / 1.8e-6, gradients 1e-4 to 8e-4 in both
    (largest 5.4e-3 / 5.4e-3 at layer3_2/conv1/bn/beta: ReLU sign changes among 1e8 pre-activations, the same in both float32
    routes); gradients that are zero in exact arithmetic are residue of 1e-8 to 7e-7 in both.  EXPERIMENTS.md, "Training mode"."""
    from pointasnl_amd.models import pointasnl_cls

    st = T.set_store(T.VariableStore(seed=3, randomize_bn=True))
    x = cloud(8, 1024)
    label = torch.arange(8, device="cuda") % 40
    with torch.no_grad():
        before, _ = pointasnl_cls.get_model(x, is_training=False)      # creates the variables (the fused inference path)
    assert folded_launches(launches)
    tr = st.trainable()
    assert len(tr) > 60

    def run():
        logits, ep = pointasnl_cls.get_model(x, is_training=True, bn_decay=0.5)
        return dict(logits=logits), torch.nn.functional.cross_entropy(logits, label)

    del launches[:]
    res, moving0 = three_routes(T, st, run)
    assert not folded_launches(launches), folded_launches(launches)
    assert "pasnl_cls_bn_train" in launches and "pasnl_cls_bn_train_grad" in launches and "pasnl_cls_dropout" in launches
    f = res["fused"]
    for n in tr:
        g = f["grad/" + n]
        assert g is not None and np.isfinite(g).all(), n
        # (a bias in front of a batch norm has a zero gradient in exact arithmetic: only rounding residue reaches it)
        if not (n.endswith("/biases") and n[:-len("biases")] + "bn/beta" in tr):
            assert np.abs(g).max() > 0, n
    for n, t in moving0.items():
        assert not np.array_equal(f["stat/" + n], t.cpu().numpy()), n   # every layer on the route took batch statistics
    assert f["out/logits"].shape == (8, 40)
    compare_routes(res, "cls")

    # the mask is a function of the counter: another dropout_calls, other logits
    st.dropout_calls = 7
    with torch.no_grad():
        other, _ = pointasnl_cls.get_model(x, is_training=True, bn_decay=1.0)   # (decay 1: the statistics stay)
    assert not np.array_equal(other.cpu().numpy(), f["out/logits"])

    # inference again: the unchanged fused path, on the UPDATED statistics -- what a fresh store loaded with them computes
    del launches[:]
    with torch.no_grad():
        after, _ = pointasnl_cls.get_model(x, is_training=False)
    assert folded_launches(launches)
    fresh = T.set_store(T.VariableStore(seed=0)).load({n: t.detach().cpu().numpy() for n, t in st.vars.items()})
    with torch.no_grad():
        want, _ = pointasnl_cls.get_model(x, is_training=False)
    assert torch.equal(after, want) and not torch.equal(after, before)


def test_decoding_layer_and_residual_layer_in_training_mode(T, launches):
    from pointasnl_amd.utils import pointasnl_util as U

    st = T.set_store(T.VariableStore(seed=8, randomize_bn=True))
    rng = np.random.default_rng(4)
    xyz1, xyz2 = cloud(2, 256, 1), cloud(2, 64, 2)
    # the shapes of pointasnl_sem_seg's fa_layer4 (coordinates as points1, 128 coarse channels, 16 neighbours) and of
    # pointasnl_sem_seg_res's layer1_2 (32 channels in, mlp [64, 64], no non-local cell, a residual), on small clouds
    p2 = torch.from_numpy(rng.standard_normal((2, 64, 128)).astype(np.float32)).cuda()
    f32 = torch.from_numpy(rng.standard_normal((2, 256, 32)).astype(np.float32)).cuda()
    prev = torch.from_numpy(rng.standard_normal((2, 64, 64)).astype(np.float32)).cuda()

    def layers(is_training):
        dec = U.PointASNLDecodingLayer(xyz1, xyz2, xyz1, p2, 16, [128, 128], is_training, 0.5, None, scope='fa')
        _, res = U.PointASNLSetAbstraction(xyz1, f32, npoint=64, nsample=32, mlp=[64, 64], is_training=is_training, bn_decay=0.5,
                                           weight_decay=None, scope='res_2', as_neighbor=0, NL=False, residual=prev)
        return dec, res

    with torch.no_grad():
        layers(False)
    assert folded_launches(launches)

    def run():
        dec, res = layers(True)
        return dict(dec=dec, res=res), (dec * dec).mean() + (res * res).mean()

    del launches[:]
    res, moving0 = three_routes(T, st, run)
    assert not folded_launches(launches), folded_launches(launches)
    assert res["fused"]["out/dec"].shape == (2, 256, 128) and res["fused"]["out/res"].shape == (2, 64, 64)
    for n, t in moving0.items():
        assert not np.array_equal(res["fused"]["stat/" + n], t.cpu().numpy()), n
    compare_routes(res, "decoder + residual layer")


def test_sem_seg_model_in_training_mode(T, launches):
    """once, at B = 2 and N = 4096 (layer 4 keeps N / 256 points and takes 32 neighbours among layer 3's N / 128)"""
    from pointasnl_amd.models import pointasnl_sem_seg

    st = T.set_store(T.VariableStore(seed=6))
    x = cloud(2, 4096, 3)
    label = (torch.arange(2 * 4096, device="cuda") % 13).reshape(2, 4096)
    with torch.no_grad():
        logits, _ = pointasnl_sem_seg.get_model(x, True, 13, bn_decay=0.9)   # creates the variables, in training mode itself
    tr = st.trainable()
    del launches[:]
    logits, ep = pointasnl_sem_seg.get_model(x, True, 13, bn_decay=0.9)
    torch.nn.functional.cross_entropy(logits.reshape(-1, 13), label.reshape(-1)).backward()
    torch.cuda.synchronize()
    assert not folded_launches(launches), folded_launches(launches)
    assert logits.shape == (2, 4096, 13) and ep['feats'].shape == (2, 4096, 128) and torch.isfinite(logits).all()
    for n, p in tr.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
