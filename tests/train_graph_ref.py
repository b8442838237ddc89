"""The training graph of the layers, cells, heads and of the classifier, restated on torch CPU tensors in a dtype of choice
(torch.float64: the reference; torch.float32: the yardstick of float32's own noise).  Written from the formulas and from this
project's oracle/cells.py (the numpy restatement of the inference graph, pinned to the golden fixtures), the way
tests/sa_grad_ref.py and tests/bn_train_ref.py are; torch differentiates it.  No pointasnl_amd import: nothing of the product is
shared -- not a branch, not a reshape, not the rank a layer presents to the Bessel rule.

    layer()   GEMM, bias, batch norm, activation.  train=True: the batch's mean and biased variance over all leading axes, eps 1e-3,
              and the new moving statistics m - (m - batch) * (1 - float32(decay)); the variance fed to the moving average is
              Bessel-corrected for the kinds "conv2d" and "fc" and not for "conv1d" -- `kind` names the reference's wrapper, which the
              CALLER states (skip, aggregation and the segmentation heads are conv1d; everything else conv2d; the classifier's
              head is fc), never the rank of the tensor at hand.
    Graph     the variables as leaves, the cells (sample_weights, adaptive_sampling, nonlocal_cell, set_abstraction,
              decoding_layer, fp_module, sa_group_all), the three heads and cls_model.  Discrete decisions (neighbour lists, three_nn,
              dropout keep masks) are GIVEN.  Every batch-normed call records its scope's kind, its update count, its new moving
              statistics and the column moments of its normalised pre-activations.
    cases     LAYER_CASES / MODEL_CASES, their seeded inputs, and run_case(): one case on a Graph -> outputs and the loss.  Shared
              by tests/test_train_graph_flow.py (CPU: the restatement against the oracle, and mutants of it against itself) and
              tests/test_gpu_training_graph.py (GPU: the product against it).

Scopes nest as the store names them: a cell re-opens the scope it was handed (oracle/cells.py _join), so the variables of layer1's
non-local cell live under layer1/layer1/conv_kv and those of its SampleWeights under layer1/layer1/layer1/conv_kv_ds."""
import hashlib
import math

import numpy as np
import torch

BN_EPS = 1e-3
BESSEL_KINDS = ("conv2d", "fc")
DECAY = 0.5


def _act(y, act):
    if act is None:
        return y
    if act == "relu":
        return torch.relu(y)
    if act == "sigmoid":
        return torch.sigmoid(y)
    if act == "leaky_relu":
        return torch.where(y > 0, y, y * 0.2)
    raise ValueError(act)


def moving_update(m, batch, decay):
    """assign_moving_average(zero_debias=False), the decay as the float32 the layer receives"""
    return m - (m - batch) * (1.0 - float(np.float32(decay)))


def layer(x, p, act, kind, train, decay):
    """x (..., cin), p = {"w","b"[,"gamma","beta","mean","var"]} of tensors -> (y, stats); stats is None without batch norm or with
    train=False, else dict(mean, var: the NEW moving statistics; batch_mean, batch_var: what the moving averages were fed;
    xhat_mean, xhat_var: the column moments of the normalised pre-activations; biased_var)"""
    if kind not in ("conv1d", "conv2d", "fc"):
        raise ValueError(kind)
    z = x @ p["w"] + p["b"]
    if "gamma" not in p:
        return _act(z, act), None
    if not train:
        return _act((z - p["mean"]) / torch.sqrt(p["var"] + BN_EPS) * p["gamma"] + p["beta"], act), None
    z2 = z.reshape(-1, z.shape[-1])
    rows = z2.shape[0]
    mean = z2.mean(dim=0)
    var = ((z2 - mean) ** 2).mean(dim=0)
    xhat = (z - mean) / torch.sqrt(var + BN_EPS)
    fed = var * (rows / max(rows - 1, 1)) if kind in BESSEL_KINDS else var
    with torch.no_grad():
        xh = xhat.reshape(-1, z.shape[-1])
        stats = dict(mean=moving_update(p["mean"], mean, decay), var=moving_update(p["var"], fed, decay), batch_mean=mean.clone(),
                     batch_var=fed.clone(), biased_var=var.clone(), xhat_mean=xh.mean(dim=0),
                     xhat_var=((xh - xh.mean(dim=0)) ** 2).mean(dim=0), rows=rows)
    return _act(xhat * p["gamma"] + p["beta"], act), stats


def _join(outer, scope):
    return scope if not outer else outer + "/" + scope


def gather(points, idx):
    """points (B,N,C), idx (B,...) int64 -> (B,...,C)"""
    b = torch.arange(points.shape[0]).reshape((-1,) + (1,) * (idx.dim() - 1))
    return points[b, idx]


def seeded_variable(seed, full, shape, kind):
    """the value a VariableStore(seed) draws for the variable `full` (its own generator, restated: a stream per (seed, name))"""
    h = hashlib.sha256(f"{int(seed)}:{full}".encode()).digest()
    rng = np.random.Generator(np.random.PCG64(int.from_bytes(h[:8], "little")))
    if kind == "xavier":
        lim = math.sqrt(6.0 / (shape[0] + shape[1]))
        v = rng.uniform(-lim, lim, size=shape)
    elif kind == "small":
        v = rng.uniform(-0.2, 0.2, size=shape)
    elif kind == "positive":
        v = rng.uniform(0.5, 1.5, size=shape)
    else:
        raise ValueError(kind)
    return v.astype(np.float32)


def seeded_scope(seed, scope, cin, cout, bn):
    """one scope's {"w","b"[,"gamma","beta","mean","var"]} as VariableStore(seed, randomize_bn=True) creates it"""
    p = {"w": seeded_variable(seed, scope + "/weights", (cin, cout), "xavier"), "b": seeded_variable(seed, scope + "/biases", (cout,), "small")}
    if bn:
        for key, name, kind in (("gamma", "gamma", "positive"), ("beta", "beta", "small"), ("mean", "moving_mean", "small"),
                                ("var", "moving_variance", "positive")):
            p[key] = seeded_variable(seed, scope + "/bn/" + name, (cout,), kind)
    return p


TRAINED = {"w": "weights", "b": "biases", "gamma": "bn/gamma", "beta": "bn/beta"}
MOVING = {"mean": "bn/moving_mean", "var": "bn/moving_variance"}


class Graph:
    """params: scope -> {"w",...} of numpy arrays (oracle.cells.params_from_tf / VariableStore.export_numpy), or None with `seed`:
    every scope is then drawn on first use as VariableStore(seed, randomize_bn=True) draws it (`numpy_params` holds them)."""

    def __init__(self, params=None, dtype=torch.float64, train=True, decay=DECAY, seed=None):
        self.dtype, self.train, self.decay, self.seed = dtype, bool(train), decay, seed
        self.numpy_params = {} if params is None else params
        self.lazy = params is None
        self.p = {}        # scope -> tensors; the trained ones are leaves
        self.stat = {}     # scope -> {"mean","var"}: the moving statistics as they stand
        self.kinds = {}    # scope -> kind, of every layer called
        self.updates = {}  # scope -> how often its moving statistics were updated
        self.norm = {}     # scope -> the stats of layer() at the scope's last call
        self.maxima = {}   # tag -> (the tensor a maximum was taken of, the axis)

    # ---- variables
    def tensor(self, a, grad=False):
        return torch.tensor(np.asarray(a), dtype=self.dtype).requires_grad_(grad)

    def variables(self, scope, cin, cout, bn):
        if scope not in self.p:
            if scope not in self.numpy_params:
                if not self.lazy:
                    raise KeyError(f"the restatement asks for the variables of '{scope}', which the store does not hold")
                self.numpy_params[scope] = seeded_scope(self.seed, scope, cin, cout, bn)
            src = self.numpy_params[scope]
            if ("gamma" in src) != bool(bn) or tuple(src["w"].shape) != (cin, cout):
                raise ValueError(f"'{scope}': stored {tuple(src['w'].shape)}, bn {'gamma' in src}; the graph needs {(cin, cout)}, bn {bn}")
            self.p[scope] = {k: self.tensor(a, k in TRAINED) for k, a in src.items()}
            if bn:
                self.stat[scope] = {k: self.p[scope][k].detach().clone() for k in MOVING}
        return self.p[scope]

    def trainable(self):
        """{the store's name: leaf} of every variable of a scope the graph used"""
        return {sc + "/" + TRAINED[k]: t for sc, p in self.p.items() for k, t in p.items() if k in TRAINED}

    def moving(self):
        """{the store's name: value after the step}"""
        return {sc + "/" + MOVING[k]: t for sc, s in self.stat.items() for k, t in s.items()}

    # ---- one layer
    def layer(self, x, scope, cout, act, kind, bn=True):
        p = self.variables(scope, x.shape[-1], cout, bn)
        if bn:
            p = dict(p, **self.stat[scope])
        y, stats = layer(x, p, act, kind, self.train, self.decay)
        self.kinds[scope] = kind
        if stats is not None:
            self.stat[scope] = {"mean": stats["mean"], "var": stats["var"]}
            self.updates[scope] = self.updates.get(scope, 0) + 1
            self.norm[scope] = stats
        return y

    def amax(self, x, dim, tag):
        """a maximum over an axis, its gradient shared among ties (tf.reduce_max); the operand is kept for undecided_maxima()"""
        self.maxima[tag] = (x.detach(), dim)
        return x.amax(dim=dim)

    # ---- the places a mutant changes (tests/test_train_graph_flow.py)
    def window(self, m):
        """the [1, C'] VALID convolution's window: (B,P,C',32) row-major -> (B,P,C'*32)"""
        return m.reshape(m.shape[0], m.shape[1], -1)

    def centres(self, new_xyz):
        """the sampled coordinates AdaptiveSampling returns, as the rest of the layer sees them"""
        return new_xyz

    def pooled_concat(self, top, res):
        return torch.cat([top, res], dim=-1)

    # ---- cells
    def sample_weights(self, new_point, grouped_xyz, mlps, scope, outer=""):
        """new_point (B,P,as,ch), grouped_xyz (B,P,as,3) -> (B,P,as,mlps[-1]), softmax over the neighbours"""
        scope = _join(outer, scope)
        cb = max(32, new_point.shape[-1] // 2)
        x = torch.cat([grouped_xyz - grouped_xyz[:, :, :1, :], new_point], dim=-1)
        kv = self.layer(x, scope + "/conv_kv_ds", 2 * cb, None, "conv2d")
        q = self.layer(x, scope + "/conv_query_ds", cb, None, "conv2d")
        k, v = kv[..., :cb], kv[..., cb:]
        w = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(cb), dim=-1)
        g = w @ v
        for i, c in enumerate(mlps):
            g = self.layer(g, scope + "/mlp2_%d" % i, c, "relu" if i < len(mlps) - 1 else None, "conv2d")
        return torch.softmax(g, dim=2)

    def adaptive_sampling(self, group_xyz, group_feature, num_neighbor, scope, outer=""):
        path = _join(outer, scope)
        if num_neighbor == 0:
            return group_xyz[:, :, 0, :], group_feature[:, :, 0, :]
        sxyz, sfeat = group_xyz[:, :, :num_neighbor, :], group_feature[:, :, :num_neighbor, :]
        w = self.sample_weights(sfeat, sxyz, [32, 1 + group_feature.shape[-1]], scope, outer=path)
        return (sxyz * w[..., :1]).sum(dim=2), (sfeat * w[..., 1:]).sum(dim=2)

    def nonlocal_cell(self, feature, new_point, mlp, scope, outer=""):
        """feature (B,N,C), new_point (B,P,C') -> (B,P,mlp[-1])"""
        scope = _join(outer, scope)
        cb = mlp[0]
        kv = self.layer(feature, scope + "/conv_kv", 2 * cb, None, "conv2d")
        q = self.layer(new_point, scope + "/conv_query", cb, None, "conv2d")
        k, v = kv[..., :cb], kv[..., cb:]
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(cb), dim=-1)
        return self.layer(att @ v, scope + "/conv_back_project", mlp[-1], "relu", "conv2d")

    def set_abstraction(self, xyz, feature, idx, mlp, scope, as_neighbor=8, NL=True, residual=None):
        """xyz (B,N,3), feature (B,N,C), idx (B,P,K) -> new_xyz (B,P,3), new_point (B,P,mlp[-1]); P == N: no sampling"""
        n, c = feature.shape[1:]
        p = idx.shape[1]
        grouped_xyz = gather(xyz, idx)
        new_point = torch.cat([grouped_xyz, gather(feature, idx)], dim=-1)
        if n == p:
            new_xyz, new_feature = xyz, feature
        else:
            new_xyz, new_feature = self.adaptive_sampling(grouped_xyz, new_point, as_neighbor, scope, outer=scope)
            if as_neighbor > 0:
                new_xyz = self.centres(new_xyz)
        grouped_xyz = grouped_xyz - new_xyz[:, :, None, :]
        new_point = torch.cat([grouped_xyz, new_point], dim=-1)
        if NL:
            nonlocal_pt = self.nonlocal_cell(feature, new_feature, [max(32, c // 2), mlp[-1]], scope, outer=scope)
        skip = self.layer(self.amax(new_point, 2, scope + "/skip"), scope + "/skip", mlp[-1], "relu", "conv1d")
        for i in range(len(mlp) - 1):
            new_point = self.layer(new_point, scope + "/conv%d" % i, mlp[i], "relu", "conv2d")
        weight = self.layer(grouped_xyz, scope + "/weight_net/wconv0", 32, "relu", "conv2d")
        new_point = new_point.transpose(2, 3) @ weight  # (B,P,C',32)
        new_point = self.layer(self.window(new_point), scope + "/after_conv", mlp[-1], "relu", "conv2d")
        new_point = new_point + skip
        if NL:
            new_point = new_point + nonlocal_pt
        new_point = self.layer(new_point, scope + "/aggregation", mlp[-1], "relu", "conv1d")
        return new_xyz, (new_point if residual is None else new_point + residual)

    def three_interpolate(self, points2, nn):
        """nn = (dist (B,N1,3) float32 squared distances, idx (B,N1,3)): the weights are taken from dist in the graph's dtype"""
        dist, idx = nn
        d = torch.clamp(torch.as_tensor(np.asarray(dist)).to(self.dtype), min=1e-10)
        w = (1.0 / d) / (1.0 / d).sum(dim=2, keepdim=True)
        g = gather(points2, torch.as_tensor(np.asarray(idx), dtype=torch.int64))
        return (g[:, :, 0] * w[:, :, 0:1] + g[:, :, 1] * w[:, :, 1:2]) + g[:, :, 2] * w[:, :, 2:3]

    def decoding_layer(self, xyz1, points1, points2, nn, kidx, mlp, scope):
        """xyz1 (B,N1,3), points1 (B,N1,C1) or None, points2 (B,N2,C2), kidx (B,N1,K) the self-kNN of xyz1 -> (B,N1,mlp[-1])"""
        interpolated = self.three_interpolate(points2, nn)
        grouped_xyz = gather(xyz1, kidx)
        grouped_feature = torch.cat([grouped_xyz, gather(interpolated, kidx)], dim=-1)
        grouped_xyz = grouped_xyz - xyz1[:, :, None, :]
        weight = self.layer(grouped_xyz, scope + "/decode_weight_net/wconv0", 32, "relu", "conv2d")
        x = grouped_feature.transpose(2, 3) @ weight
        x = self.layer(self.window(x), scope + "/decode_after_conv", mlp[0], "relu", "conv2d")
        if points1 is not None:
            x = torch.cat([x, points1], dim=-1)
        for i in range(1, len(mlp)):
            x = self.layer(x, scope + "/conv_%d" % i, mlp[i], "relu", "conv2d")
        return x

    def fp_module(self, points1, points2, nn, mlp, scope):
        x = self.three_interpolate(points2, nn)
        if points1 is not None:
            x = torch.cat([x, points1], dim=2)
        for i in range(len(mlp)):
            x = self.layer(x, scope + "/conv_%d" % i, mlp[i], "relu", "conv2d")
        return x

    def sa_group_all(self, xyz, points, mlp, scope):
        """concat, three convolutions, the maximum over the cloud (amax: its gradient is shared among ties) -> (B,mlp[-1])"""
        x = torch.cat([xyz, points], dim=2)
        for i in range(len(mlp)):
            x = self.layer(x, scope + "/conv%d" % i, mlp[i], "relu", "conv2d")
        return self.amax(x, 1, scope)

    # ---- heads
    def dropout(self, x, mask, keep_prob):
        """mask: bool keep mask of x's elements in row-major order (given); identity at inference"""
        if not self.train:
            return x
        keep = torch.as_tensor(np.asarray(mask).reshape(tuple(x.shape))).to(self.dtype)
        return x * keep * (1.0 / keep_prob)

    def cls_head(self, net, masks, num_class=40):
        net = self.layer(net, "fc1", 512, "relu", "fc")
        net = self.dropout(net, masks.get("dp1"), 0.4)
        net = self.layer(net, "fc2", 256, "relu", "fc")
        net = self.dropout(net, masks.get("dp2"), 0.4)
        return self.layer(net, "fc3", num_class, None, "fc", bn=False)

    def sem_seg_head(self, x, masks, num_class=13):
        net = self.layer(x, "fc1", 128, "relu", "conv1d")
        net = self.dropout(net, masks.get("dp1"), 0.5)
        return self.layer(net, "fc2", num_class, None, "conv1d", bn=False)

    def sem_seg_res_head(self, x, masks, num_class=13):
        net = self.layer(x, "fc1", 128, "leaky_relu", "conv1d")
        net = self.dropout(net, masks.get("dp"), 0.5)
        return self.layer(net, "fc0", num_class, None, "conv1d", bn=False)

    def cls_model(self, point_cloud, decisions, adaptive_sample=False, masks=None):
        """decisions: {"layer1": idx (B,512,32), "layer2": idx (B,128,64)}, or a callable (scope, xyz) -> idx asked when the level's
        coordinates exist; masks: {"dp1","dp2"} -> (logits, end_points)"""
        pick = decisions if callable(decisions) else (lambda scope, xyz: decisions[scope])
        as_neighbor = 12 if adaptive_sample else 0
        ix = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int64)
        l1_xyz, l1_points = self.set_abstraction(point_cloud, point_cloud, ix(pick("layer1", point_cloud)), [64, 64, 128], "layer1", as_neighbor)
        l2_xyz, l2_points = self.set_abstraction(l1_xyz, l1_points, ix(pick("layer2", l1_xyz)), [128, 128, 256], "layer2", as_neighbor)
        res = self.sa_group_all(l1_xyz, l1_points, [128, 256, 512], "layer3_1")
        top = self.sa_group_all(l2_xyz, l2_points, [256, 512, 1024], "layer3_2")
        logits = self.cls_head(self.pooled_concat(top, res), masks or {})
        return logits, {"l1_xyz": l1_xyz, "l2_xyz": l2_xyz, "l1_points": l1_points, "l2_points": l2_points}


def xent(logits, labels):
    """mean softmax cross-entropy"""
    z = logits - logits.amax(dim=-1, keepdim=True)
    lse = torch.log(torch.exp(z).sum(dim=-1))
    return (lse - z.gather(-1, torch.as_tensor(np.asarray(labels), dtype=torch.int64)[..., None])[..., 0]).mean()


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: B = 2 (batch statistics over more than one cloud), the smallest shapes that still take each branch
# ---------------------------------------------------------------------------------------------------------------------------
LAYER_CASES = {
    # neighbour-0 centres through group_point, the narrow non-local cell (cb = 32), the after_conv window
    "sa_xyz_as0": dict(kind="sa", seed=21, n=128, p=32, c=3, k=32, mlp=[16, 16, 32], as_neighbor=0, NL=True),
    # AdaptiveSampling in training: the gradient through new_xyz and new_feature
    "sa_c32_as8": dict(kind="sa", seed=22, n=128, p=32, c=32, k=32, mlp=[32, 32, 64], as_neighbor=8, NL=True),
    # the classifier's form of it (mlp2_1 is 1 + 3 + C wide), the non-local cell kept off the input-space kernel
    "sa_xyz_as12": dict(kind="sa", seed=23, n=96, p=24, c=3, k=32, mlp=[64, 64, 128], as_neighbor=12, NL=True, nl_input_space=False),
    # npoint == ndataset, the one-convolution cell, the residual sum
    "sa_full_residual": dict(kind="sa", seed=24, n=64, p=64, c=32, k=32, mlp=[64, 64], as_neighbor=0, NL=False, residual=True),
    # cb = 80: the attention's fallback chain behind two training convolutions
    "sa_c160_as4": dict(kind="sa", seed=25, n=128, p=32, c=160, k=32, mlp=[64, 64, 128], as_neighbor=4, NL=True),
    "decode": dict(kind="decode", seed=26, n1=128, n2=32, c1=32, c2=64, k=16, mlp=[64, 64]),
    "decode_no_points1": dict(kind="decode", seed=27, n1=128, n2=32, c1=0, c2=64, k=16, mlp=[64, 64]),
    "fp": dict(kind="fp", seed=28, n1=128, n2=32, c1=32, c2=64, mlp=[64, 32, 32]),
    "group_all": dict(kind="group_all", seed=29, n=64, c=32, mlp=[32, 64, 128], xyz_concat=False),
    "group_all_xyz_concat": dict(kind="group_all", seed=30, n=64, c=32, mlp=[32, 64, 128], xyz_concat=True),
    "head_cls": dict(kind="head_cls", seed=31, shape=(8, 1536), num_class=40),
    "head_sem_seg": dict(kind="head_sem_seg", seed=32, shape=(2, 64, 128), num_class=13),
    "head_sem_seg_res": dict(kind="head_sem_seg_res", seed=33, shape=(2, 64, 128), num_class=13),
}
# The seeds of the model cases are the first from 41 (42) on at which every maximum of the two group_all poolings is decided in
# the float64 restatement (undecided_maxima below, a condition on the restatement alone; tests/test_train_graph_flow.py asserts
# it).  Such a maximum carries the whole gradient of one pooled feature of one cloud into one of 512 / 128 rows; at seed 41 one of
# layer3_2's 4096 has its two largest candidates 1.4e-8 of their value apart, less than float32 resolves, and a float32
# implementation that takes the other one is 14 % off in layer3_2/conv2's weight gradient without being wrong (EXPERIMENTS.md).
# The skip connections' maxima (about 70 000 per case, a handful of them as close) are not asked to be decided: one of them moves
# one element of a (B * P, C) gradient to a neighbouring row, the size of event a ReLU sign change is, which err_chain holds.
POOLINGS = ("layer3_1", "layer3_2")
MODEL_CASES = {
    "cls": dict(kind="cls", seed=57, b=4, n=1024, adaptive_sample=False),
    "cls_adaptive": dict(kind="cls", seed=42, b=4, n=1024, adaptive_sample=True),
}
CASES = dict(LAYER_CASES, **MODEL_CASES)
B = 2
# the dropout layers of a head: (scope, keep_prob, the layer whose output it masks), in call order
DROPOUTS = {"head_cls": (("dp1", 0.4, 512), ("dp2", 0.4, 256)), "cls": (("dp1", 0.4, 512), ("dp2", 0.4, 256)),
            "head_sem_seg": (("dp1", 0.5, 128),), "head_sem_seg_res": (("dp", 0.5, 128),)}


def ball(rng, b, n):
    v = rng.standard_normal((b, n, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return (v * rng.random((b, n, 1)) ** (1 / 3)).astype(np.float32)


def case_inputs(name):
    """float32 numpy inputs of a case: what requires a gradient under its own name, the loss weights as g_*"""
    case = CASES[name]
    rng = np.random.default_rng(case["seed"])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    kind = case["kind"]
    if kind == "sa":
        inp = {"xyz": ball(rng, B, case["n"])}
        if case["c"] != 3:  # (c == 3: the features ARE the coordinates, one tensor, as in every model's first layer)
            inp["feature"] = f(B, case["n"], case["c"])
        if case.get("residual"):
            inp["residual"] = f(B, case["p"], case["mlp"][-1])
        inp["g_xyz"], inp["g_out"] = f(B, case["p"], 3), f(B, case["p"], case["mlp"][-1])
        return inp
    if kind in ("decode", "fp"):
        inp = {"xyz1": ball(rng, B, case["n1"]), "xyz2": ball(rng, B, case["n2"]), "points2": f(B, case["n2"], case["c2"])}
        if case["c1"]:
            inp["points1"] = f(B, case["n1"], case["c1"])
        inp["g_out"] = f(B, case["n1"], case["mlp"][-1])
        return inp
    if kind == "group_all":
        return {"xyz": ball(rng, B, case["n"]), "points": f(B, case["n"], case["c"]), "g_out": f(B, case["mlp"][-1])}
    if kind.startswith("head"):
        return {"x": f(*case["shape"]), "g_out": f(*case["shape"][:-1], case["num_class"])}
    if kind == "cls":
        return {"x": ball(rng, case["b"], case["n"]), "labels": (np.arange(case["b"]) * 7 % 40).astype(np.int64)}
    raise ValueError(kind)


GRAD_INPUTS = {"sa": ("xyz", "feature", "residual"), "decode": ("xyz1", "points1", "points2"), "fp": ("points1", "points2"),
               "group_all": ("xyz", "points"), "head_cls": ("x",), "head_sem_seg": ("x",), "head_sem_seg_res": ("x",), "cls": ("x",)}


def run_case(g, name, inp, dec):
    """One case on the Graph `g`.  inp: case_inputs(name); dec: the case's discrete decisions -- "idx" (sa), "nn" = (dist, idx) and
    "kidx" (decode, fp), "masks" (heads, cls), "layer1" / "layer2" (cls).
    -> (leaves {input name: tensor}, outs {name: tensor}, loss)"""
    case = CASES[name]
    kind = case["kind"]
    t = {k: g.tensor(v, k in GRAD_INPUTS[kind]) for k, v in inp.items() if k != "labels"}
    ix = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int64)
    if kind == "sa":
        new_xyz, out = g.set_abstraction(t["xyz"], t.get("feature", t["xyz"]), ix(dec["idx"]), case["mlp"], name, case["as_neighbor"],
                                         case["NL"], t.get("residual"))
        outs = {"new_xyz": new_xyz, "out": out}
        loss = (out * t["g_out"]).sum() + (new_xyz * t["g_xyz"]).sum()
    elif kind == "decode":
        out = g.decoding_layer(t["xyz1"], t.get("points1"), t["points2"], dec["nn"], ix(dec["kidx"]), case["mlp"], name)
        outs, loss = {"out": out}, (out * t["g_out"]).sum()
    elif kind == "fp":
        out = g.fp_module(t.get("points1"), t["points2"], dec["nn"], case["mlp"], name)
        outs, loss = {"out": out}, (out * t["g_out"]).sum()
    elif kind == "group_all":
        out = g.sa_group_all(t["xyz"], t["points"], case["mlp"], name)
        outs, loss = {"out": out}, (out * t["g_out"]).sum()
    elif kind.startswith("head"):
        out = getattr(g, kind[5:] + "_head")(t["x"], dec.get("masks", {}), case["num_class"])
        outs, loss = {"out": out}, (out * t["g_out"]).sum()
    else:
        logits, ep = g.cls_model(t["x"], dec if "layer1" in dec else dec["pick"], case["adaptive_sample"], dec.get("masks", {}))
        outs, loss = {"logits": logits, "l1_xyz": ep["l1_xyz"]}, xent(logits, inp["labels"])
    return {k: v for k, v in t.items() if v.requires_grad}, outs, loss


def evaluate(name, inp, dec, dtype, params=None, seed=None, graph=Graph):
    """The case's training step on a fresh graph in `dtype` -> dict of numpy arrays: "out/<name>", "grad/<input or variable name>",
    "stat/<moving statistic's name>", and the graph under "graph" """
    g = graph(params, dtype, True, DECAY, seed)
    leaves, outs, loss = run_case(g, name, inp, dec)
    loss.backward()
    res = {"out/" + k: v.detach().numpy() for k, v in outs.items()}
    res.update({"grad/" + k: (None if v.grad is None else v.grad.numpy()) for k, v in leaves.items()})
    res.update({"grad/" + k: (None if v.grad is None else v.grad.numpy()) for k, v in g.trainable().items()})
    res.update({"stat/" + k: v.numpy() for k, v in g.moving().items()})
    res["graph"] = g
    return res


def undecided_maxima(g64, g32, tags=None):
    """A maximum whose two largest candidates lie closer together than float32 computes them has no float64 answer a float32
    implementation could be held to: which candidate wins -- and so where the WHOLE gradient of that maximum goes -- is decided
    by rounding.  (tests/sa_grad_ref.py keeps its problems free of such ties for the same reason.)  A maximum is decided when
    the float64 gap between its largest and second largest candidate exceeds 4 x the float32 restatement's own error in that
    tensor (max |X32 - X64|, the yardstick of the comparison rule), or when the two are exactly equal in both types (ReLU zeros:
    the gradient is shared in both).  tags: only these maxima.  -> [(tag, position, gap, 4 x error)] of the maxima that are not."""
    bad = []
    for tag, (x64, dim) in g64.maxima.items():
        if tags is not None and tag not in tags:
            continue
        x32 = g32.maxima[tag][0].to(torch.float64)
        e = 4 * float((x32 - x64).abs().max())
        top, at = x64.topk(2, dim=dim)
        gap = top.select(dim, 0) - top.select(dim, 1)
        top32 = x32.gather(dim, at)
        tied = (gap == 0) & (top32.select(dim, 0) == top32.select(dim, 1))
        for pos in torch.nonzero((gap <= e) & ~tied).tolist():
            bad.append((tag, tuple(pos), float(gap[tuple(pos)]), e))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison rule (tests/test_gpu_training_mode.py compare_routes, restated per tensor)
# ---------------------------------------------------------------------------------------------------------------------------
def gradient_floor(r64):
    return 1e-4 * max(np.abs(v).max() for n, v in r64.items() if n.startswith("grad/") and v is not None)


def scale_of(r64, name, floor):
    """max |X64|; a bias in front of a batch norm against its layer's beta gradient; any gradient against at least `floor`"""
    scale = float(np.abs(r64[name]).max())
    if not name.startswith("grad/"):
        return max(scale, 1e-300)
    if name.endswith("/biases"):
        beta = name[:-len("biases")] + "bn/beta"
        if r64.get(beta) is not None:
            scale = float(np.abs(r64[beta]).max())
    return max(scale, floor)


def errors(got, r64):
    """{name: max |got - X64| / scale} over every array of r64 (None in `got`: inf unless X64 is exactly zero)"""
    floor = gradient_floor(r64)
    out = {}
    for name, want in r64.items():
        if name.split("/")[0] not in ("out", "grad", "stat") or want is None:
            continue
        have = got.get(name)
        if have is None:
            out[name] = 0.0 if not np.any(want) else float("inf")
            continue
        have = np.asarray(have, np.float64).reshape(want.shape)
        out[name] = float(np.abs(have - want).max() / scale_of(r64, name, floor)) if np.isfinite(have).all() else float("inf")
    return out


def allowed(err_chain):
    return max(4 * err_chain, 1e-5)


def by_kind(errs):
    """{kind: the largest error among its tensors}"""
    out = {}
    for name, e in errs.items():
        out[kind_of_name(name)] = max(out.get(kind_of_name(name), 0.0), e)
    return out


def kind_of_name(name):
    """the group a tensor is reported under: out, stat, grad, grad/biases, grad/input"""
    head = name.split("/")[0]
    if head == "grad":
        if name.endswith("/biases"):
            return "grad/biases"
        if "/" not in name[5:]:
            return "grad/input"
    return head


def dropout_rows(name):
    case = CASES[name]
    return case["b"] if case["kind"] == "cls" else int(np.prod(case["shape"][:-1]))


def dropout_masks(name, seed, stream_id, first_call=0):
    """The keep masks of a case's dropout layers as the product draws them: bn_train_ref.dropout_keep(n, keep, seed, stream word of
    the layer's scope path, call), the call word counting the store's dropout calls.  stream_id: path -> the 32-bit word."""
    import bn_train_ref

    kind = CASES[name]["kind"]
    if kind not in DROPOUTS:
        return {}
    rows = dropout_rows(name)
    return {scope: bn_train_ref.dropout_keep(rows * width, keep, seed, stream_id(scope), first_call + call).reshape(rows, width)
            for call, (scope, keep, width) in enumerate(DROPOUTS.get(kind, ()))}
