"""tests/train_graph_ref.py pinned on the CPU (no GPU): it is the reference tests/test_gpu_training_graph.py holds the product to.

  * evaluation mode: with train=False and float64 every cell and cls_model equals oracle.cells (the numpy restatement of the
    inference graph, itself pinned to the golden fixtures) to 1e-12 of scale, from the same random variables and neighbour lists;
  * training mode: every batch-normed layer of every case normalises (column mean 0, variance var / (var + eps)), updates its
    moving statistics once, by the formula, with Bessel's correction exactly where the table below -- written per scope name --
    says the reference's wrapper has it;
  * the dropout masks the GPU test hands over are addressed by a hash of the full scope path, restated here;
  * the comparison can fail: six mutants of the restatement, each in float64 against the unmutated float64 restatement on the GPU
    test's own cases and seeds, miss the GPU test's rule by more than a factor of 10 in at least one compared quantity.

The neighbour lists come from the CPU oracle here (oracle.ops: FPS, kNN, three_nn) and from the product's own searches on the GPU;
on these tie-free clouds they are the same lists (pinned by the search tests)."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import train_graph_ref as R
from oracle import cells, ops

SA = [n for n, c in R.LAYER_CASES.items() if c["kind"] == "sa"]
AS = [n for n in SA if R.CASES[n]["as_neighbor"] > 0]
DECODE = [n for n, c in R.LAYER_CASES.items() if c["kind"] == "decode"]
SEG_HEADS = ["head_sem_seg", "head_sem_seg_res"]


def stream_word(path):
    """the 32-bit stream word of a dropout layer, restated: the first four bytes of SHA-256 of its scope path, little endian"""
    return int.from_bytes(hashlib.sha256(path.encode()).digest()[:4], "little")


def rows_of(points, idx):
    return points[np.arange(points.shape[0])[:, None], idx]


def sa_search(xyz, npoint, nsample):
    """the neighbour lists of a set-abstraction layer: FPS, then kNN of the sampled rows (all rows when nothing is sampled)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    q = xyz if npoint == xyz.shape[1] else rows_of(xyz, ops.farthest_point_sample(npoint, xyz))
    return ops.knn_batch(xyz, q, nsample, omp=True)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(inputs, decisions) of a case, the decisions taken by the CPU oracle"""
    case, inp = R.CASES[name], R.case_inputs(name)
    kind = case["kind"]
    dec = {"masks": R.dropout_masks(name, case["seed"], stream_word)}
    if kind == "sa":
        dec["idx"] = sa_search(inp["xyz"], case["p"], case["k"])
    elif kind in ("decode", "fp"):
        dec["nn"] = ops.three_nn(inp["xyz1"], inp["xyz2"])
        if kind == "decode":
            dec["kidx"] = ops.knn_batch(inp["xyz1"], inp["xyz1"], case["k"], omp=True)
    elif kind == "cls":
        dec["pick"] = lambda scope, xyz: sa_search(xyz.detach().numpy(), *{"layer1": (512, 32), "layer2": (128, 64)}[scope])
    return inp, dec


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """the unmutated training step; a model's lists are taken once, by the float64 run, and shared (as the GPU test shares the
    product's)"""
    inp, dec = problem(name)
    if R.CASES[name]["kind"] == "cls":
        if dtype != torch.float64:
            dec = dict(dec, **reference(name, torch.float64)["lists"])
        else:
            lists, inner = {}, dec["pick"]
            dec = dict(dec, pick=lambda scope, xyz: lists.setdefault(scope, inner(scope, xyz)))
            res = R.evaluate(name, inp, dec, dtype, seed=R.CASES[name]["seed"])
            res["lists"] = lists
            return res
    return R.evaluate(name, inp, dec, dtype, seed=R.CASES[name]["seed"])


def decisions(name):
    inp, dec = problem(name)
    if R.CASES[name]["kind"] == "cls":
        dec = dict(dec, **reference(name, torch.float64)["lists"])
    return inp, dec


# ---------------------------------------------------------------------------------------------------------------------------
# evaluation mode against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def close(got, want):
    want = np.asarray(want, np.float64)
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", [n for n, c in R.LAYER_CASES.items() if not c["kind"].startswith("head")])
def test_evaluation_mode_equals_the_oracle(name):
    case = R.CASES[name]
    inp, dec = problem(name)
    g = R.Graph(None, torch.float64, train=False, seed=case["seed"])
    _, outs, _ = R.run_case(g, name, inp, dec)
    p = g.numpy_params
    d = {k: v.astype(np.float64) for k, v in inp.items()}
    if case["kind"] == "sa":
        feature = d.get("feature", d["xyz"])
        new_xyz, out = cells.set_abstraction(d["xyz"], feature, case["p"], case["k"], case["mlp"], p, name, case["as_neighbor"],
                                             case["NL"], knn_idx=dec["idx"])
        close(outs["new_xyz"], new_xyz)
        close(outs["out"], out + d["residual"] if case.get("residual") else out)
    elif case["kind"] == "decode":
        close(outs["out"], cells.decoding_layer(d["xyz1"], d["xyz2"], d.get("points1"), d["points2"], case["k"], case["mlp"], p, name))
    elif case["kind"] == "fp":
        close(outs["out"], cells.fp_module(d["xyz1"], d["xyz2"], d.get("points1"), d["points2"], case["mlp"], p, name))
    else:
        close(outs["out"], cells.sa_group_all(d["xyz"], d["points"], case["mlp"], p, name))
    assert not g.updates and not g.norm


@pytest.mark.parametrize("adaptive_sample", [False, True])
def test_cls_model_in_evaluation_mode_equals_the_oracle(adaptive_sample):
    name = "cls_adaptive" if adaptive_sample else "cls"
    x = R.case_inputs(name)["x"][:2]
    g = R.Graph(None, torch.float64, train=False, seed=R.CASES[name]["seed"])
    pick = lambda scope, xyz: sa_search(xyz.detach().numpy(), *{"layer1": (512, 32), "layer2": (128, 64)}[scope])
    logits, ep = g.cls_model(g.tensor(x), pick, adaptive_sample, None)
    want, wep = cells.cls_forward(x, g.numpy_params, adaptive_sample, dtype=np.float64)
    close(logits, want)
    for k in ("l1_xyz", "l2_xyz", "l1_points", "l2_points"):
        close(ep[k], wep[k])


@pytest.mark.parametrize("head,act", [("cls", "relu"), ("sem_seg", "relu"), ("sem_seg_res", "leaky_relu")])
def test_heads_in_evaluation_mode_equal_the_oracle_layers(head, act):
    name = "head_" + head
    inp, dec = problem(name)
    g = R.Graph(None, torch.float64, train=False, seed=R.CASES[name]["seed"])
    _, outs, _ = R.run_case(g, name, inp, dec)  # (dropout is the identity at inference)
    p, x = g.numpy_params, inp["x"].astype(np.float64)
    order = {"cls": ("fc1", "fc2", "fc3"), "sem_seg": ("fc1", "fc2"), "sem_seg_res": ("fc1", "fc0")}[head]
    for i, sc in enumerate(order):
        x = cells._layer(x, p[sc], None if i == len(order) - 1 else act)
    close(outs["out"], x)


# ---------------------------------------------------------------------------------------------------------------------------
# training mode: normalisation, the moving update, the kind table
# ---------------------------------------------------------------------------------------------------------------------------
def kind_by_name(case_kind, scope):
    """The reference's wrapper of every layer, by its scope name: conv1d for a set-abstraction layer's skip and aggregation and for
    the segmentation heads; fully_connected for the classifier's head; conv2d for everything else."""
    leaf = scope.split("/")[-1]
    if leaf in ("skip", "aggregation"):
        return "conv1d"
    if "/" not in scope and leaf in ("fc0", "fc1", "fc2", "fc3"):
        return "fc" if case_kind in ("head_cls", "cls") else "conv1d"
    return "conv2d"


@pytest.mark.parametrize("name", list(R.CASES))
def test_training_mode_statistics_and_the_kind_table(name):
    case = R.CASES[name]
    res = reference(name, torch.float64)
    g = res["graph"]
    normed = [sc for sc, p in g.numpy_params.items() if "gamma" in p]
    assert normed and set(g.updates) == set(normed) and set(g.updates.values()) == {1}
    keep = 1.0 - float(np.float32(R.DECAY))
    for sc in g.kinds:
        assert g.kinds[sc] == kind_by_name(case["kind"], sc), sc
    for sc in normed:
        s, p = g.norm[sc], g.numpy_params[sc]
        var = s["biased_var"].numpy()
        assert np.abs(s["xhat_mean"].numpy()).max() <= 1e-12, sc
        assert np.abs(s["xhat_var"].numpy() - var / (var + 1e-3)).max() <= 1e-12, sc
        rows = s["rows"]
        assert rows > 1
        fed = var * rows / (rows - 1) if kind_by_name(case["kind"], sc) in ("conv2d", "fc") else var
        mean0, var0 = p["mean"].astype(np.float64), p["var"].astype(np.float64)
        np.testing.assert_allclose(res["stat/" + sc + "/bn/moving_mean"], mean0 - (mean0 - s["batch_mean"].numpy()) * keep, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(res["stat/" + sc + "/bn/moving_variance"], var0 - (var0 - fed) * keep, rtol=1e-13, atol=1e-15)
    # the names are the store's: every variable of every scope, the moving statistics apart
    assert {n for n in res if n.startswith("grad/") and "/" in n[5:]} == {
        "grad/" + sc + "/" + leaf for sc, p in g.numpy_params.items() for leaf in (("weights", "biases", "bn/gamma", "bn/beta") if "gamma" in p
                                                                                     else ("weights", "biases"))}
    for n, v in res.items():
        if n.startswith("grad/"):
            assert v is not None and np.isfinite(v).all(), n


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_maxima_of_a_case_are_decided(name):
    """No maximum of a layer case (the skip connection's, the group_all module's) and no group_all maximum of a model case has its
    two largest candidates closer together than float32 computes them: the float64 gradient of every one is an answer a float32
    implementation can be held to.  (train_graph_ref.MODEL_CASES says why a model's skip maxima are not asked the same.)"""
    g64, g32 = reference(name, torch.float64)["graph"], reference(name, torch.float32)["graph"]
    assert set(g64.maxima) == set(g32.maxima)
    if name in R.MODEL_CASES:
        assert set(R.POOLINGS) < set(g64.maxima)
    assert R.undecided_maxima(g64, g32, R.POOLINGS if name in R.MODEL_CASES else None) == []


def test_scopes_nest_as_the_store_names_them():
    g = reference("sa_c32_as8", torch.float64)["graph"]
    s = "sa_c32_as8"
    assert set(g.kinds) == {f"{s}/{s}/{s}/conv_kv_ds", f"{s}/{s}/{s}/conv_query_ds", f"{s}/{s}/{s}/mlp2_0", f"{s}/{s}/{s}/mlp2_1",
                            f"{s}/{s}/conv_kv", f"{s}/{s}/conv_query", f"{s}/{s}/conv_back_project", f"{s}/skip", f"{s}/conv0", f"{s}/conv1",
                            f"{s}/weight_net/wconv0", f"{s}/after_conv", f"{s}/aggregation"}
    assert g.numpy_params[f"{s}/{s}/{s}/mlp2_1"]["w"].shape == (32, 1 + 3 + 32)
    g = reference("sa_xyz_as12", torch.float64)["graph"]
    assert g.numpy_params["sa_xyz_as12/sa_xyz_as12/sa_xyz_as12/mlp2_1"]["w"].shape == (32, 1 + 3 + 3)
    g = reference("sa_full_residual", torch.float64)["graph"]
    assert {sc.split("/", 1)[1] for sc in g.kinds} == {"skip", "conv0", "weight_net/wconv0", "after_conv", "aggregation"}
    assert reference("sa_c160_as4", torch.float64)["graph"].numpy_params["sa_c160_as4/sa_c160_as4/conv_kv"]["w"].shape == (160, 160)


# ---------------------------------------------------------------------------------------------------------------------------
# dropout: the address of a mask
# ---------------------------------------------------------------------------------------------------------------------------
def test_dropout_masks_are_addressed_by_the_scope_path():
    from pointasnl_amd.utils import tf_util

    st = tf_util.VariableStore(seed=1, device="cpu")
    for leaf in ("dp1", "dp2", "dp"):
        assert tf_util.dropout_stream_id(leaf) == stream_word(leaf)
        with st.scope("outer"), st.scope("inner"):
            assert st.path(leaf) == "outer/inner/" + leaf
            assert tf_util.dropout_stream_id(st.path(leaf)) == stream_word("outer/inner/" + leaf) != stream_word(leaf)
    assert len({stream_word(s) for s in ("dp1", "dp2", "dp")}) == 3
    # the masks of a case: one per dropout layer, in call order, about keep_prob of the elements kept, and applied as x / keep_prob
    m = R.dropout_masks("head_cls", 31, stream_word)
    assert list(m) == ["dp1", "dp2"] and m["dp1"].shape == (8, 512) and m["dp2"].shape == (8, 256)
    assert abs(m["dp1"].mean() - 0.4) < 0.05 and abs(m["dp2"].mean() - 0.4) < 0.05
    assert not np.array_equal(m["dp1"][:, :256], m["dp2"])
    assert not np.array_equal(R.dropout_masks("head_cls", 31, stream_word, first_call=1)["dp1"], m["dp1"])
    g = R.Graph(None, torch.float64, seed=0)
    x = torch.arange(1.0, 9.0, dtype=torch.float64).reshape(2, 4)
    keep = np.array([[1, 0, 1, 1], [0, 0, 1, 0]], bool)
    assert torch.equal(g.dropout(x, keep, 0.5), x * torch.from_numpy(keep) * 2.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison can fail
# ---------------------------------------------------------------------------------------------------------------------------
def mutant(what, scope=None):
    class Mutant(R.Graph):
        def layer(self, x, sc, cout, act, kind, bn=True):
            if sc != scope:
                return super().layer(x, sc, cout, act, kind, bn)
            if what == "moving statistics":  # this layer normalises with the moving statistics (and leaves them alone)
                self.train = False
                try:
                    return super().layer(x, sc, cout, act, kind, bn)
                finally:
                    self.train = True
            if what == "bessel":
                assert kind == "conv1d"
                return super().layer(x, sc, cout, act, "conv2d", bn)
            assert what == "updated twice"
            y = super().layer(x, sc, cout, act, kind, bn)
            s = self.norm[sc]
            self.stat[sc] = {"mean": R.moving_update(self.stat[sc]["mean"], s["batch_mean"], self.decay),
                             "var": R.moving_update(self.stat[sc]["var"], s["batch_var"], self.decay)}
            return y

        def window(self, m):
            return m.transpose(2, 3).reshape(m.shape[0], m.shape[1], -1) if what == "window" else super().window(m)

        def centres(self, new_xyz):
            return new_xyz.detach() if what == "detached" else new_xyz

        def pooled_concat(self, top, res):
            return torch.cat([res, top], dim=-1) if what == "concat order" else super().pooled_concat(top, res)

    return Mutant


def first_normed(name):
    return next(iter(reference(name, torch.float64)["graph"].updates))


def smallest_conv1d(name):
    """the batch-normed conv1d layer with the fewest rows: where Bessel's correction is largest"""
    g = reference(name, torch.float64)["graph"]
    return min((sc for sc in g.updates if g.kinds[sc] == "conv1d"), key=lambda sc: g.norm[sc]["rows"])


MUTANTS = (
    [("moving statistics", n, first_normed) for n in R.CASES]
    + [("bessel", n, smallest_conv1d) for n in SA + SEG_HEADS + ["cls"]]
    + [("concat order", n, None) for n in R.MODEL_CASES]
    + [("detached", n, None) for n in AS + ["cls_adaptive"]]
    + [("window", n, None) for n in SA + DECODE + ["cls"]]
    + [("updated twice", n, first_normed) for n in R.CASES]
)


@pytest.mark.parametrize("what,name,where", MUTANTS, ids=[f"{w.replace(' ', '_')}-{n}" for w, n, _ in MUTANTS])
def test_a_mutant_of_the_graph_misses_the_rule(what, name, where):
    r64, r32 = reference(name, torch.float64), reference(name, torch.float32)
    inp, dec = decisions(name)
    got = R.evaluate(name, inp, dec, torch.float64, seed=R.CASES[name]["seed"], graph=mutant(what, where(name) if where else None))
    assert {n for n in got if n != "graph"} == {n for n in r64 if n not in ("graph", "lists")}
    e, chain = R.errors(got, r64), R.errors(r32, r64)
    if R.CASES[name]["kind"] == "cls":  # per kind, as the GPU test compares a model
        e, chain = R.by_kind(e), R.by_kind(chain)
    worst = max(e, key=lambda n: e[n] / R.allowed(chain[n]))
    print(f"{what} in {name}: {worst} misses by {e[worst]:.3g} (chain {chain[worst]:.3g})")
    assert e[worst] > 10 * R.allowed(chain[worst]), (worst, e[worst], chain[worst])
