"""GPU: the grid pipelines' per-epoch evaluation on the device (csrc/grid_eval.hip: pasnl_scan_eval_confusion,
pasnl_scene_eval_vote, pasnl_scene_eval_vote_confusion; pointasnl_amd.ScanNet.scene_evaluator and
pointasnl_amd.SemanticKITTI.scan_evaluator) against the numpy restatement tests/grid_eval_flow_ref.py
(tests/test_grid_eval_flow.py pins it to the reference's own `eval_one_epoch` functions).  Counts are compared exactly, the
float64 table by bits with probabilities in and under the softmax rule of tests/test_gpu_scene_tester.py with logits in."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import grid_eval_flow_ref as R
import philox_ref as PH
from grid_train_checks import formula_holds
from guarded import ALT_BYTE, NAN_BYTE, Guarded, output_guard
from scan_flow_ref import softmax_f32
from scene_flow_ref import confusion

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_grid_eval_flow as M  # noqa: E402

NULL = ctypes.c_void_p(0)
L = ctypes.c_long


def _hip():
    from pointasnl_amd import _hip

    return _hip


def P(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def ig_of(ignored, nl):
    return (ctypes.c_int * nl)(*[1 if l in ignored else 0 for l in range(nl)])


def ignored_sets(nl):
    """the first label, one in the middle, two"""
    mid = 4 if nl > 5 else nl - 1
    return [(0,), (mid,), (0, 7 if nl > 8 else nl - 1)]


def eval_confusion(values, is_logits, truth, ignored, nl, out):
    b, npt, w = values.shape
    dv, dt = dev(values), dev(truth)
    _hip().launch("pasnl_scan_eval_confusion", "test", b, npt, w - 1 if is_logits else w, P(dv), 1 if is_logits else 0, P(dt),
                  ig_of(ignored, nl), nl, P(out))
    torch.cuda.synchronize()
    assert np.array_equal(bits(dv.cpu().numpy()), bits(values)) and np.array_equal(dt.cpu().numpy(), truth)  # inputs are read only


def want_confusion(probs, truth, ignored, nl):
    lv = np.arange(nl)
    Confs, _ = R.crop_confusions(list(probs), list(truth), lv, np.asarray(ignored), nl)
    return np.sum(Confs, axis=0).astype(np.int64)


def distinct_integer_logits(rng, b, npt, w):
    """integer-valued, pairwise distinct per row: a permutation of 0..w-1 (exp(-64) is a normal float32)"""
    return rng.permuted(np.tile(np.arange(w, dtype=np.float32), (b, npt, 1)), axis=-1)


def assert_softmax_cannot_flip(logits):
    """the CPU side of the logits cases: numpy's float32 softmax keeps a strict maximum at the argmax of the logits with
    the runner-up at most half of it (the logits' gap is >= 1: a factor e), so a few ulps on the device cannot move it"""
    p = softmax_f32(logits[:, :, 1:])
    s = np.sort(p, axis=-1)
    assert (np.argmax(p, -1) == np.argmax(logits[:, :, 1:], -1)).all() and (s[..., -1] > 0).all()
    if p.shape[-1] > 1:
        assert (s[..., -2] <= 0.5 * s[..., -1]).all()


# nc + 1 in {2, 20, 21, 65} with the first label ignored, one in the middle, two; 65 columns leave room for none (nl <= 64)
CASES = [(w, k) for w in (2, 20, 21) for k in (0, 1, 2)] + [(65, None)]


@pytest.mark.parametrize("width,which", CASES)
def test_eval_confusion_is_the_restatement(width, which):
    """probabilities in and logits in, num_point in {1, 255, 257, 1000} x b in {1, 3}: odd and even row widths, tiles that
    end inside a crop, more than one workgroup; truth entries of -1 and nl are dropped; the calls accumulate"""
    rng = np.random.default_rng(width * 10 + (which or 0))
    nc = width - 1
    for is_logits in (0, 1):
        nl = nc + (0 if which is None else 1 if which < 2 else 2)
        ignored = () if which is None else ignored_sets(nl)[which]
        assert len(set(ignored)) == nl - nc and nl <= 64
        out = torch.zeros((nl, nl), dtype=torch.int64, device="cuda")
        total = np.zeros((nl, nl), np.int64)
        for npt in (1, 255, 257, 1000):
            for b in (1, 3):
                if is_logits:
                    values = distinct_integer_logits(rng, b, npt, width)
                    assert_softmax_cannot_flip(values)
                    probs = softmax_f32(values[:, :, 1:])
                else:
                    values = probs = rng.random((b, npt, nc)).astype(np.float32)
                    if nc > 1:
                        values[:, ::7, 0] = values[:, ::7, nc - 1] = 2.0  # two equal maxima: the first
                truth = rng.integers(-1, nl + 1, (b, npt)).astype(np.int32)  # -1 and nl: dropped
                want = want_confusion(probs, truth, ignored, nl)
                assert want.sum() == np.count_nonzero((truth >= 0) & (truth < nl))
                total += want
                eval_confusion(values, is_logits, truth, ignored, nl, out)
                np.testing.assert_array_equal(out.cpu().numpy(), total, err_msg=f"logits={is_logits} npt={npt} b={b}")
        assert total[:, list(ignored)].sum() == 0 and total.sum() > 0 and (nc == 1 or np.count_nonzero(total) > nl)


@pytest.mark.parametrize("ignored", [(0,), (4,), (0, 3)])
def test_eval_confusion_edge_rows(ignored):
    """a row of equal logits (the first non-ignored class wins: distinct logits may round to equal probabilities, and
    these are equal), equal probabilities, NaN rows -- numpy's argmax takes the first NaN"""
    nl = 7
    nc = nl - len(ignored)
    first = next(l for l in range(nl) if l not in ignored)
    rng = np.random.default_rng(3)
    npt = 300
    logits = distinct_integer_logits(rng, 1, npt, nc + 1)
    logits[0, :40] = 2.5                       # equal logits
    logits[0, 40:50, 2] = np.nan               # a NaN inside: every probability is NaN
    logits[0, 50:60, 0] = np.nan               # the dropped column: nothing changes
    logits[0, 60:70, 1:3] = 30.0               # two equal maxima
    truth = rng.integers(0, nl, (1, npt)).astype(np.int32)
    with np.errstate(invalid="ignore"):
        probs = softmax_f32(logits[:, :, 1:])
    assert np.isnan(probs[0, 40:50]).all() and not np.isnan(probs[0, 50:]).any()
    want = want_confusion(probs, truth, ignored, nl)
    assert want[:, first].sum() >= 50          # the equal rows and the NaN rows predict the first kept label
    out = torch.zeros((nl, nl), dtype=torch.int64, device="cuda")
    eval_confusion(logits, 1, truth, ignored, nl, out)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    p = rng.random((1, npt, nc)).astype(np.float32)
    p[0, :40] = 0.25
    p[0, 40:50, nc - 1] = np.nan               # one NaN: it is the argmax
    p[0, 50:60] = 0                            # all zero: the first label of the expanded row, ignored or not
    p[0, 60:70, 0] = p[0, 60:70, 2] = 2.0
    want = want_confusion(p, truth, ignored, nl)
    out.zero_()
    eval_confusion(p, 0, truth, ignored, nl, out)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    if 0 in ignored:
        assert want[:, 0].sum() == np.count_nonzero(truth[0, 50:60] >= 0)  # the zero rows predict the ignored label 0


def eval_vote(values, is_logits, inds, clouds, offsets, smooth_old, smooth_new, table_ptr, win):
    b, npt, w = values.shape
    dv, di, dc, do = dev(values), dev(inds), dev(clouds), dev(offsets)
    _hip().launch("pasnl_scene_eval_vote", "test", b, npt, w - 1 if is_logits else w, P(dv), 1 if is_logits else 0, P(di), P(dc), P(do),
                  ctypes.c_double(smooth_old), ctypes.c_float(smooth_new), P(table_ptr), P(win))
    torch.cuda.synchronize()
    assert (win == -1).all()


def test_vote_is_bit_exact_and_softmax_error_is_bounded():
    """the set-up of tests/test_gpu_scene_tester.py's vote test: crops 0 and 2 of a batch on one scene sharing 500 indices,
    a repeated index inside a crop; three batches into a float64 table"""
    rng = np.random.default_rng(8)
    C, npt, B, n = 21, 3000, 3, 4000
    nc = C - 1
    offsets = np.array([0, n, 2 * n, 3 * n], np.int64)
    tables = [rng.random((n, nc)) * 0.8 for _ in range(3)]
    init = [t.copy() for t in tables]
    table = dev(np.concatenate(tables))
    win = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    clouds = np.array([0, 1, 0], np.int32)
    val_smooth = 0.95
    touched = [np.zeros(n, bool) for _ in range(3)]
    for rep in range(3):
        inds = rng.integers(0, n, (B, npt)).astype(np.int32)
        inds[0, 100:160] = 9                 # a repeated index inside a crop: the last occurrence wins
        inds[2, :500] = inds[0, :500]
        logits = (rng.standard_normal((B, npt, C)) * 3).astype(np.float32)
        probs = softmax_f32(logits[:, :, 1:])
        eval_vote(probs, 0, inds, clouds, offsets, val_smooth, np.float32(1 - val_smooth), table, win)
        for b in range(B):                   # S:346-351, literally
            c_i = clouds[b]
            tables[c_i][inds[b]] = val_smooth * tables[c_i][inds[b]] + (1 - val_smooth) * probs[b]
            touched[c_i][inds[b]] = True
        got = table.cpu().numpy()
        assert got.dtype == np.float64
        np.testing.assert_array_equal(bits(got), bits(np.concatenate(tables)))
    got = table.cpu().numpy().reshape(3, n, nc)
    assert not touched[2].any() and not touched[0].all()
    np.testing.assert_array_equal(bits(got[2]), bits(init[2]))                          # rows no crop touched keep their bits
    np.testing.assert_array_equal(bits(got[0][~touched[0]]), bits(init[0][~touched[0]]))
    # logits in: the device's float32 softmax and numpy's, both against a float64 softmax of the same logits
    zero = torch.full((3 * n, nc), 7.0, dtype=torch.float64, device="cuda")  # table = 0 * old + 1 * probs
    ident = np.tile(np.arange(npt, dtype=np.int32), (B, 1))
    eval_vote(logits, 1, ident, np.array([0, 1, 2], np.int32), offsets, 0.0, 1.0, zero, win)
    got = zero.cpu().numpy().reshape(3, n, nc)
    assert (got[:, npt:] == 7.0).all()
    w = R.softmax_f64(logits[:, :, 1:])
    err_dev = np.abs(got[:, :npt] - w).max()
    err_np = np.abs(softmax_f32(logits[:, :, 1:]).astype(np.float64) - w).max()
    print(f"softmax worst error vs float64: device {err_dev:.3e}, numpy float32 {err_np:.3e}")
    assert err_dev <= 2 * err_np
    assert (got[:, :npt] == got[:, :npt].astype(np.float32)).all()  # a float32 product widened, not a float64 softmax


LV = np.array([0, 1, 2, 4, 7, 9], np.int32)


def vote_table(rng, n, nc):
    tab = rng.random((n, nc)) * 0.5
    tab[:50, 1] = tab[:50, 3] = 0.75          # two equal maxima: the first
    tab[50:60] = 0                            # never visited: the first label of the expanded row
    return tab


def want_vote_confusion(tab, proj, labels, ignored):
    sub_probs = tab
    for l_ind, label_value in enumerate(LV):  # S:396-410
        if label_value in ignored:
            sub_probs = np.insert(sub_probs, l_ind, 0, axis=1)
    sub_idx = np.argmax(sub_probs, axis=1).astype(np.int32)
    sub_preds = LV[sub_idx]
    preds = (sub_preds[proj]).astype(np.int32)
    return sub_idx, confusion(labels.astype(np.int32), preds, LV)


@pytest.mark.parametrize("ignored", [(0,), (4,), (0, 7)])
def test_vote_confusion_is_the_restatement(ignored):
    rng = np.random.default_rng(5)
    n, nc = 3000, len(LV) - len(ignored)
    tab = vote_table(rng, n, nc)
    dt, dl = dev(tab), dev(LV)
    ig = ig_of([int(np.flatnonzero(LV == v)[0]) for v in ignored], len(LV))
    for m, with_proj in ((1, True), (257, True), (5000, True), (1, False), (257, False), (3000, False)):
        proj = rng.integers(0, n, m).astype(np.int32) if with_proj else np.arange(m, dtype=np.int32)
        if with_proj and m > 100:
            proj[:40] = rng.integers(0, 60, 40)   # the tie and the all-zero rows are projected onto
        labels = rng.choice(np.append(LV, [5, -1]), m).astype(np.int32)  # 5 and -1 are no label values: dropped
        sub_idx, want = want_vote_confusion(tab, proj, labels, ignored)
        sub = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        out = torch.zeros((6, 6), dtype=torch.int64, device="cuda")
        dp, dlab = dev(proj), dev(labels)
        for rep in range(2):                      # the second call adds the same counts
            _hip().launch("pasnl_scene_eval_vote_confusion", "test", L(n), P(dt), nc, L(m), P(dp) if with_proj else NULL, P(dlab),
                          P(dl), ig, 6, P(sub), P(out))
            np.testing.assert_array_equal(sub.cpu().numpy(), sub_idx)
            np.testing.assert_array_equal(out.cpu().numpy(), (rep + 1) * want, err_msg=f"m={m} proj={with_proj}")
        assert want.sum() == np.count_nonzero(np.isin(labels, LV))
    if ignored == (0,):
        assert (sub_idx[50:60] == 0).all()        # an all-zero row predicts the ignored label, as numpy's argmax does
    # a projection outside [0, n) is ignored
    proj = np.array([0, -1, n, 5, n + 7], np.int32)
    labels = np.array([1, 1, 1, 2, 2], np.int32)
    _, want = want_vote_confusion(tab, proj[[0, 3]], labels[[0, 3]], ignored)
    out = torch.zeros((6, 6), dtype=torch.int64, device="cuda")
    dp, dlab = dev(proj), dev(labels)
    _hip().launch("pasnl_scene_eval_vote_confusion", "test", L(n), P(dt), nc, L(5), P(dp), P(dlab), P(dl), ig, 6, P(sub), P(out))
    np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("fill", [NAN_BYTE, ALT_BYTE])
def test_only_the_outputs_are_written(fill):
    """`out`, `sub_preds` and the table sit in guarded buffers over two kinds of stale bytes: the guards stay, the table's
    unselected rows keep their bits"""
    rng = np.random.default_rng(11)
    nl, nc, b, npt, n = 21, 20, 3, 257, 1000
    ignored = (0,)
    # pasnl_scan_eval_confusion
    g_out = Guarded(nl * nl * 8, fill, output_guard(nl * 8))
    g_out.inside().zero_()
    logits = distinct_integer_logits(rng, b, npt, nc + 1)
    truth = rng.integers(0, nl, (b, npt)).astype(np.int32)
    eval_confusion(logits, 1, truth, ignored, nl, g_out.ptr)
    np.testing.assert_array_equal(g_out.array((nl, nl), np.int64), want_confusion(softmax_f32(logits[:, :, 1:]), truth, ignored, nl))
    assert g_out.guards_intact()
    # pasnl_scene_eval_vote: two scenes of n rows, the crops select rows of the first half of each
    g_tab = Guarded(2 * n * nc * 8, fill, output_guard(nc * 8))
    init = rng.random((2 * n, nc))
    g_tab.inside().copy_(dev(init).view(torch.uint8).reshape(-1))
    inds = rng.integers(0, n // 2, (b, npt)).astype(np.int32)
    clouds = np.array([1, 0, 1], np.int32)
    win = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    probs = softmax_f32(logits[:, :, 1:])
    eval_vote(probs, 0, inds, clouds, np.array([0, n, 2 * n], np.int64), 0.95, np.float32(1 - 0.95), g_tab.ptr, win)
    want = init.copy().reshape(2, n, nc)
    for k in range(b):
        want[clouds[k]][inds[k]] = 0.95 * want[clouds[k]][inds[k]] + (1 - 0.95) * probs[k]
    got = g_tab.array((2, n, nc), np.float64)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(got[:, n // 2:]), bits(init.reshape(2, n, nc)[:, n // 2:]))
    assert g_tab.guards_intact()
    # pasnl_scene_eval_vote_confusion
    g_sub = Guarded(n * 4, fill, output_guard(4))
    g_cm = Guarded(36 * 8, fill, output_guard(6 * 8))
    g_cm.inside().zero_()
    tab = vote_table(rng, n, 5)
    proj = rng.integers(0, n, 700).astype(np.int32)
    labels = rng.choice(LV, 700).astype(np.int32)
    dt, dl, dp, dlab = dev(tab), dev(LV), dev(proj), dev(labels)
    _hip().launch("pasnl_scene_eval_vote_confusion", "test", L(n), P(dt), 5, L(700), P(dp), P(dlab), P(dl), ig_of((0,), 6), 6,
                  P(g_sub.ptr), P(g_cm.ptr))
    sub_idx, want = want_vote_confusion(tab, proj, labels, (0,))
    np.testing.assert_array_equal(g_sub.array((n,), np.int32), sub_idx)
    np.testing.assert_array_equal(g_cm.array((6, 6), np.int64), want)
    assert g_sub.guards_intact() and g_cm.guards_intact()
    np.testing.assert_array_equal(bits(dt.cpu().numpy()), bits(tab))


# ---- end to end
def gap_logits_t(num_classes):
    """grid_eval_flow_ref.gap_logits on the device: integer operations on the input's bits, so both sides give the same
    float32 logits"""
    c = torch.arange(num_classes, dtype=torch.int32, device="cuda")
    sh = c % 20

    def model(x):
        h = x[:, :, :3].contiguous().view(torch.int32)
        u = ((h[:, :, 0] >> 1) ^ (h[:, :, 1] >> 3) ^ (h[:, :, 2] >> 2)) & 0x7FFFFFFF
        base = (u[:, :, None] >> sh) & 7
        k = 1 + (u >> 5) % (num_classes - 1)
        return (base + 9 * (c == k[:, :, None])).to(torch.float32)

    return model


def make_scene(augment, seed=0, rng_seed=None):
    from pointasnl_amd.ScanNet.scene_evaluator import SceneEvaluator

    pts, cols, labels, vlab, proj = M.scenes()
    return SceneEvaluator(pts, labels, colors=cols, validation_labels=vlab, validation_proj=proj, num_classes=M.CLASSES["scene"],
                          num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER, batch_size=M.BATCH, validation_size=M.VALIDATION_SIZE,
                          label_values=M.LABEL_VALUES, ignored_labels=M.IGNORED, rng=np.random.RandomState(rng_seed or M.SEED["scene"]),
                          seed=seed, augment=augment)


def spy(model, log):
    def wrapped(x):
        out = model(x)
        log.append((x.cpu().numpy().copy(), out.cpu().numpy().copy()))
        return out
    return wrapped


def test_scene_evaluator_three_epochs_equal_the_restatement():
    ev = make_scene(augment=False)
    ref, ref64 = M.scene_ref(), M.scene_ref(softmax=R.softmax_f64)
    gold = np.load(os.path.join(HERE, "golden", "grid_eval_flow.npz"))
    np.testing.assert_array_equal(bits(ev.val_proportions), bits(np.array(
        [sum(int(np.sum(v == l)) for v in M.scenes()[3]) for l in M.LABEL_VALUES if l not in M.IGNORED], np.float32)))
    model_np = M.model("scene")
    log = []
    model = spy(gap_logits_t(M.CLASSES["scene"]), log)
    for e in range(M.EPOCHS):
        del log[:]
        got = ev.run(model, vote=M.VOTE[e])
        want = ref.eval_one_epoch(model_np, vote=M.VOTE[e], seg_label_to_cat=M.CATS)
        want64 = ref64.eval_one_epoch(model_np, vote=M.VOTE[e], seg_label_to_cat=M.CATS)
        assert len(log) == M.VALIDATION_SIZE
        for (x, lg), fed, wl in zip(log, want["fed"], want["logits"]):   # the CPU side: same inputs, same logits, the gap
            np.testing.assert_array_equal(bits(x), bits(fed))
            np.testing.assert_array_equal(bits(lg), bits(wl))
            assert R.top_two_gap(wl) >= 2
        np.testing.assert_array_equal(ev.confusion(), want["Confs"])
        np.testing.assert_array_equal(ev.confusion(), gold["scene/%d/confusion" % e])
        assert ev.confusion().dtype == np.int64 and ev.scored == M.VALIDATION_SIZE
        assert type(got[0]) is np.float32 and got[0] == want["mIoU"] == np.float32(gold["scene/%d/miou" % e][0])
        # the float64 table: the device's against a float64 softmax, no worse than twice numpy-float32's own error
        table = np.concatenate([ev.validation_probs(i).cpu().numpy() for i in range(3)])
        t32, t64 = np.concatenate(ref.validation_probs), np.concatenate(ref64.validation_probs)
        err_dev, err_np = np.abs(table - t64).max(), np.abs(t32 - t64).max()
        print(f"epoch {e}: table worst error vs float64 softmax: device {err_dev:.3e}, numpy float32 {err_np:.3e}")
        assert table.dtype == np.float64 and err_dev <= 2 * err_np
        np.testing.assert_array_equal(table.sum(1) == 0, t32.sum(1) == 0)  # the same points were visited
        if M.VOTE[e]:
            # the CPU side of the voted counts: every visited row of the restatement's table keeps its argmax by far more
            # than the tables differ
            s = np.sort(t32[t32.sum(1) > 0], axis=1)
            assert (s[:, -1] - s[:, -2]).min() > 100 * max(err_dev, err_np)
            np.testing.assert_array_equal(ev.vote_confusion(), want["Confs_vote"])
            assert type(got[1]) is np.float64 and got[1] == want["mIoU_vote"] == gold["scene/%d/miou" % e][1]
        else:
            assert got[1] == 0 and want["mIoU_vote"] == 0
        assert ev.report(M.CATS) == R.report_lines(want["log"]) == R.report_lines(list(gold["scene/%d/log" % e]))
    for a, b in zip(ref.gen.potentials, range(3)):
        np.testing.assert_array_equal(bits(a), bits(ev.potentials_of(b).cpu().numpy()))
    assert ev.rng.randint(1 << 30) == ref.gen.rng.randint(1 << 30)


def test_scene_evaluator_augmented_epoch_scores_what_the_model_saw():
    """augment=True: the crop sequence does not move, the model sees the validation split's augmentation (no symmetry) of
    the restatement's crops, bit for bit the kernel's formula, and the counts are numpy's over what it answered"""
    seed = 0xC0FFEE1234567
    ev = make_scene(augment=True, seed=seed)
    ref = M.scene_ref()
    log = []
    got = ev.run(spy(gap_logits_t(M.CLASSES["scene"]), log), vote=False)
    want = ref.eval_one_epoch(M.model("scene"), vote=False)
    predictions, targets = [], []
    for n, (x, lg) in enumerate(log):
        formula_holds(x, want["fed"][n], seed, n * M.BATCH, cfg=R.VALIDATION)
        np.testing.assert_array_equal(bits(lg), bits(R.gap_logits(x, M.CLASSES["scene"])))
        predictions += list(softmax_f32(lg[:, :, 1:]))
        targets += [M.scenes()[2][c][i] for c, i in zip(want["clouds"][n], want["inds"][n])]
    Confs, _ = R.crop_confusions(predictions, targets, M.LABEL_VALUES, np.asarray(M.IGNORED), M.CLASSES["scene"])
    np.testing.assert_array_equal(ev.confusion(), np.sum(Confs, axis=0))
    assert ev.item == M.VALIDATION_SIZE * M.BATCH and got[0] > 0 and got[1] == 0
    assert PH.crop_params(seed, 0, R.VALIDATION)["scales"].min() > 0  # no symmetry: no negative scale


def make_scan(augment, seed=0):
    from pointasnl_amd.SemanticKITTI.scan_evaluator import ScanEvaluator

    sc, sl = M.scans()
    return ScanEvaluator(sc, sl, num_classes=M.CLASSES["scan"], num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER, batch_size=M.BATCH,
                         ignored_labels=M.IGNORED, rng=np.random.RandomState(M.SEED["scan"]), seed=seed, augment=augment)


def test_scan_evaluator_three_epochs_equal_the_restatement():
    ev = make_scan(augment=False)
    ref = M.scan_ref()
    gold = np.load(os.path.join(HERE, "golden", "grid_eval_flow.npz"))
    model_np = M.model("scan")
    log = []
    model = spy(gap_logits_t(M.CLASSES["scan"]), log)
    assert ev.steps_per_epoch == 3
    for e in range(M.EPOCHS):
        del log[:]
        got = ev.run(model)
        want = ref.eval_one_epoch(model_np, M.CATS)
        assert len(log) == 3
        for (x, lg), fed, wl in zip(log, want["fed"], want["logits"]):
            np.testing.assert_array_equal(bits(x), bits(fed))
            np.testing.assert_array_equal(bits(lg), bits(wl))
            assert R.top_two_gap(wl) >= 2
        np.testing.assert_array_equal(ev.confusion(), want["Confs"])
        np.testing.assert_array_equal(ev.confusion(), gold["scan/%d/confusion" % e])
        assert type(got) is np.float32 and got == want["mIoU"] == np.float32(gold["scan/%d/miou" % e][0])
        assert ev.report(M.CATS) == R.report_lines(want["log"]) == R.report_lines(list(gold["scan/%d/log" % e]))
    assert ev.gen.rng.randint(1 << 30) == ref.gen.rng.randint(1 << 30)


def test_scan_evaluator_augmented_epoch_scores_what_the_model_saw():
    seed = 77
    ev = make_scan(augment=True, seed=seed)
    ref = M.scan_ref()
    log = []
    got = ev.run(spy(gap_logits_t(M.CLASSES["scan"]), log))
    want = ref.eval_one_epoch(M.model("scan"), M.CATS)
    predictions, targets = [], []
    labels = M.scans()[1]
    for n, (x, lg) in enumerate(log):
        formula_holds(x, want["fed"][n], seed, n * M.BATCH, cfg=R.VALIDATION)
        predictions += list(softmax_f32(lg[:, :, 1:]))
        targets += [labels[c][i] for c, i in zip(want["clouds"][n], want["inds"][n])]
    Confs, _ = R.crop_confusions(predictions, targets, np.arange(5), np.asarray(M.IGNORED), 5)
    np.testing.assert_array_equal(ev.confusion(), np.sum(Confs, axis=0))
    assert got > 0


def test_a_batch_enqueues_without_host_synchronisation():
    """one batch of each evaluator -- the generator's chain, the forward, the vote and the confusions -- captured into a
    graph (a synchronisation would fail the capture) and replayed after every `stage`: the matrix, the table and the
    potentials equal the eager evaluator's"""
    for make, is_scene in ((make_scene, True), (make_scan, False)):
        eager, cap = make(augment=True, seed=5), make(augment=True, seed=5)
        name = "scene" if is_scene else "scan"
        model = gap_logits_t(M.CLASSES[name])
        ge, gc = (eager, cap) if is_scene else (eager.gen, cap.gen)
        for n in range(3):
            ge.stage(ge.draw_batch() if is_scene else ge.draw_batch(n * M.BATCH))
            eager.enqueue_batch(model)
        gc.stage(gc.draw_batch() if is_scene else gc.draw_batch(0))
        B, npt, W = M.BATCH, M.NUM_POINT, 6 if is_scene else 3
        out = (torch.empty((B, npt, W), device="cuda"), torch.empty((B, npt), dtype=torch.int32, device="cuda"),
               torch.empty((B, npt), device="cuda"), torch.empty((B, npt), dtype=torch.int32, device="cuda"),
               torch.empty((B,), dtype=torch.int32, device="cuda"))
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                cap.enqueue_batch(model, out)
        torch.cuda.current_stream().wait_stream(s)
        g.replay()
        for n in range(1, 3):
            if is_scene:
                gc.stage(gc.draw_batch())
                g.replay()
            else:  # the scan indices are kernel arguments of the captured pick: the other list positions run eagerly
                gc.stage(gc.draw_batch(n * M.BATCH))
                cap.enqueue_batch(model)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(cap.confusion_dev.cpu().numpy(), eager.confusion_dev.cpu().numpy())
        assert int(cap.confusion_dev.sum()) == 3 * B * npt
        if is_scene:
            np.testing.assert_array_equal(bits(cap.probs.cpu().numpy()), bits(eager.probs.cpu().numpy()))
            np.testing.assert_array_equal(bits(cap.potentials.cpu().numpy()), bits(eager.potentials.cpu().numpy()))
            assert float(cap.probs.sum()) > 0
