"""GPU: the ScanNet grid training input loop on the device (pointasnl_amd.ScanNet.scene_trainer: SceneTester's chain,
pasnl_scan_train_labels, pasnl_scan_augment, pasnl_block_train_score) against the numpy restatement
tests/grid_train_flow_ref.py run live under the same seed (tests/test_grid_train_flow.py pins it to the reference's own
generator).  Indices, clouds, labels, weights, potentials and unaugmented inputs are compared by bits; augmented inputs
against the kernel's formula by bits; the tallies exactly; the loss within the block trainers' tolerance."""
import numpy as np
import pytest

import grid_train_flow_ref as R
from grid_train_checks import bits, formula_holds, host, same_batch, same_epoch, stand_in_step
from scene_flow_ref import scene

pytestmark = pytest.mark.gpu

SIZES, NPOINT, BUFFER, B, STEPS = (700, 450, 900), 64, 24, 2, 5
LABEL_VALUES = np.array([0, 1, 2, 4, 7, 9])
C = len(LABEL_VALUES)
WEIGHTS = np.array([0.0, 1.3, 0.7, 2.1, 1.0, 1.9])
AUG_SEED = 0xC0FFEE1234567


@pytest.fixture(scope="module")
def data():
    pc = [scene(900 + i, n) for i, n in enumerate(SIZES)]
    lrng = np.random.default_rng(2)
    return [p for p, _ in pc], [c for _, c in pc], [lrng.choice(LABEL_VALUES, n).astype(np.int32) for n in SIZES]


def make(data, rng_seed, with_rgb=True, **kw):
    from pointasnl_amd.ScanNet.scene_trainer import SceneTrainer

    scenes, colors, labels = data
    t = SceneTrainer(scenes, labels, colors=colors if with_rgb else None, num_classes=C, num_point=NPOINT, num_buffer=BUFFER,
                     batch_size=B, epoch_steps=STEPS, label_values=LABEL_VALUES, label_weights=WEIGHTS, with_rgb=with_rgb,
                     rng=np.random.RandomState(rng_seed), **kw)
    ref = R.SceneTrainFlowRef(scenes, labels, colors=colors, label_weights=WEIGHTS, num_classes=C, num_point=NPOINT,
                              num_buffer=BUFFER, batch_size=B, epoch_steps=STEPS, label_values=LABEL_VALUES,
                              rng=np.random.RandomState(rng_seed))
    return t, ref


def same_state(t, ref):
    for i in range(len(SIZES)):
        np.testing.assert_array_equal(bits(host(t.potentials_of(i))), bits(ref.potentials[i]))
    np.testing.assert_array_equal(bits(t.min_potentials()), bits(np.asarray(ref.min_potentials, np.float64)))


@pytest.mark.parametrize("with_rgb", [True, False])
def test_sixty_crops_equal_the_restatement(data, with_rgb):
    """30 batches of 2 crops, unaugmented: everything by bits, the potentials after every batch, the RNG still in step"""
    t, ref = make(data, 11, with_rgb=with_rgb, augment=False)
    same_state(t, ref)
    for _ in range(30):
        got = t.next_batch()
        want = ref.batch(with_rgb=with_rgb)
        x = same_batch(got, want)
        assert x.shape == (B, NPOINT, 6 if with_rgb else 3)
        same_state(t, ref)
    assert t.rng.randint(1 << 30) == ref.rng.randint(1 << 30)
    assert t.item == 0  # nothing was augmented


def test_augmented_batches_are_the_formula(data):
    """the same 60 crops with the augmentation on: the crop sequence does not move (the augmentation draws nothing from
    numpy), every input equals the formula under (seed, running crop number), colours are kept at augment_color = 1.0"""
    t, ref = make(data, 11, augment=True, seed=AUG_SEED)
    for n in range(30):
        got = t.next_batch()
        want = ref.batch()
        x = same_batch(got, want, augmented=True)
        formula_holds(x, want[0], AUG_SEED, n * B)
        np.testing.assert_array_equal(bits(x[:, :, 3:]), bits(want[0][:, :, 3:]))
    same_state(t, ref)
    assert t.item == 60


def test_colour_drop_and_validation_generator(data):
    """augment_color = 0.5 drops whole crops' colours; symmetries off and weights of zero give D's validation split"""
    t, ref = make(data, 12, augment=True, seed=3, augment_config=dict(augment_color=0.5, augment_symmetries=(False, False, False)))
    kept = set()
    for n in range(8):
        x = host(t.next_batch()[0])
        want = ref.batch()
        for c in range(B):
            k = float(np.abs(x[c, :, 3:]).max() > 0)
            kept.add(k)
            np.testing.assert_array_equal(bits(x[c, :, 3:]), bits((want[0][c, :, 3:] * np.float32(k)).astype(np.float32)))
    assert kept == {0.0, 1.0}


def test_one_epoch_of_run(data):
    t, ref = make(data, 13, augment=True, seed=AUG_SEED)
    w, b = R.stand_in_weights(7, C)
    log = []
    acc = t.run(stand_in_step(w, b, log))
    assert len(log) == STEPS
    same_epoch(t, acc, log, C)
    for n in range(STEPS):  # what the step saw: the restatement's crops, augmented
        want = ref.batch()
        np.testing.assert_array_equal(log[n][1], want[1])
        np.testing.assert_array_equal(bits(log[n][2]), bits(want[2]))
        formula_holds(log[n][0], want[0], AUG_SEED, n * B)
    same_state(t, ref)
    acc2 = t.run(stand_in_step(w, b, log))  # a second epoch goes on from the first one's potentials and crop numbers
    assert len(log) == 2 * STEPS and t.item == 2 * STEPS * B and 0 < acc2 < 1
    same_epoch(t, acc2, log[STEPS:], C)
    for n in range(STEPS):
        ref.batch()
    same_state(t, ref)


def test_captured_chain_replays_with_fresh_numbers(data):
    """`enqueue` captured once and replayed after every `stage`: crops, labels, weights and augmented inputs equal the eager
    trainer's batch after batch -- the draws and the augmentation's crop number reach the replay through the staged buffers"""
    import torch

    eager, _ = make(data, 17, augment=True, seed=AUG_SEED)
    cap, _ = make(data, 17, augment=True, seed=AUG_SEED)
    want = [[host(t).copy() for t in eager.next_batch()] for _ in range(4)]
    out = (torch.empty((B, NPOINT, 6), device="cuda"), torch.empty((B, NPOINT), dtype=torch.int32, device="cuda"),
           torch.empty((B, NPOINT), device="cuda"), torch.empty((B, NPOINT), dtype=torch.int32, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cap.enqueue(out)
    torch.cuda.current_stream().wait_stream(s)
    for n, w in enumerate(want):
        cap.stage(cap.draw_batch())
        g.replay()
        for a, b in zip(out, w):
            np.testing.assert_array_equal(bits(host(a)), bits(b))
        if n:
            assert (bits(want[n][0]) != bits(want[n - 1][0])).any()
    assert cap.item == eager.item == 4 * B
    same = [np.array_equal(bits(host(cap.potentials_of(i))), bits(host(eager.potentials_of(i)))) for i in range(len(SIZES))]
    assert all(same)


def test_error_paths(data):
    from pointasnl_amd.ScanNet.scene_trainer import SceneTrainer

    scenes, colors, labels = data
    kw = dict(colors=colors, num_classes=C, num_point=NPOINT, num_buffer=BUFFER, batch_size=B, epoch_steps=STEPS,
              label_values=LABEL_VALUES, label_weights=WEIGHTS)
    with pytest.raises(IndexError):  # class index 5 has no weight
        SceneTrainer(scenes, labels, **dict(kw, label_weights=WEIGHTS[:5]))
    with pytest.raises(KeyError):    # a label that label_to_idx does not hold
        SceneTrainer(scenes, [np.full_like(l, 3) for l in labels], **kw)
    with pytest.raises(ValueError, match="scene 1 has 450 points"):
        SceneTrainer(scenes, labels, **dict(kw, num_point=440))  # 440 + 24 + 6 - 1 = 469 > 450
    with pytest.raises(NotImplementedError):
        SceneTrainer(scenes, labels, in_radius=1.0, **kw)
    with pytest.raises(ValueError):
        SceneTrainer(scenes, labels[:2], **kw)
    with pytest.raises(TypeError):
        SceneTrainer(scenes, labels, abs_coords=True, **kw)  # tf_map drops those columns (D:562)
