"""CPU: tests/philox_ref.py, the host restatement of pasnl_scan_augment's generator -- Philox4x32-10 against the known
answers of the Random123 distribution (kat_vectors: philox4x32 10), the uniform's range, the symmetry rule against
tf.round(u) * 2 - 1 and the colour drop at the reference's augment_color = 1.0."""
import numpy as np

import philox_ref as P

KAT = [  # counter, key, expected words
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = P.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert tuple(int(v) for v in got) == want
    batch = P.philox4x32_10(np.array([k[0] for k in KAT[:1] * 3], np.uint32), np.array(KAT[0][1], np.uint32))
    assert batch.shape == (3, 4) and (batch == np.array(KAT[0][2], np.uint32)).all()


def test_counter_layout():
    """words(seed, item, j, stream) is the block at counter (j, item lo, item hi, stream) under key (seed lo, seed hi)"""
    seed, item = 0x299f31d0a4093822, 0x1319_8a2e_85a3_08d3
    got = P.words(seed, item, 0x243f6a88, 0x03707344)
    assert tuple(int(v) for v in got) == KAT[2][2]
    many = P.words(seed, item, np.array([0x243f6a88, 7]), 0x03707344)
    assert many.shape == (2, 4) and tuple(int(v) for v in many[0]) == KAT[2][2]
    assert not (many[1] == many[0]).any()


def test_uniform_is_exact_and_half_open():
    u = P.uniform(np.array([0, 0xff, 0x100, 0x80000000, 0xffffffff], np.uint32))
    assert u.dtype == np.float32
    assert list(u) == [0.0, 0.0, 2.0 ** -24, 0.5, 1 - 2.0 ** -24] and u.max() < 1


def test_symmetry_rule_is_tf_round():
    u = np.array([0, 0.5, 0.5 + 2.0 ** -24, 1 - 2.0 ** -24], np.float32)
    assert u[2] > u[1]  # representable
    np.testing.assert_array_equal(P.symmetry(u), (np.round(u) * 2 - 1).astype(np.float32))  # np.round: half to even, as tf.round
    assert list(P.symmetry(u)) == [-1, -1, 1, 1]


def test_keep_is_always_one_at_color_one():
    for item in range(400):
        assert P.crop_params(5, item)["keep"] == 1
    cfg = dict(P.DEFAULT, color=0.5)
    kept = sum(int(P.crop_params(5, item, cfg)["keep"]) for item in range(400))
    assert 150 < kept < 250  # 200 +- 5 sigma of a fair coin (sigma = sqrt(400) / 2 = 10)


def test_params_follow_the_config():
    q = P.crop_params(9, 3)
    assert q["theta"].dtype == np.float32 and 0 <= q["theta"] < np.float32(2 * np.pi) * 1
    assert (np.abs(q["scales"]) >= np.float32(0.9)).all() and (np.abs(q["scales"]) <= np.float32(1.1) + np.float32(2.0 ** -23)).all()
    assert (q["scales"][1:] > 0).all()  # only x may flip
    iso = P.crop_params(9, 3, dict(P.DEFAULT, anisotropic=False, symmetries=(False,) * 3))
    assert iso["scales"][0] == iso["scales"][1] == iso["scales"][2] == abs(q["scales"][0])
    none = P.crop_params(9, 3, dict(P.DEFAULT, rotation="none"))
    assert none["theta"] == 0 and (none["scales"] == q["scales"]).all()


def test_host_augmentation_is_the_formula():
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((2, 50, 6)).astype(np.float32)
    out = P.augment(pts, 17, 40)
    again = P.augment(pts, 17, 40)
    np.testing.assert_array_equal(out.view(np.int32), again.view(np.int32))
    np.testing.assert_array_equal(out[:, :, 3:], pts[:, :, 3:])  # color = 1.0
    assert np.abs(np.linalg.norm(out[:, :, :2], axis=2) / np.linalg.norm(pts[:, :, :2], axis=2) - 1).max() < 0.12
    n = P.normals64(17, 40, 4096)
    se = 1 / np.sqrt(n.size)
    assert abs(n.mean()) < 5 * se and abs(n.var() - 1) < 5 * np.sqrt(2) * se
