"""fps_kernel's tie rule (csrc/sampling.hip) -- largest distance, then lowest k mod 512, then lowest k -- with equal maxima
planted where each stage of its reduction has to tell them apart: in two leaves of one lane's tournament (lane t keeps points
i*T + t, T = 64 * waves), in two lanes of one wave, in two waves, and at k and k + 512; lattice clouds sampled to the last point
end on rounds whose maximum is 0, where every remaining point ties.  Picks are compared index for index with the oracle, the
gathered coordinates bit for bit with O.gather_point, through both entry points."""
import functools

import numpy as np
import pytest
import torch

from conftest import clouds
from oracle import ops as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import pointasnl_amd

    return pointasnl_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_fps(P, xyz, m, want, entry):
    b = xyz.shape[0]
    if entry == "plain":
        got = P.tf_sampling.farthest_point_sample(m, dev(xyz)).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (b, m)
        np.testing.assert_array_equal(got, want)
    else:
        idx, new_xyz = P.tf_sampling.farthest_point_sample_gather(m, dev(xyz))
        idx, new_xyz = idx.cpu().numpy(), new_xyz.cpu().numpy()
        assert idx.dtype == np.int32 and idx.shape == (b, m) and new_xyz.dtype == np.float32 and new_xyz.shape == (b, m, 3)
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_array_equal(new_xyz.view(np.uint32), O.gather_point(xyz, want).view(np.uint32))


LATER = 5  # the "later pick": round 5


def plant(base, pairs):
    """A cloud with the geometry of `base` (b, n, 3; no ties of its own) in which the point farthest from point 0 -- the pick of
    round 1 -- sits at both indices of pairs[0] and the pick of round LATER at both of pairs[1].  Two points that no early round
    picks make room, so rounds 1 .. LATER choose the same positions as in `base`, each of the two now from a tie."""
    b, n, _ = base.shape
    picks = O.farthest_point_sample(LATER + 3, base)
    (u1, v1), (u2, v2) = pairs
    targets = {u1: 1, v1: 1, u2: LATER, v2: LATER}
    assert len(targets) == 4 and 0 not in targets and max(targets) < n
    free = [i for i in range(n) if i not in targets]
    out = np.empty_like(base)
    for c in range(b):
        early = set(picks[c].tolist())
        rest = [i for i in range(n) if i not in (picks[c, 1], picks[c, LATER])]
        drop = [i for i in reversed(rest) if i not in early][:2]
        rest = [i for i in rest if i not in drop]
        assert rest[0] == 0 and len(rest) == len(free)
        out[c, free] = base[c, rest]
        for pos, rnd in targets.items():
            out[c, pos] = base[c, picks[c, rnd]]
    return out


# (n, lanes of the workgroup T, kernel form): fps_dispatch's choice for b <= 640
SHAPES = [(1024, 256, "<4,4,4>"), (700, 256, "<4,4,4> padded"), (512, 64, "<1,8>"), (300, 64, "<1,8> padded"), (200, 64, "<1,4>"),
          (100, 64, "<1,2>"), (2048, 256, "<4,8>")]
U1, U2 = 5, 20


def tie_pairs(where, n, T):
    """(round 1's pair, round LATER's pair).  The lower index wins wherever it has the lower k mod 512; where the cloud reaches
    past index 512 the later pair of "leaves" and "waves" straddles it, so that there the HIGHER index has to win."""
    d = {"leaves": T, "lanes": 1, "waves": 64, "mod512": 512}[where]
    u2 = U2
    if n > 600 and where in ("leaves", "waves"):
        u2 = 300 if where == "leaves" else 480  # (300, 556) and (480, 544): k mod 512 = 44 and 32 for the second
    return ((U1, U1 + d), (u2, u2 + d))


CASES = [(n, T, where) for n, T, _ in SHAPES for where in ("leaves", "lanes", "waves", "mod512")
         if U2 + {"leaves": T, "lanes": 1, "waves": 64, "mod512": 512}[where] < n and not (where == "waves" and T == 64)]


@functools.lru_cache(maxsize=None)
def planted_case(n, T, where):
    m = 64
    pairs = tie_pairs(where, n, T)
    xyz = plant(clouds(4000 + n, 2, n, "ball"), pairs)
    want = O.farthest_point_sample(m, xyz)
    # the ties are there: both rounds chose one of their two positions, and the positions hold one point
    for (u, v), rnd in zip(pairs, (1, LATER)):
        assert np.isin(want[:, rnd], (u, v)).all() and (xyz[:, u] == xyz[:, v]).all()
    if pairs[1][0] != U2:
        assert (want[:, LATER] == pairs[1][1]).all()  # the pair across index 512: the higher index wins
    return xyz, m, want


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("n,T,where", CASES, ids=[f"n{n}-{w}" for n, _, w in CASES])
def test_fps_planted_ties(P, n, T, where, entry):
    xyz, m, want = planted_case(n, T, where)
    check_fps(P, xyz, m, want, entry)


@functools.lru_cache(maxsize=None)
def lattice_case(n):
    xyz = clouds(4100 + n, 2, n, "lattice")  # at most 729 positions: ties in most rounds, and nothing but zeros at the end
    want = O.farthest_point_sample(n, xyz)
    return xyz, want


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("n", [513, 1024])
def test_fps_lattice_every_point_sampled(P, n, entry):
    xyz, want = lattice_case(n)
    assert len(np.unique(xyz[0], axis=0)) < n  # the last rounds run with maximum 0
    check_fps(P, xyz, n, want, entry)


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("n", [100, 512, 1024, 2048])
def test_fps_single_pick(P, n, entry):
    xyz = clouds(4200 + n, 2, n, "ball")
    check_fps(P, xyz, 1, np.zeros((2, 1), np.int32), entry)


@functools.lru_cache(maxsize=None)
def one_wave_case(n):
    """b = 641 clouds of 513..1024 points: fps_kernel<1,16>, lane t keeps points i*64 + t, i < 16.  Leaves i and i + 8 of a lane
    are 512 indices apart.  At n = 513 leaf 8 holds index 512 alone (lane 0) and its partner in leaf 0 is index 0, the start point,
    which no round can pick: there the ties are planted in lane 0's leaves 4 and 8 (256, 512) and in lane 5's leaves 0 and 5
    (5, 325); at n = 1024 in leaves 0 and 8 of lane 5 and leaves 1 and 9 of lane 20 (same k mod 512: the lower index wins)."""
    pairs = ((256, 512), (5, 325)) if n == 513 else ((5, 517), (84, 596))
    xyz = plant(clouds(4300 + n, 641, n, "ball"), pairs)
    want = O.farthest_point_sample(16, xyz)
    for (u, v), rnd in zip(pairs, (1, LATER)):
        assert np.isin(want[:, rnd], (u, v)).all()
    if n == 1024:
        assert (want[:, 1] == 5).all() and (want[:, LATER] == 84).all()
    return xyz, want


@pytest.mark.parametrize("entry", ["plain", "gather"])
@pytest.mark.parametrize("n", [513, 1024])
def test_fps_one_wave_sixteen_leaves(P, n, entry):
    xyz, want = one_wave_case(n)
    check_fps(P, xyz, 16, want, entry)
