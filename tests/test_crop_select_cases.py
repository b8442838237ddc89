"""CPU side of tests/test_gpu_crop_select.py: every case of tests/crop_select_cases.py is where it claims to be in the pass
structure of csrc/crop.hip (the mirror's trace says so), the oracle's selection equals a second statement of it (one full sort by
(key, index)) and the mirror's, and the cases can tell the mirror from four wrong versions of it -- so nobody has to break a
kernel on a GPU to know that the GPU tests would notice.  Oracle and numpy alone."""
import numpy as np
import pytest

import crop_select_cases as E


def crops(case):
    """(crop, keys, k, claim) of a k-form direct case"""
    for c in range(case["b"]):
        yield c, E.key_bits(E.scan_of(case, c), case["centres"][c]), min(case["ks"][c], case["kcap"]), case["claims"][c]


def test_restated_constants():
    assert sum(E.WIDTHS) == 63 and all(E.SHIFTS[p] == sum(E.WIDTHS[p + 1:]) for p in range(5))
    assert E.CR_BLOCK == 2048 and E.CR_WAVE == 512 and E.PER == 32 and E.PER * E.CR_THREADS == 1 << E.WIDTHS[0]
    assert E.find_bin(np.array([0, 2, 0, 3]), 1) == (1, 0, 2) and E.find_bin(np.array([0, 2, 0, 3]), 2) == (1, 0, 2)
    assert E.find_bin(np.array([0, 2, 0, 3]), 3) == (3, 2, 3) and E.find_bin(np.array([0, 2, 0, 3]), 5) == (3, 2, 3)
    assert E.find_bin(np.array([0, 2, 0, 3]), 6) == (0, 0, 0) and E.find_bin(np.array([0, 2, 0, 3]), 0) == (0, 0, 0)
    assert len(E.RING_JL) == 1644 and len(np.unique((E.RING_JL ** 2).sum(1))) == 630 and (E.RING_JL ** 2).sum(1).max() == 2045
    assert all(len(E.DIRECT[name]()["points"]) <= 10000 for name in E.DIRECT)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_digit_cases_are_decided_in_their_pass(p):
    case = E.digit_case(p)
    ring = case["claims"][0]["ring"]
    # the ring lies in at least 3 blocks and does not start on a block's edge
    assert len(np.unique(ring // E.CR_BLOCK)) >= 3 and ring[0] % E.CR_BLOCK != 0
    kx = E.bits_of(np.array([np.float64(E.ring_x0(p)) ** 2]))
    assert all(E.digit(kx, q)[0] != 0 for q in range(5) if q != p)
    seen = {}
    for c, keys, k, claim in crops(case):
        assert len(np.unique(keys[ring])) == 630 and claim["nearer"] == 300 and k == 300 + claim["r0"]
        assert all(len(np.unique(E.digit(keys[ring], q))) == 1 for q in range(5) if q != p)   # they differ in digit p alone
        recs = E.trace(keys, k)
        rec = recs[p]
        print(f"digit_p{p} {claim['variant']}: k = {k}, pass {p}, bin {rec['bin']}, before {rec['before']}, inbin {rec['inbin']}, "
              f"r {rec['r']}, {rec['nonempty']} bins, {len(recs)} passes run")
        assert E.deciding_pass(recs) == p and rec["nonempty"] == 630 and rec["before"] > 0
        assert all(recs[q]["bin"] != 0 for q in range(p)) and recs[0]["nonempty"] >= 2
        assert all(recs[q]["nonempty"] == 1 and recs[q]["before"] == 0 for q in range(1, len(recs)) if q != p)
        v = claim["variant"]
        if v == "one_of_many":
            assert rec["inbin"] >= 2 and rec["r"] == 1 and len(recs) == 5
        elif v == "inside_tie":
            assert rec["inbin"] >= 3 and 1 < rec["r"] < rec["inbin"] and len(recs) == 5
        elif v == "whole":
            assert rec["inbin"] >= 2 and rec["r"] == rec["inbin"] and len(recs) == p + 1   # the early end, in pass p
        else:
            assert rec["bin"] == rec["last"] and rec["r"] < rec["inbin"]
            assert p < 4 or rec["bin"] == 2045
        seen[v] = rec["bin"]
    assert len(set(seen.values())) == 4


@pytest.mark.parametrize("b", list(E.SEAMS))
def test_findbin_cases_sit_on_the_seams(b):
    case = E.findbin_case(b)
    assert (b % E.PER, (b // E.PER) % 64) == E.SEAMS[b]
    for c, keys, k, claim in crops(case):
        rec = E.trace(keys, k)[0]
        print(f"findbin_{b} {claim['at']}: k = {k}, pass 0, bin {rec['bin']} (bin % 32 = {b % 32}, thread {b // 32}), before {rec['before']}, "
              f"inbin {rec['inbin']}")
        assert rec["bin"] == b and rec["inbin"] >= 4 and (rec["before"] > 0 or b == 0) and rec["nonempty"] >= 3
        assert k == rec["before"] + (1 if claim["at"] == "first" else rec["inbin"])   # r == base + 1 | r == base + sum
    # the seams, taken together: a thread's first and last bin, a wave's first and last thread, every wave's partial sums
    assert {s[0] for s in E.SEAMS.values()} >= {0, 31} and {s[1] for s in E.SEAMS.values()} == {0, 63}
    assert {x // E.PER // 64 for x in E.SEAMS} == {0, 1, 2, 3}


@pytest.mark.parametrize("cloud", ["copies", "scattered"])
def test_tiecut_cases_cut_where_they_claim(cloud):
    case = E.tiecut_case(cloud)
    cuts = []
    for c, keys, k, claim in crops(case):
        sel = E.lexsort_select(keys, k)
        cut = E.cut_position(keys, sel)
        assert cut["ties"] == claim["ties"] and cut["kept"] == k - claim["nearer"] and 0 < cut["kept"] < cut["ties"]
        cuts.append(cut)
    kept = [cut["kept"] for cut in cuts]
    assert kept[:-1] == [1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4096, 4097] and kept[-1] == cuts[0]["ties"] - 1
    if cloud == "copies":  # the cut is at index k - 1: the last item of a thread, of a wave, of a block, and one to either side
        assert [cut["index"] for cut in cuts] == [k - 1 for k in kept]
        assert [cut["item"] for cut in cuts[:4]] == [0, 6, 7, 0]
        assert [(cut["block"], cut["wave"], cut["item"]) for cut in cuts[4:12]] == [(0, 0, 6), (0, 0, 7), (0, 1, 0), (0, 3, 6), (0, 3, 7),
                                                                                    (1, 0, 0), (1, 3, 7), (2, 0, 0)]
        assert cuts[-1]["block"] == 3 and cuts[-1]["index"] == E.TIE_N - 2
    else:                  # scattered: the cuts fall in every block, every wave and most item positions
        assert len({cut["block"] for cut in cuts}) >= 4 and {cut["wave"] for cut in cuts} == {0, 1, 2, 3}
        assert len({cut["item"] for cut in cuts}) >= 5


def test_radius_and_nonfinite_cases():
    tiny, huge, on = E.radius_case("tiny"), E.radius_case("huge"), E.radius_case("on_radius")
    with np.errstate(over="ignore", under="ignore"):
        assert np.float64(tiny["radius"]) ** 2 == 0.0 and np.float64(huge["radius"]) ** 2 == np.inf
    assert [len(E.want(tiny, c)[0]) for c in range(2)] == [5, 1]            # the copies of the centre | the centre's own point
    assert [len(E.want(huge, c)[0]) for c in range(2)] == [2999, 2999]      # everything but the NaN key, +inf included
    keys = E.key_bits(on["points"], on["centres"][0])
    r2 = E.bits_of(np.array([np.float64(on["radius"]) ** 2]))[0]
    sel, _ = E.want(on, 0)
    assert r2 == keys[on["claims"][0]["on"]] and (keys == r2).sum() >= 2 and (keys[sel] == r2).sum() == (keys == r2).sum()
    assert (keys > r2).any() and E.digit(keys[keys == r2], 4)[0] != 0
    case = E.nonfinite_case()
    keys = E.key_bits(case["points"], case["centres"][0])
    nan = sorted(E.NONFINITE["nan"] + E.NONFINITE["neg_nan"])
    assert (keys[nan] == 0x7FF8000000000000).all() and (keys[list(E.NONFINITE["inf"])] == 0x7FF0000000000000).all()
    assert (keys < 0x7FF0000000000000).sum() == case["n"] - 7
    raw = E.crop_d2(case["points"], case["centres"][0]).view(np.uint64)
    print("sign bit of the host's d2 at the sign-set NaN points:", (raw[list(E.NONFINITE["neg_nan"])] >> np.uint64(63)).tolist())
    for c, drop in enumerate([[], nan[-1:], nan[-2:], nan[-3:]]):   # "NaNs included": dropped from the highest index down
        sel, d2 = E.want(case, c)
        np.testing.assert_array_equal(sel, np.setdiff1d(np.arange(case["n"]), drop))
        np.testing.assert_array_equal(d2, keys[sel])


@pytest.mark.parametrize("name", list(E.DIRECT))
def test_oracle_agrees_with_a_full_sort_and_with_the_mirror(name):
    case = E.DIRECT[name]()
    for c in range(case["b"]):
        keys = E.key_bits(E.scan_of(case, c), case["centres"][c])
        sel, d2 = E.want(case, c)
        if case["radius"] > 0:
            with np.errstate(over="ignore", under="ignore"):
                r2 = E.bits_of(np.array([np.float64(case["radius"]) * np.float64(case["radius"])]))[0]
            second = np.nonzero(keys <= r2)[0]
        else:
            k = min(case["ks"][c], case["kcap"])
            second = E.lexsort_select(keys, k)
            np.testing.assert_array_equal(E.select(keys, k)[1], sel)
        np.testing.assert_array_equal(second, sel)
        np.testing.assert_array_equal(d2, keys[sel])
        assert sel.dtype == np.int32 and (np.diff(sel) > 0).all()


def test_desc_multi_and_sort_sweep_inputs():
    case = E.desc_multi()
    assert case["ns"] == [700, 2048, 5000] and case["nmax"] == 5000 and len(case["points"]) == 7748
    assert case["ks"][0] == 0 and case["ks"][1] >= case["ns"][1] and 0 < case["ks"][2] < case["ns"][2] and max(case["ks"]) <= case["kcap"]
    assert (case["scene_desc"]["cx"] == case["scan_desc"]["cx"]).all()   # float32-representable centres
    lo = int(case["offsets"][2])
    keys = E.key_bits(case["points"][lo:], case["centres"][2])
    recs = E.trace(keys, case["ks"][2])
    assert E.deciding_pass(recs) == 3 and recs[3]["before"] > 0 and recs[3]["inbin"] >= 2 and recs[3]["r"] == 1
    for c in range(3):
        sel, d2 = E.want_desc(case, c)
        np.testing.assert_array_equal(sel, E.select(E.key_bits(case["points"][int(case["offsets"][c]):][:case["ns"][c]], case["centres"][c]), case["ks"][c])[1])
    assert E.SORT_M[:130] == list(range(1, 131)) and E.SORT_M[-2:] == [14335, 14336] and len(E.SORT_M) == 150
    assert {255, 256, 257, 8191, 8192, 8193} <= set(E.SORT_M)
    groups = E.sort_groups()
    assert sorted(m for g in groups for m, _ in g) == sorted(E.SORT_M * 3) and all(len(g) <= 64 for g in groups)
    assert [m for m, _ in groups[-1]] == [E.OP_CAP] * 3
    g = E.sort_group(2)
    for c, m in enumerate(g["ms"]):
        assert (np.diff(g["idx"][c, :m]) > 0).all() and sorted(g["perm"][c, :m]) == list(range(m)) and len(np.unique(g["d2"][c, :m])) <= 5
        assert g["perm"][c].max() < m and set(g["select"][c]) <= set(g["idx"][c, :m])


def test_the_cases_discriminate():
    """Every wrong version of the mirror changes the selected set of at least one case, and every variant of digit_p3 and
    digit_p4 is changed by at least one of them."""
    caught = {m: [] for m in E.MUTANTS}
    by_variant = {}
    for name in E.DIRECT:
        case = E.DIRECT[name]()
        if case["radius"] > 0:
            continue
        for c, keys, k, claim in crops(case):
            right = E.select(keys, k)[1]
            for m in E.MUTANTS:
                if not np.array_equal(E.select(keys, k, m)[1], right):
                    caught[m].append((name, c))
                    if claim.get("kind") == "digit":
                        by_variant.setdefault((claim["p"], claim["variant"]), []).append(m)
    for m in E.MUTANTS:
        print(f"{m}: changes {len(caught[m])} crops, first {caught[m][:4]}")
        assert caught[m], m
    for p in (3, 4):
        for v in E.VARIANTS:
            print(f"digit_p{p} {v}: changed by {by_variant.get((p, v))}")
            assert by_variant.get((p, v)), (p, v)
