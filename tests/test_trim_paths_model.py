"""tests/trim_paths_model.py, the string-level restatement of runTrimPaths that mc_trim_paths is held to, against the oracle's
own trim (oracle/ mco_bfs with trim: `kept`) on walks whose caps bite, and against hand-written answers on designed shapes.
No GPU."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import trim_paths_model as tm


def oracle_case(k, mode):
    """the walk case's table (oracle), seeds and max_radius"""
    codes, off, seeds, radius = tm.walk_case(k)
    t = po.Table()
    t.count_reads(codes, off, k, mode)
    return t, seeds, radius


ORACLE_CASES = [(5, po.KEY_PACKED), (21, po.KEY_PACKED), (31, po.KEY_PACKED), (33, po.KEY_POLY), (63, po.KEY_POLY)]


@pytest.mark.parametrize("k,mode", ORACLE_CASES)
@pytest.mark.parametrize("direction", [-1, 1, 0])
def test_model_is_the_oracles_trim(k, mode, direction):
    t, seeds, radius = oracle_case(k, mode)
    r = po.bfs(t, k, mode, seeds, direction, 2, -1, radius, True)
    assert r is not None
    n = len(r["lo"])
    assert 0 < int(r["kept"].sum()) < n  # (the trim bites, and not everything goes)
    got = tm.kept_mask(tm.unpack_kmers(r["hi"], r["lo"], k), r["last"], direction)
    assert np.array_equal(got, r["kept"])


def test_packing_round_trip():
    rng = np.random.default_rng(3)
    for k in (1, 2, 31, 32, 33, 63):
        kmers = ["".join(tm.NUCLEOTIDES[c] for c in rng.integers(0, 4, k)) for _ in range(20)] + ["T" * k, "A" * k]
        hi, lo = tm.pack_kmers(kmers)
        assert tm.unpack_kmers(hi, lo, k) == kmers
        assert (k > 32) == bool(hi.any())
    hi, lo = tm.pack_kmers(["T" * 32, "GA"])
    assert int(lo[0]) == 2 ** 64 - 1 and int(lo[1]) == 0b0100
    assert tm.revcomp("AAGC") == "GCTT"


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_chain_by_hand(n):
    kmers, last = tm.chain(np.random.default_rng(n), 21, n)
    at = n // 3
    assert sum(last) == 1 and last[at] == 1
    assert tm.kept_mask(kmers, last, +1).tolist() == [1] * (at + 1) + [0] * (n - at - 1)  # what reaches it by right steps: before it
    assert tm.kept_mask(kmers, last, -1).tolist() == [0] * at + [1] * (n - at)
    assert tm.kept_mask(kmers, last, 0).tolist() == [1] * n
    assert tm.kept_mask(kmers, [0] * n, +1).tolist() == [0] * n  # no `last`: nothing


@pytest.mark.parametrize("k", [21, 41])
def test_fork_by_hand(k):
    kmers, last, (stem, live, dead) = tm.fork(np.random.default_rng(k), k)
    assert len(kmers) == len(stem) + len(live) + len(dead)
    want = [1] * (len(stem) + len(live)) + [0] * len(dead)  # the dead arm goes, the stem stays
    assert tm.kept_mask(kmers, last, +1).tolist() == want
    assert tm.kept_mask(kmers, last, -1).tolist() == [1 if x else 0 for x in last]  # left steps from the arm's end lead nowhere
    assert tm.kept_mask(kmers, last, 0).tolist() == [1] * len(kmers)
    kmers, last, _ = tm.fork(np.random.default_rng(k), k, live=(False, False))
    assert not any(last) and not tm.kept_mask(kmers, last, +1).any()


def test_designed_shapes_by_hand():
    rng, k = np.random.default_rng(5), 21
    kmers, last = tm.bubble(rng, k)
    assert tm.kept_mask(kmers, last, +1).all()  # both arms rejoin and reach the end
    kmers, last = tm.cycle(rng, k, 70, 0)
    assert len(kmers) == 70 and not tm.kept_mask(kmers, last, +1).any()
    kmers, last = tm.cycle(rng, k, 70, 1)
    assert tm.kept_mask(kmers, last, +1).all() and tm.kept_mask(kmers, last, -1).all()
    kmers, last = tm.cycle_with_tail_out(rng, k)
    assert tm.kept_mask(kmers, last, +1).all() and tm.kept_mask(kmers, last, -1).sum() == 1
    kmers, last = tm.last_into_cycle(rng, k)
    assert tm.kept_mask(kmers, last, +1).sum() == 1 and tm.kept_mask(kmers, last, -1).all()
    both = ["ACGGTCA", tm.revcomp("ACGGTCA")]  # x and its reverse complement: two unrelated entries
    assert tm.kept_mask(both, [1, 0], 0).tolist() == [1, 0]


# ---- the restated phases of csrc/trim_paths.hip against runTrimPaths, and what the deeper shapes are named for

@pytest.mark.parametrize("k", [21, 41])
@pytest.mark.parametrize("name", tm.SHAPES)
def test_the_phase_model_keeps_what_the_walk_keeps(name, k):
    kmers, last = tm.shape(name, k)
    for direction, entries in ((1, kmers), (-1, tm.twin(kmers)), (-1, kmers), (1, tm.twin(kmers))):
        kept, phases, took = tm.phase_model(entries, last, direction)
        assert np.array_equal(kept, tm.kept_mask(entries, last, direction)), (name, k, direction)
        assert phases <= len(kmers) + 1
    by_right, by_left = tm.phase_model(kmers, last, 1), tm.phase_model(tm.twin(kmers), last, -1)
    # the twin is the same shape (its neighbours come in the opposite order of bases: which arm of two is the `rejoin` may differ)
    assert np.array_equal(by_right[0], by_left[0]) and by_right[1] == by_left[1] and set().union(*by_right[2]) == set().union(*by_left[2])
    if name in tm.SHAPE_MEETS:
        phases, branches = tm.SHAPE_MEETS[name]
        assert by_right[1] >= phases and branches <= set().union(*by_right[2]), (by_right[1], sorted(set().union(*by_right[2])))


def test_all_branches_are_met_and_the_deep_nest_needs_more_than_three_phases():
    met = set()
    for name in tm.NEW_SHAPES:
        met |= set().union(*tm.phase_model(*tm.shape(name, 21), 1)[2])
    assert met == set(tm.BRANCHES)
    assert tm.phase_model(*tm.shape("fork_nest_6", 21), 1)[1] > 3 and tm.phase_model(*tm.shape("chain", 21), 1)[1] == 2


@pytest.mark.parametrize("k", [21, 41])
def test_the_deeper_shapes_by_hand(k):
    rng = np.random.default_rng(k)
    for depth in (2, 3, 6):  # the stem, and one arm a level down to the live tip
        kmers, last = tm.fork_nest(rng, k, depth)
        assert len(kmers) == 5 + 3 * (2 ** (depth + 1) - 2) and sum(last) == 1
        assert int(tm.kept_mask(kmers, last, 1).sum()) == 5 + 3 * depth
    for width in (3, 4):
        kmers, last, parts = tm.fan(rng, k, width)
        kept = dict(zip(kmers, tm.kept_mask(kmers, last, 1)))
        for p, (stem, arms) in enumerate(parts):
            assert set(tm.right_neighbors(stem[-1])) & set(kmers) == {a[0] for a in arms} and len(arms) == width
            assert all(kept[x] for x in stem) and [all(kept[x] for x in a) for a in arms] == [j == p for j in range(width)]
            assert [any(kept[x] for x in a) for a in arms] == [j == p for j in range(width)]
    kmers, last, xs = tm.rejoin_through_pass(rng, k)
    kept = dict(zip(kmers, tm.kept_mask(kmers, last, 1)))
    assert len(xs) == 24 and [kept[x] for x, variant in xs] == [1 if variant in (0, 1) else 0 for x, variant in xs]
    assert {len(set(tm.right_neighbors(x)) & set(kmers)) for x, variant in xs} == {2, 3}
    for with_last in (False, True):
        for make in (tm.figure_eight, tm.open_triangle):
            kmers, last = make(rng, k, with_last)
            kept = tm.kept_mask(kmers, last, 1)
            assert not kept.any() if not with_last else (kept.all() if make is tm.figure_eight else kept.sum() > 3 * k)
    kmers, last = tm.dead_beside_cycle(rng, k)
    assert not tm.kept_mask(kmers, last, 1).any() and not any(last)
    kmers, last, (q, f) = tm.kept_through_pass(rng, k)
    kept = dict(zip(kmers, tm.kept_mask(kmers, last, 1)))
    assert kept[q] and kept[f] and sum(kept.values()) == 5 + (k + 40) + 1 + 4
