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
