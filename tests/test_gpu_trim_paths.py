"""GPU: mc_trim_paths through the C ABI against tests/trim_paths_model.py, the string-level runTrimPaths (which
tests/test_trim_paths_model.py holds to the oracle's trim), on a context that has counted nothing: the table plays no part.
The unit (csrc/trim_paths.hip) changes its code path at one constant, TP_WIDE_K = 33: one word a k-mer below it, two from it on;
k = 32 and k = 33 stand on either side of it in the word-edge tests.  Every other path is a choice by `dir`, taken by every case."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import trim_paths_model as tm

pytestmark = pytest.mark.gpu

EINVAL = -1  # MC_EINVAL
DIRS = (-1, 1, 0)


@functools.lru_cache(maxsize=None)
def _ctx(k):
    import metacherchant_amd as m
    return m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)


def _gpu(k, kmers, last, direction, hi_none=False):
    hi, lo = tm.pack_kmers(kmers)
    return _ctx(k).trim_paths(None if hi_none else hi, lo, np.array(last, dtype=np.uint8), direction)


def _check(k, kmers, last, dirs=DIRS):
    """the GPU's mask is the model's, in every direction; returns the masks"""
    out = {}
    for d in dirs:
        want = tm.kept_mask(kmers, last, d)
        got = _gpu(k, kmers, last, d)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (k, d, len(kmers), np.nonzero(got != want)[0][:8])
        out[d] = got
    return out


def test_no_entries_and_one():
    for k in (21, 33):
        for d in DIRS:
            assert len(_gpu(k, [], [], d)) == 0
            assert _gpu(k, [("ACGGT" * 13)[:k]], [0], d).tolist() == [0]
            assert _gpu(k, [("ACGGT" * 13)[:k]], [1], d).tolist() == [1]


@pytest.mark.parametrize("n", [63, 64, 65, 257, 1025, 5000])
def test_chains(n):
    k = 21 if n != 1025 else 41
    kmers, last = tm.chain(np.random.default_rng(n), k, n)
    at = n // 3
    got = _check(k, kmers, last)
    assert got[1].tolist() == [1] * (at + 1) + [0] * (n - at - 1)
    assert got[-1].tolist() == [0] * at + [1] * (n - at)
    assert got[0].all()
    order = np.random.default_rng(n + 1).permutation(n)  # the same entries in shuffled order
    shuffled = _check(k, [kmers[i] for i in order], [last[i] for i in order])
    for d in DIRS:
        assert np.array_equal(shuffled[d], got[d][order])


@pytest.mark.parametrize("k", [21, 41])
def test_forks(k):
    kmers, last, (stem, live, dead) = tm.fork(np.random.default_rng(k), k)
    got = _check(k, kmers, last)
    assert got[1].tolist() == [1] * (len(stem) + len(live)) + [0] * len(dead)  # the dead arm goes, the stem stays
    kmers, last, _ = tm.fork(np.random.default_rng(k), k, live=(False, False))
    assert not any(g.any() for g in _check(k, kmers, last).values())  # both arms dead: nothing
    kmers, last, _ = tm.fork(np.random.default_rng(k), k, live=(True, True))
    assert _check(k, kmers, last)[1].all()
    kmers, last = tm.bubble(np.random.default_rng(k + 1), k)  # a branch node whose arms rejoin
    assert _check(k, kmers, last)[1].all()


@pytest.mark.parametrize("k", [11, 33])
def test_cycles(k):
    rng = np.random.default_rng(k)
    kmers, last = tm.cycle(rng, k, 70, 0)
    assert not any(g.any() for g in _check(k, kmers, last).values())
    kmers, last = tm.cycle(rng, k, 70, 1)
    got = _check(k, kmers, last)
    assert got[1].all() and got[-1].all()
    kmers, last = tm.cycle_with_tail_out(rng, k)
    got = _check(k, kmers, last)
    assert got[1].all() and got[-1].sum() == 1
    kmers, last = tm.last_into_cycle(rng, k)
    got = _check(k, kmers, last)
    assert got[1].sum() == 1 and got[-1].all()


@pytest.mark.parametrize("k", [21, 41])
@pytest.mark.parametrize("name", tm.NEW_SHAPES)
def test_deeper_shapes(name, k):
    """nests of forks that take more than three phases, nodes with three and four ways on, arms that rejoin through PASS pointers of
    different lengths beside a second stop, two cycles through one node, forks that stay OPEN for good, a dead tip beside a closed
    cycle, a KEPT stop found through a long PASS chain (tests/test_trim_paths_model.py holds each shape to the branches of
    k_tp_classify it is named for): by right steps as built, by left steps as the reverse-complement twins, and dir = 0"""
    kmers, last = tm.shape(name, k)
    by_right = _check(k, kmers, last)
    by_left = _check(k, tm.twin(kmers), last)
    assert np.array_equal(by_right[1], by_left[-1]) and np.array_equal(by_right[-1], by_left[1]) and np.array_equal(by_right[0], by_left[0])
    order = np.random.default_rng(len(kmers)).permutation(len(kmers))  # the same entries in shuffled order
    shuffled = _check(k, [kmers[i] for i in order], [last[i] for i in order], dirs=(1,))
    assert np.array_equal(shuffled[1], by_right[1][order])


@pytest.mark.parametrize("k", [21, 32, 33])
def test_self_loops(k):
    a = "A" * k
    for last in ([0], [1]):
        _check(k, [a], last)
    run = tm.windows("GC" + "A" * k + "GGTC", k)  # ... and in the middle of a chain, its own left and right neighbour
    assert a in run and len(set(run)) == len(run)
    for at in (0, run.index(a), len(run) - 1):
        _check(k, run, [1 if i == at else 0 for i in range(len(run))])


def test_the_all_ones_word_at_k_32():
    k, t = 32, "T" * 32
    run = tm.windows("GAC" + "T" * 32 + "CAGG", k)
    assert t in run and int(tm.pack_kmers([t])[1][0]) == 2 ** 64 - 1
    for at in (0, run.index(t), len(run) - 1):  # in the set, and as the `last`
        _check(k, run, [1 if i == at else 0 for i in range(len(run))])
    _check(k, [t], [1])
    _check(k, [t], [0])


@pytest.mark.parametrize("k", [5, 31, 32, 33, 63])
def test_a_kmer_and_its_reverse_complement_are_unrelated(k):
    rng = np.random.default_rng(k)
    s = tm.repeat_free(rng, k + 30, k) if k > 5 else "ACGGTTCAGA"
    fw = tm.windows(s, k)
    rc = [tm.revcomp(x) for x in fw]
    assert len(set(fw + rc)) == len(fw + rc)
    last = [0] * len(fw + rc)
    last[len(fw) - 1] = 1  # the end of the forward chain alone
    got = _check(k, fw + rc, last)
    assert got[1].tolist() == [1] * len(fw) + [0] * len(rc)
    assert got[0].tolist() == [1] * len(fw) + [0] * len(rc)


@pytest.mark.parametrize("k", [1, 2])
def test_the_full_sets_of_k_1_and_2(k):
    kmers = ["".join(tm.NUCLEOTIDES[(i >> (2 * (k - 1 - j))) & 3] for j in range(k)) for i in range(4 ** k)]
    for at in (0, len(kmers) - 1):
        assert all(g.all() for g in _check(k, kmers, [1 if i == at else 0 for i in range(len(kmers))]).values())
    assert not any(g.any() for g in _check(k, kmers, [0] * len(kmers)).values())
    _check(k, kmers[1:3], [1, 0])


@pytest.mark.parametrize("k", [31, 32, 33, 63])
def test_word_edges_and_garbage_bits(k):
    """both sides of TP_WIDE_K = 33, the longest k, and the longest that is one short of a word"""
    rng = np.random.default_rng(1000 + k)
    kmers, last, _ = tm.fork(rng, k)
    more, more_last = tm.cycle_with_tail_out(rng, k)
    kmers, last = kmers + more, last + more_last
    want = _check(k, kmers, last)
    hi, lo = tm.pack_kmers(kmers)
    ghi, glo = hi.copy(), lo.copy()
    junk = rng.integers(0, 2 ** 63, len(kmers), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    if k > 32:
        ghi |= junk << np.uint64(2 * k - 64)
    else:
        ghi = junk  # (not read at all)
    if k < 32:
        glo |= junk << np.uint64(2 * k)
    assert not np.array_equal(ghi, hi) and (k >= 32 or not np.array_equal(glo, lo))
    for d in DIRS:
        got = _ctx(k).trim_paths(ghi, glo, np.array(last, dtype=np.uint8) * 255, d)  # (`last`: anything but 0 is 1)
        assert np.array_equal(got, want[d])
        if k <= 32:
            assert np.array_equal(_gpu(k, kmers, last, d, hi_none=True), want[d])


@functools.lru_cache(maxsize=None)
def _dense(k):
    kmers, last = tm.dense(np.random.default_rng(7000 + k), k)
    return tuple(kmers), tuple(last)


@pytest.mark.parametrize("k", [7, 41])
def test_dense_random_sets(k):
    kmers, last = _dense(k)
    assert len(kmers) > 2500 and 3 < sum(last) < 40
    got = _check(k, list(kmers), list(last))
    assert all(0 < int(g.sum()) for g in got.values()) and int(got[1].sum()) < len(kmers)


def test_errors():
    import metacherchant_amd as m
    from metacherchant_amd import native
    L = native.load()
    for k in (21, 33):
        kmers, last = tm.chain(np.random.default_rng(k), k, 50)
        with pytest.raises(m.McError) as e:
            _gpu(k, kmers + [kmers[7]], last + [0], 1)
        assert e.value.code == EINVAL and "same oriented k-mer" in str(e.value)
        with pytest.raises(m.McError) as e:
            _gpu(k, kmers, last, 2)
        assert e.value.code == EINVAL and "dir" in str(e.value)
        assert np.array_equal(_gpu(k, kmers + [tm.revcomp(kmers[7])], last + [0], 1)[:50], _gpu(k, kmers, last, 1))  # (no duplicate)
        hi, lo = tm.pack_kmers(kmers)
        lst, kept = np.array(last, dtype=np.uint8), np.zeros(50, dtype=np.uint8)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        ctx = _ctx(k)
        good = [p(hi, C.c_uint64), p(lo, C.c_uint64), p(lst, C.c_uint8), 50, 1, p(kept, C.c_uint8), None]
        assert L.mc_trim_paths(ctx._h, *good) == 0
        for at in (1, 2, 5) + ((0,) if k > 32 else ()):
            bad = list(good)
            bad[at] = None
            assert L.mc_trim_paths(ctx._h, *bad) == EINVAL
            assert L.mc_trim_paths_dev(ctx._h, *bad) == EINVAL  # (null before anything is read)
        bad = list(good)
        bad[3] = 1 << 31
        assert L.mc_trim_paths(ctx._h, *bad) == EINVAL
        for d in (-2, 2):
            bad = list(good)
            bad[4] = d
            assert L.mc_trim_paths(ctx._h, *bad) == EINVAL
        assert L.mc_trim_paths(None, *good) == EINVAL


@pytest.mark.parametrize("k", [31, 63])
def test_the_device_form_and_two_calls(k):
    import torch
    rng = np.random.default_rng(k)
    kmers, last = tm.chain(rng, k, 3000)
    more, more_last, _ = tm.fork(rng, k)
    kmers, last = kmers + more, last + more_last
    hi, lo = tm.pack_kmers(kmers)
    as_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    d_hi, d_lo = as_dev(hi), as_dev(lo)
    d_last = torch.from_numpy(np.array(last, dtype=np.uint8)).cuda()
    ctx = _ctx(k)
    for d in DIRS:
        a = _gpu(k, kmers, last, d)
        b = _gpu(k, kmers, last, d)
        assert a.tobytes() == b.tobytes()
        d_kept = torch.full((len(lo),), 0x55, dtype=torch.uint8, device="cuda")
        ms = ctx.trim_paths_dev(d_hi if k > 32 else None, d_lo, d_last, len(lo), d, d_kept)
        assert ms > 0 and d_kept.cpu().numpy().tobytes() == a.tobytes()
    assert np.array_equal(d_lo.cpu().numpy().view(np.uint64), lo)  # (inputs are only read)


@pytest.mark.parametrize("k,mode", [(21, po.KEY_PACKED), (41, po.KEY_POLY)])
def test_end_to_end_with_the_walk(k, mode):
    """count, mc_bfs, mc_trim_paths on its result: the oracle's trimmed walk; and the walk answers the same after the trim"""
    import metacherchant_amd as m
    from tests.helpers import assert_bfs_equal, seed_windows
    codes, off, seeds, radius = tm.walk_case(k)
    t = po.Table()
    t.count_reads(codes, off, k, mode)
    with m.Context(k, m.KEY_PACKED if mode == po.KEY_PACKED else m.KEY_POLY, 0, 0) as ctx:
        ctx.add_reads_packed(po.pack(codes), off)
        ctx.finalize()
        parts = [seed_windows(s, k) for s in seeds]
        shi, slo = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        for d in DIRS:
            want = po.bfs(t, k, mode, seeds, d, 2, -1, radius, True)
            got = ctx.bfs(shi, slo, d, 2, -1, radius)
            assert_bfs_equal(got, want)
            kept = ctx.trim_paths(got["hi"], got["lo"], got["last"], d)
            assert 0 < int(want["kept"].sum()) < len(kept)  # (the caps bite)
            assert np.array_equal(kept, want["kept"])
            assert_bfs_equal(ctx.bfs(shi, slo, d, 2, -1, radius), want)  # a walk after the call answers as before it
