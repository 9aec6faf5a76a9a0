"""Every k the library accepts, in every key mode, on the GPU: packed keys k = 1 .. 31, polynomial and FNV-1a hashes k = 1 .. 63
(157 combinations), each on both counting paths, bit for bit against the CPU oracle (oracle/pyoracle.py) and the Python models
(tests/classifier_model.py, tests/seq_cov_model.py): counting, look-ups, the keys of oriented k-mers, walks in three directions
and a radius-bounded one, the reads-classifier's numbers and verdicts, seq-cov's sums.  k = 32 -- a k-mer fills a 64-bit word
exactly: shifts by 64 - 2k = 0, masks of all ones, an empty tail in path_open, hash keys through the per-window pipeline with a
NULL seed_hi -- is one of them, 22 / 23 either side of SK_MIN_K are two more, and 33 .. 63 with polynomial keys run again as long
records (count_long.h).  A last test counts the walk's round trips with and without read pointers at k = 31, 32 and 33: a wrong
look-ahead cannot change a result (the walk verifies every guess), only cost round trips.

The GPU tests carry the gpu mark one by one: test_inputs_of_the_sweep runs without a GPU and asserts, from the oracle alone, what
the sweep relies on for every combination."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import classifier_model as cm
from tests import seq_cov_model as sm
from tests.helpers import assert_bfs_equal, oracle_table, ragged_case, seed_windows, synth_case

gpu = pytest.mark.gpu

COMBOS = [(k, po.KEY_PACKED) for k in range(1, 32)] + [(k, m) for m in (po.KEY_POLY, po.KEY_FNV1A) for k in range(1, 64)]
MODE_NAMES = {po.KEY_PACKED: "packed", po.KEY_POLY: "poly", po.KEY_FNV1A: "fnv1a"}
COMBO_IDS = ["k%d-%s" % (k, MODE_NAMES[m]) for k, m in COMBOS]
assert len(COMBOS) == 157

MIN_COV = 2
WALKS = [(-1, 400, -1), (1, 400, -1), (0, 400, -1), (0, -1, 25)]  # (direction, max_kmers, max_radius): the last one bounded by radius alone


def sweep_reads(k, mode):
    """700 ragged reads of a 5000-base genome, reads of exactly k - 1, k and k + 1 bases, one error-free stretch of 2000 bases"""
    genome, codes, off = ragged_case(np.random.default_rng(1000 + 3 * k + mode), 700)
    extra = [genome[5:5 + k - 1], genome[50:50 + k], genome[90:90 + k + 1], genome[1000:3000]]
    lens = np.diff(off).astype(np.int64).tolist() + [len(e) for e in extra]
    codes = np.concatenate([codes] + extra)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return genome, codes, off


def sweep_seed(genome, k):
    return genome[1000:1000 + k + 40]


def query_reads(genome, k, rng):
    """about 60 (codes, phred) reads: lengths 0, k - 1, k, k + 1 and 2k, reverse complements, mutated reads, absent random reads,
    and reads with a single low-quality position (whose base is wrong: the correction has something to find)"""
    def cut(L):
        s = int(rng.integers(0, len(genome) - L + 1))
        return genome[s:s + L].copy()

    reads = [cut(L) for L in (0, k - 1, k, k + 1, 2 * k) for _ in range(8)]
    reads += [(3 - cut(int(rng.integers(k, 2 * k + 60)))[::-1]).astype(np.uint8) for _ in range(6)]
    for _ in range(6):
        r = cut(int(rng.integers(k + 1, 2 * k + 60)))
        p = int(rng.integers(0, len(r)))
        r[p] = (int(r[p]) + 1 + int(rng.integers(0, 3))) & 3
        reads.append(r)
    reads += [rng.integers(0, 4, int(rng.integers(k, 2 * k + 60))).astype(np.uint8) for _ in range(4)]
    phreds = [np.full(len(r), 35, dtype=np.uint8) for r in reads]
    for _ in range(4):
        r = cut(int(rng.integers(k + 1, 2 * k + 60)))
        q = np.full(len(r), 35, dtype=np.uint8)
        p = int(rng.integers(0, len(r)))
        r[p] = (int(r[p]) + 1) & 3
        q[p] = 5
        reads.append(r)
        phreds.append(q)
    return list(zip(reads, phreds))


def pack_queries(reads):
    codes = np.concatenate([r for r, _ in reads])
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r, _ in reads])
    bad = np.array([cm.bad_pos(q) for _, q in reads], dtype=np.int32)
    return codes, off, bad


@functools.lru_cache(maxsize=None)
def sweep_case(k, mode):
    """the inputs of one combination and everything the oracle and the models say about them (both counting paths share it)"""
    genome, codes, off = sweep_reads(k, mode)
    t, n = oracle_table(codes, off, k, mode)
    seed = sweep_seed(genome, k)
    walks = [po.bfs(t, k, mode, [seed], d, MIN_COV, mk, mr) for d, mk, mr in WALKS]
    queries = query_reads(genome, k, np.random.default_rng(7000 + 3 * k + mode))
    get = cm.table_getter(t, k, mode)
    numbers = [cm.numbers(r, k, get) for r, _ in queries]
    verdicts = {corr: [cm.classify(rd, k, get, 90, 1.0, corr) for rd in queries] for corr in (False, True)}
    q_codes, q_off, q_bad = pack_queries(queries)
    cov = sm.store_coverage(q_codes, q_off, k, mode, t)
    return dict(genome=genome, codes=codes, off=off, table=t, windows=n, seed=seed, walks=walks, queries=queries, numbers=numbers,
                verdicts=verdicts, q_codes=q_codes, q_off=q_off, q_bad=q_bad, cov=cov)


@pytest.mark.parametrize("k,mode", COMBOS, ids=COMBO_IDS)
def test_inputs_of_the_sweep(k, mode):
    """No GPU: what the sweep relies on, from the oracle alone.  Every walk finds a seed (a result, never None), the reads hold one
    shorter than k and one of exactly k bases, the query set has reads with and without covered windows."""
    c = sweep_case(k, mode)
    assert all(w is not None and len(w["lo"]) >= 1 for w in c["walks"])
    lens = np.diff(c["off"]).astype(np.int64)
    assert (lens < k).any() and (lens == k).any() and (lens == k - 1).any() and (lens == k + 1).any() and lens[-1] == 2000
    assert len(c["off"]) - 1 == 704 and len(c["seed"]) == k + 40
    assert any(n[1] == 0 for n in c["numbers"]) and any(n[1] > 0 for n in c["numbers"])
    assert 55 <= len(c["queries"]) <= 65 and sum(1 for b in c["q_bad"] if b >= 0) == 4
    assert {len(r) for r, _ in c["queries"]} >= {0, k - 1, k, k + 1, 2 * k}
    assert (c["cov"][:, 1] == 0).any() and (c["cov"][:, 1] > 0).any()
    assert [int(x) for x in c["cov"][:, 1]] == [n[1] for n in c["numbers"]]  # (the two models agree on the breadth)


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


@pytest.fixture(params=["direct", "partition"])
def count_path(request, monkeypatch):
    """Both counting kernels: the direct one (an atomic per occurrence) and the partitioned pipeline.  Read at mc_create."""
    monkeypatch.setenv("MC_COUNT_PATH", request.param)
    return request.param


def _count_and_walk(ctx, c, k, mode):
    t = c["table"]
    ctx.add_reads_packed(po.pack(c["codes"]), c["off"])
    assert ctx.finalize() == t.size()
    assert ctx.stats().windows == c["windows"]
    ok, oc = t.dump()
    gk, gc = ctx.export(0)
    assert np.array_equal(gk, ok) and np.array_equal(gc, oc)
    # look-ups: present keys, keys drawn from the key space (absent, all but surely, where the space is large), key 0
    rng = np.random.default_rng(k)
    absent = rng.integers(0, 1 << (2 * k), 500) if mode == po.KEY_PACKED else rng.integers(-(1 << 63), (1 << 63) - 1, 500)
    q = np.concatenate([ok[:1000], ok[-1000:], absent, [0]]).astype(np.int64)
    assert np.array_equal(ctx.get(q), t.get_many(q))
    # the keys of the seed's oriented k-mers (no high words up to k = 32)
    hi, lo = seed_windows(c["seed"], k)
    assert k > 32 or not hi.any()
    assert np.array_equal(ctx.kmer_keys(hi if k > 32 else None, lo), sm.window_keys(c["seed"], k, mode))
    for (d, mk, mr), want in zip(WALKS, c["walks"]):
        assert_bfs_equal(ctx.bfs(hi if k > 32 else None, lo, d, MIN_COV, mk, mr), want)


@gpu
@pytest.mark.parametrize("k,mode", COMBOS, ids=COMBO_IDS)
def test_every_k(mc, k, mode, count_path):
    c = sweep_case(k, mode)
    with mc.Context(k, mode, 0, 0) as ctx:
        _count_and_walk(ctx, c, k, mode)
        # reads-classifier: the three numbers of every read and the verdicts, without and with the correction
        for corr in (False, True):
            s, cv, last, f = ctx.classify_reads(c["q_codes"], c["q_off"], c["q_bad"] if corr else None, found=90, z=1.0, correction=corr)
            got = list(zip(s.tolist(), cv.tolist(), last.tolist()))
            assert got == c["numbers"], [i for i in range(len(got)) if got[i] != c["numbers"][i]][:5]
            assert [bool(x) for x in f] == c["verdicts"][corr], corr
        # seq-cov: depth and breadth of every query in one table, and in the same table twice
        got = mc.seq_coverage([ctx], c["q_codes"], c["q_off"])
        assert got.shape == (len(c["queries"]), 1, 2) and np.array_equal(got[:, 0], c["cov"])
        got = mc.seq_coverage([ctx, ctx], c["q_codes"], c["q_off"])
        assert got.shape == (len(c["queries"]), 2, 2) and np.array_equal(got[:, 0], c["cov"]) and np.array_equal(got[:, 1], c["cov"])


@gpu
@pytest.mark.parametrize("k", list(range(32, 64)))
def test_every_k_of_long_records(mc, monkeypatch, k):
    """Polynomial keys through the partitioned pipeline into a table a capacity hint vouches for: long records for k = 33 .. 63
    (count_long.h shifts by 2 * (k - 32)), as its header promises -- and at k = 32 the per-window pipeline.  Same pairs, same walks."""
    monkeypatch.setenv("MC_COUNT_PATH", "partition")
    monkeypatch.delenv("MC_LONG_RECORDS", raising=False)
    monkeypatch.delenv("MC_LONG_BINS", raising=False)
    c = sweep_case(k, po.KEY_POLY)
    with mc.Context(k, mc.KEY_POLY, 0, 100000) as ctx:
        _count_and_walk(ctx, c, k, po.KEY_POLY)
        long_runs = ctx.stats().long_runs
        assert (long_runs == 0) if k == 32 else (long_runs >= 1), long_runs


@gpu
def test_look_ahead_at_k_31_32_33(mc, monkeypatch):
    """The walk's look-ahead along the reads (bfs_device.h path_open; its k == 32 arm: the walker's own bases fill word 0, the tail
    starts empty).  20000 k-mers leftwards over error-free reads, on a context that kept read pointers while counting and on one
    that did not (mc_set_read_pointers(0)): equal results, strictly fewer round trips with pointers.  k = 31 packed keys, 32 and 33
    polynomial keys; the ratios are printed (python -m pytest -s)."""
    monkeypatch.delenv("MC_COUNT_PATH", raising=False)
    monkeypatch.delenv("MC_LONG_RECORDS", raising=False)
    genome, reads, off = synth_case(1, 60000, 20000, 150, 0)
    words = po.pack(reads)
    for k, mode in ((31, po.KEY_PACKED), (32, po.KEY_POLY), (33, po.KEY_POLY)):
        hi, lo = seed_windows(genome[30000:30200], k)
        t, _ = oracle_table(reads, off, k, mode)
        res = {}
        for name in ("with", "without"):
            with mc.Context(k, mode, 0, 0) as ctx:
                if name == "without":
                    ctx.set_read_pointers(0)
                ctx.add_reads_packed(words, off)
                assert ctx.finalize() == t.size()
                res[name] = ctx.bfs(hi, lo, -1, 3, 20000, -1)
        assert_bfs_equal(res["with"], res["without"])
        assert_bfs_equal(res["with"], po.bfs(t, k, mode, [genome[30000:30200]], -1, 3, 20000, -1))
        print("look-ahead k=%d: %d rounds with read pointers, %d without, %d levels: ratio %.2f" % (
            k, res["with"]["rounds"], res["without"]["rounds"], res["with"]["levels"], res["without"]["rounds"] / res["with"]["rounds"]))
        assert res["with"]["rounds"] < res["without"]["rounds"], (k, res["with"]["rounds"], res["without"]["rounds"])
