"""GPU: mc_classify_reads through the C ABI against the oracle's table and the model (tests/classifier_model.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import classifier_model as cm
from tests.helpers import ragged_case

pytestmark = pytest.mark.gpu

CASES = [(15, 0), (31, 0), (45, 1), (63, 1), (63, 2), (32, 1), (32, 2), (22, 0)]  # (k, key mode): packed, polynomial, FNV-1a


def _graph_reads(k):
    """ragged reads of a small genome, plus a poly-A stretch long enough to saturate its counter"""
    rng = np.random.default_rng(100 + k)
    genome, codes, off = ragged_case(rng, 700, max_len=220, genome_len=4000)
    poly_a = np.zeros(33000 + k, dtype=np.uint8)
    codes = np.concatenate([codes, poly_a])
    off = np.concatenate([off, [off[-1] + len(poly_a)]]).astype(np.uint64)
    return genome, codes, off


def _query_reads(genome, k, rng):
    """reads that overlap the graph's, with every edge case: lengths 0, k - 1, k, k + 1, N (as base 0), poly-A windows, mutations,
    and 0, 1 or 2 low-quality positions"""
    reads = []
    for L in (0, k - 1, k, k + 1, 2 * k, 150, 150, 220):
        for _ in range(6):
            s = int(rng.integers(0, len(genome) - L + 1))
            reads.append(genome[s:s + L].copy())
    for _ in range(250):
        L = int(rng.integers(k, 200))
        s = int(rng.integers(0, len(genome) - L + 1))
        r = genome[s:s + L].copy()
        if rng.integers(0, 2):
            r = (3 - r[::-1]).astype(np.uint8)
        for _ in range(int(rng.integers(0, 3))):  # sequencing errors
            r[int(rng.integers(0, L))] = int(rng.integers(0, 4))
        reads.append(r)
    reads.append(np.zeros(120, dtype=np.uint8))                          # poly-A: saturated counts
    reads.append(np.concatenate([np.zeros(k + 5, dtype=np.uint8), genome[100:200]]))
    reads.append(rng.integers(0, 4, 130).astype(np.uint8))               # absent
    phreds = []
    for r in reads:
        q = np.full(len(r), 35, dtype=np.uint8)
        n_low = int(rng.integers(0, 3)) if len(r) else 0
        for _ in range(n_low):
            p = int(rng.integers(0, len(r)))
            if rng.integers(0, 2):  # an N: base 0, phred 0
                r[p] = 0
                q[p] = 0
            else:
                q[p] = int(rng.integers(1, 10))
        phreds.append(q)
    return list(zip(reads, phreds))


def _pack(reads):
    codes = np.concatenate([r for r, _ in reads]) if reads else np.zeros(0, dtype=np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r, _ in reads])
    bad = np.array([cm.bad_pos(q) for _, q in reads], dtype=np.int32)
    return codes, off, bad


def _check(ctx, reads, k, get, tag):
    codes, off, bad = _pack(reads)
    want = [cm.numbers(r, k, get) for r, _ in reads]
    assert any(w[2] == 32767 for w in want) and any(w[1] == 0 for w in want) and any(cm.bad_pos(q) >= 0 for _, q in reads)
    for found in (0, 50, 90, 100):
        for z in (1.0, 1.96):
            for corr in (False, True):
                s, c, last, f = ctx.classify_reads(codes, off, bad if corr else None, found=found, z=z, correction=corr)
                got = list(zip(s.tolist(), c.tolist(), last.tolist()))
                assert got == want, (tag, [i for i in range(len(want)) if got[i] != want[i]][:5])
                exp = [cm.classify(rd, k, get, found, z, corr) for rd in reads]
                bad_i = [i for i in range(len(exp)) if bool(f[i]) != exp[i]]
                assert not bad_i, (tag, found, z, corr, bad_i[:5])
    # the packed form of the same reads gives the same answer
    from oracle import pyoracle as po
    s2, c2, l2, f2 = ctx.classify_reads(po.pack(codes), off, bad, found=90, z=1.0, correction=True)
    s1, c1, l1, f1 = ctx.classify_reads(codes, off, bad, found=90, z=1.0, correction=True)
    assert np.array_equal(s1, s2) and np.array_equal(f1, f2)


@pytest.mark.parametrize("k,mode", CASES)
def test_classify_matches_the_oracle_and_the_model(k, mode, oracle, tmp_path):
    import metacherchant_amd as m
    genome, codes, off = _graph_reads(k)
    t = oracle.Table()
    t.count_reads(codes, off, k, mode)
    get = cm.table_getter(t, k, mode)
    reads = _query_reads(genome, k, np.random.default_rng(k * 7 + mode))
    with m.Context(k, mode, 0, 0) as ctx:
        ctx.add_reads_packed(oracle.pack(codes), off)
        ctx.finalize()
        _check(ctx, reads, k, get, "counted")
        bin_path = str(tmp_path / "g.kmers.bin")
        ctx.save_kmers(bin_path)
    # the same table through mc_save_kmers -> mc_load_kmers into a fresh context
    with m.Context(k, mode, 0, 0) as ctx2:
        ctx2.load_kmers(bin_path, 0)
        ctx2.finalize()
        _check(ctx2, reads, k, get, "loaded")


def test_classify_a_table_in_minimizer_bins(oracle):
    """k = 63 polynomial keys counted as long records (a capacity hint, batches of more than 2^22 windows): the table is in
    minimizer bins, and classifying moves it to hash-prefix regions once (mc_stats.left_bins = 1) with the same answers"""
    import metacherchant_amd as m
    from tests.helpers import synth_case
    k, mode = 63, oracle.KEY_POLY
    genome, codes, off = synth_case(1, 100000, 60000, 150, 100)
    t = oracle.Table()
    t.count_reads(codes, off, k, mode)
    get = cm.table_getter(t, k, mode)
    reads = _query_reads(genome[:100000], k, np.random.default_rng(5))
    with m.Context(k, mode, 0, 8000000) as ctx:
        ctx.add_reads_packed(oracle.pack(codes), off)
        ctx.finalize()
        st = ctx.stats()
        assert st.long_runs > 0 and st.left_bins == 0, (st.long_runs, st.left_bins)
        q_codes, q_off, bad = _pack(reads)
        want = [cm.numbers(r, k, get) for r, _ in reads]
        s, c, last, f = ctx.classify_reads(q_codes, q_off, bad, found=90, z=1.0, correction=True)
        assert list(zip(s.tolist(), c.tolist(), last.tolist())) == want
        assert [bool(x) for x in f] == [cm.classify(rd, k, get, 90, 1.0, True) for rd in reads]
        assert ctx.stats().left_bins == 1
        s2, _, _, f2 = ctx.classify_reads(q_codes, q_off, bad, found=90, z=1.0, correction=True)  # (now by key, directly)
        assert np.array_equal(s, s2) and np.array_equal(f, f2)


def test_classify_errors(oracle):
    import metacherchant_amd as m
    from metacherchant_amd import native
    codes = np.zeros(40, dtype=np.uint8)
    off = np.array([0, 40], dtype=np.uint64)
    with m.Context(21, 0, 0, 0) as ctx:
        with pytest.raises(native.McError) as e:
            ctx.classify_reads(codes, off)
        assert e.value.code == -4  # MC_ESTATE before mc_finalize_counts
        ctx.add_reads_packed(oracle.pack(codes), off)
        ctx.finalize()
        for bad_found in (-1, 101):
            with pytest.raises(native.McError) as e:
                ctx.classify_reads(codes, off, found=bad_found)
            assert e.value.code == -1
        out = (native.ReadCov * 1)()
        L = native.load()
        assert L.mc_classify_reads(ctx._h, None, None, 1, None, 90, 1.0, 0, out) == -1  # MC_EINVAL: null pointers
        assert L.mc_classify_reads_dev(ctx._h, None, None, 1, None, 90, 1.0, 0, None) == -1
        assert L.mc_classify_reads(None, None, None, 0, None, 90, 1.0, 0, None) == -1
        assert L.mc_classify_reads(ctx._h, None, None, 0, None, 90, 1.0, 0, None) == 0  # nothing to do
        s, c, last, f = ctx.classify_reads(codes, off)
        # poly-A: its 20 windows are one k-mer of count 20 -> sum 400, breadth 1
        assert (int(s[0]), int(c[0]), int(last[0]), bool(f[0])) == (400, 20, 20, True)
    assert C.sizeof(native.ReadCov) == 12
