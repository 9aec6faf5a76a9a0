"""GPU: mc_seq_coverage through the C ABI against the model (tests/seq_cov_model.py) over the oracle's tables."""
import ctypes as C

import numpy as np
import pytest

from tests import seq_cov_model as sm
from tests.helpers import synth_case

pytestmark = pytest.mark.gpu

CASES = [(21, 0), (31, 0), (41, 1), (63, 1), (63, 2), (32, 1)]  # (k, key mode): packed, polynomial, FNV-1a
GENOME = 200000


def _tables(oracle, k, mode):
    """four read subsets of one genome (different reads, different depths), as oracle tables with their reads"""
    out = []
    for first, n in ((0, 4000), (4000, 7000), (11000, 2500), (13500, 9000)):
        _, reads, off = synth_case(1, GENOME, n, 150, 100, first_read=first)
        t = oracle.Table()
        t.count_reads(reads, off, k, mode)
        out.append((t, reads, off))
    return out


def _sequences(genome, k, rng):
    """long sequences first, in the middle and last (tiles start and end inside them), 100 kbase ones at and between them, and
    thousands of reads of 30 .. 300 bases in between: shorter than k, empty, with N (base 0), reverse complements, random"""
    def long_seq(n):
        s = np.concatenate([genome[int(rng.integers(0, GENOME // 2)):]] * (n // (GENOME // 2) + 1))[:n].copy()
        errs = rng.integers(0, n, n // 200)
        s[errs] = rng.integers(0, 4, len(errs))
        return s.astype(np.uint8)

    def reads(n):
        out = []
        for i in range(n):
            kind = i % 10
            L = int(rng.integers(30, 301))
            if kind == 0:
                L = int(rng.integers(0, k))        # shorter than k
            elif kind == 1:
                L = 0
            s = int(rng.integers(0, GENOME - L + 1))
            r = genome[s:s + L].copy()
            if kind == 2:
                r = rng.integers(0, 4, L).astype(np.uint8)  # not in any table
            if kind == 3:
                r = (3 - r[::-1]).astype(np.uint8)
            if kind == 4 and L:
                r[rng.integers(0, L, 2)] = 0                  # N
            out.append(r)
        return out

    seqs = [long_seq(2 * 1024 * 1024 + 12345)] + reads(1500) + [long_seq(100000)] + reads(1) + [long_seq(100000), long_seq(2100000)]
    seqs += reads(1500) + [np.zeros(0, dtype=np.uint8)] * 3000
    # one-base sequences up to the middle of a tile of 2048 positions, then a covered sequence: it is beyond the tile's 256th
    n_one = 2500 + (1024 - (sum(len(s) for s in seqs) + 2500)) % 2048
    seqs += [genome[:1].copy()] * n_one + [long_seq(100000), long_seq(2 * 1024 * 1024)]
    codes = np.concatenate(seqs)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return codes, off


@pytest.mark.parametrize("k,mode", CASES)
def test_seq_coverage_matches_the_model(k, mode, oracle):
    import torch

    import metacherchant_amd as m
    genome = oracle.synth_genome(20240531, GENOME)
    tabs = _tables(oracle, k, mode)
    codes, off = _sequences(genome, k, np.random.default_rng(k * 11 + mode))
    wk = sm.window_keys(codes, k, mode)
    want = np.stack([sm.store_coverage(codes, off, k, mode, t, wk) for t, _, _ in tabs], axis=1)  # [n_seqs, 4, 2]
    # the test's own input: every column has zero and nonzero entries, no two tables' columns are equal
    for t in range(4):
        for f in range(2):
            assert (want[:, t, f] == 0).any() and (want[:, t, f] != 0).any(), (t, f)
        for u in range(t):
            assert not np.array_equal(want[:, t, 0], want[:, u, 0]) and not np.array_equal(want[:, t, 1], want[:, u, 1]), (t, u)
    # ... and a covered sequence is beyond the 256th of the tile of 2048 positions it starts in (the kernel's path past its LDS entries)
    s_far = len(off) - 3
    tile_first = int(off[s_far]) // 2048 * 2048
    assert s_far - (int(np.searchsorted(off, tile_first, side="right")) - 1) >= 256 and int(off[s_far]) - tile_first == 1024
    assert (want[s_far] > 0).all() and int(off[s_far + 1] - off[s_far]) == 100000
    ctxs = []
    try:
        for _, reads, roff in tabs:
            c = m.Context(k, mode, 0, 0)
            ctxs.append(c)
            c.add_reads_packed(oracle.pack(reads), roff)
            c.finalize()
        for pick in ([0], [2], [1, 3], [3, 0], [0, 1, 2, 3], [3, 2, 1, 0]):
            got = m.seq_coverage([ctxs[i] for i in pick], codes, off)
            assert got.shape == (len(off) - 1, len(pick), 2) and got.dtype == np.uint64
            bad = np.argwhere(got != want[:, pick, :])
            assert len(bad) == 0, (pick, bad[:5], got[bad[0][0]], want[bad[0][0], pick])
        # one context four times: its column four times
        got = m.seq_coverage([ctxs[1]] * 4, codes, off)
        assert all(np.array_equal(got[:, t], want[:, 1]) for t in range(4))
        # the device form, over packed words
        dev = torch.device("cuda", 0)
        d_words = torch.from_numpy(oracle.pack(codes).view(np.int64)).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_out = torch.full((len(off) - 1, 4, 2), -1, dtype=torch.int64, device=dev)  # (the call zeroes it)
        m.seq_coverage_dev(ctxs, d_words, d_off, len(off) - 1, d_out)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
        assert np.array_equal(m.seq_coverage(ctxs, oracle.pack(codes), off), want)  # (host form, words already packed)
    finally:
        for c in ctxs:
            c.close()


def test_seq_coverage_of_a_saturated_repeat_passes_an_int(oracle):
    """poly-A counted 40 000 times saturates at 32767; 70 000 windows of it sum to 2 293 690 000 > 2^31"""
    import metacherchant_amd as m
    k = 31
    a = np.zeros(40000 + k - 1, dtype=np.uint8)
    with m.Context(k, 0, 0, 0) as ctx:
        ctx.add_reads_packed(oracle.pack(a), np.array([0, len(a)], dtype=np.uint64))
        ctx.finalize()
        q = np.zeros(70000 + k - 1, dtype=np.uint8)
        got = m.seq_coverage([ctx], q, np.array([0, 0, len(q)], dtype=np.uint64))
        assert got[1, 0].tolist() == [32767 * 70000, 70000] and got[0, 0].tolist() == [0, 0]


def test_seq_coverage_refusals(oracle):
    import metacherchant_amd as m
    from metacherchant_amd import native
    L = native.load()
    codes = np.zeros(40, dtype=np.uint8)
    off = np.array([0, 40], dtype=np.uint64)
    words = oracle.pack(codes)

    def call(ctxs, n_tables=None, words_=words, off_=off, n=1, dev=False):
        out = np.full((1, 4, 2), 77, dtype=np.uint64)
        h = (C.c_void_p * 5)(*[c._h if c is not None else None for c in ctxs])
        f = L.mc_seq_coverage_dev if dev else L.mc_seq_coverage
        wp = None if words_ is None else (C.c_void_p(words_.ctypes.data) if dev else words_.ctypes.data_as(C.POINTER(C.c_uint64)))
        op = None if off_ is None else (C.c_void_p(off_.ctypes.data) if dev else off_.ctypes.data_as(C.POINTER(C.c_uint64)))
        rc = f(h, len(ctxs) if n_tables is None else n_tables, wp, op, n, out.ctypes.data_as(C.c_void_p))
        assert rc == 0 or (out == 77).all()  # an error leaves the output untouched
        return rc

    def msg(c):
        return (L.mc_last_error(c._h) or b"").decode()

    with m.Context(21, 0, 0, 0) as a, m.Context(21, 0, 0, 0) as b, m.Context(31, 0, 0, 0) as k31, m.Context(41, 1, 0, 0) as p41, \
            m.Context(41, 2, 0, 0) as f41:
        assert call([a]) == -4 and "mc_finalize_counts" in msg(a)  # MC_ESTATE
        for c, kk in ((a, 21), (b, 21), (k31, 31), (p41, 41), (f41, 41)):
            c.add_reads_packed(words, off)
        a.finalize()
        assert call([a, b]) == -4 and "table 1" in msg(a)
        for c in (b, k31, p41, f41):
            c.finalize()
        assert call([a, b]) == 0
        assert call([a], n_tables=0) == -1  # (no table 0 to take a message)
        assert call([a] * 5, n_tables=5) == -1 and "tables" in msg(a)
        assert call([a, None]) == -1 and "null" in msg(a)
        assert call([None, a]) == -1
        assert L.mc_seq_coverage(None, 1, None, None, 0, None) == -1
        assert call([a, k31]) == -1 and "k = 31" in msg(a)       # another k
        assert call([p41, f41]) == -1 and "key mode" in msg(p41)  # another key mode
        assert call([a], words_=None) == -1 and "null" in msg(a)
        assert call([a], off_=None) == -1
        assert call([a], words_=None, off_=None, dev=True) == -1 and "null" in msg(a)
        assert call([a], words_=None, off_=None, n=0) == 0          # nothing to do, after the checks
        assert call([a, k31], words_=None, off_=None, n=0) == -1
        got = m.seq_coverage([a, b], codes, off)
        # poly-A: 20 windows of one k-mer counted 20 times
        assert got.tolist() == [[[400, 20], [400, 20]]]
        with pytest.raises(native.McError) as e:
            m.seq_coverage([a, k31], codes, off)
        assert e.value.code == -1
