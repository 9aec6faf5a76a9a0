"""GPU: mc_kmer_presence through the C ABI against the oracle's tables (BigLong2ShortHashMap.contains: get() != -1)."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import synth_case

pytestmark = pytest.mark.gpu

CASES = [(31, 0), (5, 0), (41, 1), (63, 1), (41, 2)]  # (k, key mode): packed, polynomial, FNV-1a


def _windows(codes, off, k):
    """every k-window of the reads as oriented packed k-mers: (hi, lo) uint64 arrays"""
    m = (1 << (2 * k)) - 1
    out = []
    for r in range(len(off) - 1):
        v = 0
        a, b = int(off[r]), int(off[r + 1])
        for i in range(a, b):
            v = ((v << 2) | int(codes[i])) & m
            if i - a + 1 >= k:
                out.append(v)
    return out


def _rc(v, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (v & 3))
        v >>= 2
    return r


def _split(vals):
    return (np.array([v >> 64 for v in vals], dtype=np.uint64), np.array([v & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64))


def _codes(v, k):
    return np.array([(v >> (2 * (k - 1 - i))) & 3 for i in range(k)], dtype=np.uint8)


def _case(oracle, k, mode):
    """A thin synthetic read set (most k-mers are in one to three reads); read i goes to table t when bit t of i % 16 is set, so the
    tables are different, overlapping parts of it.  Table 0 also gets a poly-A read.  Queries: every window of the first reads,
    random k-mers, poly-A."""
    if k >= 23:
        genome_len, n_reads, L, n_query_reads, first = 200000, 2000, 150, 250, 0
    else:  # 512 canonical 5-mers: reads of a dozen bases, or every table holds everything (these reads hold no AAAAA or TTTTT)
        genome_len, n_reads, L, n_query_reads, first = 4000, 48, 12, 48, 100
    _, reads, off = synth_case(1, genome_len, n_reads, L, 100, first_read=first)
    parts = []
    for t in range(4):
        pick = [i for i in range(n_reads) if (i % 16) >> t & 1]
        codes = np.concatenate([reads[i * L:(i + 1) * L] for i in pick] + ([np.zeros(k + 3, dtype=np.uint8)] if t == 0 else []))
        o = np.concatenate([np.arange(len(pick) + 1, dtype=np.uint64) * L, np.array([len(pick) * L + k + 3] if t == 0 else [], dtype=np.uint64)])
        tab = oracle.Table()
        tab.count_reads(codes, o, k, mode)
        parts.append((tab, codes, o))
    rng = np.random.default_rng(1000 * k + mode)
    q = _windows(reads, off[:n_query_reads + 1], k)
    q += [int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * k)) - 1) for _ in range(len(q))]
    q.append(0)  # poly-A
    want = np.zeros(len(q), dtype=np.uint8)
    for i, v in enumerate(q):
        key = oracle.key(_codes(v, k), k, mode)
        for t in range(4):
            if parts[t][0].get(key) != -1:
                want[i] |= 1 << t
    return parts, q, want


@pytest.mark.parametrize("k,mode", CASES)
def test_presence_matches_the_oracle(k, mode, oracle):
    import torch

    import metacherchant_amd as m
    parts, q, want = _case(oracle, k, mode)
    # the test's own input, on the oracle's answer: all 16 masks occur; poly-A is in table 0 and not in table 1
    assert sorted(set(want.tolist())) == list(range(16)), sorted(set(want.tolist()))
    assert q[-1] == 0 and want[-1] & 1 and not want[-1] & 2
    hi, lo = _split(q)
    rhi, rlo = _split([_rc(v, k) for v in q])
    ctxs = []
    try:
        for _, codes, o in parts:
            c = m.Context(k, mode, 0, 0)
            ctxs.append(c)
            c.add_reads_packed(oracle.pack(codes), o)
            c.finalize()
        got = m.kmer_presence(ctxs, hi, lo)
        assert got.dtype == np.uint8 and got.shape == want.shape
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
        assert np.array_equal(m.kmer_presence(ctxs, rhi, rlo), want)  # the reverse complements
        if k <= 32:
            assert not hi.any() and np.array_equal(m.kmer_presence(ctxs, None, lo), want)
        for pick in ([0], [3], [1, 2], [3, 0], [2, 1, 0], [3, 2, 1, 0]):  # one, two, three and four tables, in any order
            w = np.zeros_like(want)
            for j, t in enumerate(pick):
                w |= ((want >> t) & 1) << j
            assert np.array_equal(m.kmer_presence([ctxs[t] for t in pick], hi, lo), w), pick
        # one context named twice (and four times): its bit twice
        assert np.array_equal(m.kmer_presence([ctxs[1], ctxs[1]], hi, lo), ((want >> 1) & 1) * 3)
        assert np.array_equal(m.kmer_presence([ctxs[2]] * 4, hi, lo), ((want >> 2) & 1) * 15)
        # poly-A present (table 0) and absent (table 1), alone in a call
        assert m.kmer_presence([ctxs[0], ctxs[1]], hi[-1:], lo[-1:]).tolist() == [1]
        # nothing to look up
        assert m.kmer_presence(ctxs, hi[:0], lo[:0]).shape == (0,)
        # the device form gives the host form's answer
        dev = torch.device("cuda", 0)
        d_hi = torch.from_numpy(hi.view(np.int64)).to(dev)
        d_lo = torch.from_numpy(lo.view(np.int64)).to(dev)
        d_mask = torch.full((len(q),), 0xEE, dtype=torch.uint8, device=dev)
        m.kmer_presence_dev(ctxs, d_hi, d_lo, len(q), d_mask)
        assert np.array_equal(d_mask.cpu().numpy(), want)
        if k <= 32:
            d_mask.fill_(0xEE)
            m.kmer_presence_dev(ctxs, None, d_lo, len(q), d_mask)
            assert np.array_equal(d_mask.cpu().numpy(), want)
        m.kmer_presence_dev(ctxs, d_hi, d_lo, 0, d_mask)
    finally:
        for c in ctxs:
            c.close()


def test_presence_refusals(oracle):
    import metacherchant_amd as m
    from metacherchant_amd import native
    L = native.load()
    codes = np.zeros(40, dtype=np.uint8)
    off = np.array([0, 40], dtype=np.uint64)
    words = oracle.pack(codes)
    hi0, lo0 = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)

    def call(ctxs, n_tables=None, hi=hi0, lo=lo0, n=3, dev=False, no_mask=False):
        out = np.full(3, 77, dtype=np.uint8)
        h = (C.c_void_p * 5)(*[c._h if c is not None else None for c in ctxs])
        f = L.mc_kmer_presence_dev if dev else L.mc_kmer_presence
        ptr = lambda a: None if a is None else (C.c_void_p(a.ctypes.data) if dev else a.ctypes.data_as(C.POINTER(C.c_uint64)))  # noqa: E731
        op = None if no_mask else (C.c_void_p(out.ctypes.data) if dev else out.ctypes.data_as(C.POINTER(C.c_uint8)))
        rc = f(h, len(ctxs) if n_tables is None else n_tables, ptr(hi), ptr(lo), n, op)
        assert rc == 0 or (out == 77).all()  # an error leaves the mask untouched
        return rc

    def msg(c):
        return (L.mc_last_error(c._h) or b"").decode()

    with m.Context(21, 0, 0, 0) as a, m.Context(21, 0, 0, 0) as b, m.Context(31, 0, 0, 0) as k31, m.Context(41, 1, 0, 0) as p41, \
            m.Context(41, 2, 0, 0) as f41:
        assert call([a]) == -4 and "mc_finalize_counts" in msg(a)  # MC_ESTATE
        for c in (a, b, k31, p41, f41):
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
        assert L.mc_kmer_presence(None, 1, None, None, 0, None) == -1
        assert call([a, k31]) == -1 and "k = 31" in msg(a)       # another k
        assert call([p41, f41]) == -1 and "key mode" in msg(p41)  # another key mode
        assert call([a], lo=None) == -1 and "null" in msg(a)
        assert call([a], no_mask=True) == -1
        assert call([p41], hi=None) == -1 and "null" in msg(p41)  # k > 32 needs the high words
        assert call([a], hi=None) == 0                             # ... k <= 32 does not
        assert call([a], hi=None, lo=None, dev=True) == -1 and "null" in msg(a)
        assert call([a], hi=None, lo=None, n=0) == 0               # nothing to do, after the checks
        assert call([a, k31], hi=None, lo=None, n=0) == -1
        assert call([a], n_tables=1, hi=None, lo=None, n=0, dev=True) == 0
        # poly-A, counted above: in both tables
        assert m.kmer_presence([a, b], None, lo0).tolist() == [3, 3, 3]
        with pytest.raises(native.McError) as e:
            m.kmer_presence([a, k31], None, lo0)
        assert e.value.code == -1


def test_tables_in_bins_and_in_hash_prefix_regions_in_one_call(oracle, monkeypatch):
    """Tables of one call that disagree on mm_k (packed k = 31): tables 0 and 2 in minimizer bins, tables 1 and 3 -- created with
    MC_SUPERKMERS=0 -- in hash-prefix regions; mc_kmer_presence and mc_seq_coverage against the oracle, for two lists of tables."""
    import metacherchant_amd as m
    k, mode = 31, 0
    parts, q, want = _case(oracle, k, mode)
    assert sorted(set(want.tolist())) == list(range(16)), sorted(set(want.tolist()))
    _, reads, off = synth_case(1, 200000, 2000, 150, 100, first_read=0)
    n_seqs = 250
    codes, seq_off = reads[:int(off[n_seqs])], off[:n_seqs + 1]
    get = np.zeros((n_seqs, 4, 2), dtype=np.uint64)  # per sequence and table: the sum of max(get, 0), the windows with get > 0
    for s in range(n_seqs):
        for v in _windows(codes[int(seq_off[s]):int(seq_off[s + 1])], np.array([0, int(seq_off[s + 1] - seq_off[s])]), k):
            key = oracle.key(_codes(v, k), k, mode)
            for t in range(4):
                c = max(parts[t][0].get(key), 0)
                get[s, t, 0] += c
                get[s, t, 1] += c > 0
    hi, lo = _split(q)
    ctxs = []
    try:
        for t, (_, pcodes, o) in enumerate(parts):
            with monkeypatch.context() as mp:  # (the switch is read once per context, by mc_create)
                if t & 1:
                    mp.setenv("MC_SUPERKMERS", "0")
                else:
                    mp.delenv("MC_SUPERKMERS", raising=False)
                c = m.Context(k, mode, 0, 0)
            ctxs.append(c)
            c.add_reads_packed(oracle.pack(pcodes), o)
            c.finalize()
        for pick in ([0, 1, 2, 3], [1, 0]):
            w = np.zeros_like(want)
            for j, t in enumerate(pick):
                w |= ((want >> t) & 1) << j
            assert np.array_equal(m.kmer_presence([ctxs[t] for t in pick], hi, lo), w), pick
            assert np.array_equal(m.seq_coverage([ctxs[t] for t in pick], codes, seq_off), get[:, pick, :]), pick
    finally:
        for c in ctxs:
            c.close()
