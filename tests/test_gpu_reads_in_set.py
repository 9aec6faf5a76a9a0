"""GPU: mc_reads_in_set through the C ABI against the string-level model of ReadsFilter (tests/reads_filter_model.py): hits and
keep exactly, for one- and two-word k-mers, with and without the bit filter, for sets from empty to 200 000 k-mers."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import reads_filter_model as rf

pytestmark = pytest.mark.gpu

KS = (5, 16, 31, 32, 33, 55, 63)
PCTS = (0, 1, 50, 100)
GENOME_LEN = 50000
STRETCH = 20000  # where the ~500 k-mers of the small set start in the genome


def _batch(k):
    """~3 000 reads off a 50 kb random genome with 1 % substitutions, every fourth reverse-complemented, every ninth with two of its
    bases read as N (code 0): lengths 0 .. 400, the lengths around k and around the packed words' ends, and two reads of ~20 000
    bases.  Returns (genome text, list of read texts)."""
    rng = np.random.default_rng(7000 + k)
    genome = rng.integers(0, 4, GENOME_LEN).astype(np.uint8)
    lens = [k - 1, k, k + 1, k + 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 1]
    lens += rng.integers(0, 401, 2900).tolist()
    lens[100], lens[2000] = 20011, 19997
    reads = []
    for i, n in enumerate(lens):
        # (every fourth read near the small set's stretch, so that set hits some reads often and most never)
        s = int(rng.integers(STRETCH - 300, STRETCH + 800)) if i % 4 == 3 and n <= 400 else int(rng.integers(0, GENOME_LEN - n + 1))
        r = genome[s:s + n].copy()
        flip = rng.random(n) < 0.01
        r[flip] = (r[flip] + rng.integers(1, 4, int(flip.sum()))) & 3
        if i % 4 == 1:
            r = (3 - r[::-1]).astype(np.uint8)
        if i % 9 == 2 and n >= 2:
            r[[n // 3, n - 1]] = 0
        reads.append(po.decode(r))
    return po.decode(genome), reads


def _pack_set(kmers, k):
    """oriented packed k-mers (hi, lo): the first base most significant, 2k bits right-aligned in 128"""
    codes = np.asarray(po.encode("".join(kmers)), dtype=np.uint64).reshape(-1, k)
    hi, lo = np.zeros(len(codes), dtype=np.uint64), np.zeros(len(codes), dtype=np.uint64)
    for j in range(k):
        hi = (hi << np.uint64(2)) | (lo >> np.uint64(62))
        lo = (lo << np.uint64(2)) | codes[:, j]
    return hi, lo


def _sets(genome, k, rng):
    """name -> k-mer strings, oriented as given to the library"""
    one = [genome[STRETCH + 40:STRETCH + 40 + k]]
    stretch = [genome[i:i + k] for i in range(STRETCH, STRETCH + 500)]
    mixed = [rf.reverse_complement(x) if i % 3 == 0 else x for i, x in enumerate(stretch)] + stretch[:50] + [rf.reverse_complement(x) for x in stretch[10:30]]
    # 200 000: a third of the genome's k-mers (reads outside it still miss) and random k-mers, duplicates among them at small k
    letters = np.array(list("AGCT"))
    rand = ["".join(row) for row in letters[rng.integers(0, 4, (200000 - 16000, k))]]
    big = [genome[i:i + k] for i in range(5000, 21000)] + rand
    return {"empty": [], "one": one, "stretch": mixed, "big": big}


def _offsets(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return off


@pytest.fixture(scope="module")
def cases():
    """k -> (codes, offsets, read lengths, {set name: (hi, lo, model hits)}), worked out once"""
    cache = {}

    def get(k):
        if k not in cache:
            genome, reads = _batch(k)
            windows = [rf.tested_windows(r, k) for r in reads]
            sets = {}
            for name, kmers in _sets(genome, k, np.random.default_rng(k)).items():
                members = rf.make_set(kmers)
                hits = np.array([sum(1 for w in ws if w in members) for ws in windows], dtype=np.uint32)
                sets[name] = _pack_set(kmers, k) + (hits,)
            cache[k] = (np.asarray(po.encode("".join(reads)), dtype=np.uint8), _offsets(reads), np.array([len(r) for r in reads]), sets)
        return cache[k]
    return get


def _keep(hits, lens, k, pct):
    return np.array([n > k and h >= rf.threshold(int(n), k, pct) for h, n in zip(hits.tolist(), lens.tolist())])


@pytest.mark.parametrize("k", KS)
def test_hits_and_keep_are_the_models(k, cases):
    import metacherchant_amd as m
    codes, off, lens, sets = cases(k)
    # the test's own input, on the model's answer: the small sets hit some reads and miss most; a long read is hit in the big set
    # (at k = 5 a set of 500 holds nearly all 512 canonical 5-mers)
    assert (sets["one"][2] > 0).any() and (sets["big"][2] > 0).sum() > 100 and not sets["empty"][2].any()
    assert 0 < (sets["stretch"][2] > 0).sum() < (len(lens) // 2 if k >= 16 else len(lens))
    assert k < 16 or ((sets["big"][2] == 0) & (lens > k)).any()
    assert {k - 1, k, k + 1, k + 2, 31, 32, 33, 63, 64, 65, 127, 128, 129} <= set(lens.tolist()) and (lens > 19000).sum() == 2
    ctx = m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)  # (no reads counted, no mc_finalize_counts: none is needed)
    for name, (hi, lo, want) in sets.items():
        for weak in (False, True):
            for pct in PCTS:
                hits, keep = m.reads_in_set(ctx, codes, off, hi if k > 32 or name == "stretch" else None, lo, pct=pct, weak=weak)
                assert hits.dtype == np.uint32 and keep.dtype == bool
                bad = np.nonzero(hits != want)[0]
                assert len(bad) == 0, (name, weak, pct, len(bad), bad[:8], hits[bad[:8]], want[bad[:8]], lens[bad[:8]])
                assert np.array_equal(keep, _keep(want, lens, k, pct)), (name, weak, pct)
                if pct == 100:
                    assert not keep.any()  # at most L - k hits against a threshold of L - k + 1
        if name == "stretch":
            assert _keep(want, lens, k, 50).any() and not _keep(want, lens, k, 1).all()


@pytest.mark.parametrize("k", (31, 33))
def test_the_key_mode_plays_no_part(k, cases):
    import metacherchant_amd as m
    codes, off, lens, sets = cases(k)
    hi, lo, want = sets["stretch"]
    modes = (m.KEY_PACKED, m.KEY_POLY, m.KEY_FNV1A)
    for mode in modes:
        if mode == m.KEY_PACKED and k > 31:  # (the library has no packed keys above k = 31: no such context exists)
            with pytest.raises(m.McError):
                m.Context(k, mode, 0, 0)
            continue
        ctx = m.Context(k, mode, 0, 0)
        for weak in (False, True):
            hits, keep = m.reads_in_set(ctx, codes, off, hi, lo, pct=1, weak=weak)
            assert np.array_equal(hits, want) and np.array_equal(keep, _keep(want, lens, k, 1)), (mode, weak)


@pytest.mark.parametrize("k", (31, 55))
def test_device_pointers_and_a_counted_context_agree(k, cases):
    import torch

    import metacherchant_amd as m
    codes, off, lens, sets = cases(k)
    hi, lo, want = sets["stretch"]
    ctx = m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)
    words = m.Context._words(codes, off, None)
    as_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    d_words, d_off, d_hi, d_lo = as_dev(words), as_dev(off), as_dev(hi), as_dev(lo)
    n = len(lens)

    def run(weak):
        d_hits = torch.full((n,), 0x55555555, dtype=torch.int32, device="cuda")
        d_keep = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
        m.reads_in_set_dev(ctx, d_words, d_off, n, d_hi, d_lo, len(lo), d_hits, d_keep, pct=1, weak=weak)
        return d_hits.cpu().numpy().view(np.uint32), d_keep.cpu().numpy().astype(bool)
    for weak in (False, True):  # before mc_finalize_counts
        hits, keep = run(weak)
        assert np.array_equal(hits, want) and np.array_equal(keep, _keep(want, lens, k, 1))
    ctx.add_reads_packed(words, off)
    ctx.finalize()
    hits, keep = run(False)  # ... and after
    assert np.array_equal(hits, want) and np.array_equal(keep, _keep(want, lens, k, 1))
    # an offset array that does not start at base 0: the reads from number 7 on
    d_hits = torch.zeros(n - 7, dtype=torch.int32, device="cuda")
    d_keep = torch.zeros(n - 7, dtype=torch.uint8, device="cuda")
    m.reads_in_set_dev(ctx, d_words, d_off[7:], n - 7, d_hi, d_lo, len(lo), d_hits, d_keep, pct=1)
    assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), want[7:])


def test_errors_leave_the_outputs_alone(cases):
    import metacherchant_amd as m
    from metacherchant_amd import native
    k = 33
    codes, off, lens, sets = cases(k)
    hi, lo, _ = sets["one"]
    ctx = m.Context(k, m.KEY_POLY, 0, 0)
    L = native.load()
    words = m.Context._words(codes, off, None)
    n = len(lens)
    hits, keep = np.full(n, 0xABABABAB, dtype=np.uint32), np.full(n, 0xAB, dtype=np.uint8)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None
    out = (hits.ctypes.data_as(C.POINTER(C.c_uint32)), keep.ctypes.data_as(C.POINTER(C.c_uint8)))

    def call(w=words, o=off, nr=n, h=hi, l=lo, ns=1, pct=1, outs=out):
        return L.mc_reads_in_set(ctx._h, p64(w), p64(o), nr, p64(h), p64(l), ns, pct, 0, outs[0], outs[1])
    EINVAL = -1
    assert call(pct=-1) == EINVAL and call(pct=101) == EINVAL
    assert call(ns=1 << 31) == EINVAL
    assert call(w=None) == EINVAL and call(o=None) == EINVAL and call(l=None) == EINVAL
    assert call(h=None) == EINVAL  # k > 32: the high words are needed
    assert call(outs=(None, out[1])) == EINVAL and call(outs=(out[0], None)) == EINVAL
    assert L.mc_reads_in_set_dev(ctx._h, None, None, n, None, None, 1, 1, 0, None, None) == EINVAL
    assert L.mc_reads_in_set_dev(ctx._h, None, None, 0, None, None, 0, 101, 0, None, None) == EINVAL
    assert (hits == 0xABABABAB).all() and (keep == 0xAB).all()
    assert "mc_reads_in_set" in (L.mc_last_error(ctx._h) or b"").decode()
    # no reads: nothing to do, whatever the pointers; no set: every output 0
    assert call(nr=0, w=None, o=None, outs=(None, None)) == 0
    assert L.mc_reads_in_set_dev(ctx._h, None, None, 0, None, None, 0, 1, 0, None, None) == 0
    assert call(ns=0, h=None, l=None) == 0
    assert not hits.any() and not keep.any()
    ctx31 = m.Context(31, m.KEY_PACKED, 0, 0)  # k <= 32: no high words needed
    c31, o31, l31, s31 = cases(31)
    assert np.array_equal(m.reads_in_set(ctx31, c31, o31, None, s31["one"][1])[0], s31["one"][2])
