"""tests/crowded_tables.py against the C code (no GPU): its restatements of fmix64, sk_order, sk_bin and sk_hmin_of_kmer equal what
`mc_hosttest placement` prints from csrc/kmer_hash.h, the two 15-mers have the order and bin the cases rely on, every kept locus has
its 15-mer for the minimizer of all its windows, and every selected k-mer of a pool has the chosen hash prefix."""
import subprocess

import numpy as np
import pytest

from tests import crowded_tables as ct
from tests import seq_cov_model as sm


@pytest.fixture(scope="module")
def hosttest():
    from metacherchant_amd import build
    build.build_host()
    return build.HOSTTEST


def placement(hosttest, k, words):
    text = "".join("%x\n" % int(w) for w in words)
    out = subprocess.run([hosttest, "placement", str(k)], input=text, check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == 4 * len(words)
    return np.array([int(x, 16) for x in out], dtype=np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("k", [31, 23, 15, 32])
def test_the_restatements_give_what_the_header_gives(hosttest, k):
    rng = np.random.default_rng(k)
    words = rng.integers(0, 1 << 63, 4000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 4000, dtype=np.uint64)
    words[:6] = [0, 1, 0xFFFFFFFFFFFFFFFF, ct.M_INTERIOR, ct.M_LAST, 0xCCFF8DF3]
    got = placement(hosttest, k, words)
    assert np.array_equal(got[:, 0], ct.fmix64(words))
    assert np.array_equal(got[:, 1], ct.sk_order(words & np.uint64(0xFFFFFFFF)))
    assert np.array_equal(got[:, 2], ct.sk_bin(words & np.uint64(0xFFFFFFFF)))
    kmers = words if k == 32 else words & np.uint64((1 << (2 * k)) - 1)
    assert np.array_equal(got[:, 3], ct.sk_hmin_of_kmer(kmers, k))
    # either strand of a k-mer has the same minimizer
    rc = np.array([int(ct.pack_windows(ct.revcomp([(int(w) >> (2 * (k - 1 - i))) & 3 for i in range(k)]), k)[1][0]) for w in kmers[:50]], dtype=np.uint64)
    assert np.array_equal(ct.sk_hmin_of_kmer(rc, k), got[:50, 3])


def test_the_two_minimizers(hosttest):
    for m, order, sbin in ((ct.M_INTERIOR, 1, 0x688990c0), (ct.M_LAST, 1467272, 0xfffff483)):
        assert m < 1 << 30 and m <= int(ct.rc_mmer(np.array([m]))[0])  # canonical as written
        got = placement(hosttest, 15, [m, order])
        assert int(got[0, 1]) == order and int(got[1, 2]) == sbin and int(got[0, 3]) == order
        assert int(ct.sk_order(np.array([m]))[0]) == order and int(ct.sk_bin(np.array([order]))[0]) == sbin
    for n in [1 << x for x in range(21)] + [1000, 3 * 1024, 999983]:
        assert int(ct.region_of_bin(np.array([1467272]), n)[0]) == n - 1      # the last region, for every n_regions up to 2^20
        r = int(ct.region_of_bin(np.array([1]), n)[0])
        assert n < 4 or 0 < r < n - 1                                          # an interior one
    assert int(ct.sk_order(np.array([0]))[0]) == 0  # poly-A has order 0: not used


def test_every_window_of_a_kept_locus_has_the_minimizer():
    rng = np.random.default_rng(3)
    for m, order in ((ct.M_INTERIOR, 1), (ct.M_LAST, 1467272)):
        a = ct.loci(rng, m, 350)
        assert a.shape == (350, ct.LOCUS_LEN) and (a[:, 16:31] == ct.mmer_codes(m)).all()
        codes, off = ct.store(list(a))
        at, _ = ct.store_windows(codes, off, 31)
        assert len(at) == 350 * 17
        keys = sm.window_keys(codes, 31, 0)[at]
        assert len(np.unique(keys)) == 5950
        assert (ct.sk_hmin_of_kmer(keys, 31) == order).all()                   # the key is the canonical k-mer: either strand
        assert (ct.sk_hmin_of_kmer(ct.pack_windows(codes, 31)[1][at], 31) == order).all()
        assert len(np.unique(ct.region_of_bin(ct.sk_hmin_of_kmer(keys, 31), 1024))) == 1
    # unfiltered loci around the second 15-mer do hold smaller 15-mers now and then: the filter is not idle
    raw = rng.integers(0, 4, (3500, ct.LOCUS_LEN)).astype(np.uint8)
    raw[:, 16:31] = ct.mmer_codes(ct.M_LAST)
    codes, off = ct.store(list(raw))
    at, _ = ct.store_windows(codes, off, 31)
    assert (ct.sk_hmin_of_kmer(ct.pack_windows(codes, 31)[1][at], 31) < 1467272).any()


@pytest.mark.parametrize("k,mode", [(21, 0), (41, 1), (41, 2)])
def test_selected_pool_kmers_have_the_prefix(k, mode, oracle):
    p = ct.pool(5, k, mode, 1 << 20)
    for prefix in (ct.HASH_INTERIOR, ct.HASH_LAST):
        kmers, keys = ct.pool_region(p, prefix, k)
        assert 900 < len(kmers) < 1150 and len(np.unique(keys)) == len(keys)
        assert [oracle.key(x, k, mode) for x in kmers[:200]] == keys[:200].tolist()
        assert (ct.fmix64(keys) >> np.uint64(54) == prefix).all()
        assert (ct.region_of_hash(keys, 1024) == prefix).all()
        assert (ct.region_of_hash(keys, 2048) >> np.uint64(1) == prefix).all()
    assert (ct.region_of_hash(ct.pool_region(p, ct.HASH_LAST, k)[1], 1024) == 1023).all()


def test_store_windows_and_pack_windows():
    reads = [np.array([0, 1, 2, 3, 0], dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.array([3, 3], dtype=np.uint8), np.array([1, 2, 3], dtype=np.uint8)]
    codes, off = ct.store(reads)
    at, seq = ct.store_windows(codes, off, 3)
    assert at.tolist() == [0, 1, 2, 7] and seq.tolist() == [0, 0, 0, 3]
    hi, lo = ct.pack_windows(np.arange(40) % 4, 35)
    v = 0
    for c in (np.arange(35) % 4):
        v = (v << 2) | int(c)
    assert (int(hi[0]) << 64 | int(lo[0])) == v and len(lo) == 6


def test_solid_layout_against_linear_probing_done_slot_by_slot():
    """the longest run of occupied slots, wrap included, whatever the order of insertion; and the displacement in home order"""
    rng = np.random.default_rng(11)
    for n, clump in ((300, 0), (1000, 0), (700, 600), (400, 100)):
        keys = rng.integers(0, 1 << 62, 200 * n).astype(np.int64)
        lg = 12
        while (1 << lg) < 4 * n:
            lg += 1
        slot = (ct.fmix64(keys) >> np.uint64(64 - lg)).astype(np.int64)
        if clump:  # keys whose homes are the last 40 slots of region 0: the run wraps to the region's first slots
            at_end = keys[(slot >= 2048 - 40) & (slot < 2048)]
            assert len(at_end) >= clump
            keys = np.concatenate([at_end[:clump], keys[slot >= 2048][:n - clump]])
        keys = keys[:n]
        slot = (ct.fmix64(keys) >> np.uint64(64 - lg)).astype(np.int64)
        occupied = np.zeros(1 << lg, dtype=bool)
        for s in slot[rng.permutation(len(slot))]:
            r, h = s >> 11, s & 2047
            while occupied[(r << 11) | h]:
                h = (h + 1) & 2047
            occupied[(r << 11) | h] = True
        best = 0
        for r in range((1 << lg) >> 11):
            run = 0
            for o in np.tile(occupied[r << 11:(r + 1) << 11], 2):
                run = run + 1 if o else 0
                best = max(best, run)
        longest, displaced = ct.solid_layout(keys)
        assert longest == best, (n, clump, longest, best)
        assert (displaced >= 128) == (clump >= 40 + 128), (n, clump, displaced)
