"""GPU: mc_components through the C ABI against tests/components_model.py (FMTVisualizer's scan and KmerEnvCalculator's walks over a
dict that they zero).  n_components, seed_seq, seed_pos and member 0 are compared exactly, every component as a set of (canonical
k-mer, count); the device form gives the host form's answer and the context's mc_get answers stay what they were."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from oracle.host_oracle import normalize_dna, reverse_complement
from tests import components_model as cm

pytestmark = pytest.mark.gpu

CASES = [(31, 0), (5, 0), (4, 0), (41, 1), (63, 1), (41, 2)]  # (k, key mode): packed, polynomial, FNV-1a


def _rand(rng, n):
    return po.decode(rng.integers(0, 4, n).astype(np.uint8))


def _flat(reads):
    codes = np.concatenate([po.encode(r) for r in reads] + [np.zeros(0, dtype=np.uint8)]).astype(np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return codes, off


def _model(k, mode, counted, scanned):
    return cm.phase(k, mode, cm.count_table(counted, k, mode), None, scanned, pictures=False)[1]


def _kmer(hi, lo, k):
    return po.kmer_string(int(hi), int(lo), k)


def _check(k, mode, counted, scanned, want=None):
    """counts `counted`, asks for the components of `scanned`, compares with the model (or `want`); returns the model's components"""
    import torch

    import metacherchant_amd as m
    want = _model(k, mode, counted, scanned) if want is None else want
    codes, off = _flat(counted)
    scodes, soff = _flat(scanned)
    keys = np.array(sorted(cm.count_table(counted, k, mode)) + [12345], dtype=np.int64)
    with m.Context(k, mode, 0, 0) as c:
        c.add_reads_packed(po.pack(codes), off)
        c.finalize()
        before = c.get(keys)
        got = m.components(c, scodes, soff)
        assert got["n_components"] == len(want), (got["n_components"], len(want))
        assert got["seed_seq"].tolist() == [w[0] for w in want] and got["seed_pos"].tolist() == [w[1] for w in want]
        co = got["comp_offsets"]
        assert len(co) == len(want) + 1 and int(co[0]) == 0 and int(co[-1]) == got["n_kmers"] == sum(len(w[2]) for w in want)
        if k <= 32:
            assert not got["hi"].any()
        for ci, (s, p, members) in enumerate(want):
            a, b = int(co[ci]), int(co[ci + 1])
            assert _kmer(got["hi"][a], got["lo"][a], k) == scanned[s][p:p + k], ci  # member 0: the seed window as the read has it
            have = {(normalize_dna(_kmer(got["hi"][i], got["lo"][i], k)), int(got["cov"][i])) for i in range(a, b)}
            assert len(have) == b - a and have == set(members.items()), (ci, sorted(have ^ set(members.items()))[:6])
        # the device form
        dev = torch.device("cuda", 0)
        words = m.Context._words(scodes, soff, None)
        d_words = torch.from_numpy(words.view(np.int64)).to(dev)
        d_off = torch.from_numpy(soff.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        g2 = m.components_dev(c, d_words, d_off, len(scanned))
        for f in ("n_components", "n_kmers"):
            assert g2[f] == got[f]
        for f in ("comp_offsets", "seed_seq", "seed_pos"):
            assert np.array_equal(g2[f], got[f]), f
        for ci in range(len(want)):
            a, b = int(co[ci]), int(co[ci + 1])
            assert (g2["hi"][a], g2["lo"][a], g2["cov"][a]) == (got["hi"][a], got["lo"][a], got["cov"][a])
            assert sorted(zip(g2["hi"][a:b].tolist(), g2["lo"][a:b].tolist(), g2["cov"][a:b].tolist())) == \
                sorted(zip(got["hi"][a:b].tolist(), got["lo"][a:b].tolist(), got["cov"][a:b].tolist()))
        assert np.array_equal(c.get(keys), before)  # the table is only read
    return want


def _partition(comps):
    return sorted(tuple(sorted(m)) for _, _, m in comps)


@pytest.mark.parametrize("k,mode", CASES)
def test_bridge_hub_and_strand(k, mode):
    rng = np.random.default_rng(77 * k + mode)
    if k < 23:  # 4^k k-mers in all: short sequences, or everything hangs together
        g = _rand(rng, 30)
        a, b = g[:15], g[15 - k + 1:]
    else:
        g = _rand(rng, 200)
        a, b = g[:100], g[100 - k + 1:]
    # bridge: the last k-mer of A and the first of B are neighbours, and no read spans the junction (holds both in a row)
    want = _model(k, mode, [a, b], [a, b])
    if k >= 23:
        assert len(want) == 1 and len(want[0][2]) == 200 - k + 1
    assert not any(a[-k:] + b[k - 1] in r for r in (a, b)) and a[-k + 1:] == b[:k - 1] and b[:k] in cm.all_neighbors(a[-k:])
    _check(k, mode, [a, b], [a, b], want)
    if k < 23:  # (hub and strand need k-mers that do not repeat by chance: 2k-base cores and flanks of 20 random bases do at k <= 5)
        return
    # hub: 64 reads share a core of 2k bases between random flanks
    core = _rand(rng, 2 * k)
    hub = [_rand(rng, 20) + core + _rand(rng, 20) for _ in range(64)]
    w = _check(k, mode, hub, hub)
    assert len(w) == 1
    # strand: the reads and their reverse complements as further reads give the same partition
    few = [_rand(rng, k + 30) for _ in range(20)] + [a, b]
    w1 = _check(k, mode, few, few)
    w2 = _check(k, mode, few + [reverse_complement(r) for r in few], few + [reverse_complement(r) for r in few])
    assert _partition(w1) == _partition(w2) and [x[:2] for x in w1] == [x[:2] for x in w2]


# (k = 5 and k = 4 hold 512 and 136 canonical k-mers: a 20 000-base sequence is the complete graph there, which the dense case covers)
@pytest.mark.parametrize("k,mode", [(31, 0), (41, 1), (63, 1), (41, 2)])
def test_chain_of_20000_bases_is_one_component(k, mode):
    g = _rand(np.random.default_rng(5 + k), 20000)
    w = _check(k, mode, [g], [g])
    assert len(w) == 1 and len(w[0][2]) == 20000 - k + 1


@pytest.mark.parametrize("k,mode", CASES)
def test_many_small_components_are_numbered_in_scan_order(k, mode):
    rng = np.random.default_rng(9 + k)
    reads = [_rand(rng, k + int(rng.integers(0, 3))) for _ in range(3000)]
    w = _check(k, mode, reads, reads)
    if k >= 23:  # (random reads of k < 23 share k-mers: fewer components, still the model's)
        assert len(w) == 3000 and [x[0] for x in w] == list(range(3000))


def test_palindrome_poly_a_and_dense_small_k():
    # k = 4: AATT, ACGT are their own reverse complements; poly-A is its own neighbour
    _check(4, 0, ["AATT", "GGACGTCC", "AAAAAAA", "CCC"], ["AATT", "GGACGTCC", "AAAAAAA", "CCC"])
    for k, mode in ((31, 0), (41, 1)):
        w = _check(k, mode, ["A" * (k + 5)], ["A" * (k + 5)])
        assert len(w) == 1 and list(w[0][2].values()) == [6]
    # dense k = 5 (the read set of tests/test_gpu_presence.py: 48 reads of 12 bases over 512 canonical 5-mers): cycles
    from tests.helpers import synth_case
    _, reads, off = synth_case(1, 4000, 48, 12, 100, first_read=100)
    dense = [po.decode(reads[int(off[i]):int(off[i + 1])]) for i in range(48)]
    _check(5, 0, dense, dense)


# Not at k = 5 and k = 4.  A key that no window of the scan holds is no vertex of mc_components, while the model, like the reference,
# walks every key of the table; the two agree whenever the counted-only k-mers are not neighbours of scanned ones, which is this
# case's premise ("its k-mers are in no component") and cannot hold among 512 or 136 canonical k-mers: there the model's
# component has the counted-only k-mers in it (measured on the GPU: 104 members against the model's 128 at k = 4).
@pytest.mark.parametrize("k,mode", [c for c in CASES if c[0] >= 23])
def test_the_scan_differs_from_what_was_counted(k, mode):
    rng = np.random.default_rng(31 + k)
    r = [_rand(rng, 80) for _ in range(6)]
    # r[1] is counted in two pieces without its base 40 (the N), so the table lacks every window over it; the scan has A there
    counted = [r[0], r[1][:40], r[1][41:], r[2], r[3], r[4], r[5]]
    scanned = [r[0], r[1][:40] + "A" + r[1][41:], r[2][:k - 1], "", r[3], r[0]]  # ... shorter than k, empty, r[0] again
    table = cm.count_table(counted, k, mode)
    assert all(cm.kmer_key(scanned[1][i:i + k], k, mode) not in table for i in range(max(41 - k, 0), min(41, 81 - k)))
    w = _check(k, mode, counted, scanned)
    # the pieces of r[1] are 40 and 39 bases: two components at k = 31, no window at k = 41 and k = 63
    assert [x[0] for x in w] == ([0, 1, 1, 4] if k == 31 else [0, 4])
    inside = set().union(*[set(m) for _, _, m in w])  # r[2], r[4] and r[5] are counted and not scanned: in no component
    assert not any(normalize_dna(x[i:i + k]) in inside for x in (r[2], r[4], r[5]) for i in range(80 - k + 1))


def test_refusals():
    import metacherchant_amd as m
    from metacherchant_amd import native
    L = native.load()
    codes, off = _flat(["ACGTTGCAACGTAGCTAGCTAGGATCGATCGATTTGACC"])
    words = m.Context._words(codes, off, None)
    u64p = C.POINTER(C.c_uint64)
    with m.Context(21, 0, 0, 0) as c:
        r = native._Components()
        wp, op = words.ctypes.data_as(u64p), off.ctypes.data_as(u64p)
        assert L.mc_components(c._h, wp, op, 1, C.byref(r)) == -4 and b"mc_finalize_counts" in L.mc_last_error(c._h)  # MC_ESTATE
        c.add_reads_packed(words, off)
        c.finalize()
        assert L.mc_components(c._h, None, op, 1, C.byref(r)) == -1 and b"null" in L.mc_last_error(c._h)
        assert L.mc_components(c._h, wp, None, 1, C.byref(r)) == -1
        assert L.mc_components(c._h, wp, op, 1, None) == -1
        assert L.mc_components_dev(c._h, None, None, 1, C.byref(r)) == -1
        assert L.mc_components(None, wp, op, 1, C.byref(r)) == -1
        assert r.n_components == 0 and not r.comp_offsets
        for f in (L.mc_components, L.mc_components_dev):  # n_seqs == 0: an empty result
            assert f(c._h, None, None, 0, C.byref(r)) == 0
            assert r.n_components == 0 and r.n_kmers == 0 and r.comp_offsets[0] == 0
            L.mc_components_free(C.byref(r))
            assert not r.comp_offsets
        L.mc_components_free(C.byref(r))  # (a freed result again, and NULL)
        L.mc_components_free(None)
        got = m.components(c, codes, off)
        assert got["n_components"] == 1 and got["n_kmers"] == len(codes) - 20
        got = m.components(c, codes[:0], off[:1])
        assert got["n_components"] == 0 and got["comp_offsets"].tolist() == [0]
