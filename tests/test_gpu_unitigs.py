"""GPU: mc_unitigs through the C ABI against the string-level link analysis of tests/unitigs_model.py (which
tests/test_unitigs_model.py pins to the reference's loop): deg / nbr, first / last_rc, the packed bases and the irregular list must
be identical.  One- and two-word k-mers, a (k-1)-prefix of exactly one word, even and odd k; chains from 1 to 70 000 entries in
shuffled node order and orientation beside a class change, a branch, a cycle, a self-loop, a hairpin and a palindrome."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests import unitigs_model as um

pytestmark = pytest.mark.gpu

KS = (4, 5, 21, 31, 32, 33, 63)
EINVAL = -1  # MC_EINVAL


def _ctx(k):
    import metacherchant_amd as m
    return m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)  # (no reads counted: the table plays no part)


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """(kmers, cls, the model's result): computed once, shared, never changed"""
    if name == "mixed":
        kmers, cls = um.mixed_set(100 + k, k, (1, 2, 3) if k <= 5 else (1, 2, 3, 64, 65, 1000))
    elif name == "dense":
        kmers, cls = um.random_set({4: 206, 5: 205}[k], k, {4: 40, 5: 200}[k])  # (sets that hold regular and irregular chains)
    else:  # one chain of 70 000 entries (more than 16 rounds of pointer jumping, many workgroups) beside the mixed set
        rng = random.Random(300 + k)
        long = "".join(rng.choice("ACGT") for _ in range(70000 + k - 1))
        mixed, mixed_cls = _case("mixed", k)[:2]
        kmers = um.shuffled(rng, um.entries_of([long], k)) + list(mixed)
        cls = [0] * (len(kmers) - len(mixed)) + list(mixed_cls)
        assert len(kmers) == 70000 + len(mixed)  # (no k-mer of the chain repeats, none is in the mixed set)
    return tuple(kmers), tuple(cls), um.link_analysis(kmers, cls, k)


def _check(got, want):
    offsets, words = um.pack_unitigs(want["seqs"])
    assert got["n_nodes"] == len(want["deg"]) and got["n_unitigs"] == len(want["first"]) and got["n_irregular"] == len(want["irregular"])
    assert got["deg"].tolist() == want["deg"]
    assert got["nbr"].tolist() == want["nbr"]
    assert got["first"].tolist() == want["first"] and got["last_rc"].tolist() == want["last_rc"]
    assert got["irregular"].tolist() == want["irregular"]
    assert np.array_equal(got["base_offsets"], offsets)
    assert np.array_equal(got["bases"], words)


@pytest.mark.parametrize("k", KS)
def test_mixed_shapes_match_the_model(k):
    kmers, cls, want = _case("mixed", k)
    assert want["irregular"] and want["first"] and max(want["deg"]) >= 2
    if k > 5:
        assert {64, 65, 1000} <= {len(s) - k + 1 for s in want["seqs"]}  # (beside the branch's stem and the other shapes' chains)
    hi, lo = um.pack_kmers(kmers)
    _check(_ctx(k).unitigs(hi, lo, np.array(cls, dtype=np.uint8)), want)


@pytest.mark.parametrize("k", (4, 5))
def test_dense_random_sets_match_the_model(k):
    kmers, cls, want = _case("dense", k)
    assert want["irregular"] and want["first"]
    hi, lo = um.pack_kmers(kmers)
    _check(_ctx(k).unitigs(hi, lo, np.array(cls, dtype=np.uint8)), want)


@pytest.mark.parametrize("k", (21, 33))
def test_a_chain_of_70000_entries(k):
    kmers, cls, want = _case("long", k)
    assert max(len(s) for s in want["seqs"]) == 70000 + k - 1
    hi, lo = um.pack_kmers(kmers)
    _check(_ctx(k).unitigs(hi, lo, np.array(cls, dtype=np.uint8)), want)


WORD_EDGE_CASES = [(k, g) for k in (5, 31, 32, 33, 63) for g in range(len(um.word_edge_groups(k)))]


@pytest.mark.parametrize("odd_head", (False, True), ids=("even_head", "odd_head"))
@pytest.mark.parametrize("k,group", WORD_EDGE_CASES, ids=["%d-%s" % (k, "_".join(map(str, um.word_edge_groups(k)[g]))) for k, g in WORD_EDGE_CASES])
def test_unitig_lengths_at_word_edges(k, group, odd_head):
    """k_ut_bases: the head's k-mer over one or two words, every other node's last base at word (rank + k - 1) >> 5: unitigs of a word
    of bases, one less and one more, side by side (a base written a word late lands in the next unitig's first word), listed from an
    even node (the k-mer as given) and from an odd one (its reverse complement).  Every length of 31, 32, 33, 63, 64, 65, 96, 97 that
    has two entries at this k; at k = 5, where the 4-mers do not last for all of them at once, in six calls"""
    groups = um.word_edge_groups(k)
    assert sorted({n for g in groups for n in g} - {6}) == [n for n in um.WORD_EDGE_LENGTHS if n >= k + 1]  # (6: the short neighbour at k = 5)
    kmers, cls, lengths = um.word_edge_chains(500 + k, k, odd_head, group)
    want = um.link_analysis(kmers, cls, k)
    assert [len(s) for s in want["seqs"]] == lengths == groups[group] and len(lengths) >= 2 and not want["irregular"]
    assert all(h % 2 == (1 if odd_head else 0) for h in want["first"])
    hi, lo = um.pack_kmers(kmers)
    _check(_ctx(k).unitigs(hi, lo, np.array(cls, dtype=np.uint8)), want)


def test_no_entries():
    r = _ctx(21).unitigs(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8))
    assert r["n_nodes"] == 0 and r["n_unitigs"] == 0 and r["n_irregular"] == 0 and r["base_offsets"].tolist() == [0]
    assert len(r["deg"]) == len(r["nbr"]) == len(r["bases"]) == len(r["irregular"]) == 0


@pytest.mark.parametrize("k", (21, 33))
def test_an_entry_given_twice_is_an_error(k):
    import metacherchant_amd as m
    kmers, cls, _ = _case("mixed", k)
    for again in (kmers[5], um.rc(kmers[5])):
        hi, lo = um.pack_kmers(list(kmers) + [again])
        ctx = _ctx(k)
        with pytest.raises(m.McError) as e:
            ctx.unitigs(hi, lo, np.array(list(cls) + [0], dtype=np.uint8))
        assert e.value.code == EINVAL and "same k-mer" in str(e.value)


def test_errors_leave_a_zeroed_result():
    from metacherchant_amd import native
    ctx, L = _ctx(33), native.load()
    hi, lo = um.pack_kmers(["A" * 33, "C" * 33, "G" * 33])  # (C...C and G...G are each other's reverse complement)
    cls = np.zeros(3, dtype=np.uint8)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    for args in ((p(hi, C.c_uint64), p(lo, C.c_uint64), p(cls, C.c_uint8), 3),          # a duplicate
                 (None, p(lo, C.c_uint64), p(cls, C.c_uint8), 3),                        # no high words at k = 33
                 (p(hi, C.c_uint64), None, p(cls, C.c_uint8), 3),
                 (p(hi, C.c_uint64), p(lo, C.c_uint64), None, 3),
                 (p(hi, C.c_uint64), p(lo, C.c_uint64), p(cls, C.c_uint8), 1 << 30)):   # too many (nothing is read)
        r = native._Unitigs()
        C.memset(C.byref(r), 0x55, C.sizeof(r))
        assert L.mc_unitigs(ctx._h, *args, C.byref(r)) == EINVAL
        assert bytes(r) == bytes(C.sizeof(r))
    assert L.mc_unitigs(ctx._h, p(hi, C.c_uint64), p(lo, C.c_uint64), p(cls, C.c_uint8), 2, None) == EINVAL
    assert L.mc_unitigs_dev(ctx._h, None, None, None, 2, C.byref(native._Unitigs())) == EINVAL
    L.mc_unitigs_free(None)
    L.mc_unitigs_free(C.byref(native._Unitigs()))


@pytest.mark.parametrize("k", (21, 32))
def test_high_words_may_be_missing_up_to_k_32(k):
    kmers, cls, want = _case("mixed", k)
    hi, lo = um.pack_kmers(kmers)
    assert not hi.any()
    ctx = _ctx(k)
    _check(ctx.unitigs(None, lo, np.array(cls, dtype=np.uint8)), want)
    _check(ctx.unitigs(~hi, lo, np.array(cls, dtype=np.uint8)), want)  # (given, they are not read)


@pytest.mark.parametrize("k", (31, 63))
def test_the_device_form(k):
    import torch
    kmers, cls, want = _case("mixed", k)
    hi, lo = um.pack_kmers(kmers)
    as_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    d_hi, d_lo = as_dev(hi), as_dev(lo)
    d_cls = torch.from_numpy(np.array(cls, dtype=np.uint8)).cuda()
    ctx = _ctx(k)
    _check(ctx.unitigs_dev(d_hi if k > 32 else None, d_lo, d_cls, len(lo)), want)
    assert np.array_equal(d_lo.cpu().numpy().view(np.uint64), lo)  # (inputs are only read)


@pytest.mark.parametrize("k", (5, 33))
def test_two_calls_give_the_same_bytes(k):
    kmers, cls, _ = _case("mixed" if k == 5 else "long", k)
    hi, lo = um.pack_kmers(kmers)
    ctx = _ctx(k)
    a = ctx.unitigs(hi, lo, np.array(cls, dtype=np.uint8))
    b = ctx.unitigs(hi, lo, np.array(cls, dtype=np.uint8))
    for name in ("deg", "nbr", "first", "last_rc", "base_offsets", "bases", "irregular"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["device_ms"] > 0
