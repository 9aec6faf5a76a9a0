"""GPU: the designed key sets of tests/set_keys.py (which tests/test_set_keys_model.py holds to their names) through the C ABI of the
four units that build a k-mer set for one call and probe it, each result held exactly against the model the unit already has:
mc_reads_in_set against reads_filter_model.hits_and_keep, mc_unitigs against unitigs_model.link_analysis + pack_unitigs, mc_env_join
against env_join_model.join, mc_trim_paths against trim_paths_model.kept_mask in all three directions.  A long run of occupied slots
that passes slot cap - 1 and goes on at slot 0, look-ups that end only behind it, two-word keys that share their first word (the trim:
their low word), load exactly 0.5 and the doubled table one entry on; the entries in two shuffled orders, the second with every other
entry on the other strand where the unit folds the strands; host and device form; and one duplicate inside the crowded run a unit."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import env_join_model as ejm
from tests import reads_filter_model as rf
from tests import set_keys as sk
from tests import trim_paths_model as tm
from tests import unitigs_model as um

pytestmark = pytest.mark.gpu

EINVAL = -1  # MC_EINVAL
RUN_KS = (31, 32, 33, 47, 63)
HALF_K = {32: 31, 33: 33, 64: 32, 65: 47, 128: 63, 129: 33}


def _cases(unit):
    out = [("run_wrap", k, 0) for k in RUN_KS] + [("run_big", k, 0) for k in (31, 63)]
    out += [("shared_low_word", k, 0) for k in (33, 41, 63)] if unit == sk.TRIM_PATHS else [("shared_first_word", k, 0) for k in (33, 47, 63)]
    return out + [("half_full", HALF_K[n], n) for n in sk.HALF_FULL_N]


def _ids(unit):
    return ["%s-k%d%s" % (name, k, "-n%d" % n if n else "") for name, k, n in _cases(unit)]


def _make(name, k, unit, n):
    if name == "half_full":
        return sk.half_full(k, unit, n)
    if name == "shared_low_word":
        return sk.shared_low_word(k)
    return getattr(sk, name)(k, unit)


@functools.lru_cache(maxsize=None)
def _ctx(k):
    import metacherchant_amd as m
    return m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)  # (no reads counted: the counting table plays no part)


def _orders(n, fold):
    """two shuffled orders of n entries: (permutation, which entries go on the other strand)"""
    a, b = np.random.default_rng(n).permutation(n), np.random.default_rng(n + 1).permutation(n)
    return [(a, np.zeros(n, dtype=bool)), (b, (np.arange(n) % 2 == 1) & fold)]


def _arranged(strings, order, flip):
    return [sk.rc(strings[i]) if f else strings[i] for i, f in zip(order, flip)]


def _device(a, dtype=np.int64):
    """a numpy array of 4- or 8-byte words as a torch tensor on the device"""
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


# ---- reads-in-set

def _reads_inputs(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.asarray(po.encode("".join(reads)), dtype=np.uint8), off


def _reads_want(reads, k, members, pct):
    mem = rf.make_set(members)
    got = [rf.hits_and_keep(r, k, mem, pct) for r in reads]
    return np.array([g[0] for g in got], dtype=np.uint32), np.array([g[1] for g in got], dtype=bool)


@pytest.mark.parametrize("name,k,n", _cases(sk.READS_IN_SET), ids=_ids(sk.READS_IN_SET))
def test_reads_in_set(name, k, n):
    import metacherchant_amd as m
    case = _make(name, k, sk.READS_IN_SET, n)
    reads, members, pct = sk.reads_case(case)
    codes, off = _reads_inputs(reads)
    want_hits, want_keep = _reads_want(reads, k, members, pct)
    assert want_keep.any() and not want_keep.all()
    ctx = _ctx(k)
    for order, flip in _orders(len(members), True):
        hi, lo = um.pack_kmers(_arranged(members, order, flip))
        for weak in (False, True):
            hits, keep = m.reads_in_set(ctx, codes, off, hi if k > 32 else None, lo, pct=pct, weak=weak)
            bad = np.nonzero(hits != want_hits)[0]
            assert len(bad) == 0, (weak, bad[:8], hits[bad[:8]], want_hits[bad[:8]])
            assert np.array_equal(keep, want_keep), weak


@pytest.mark.parametrize("k", (31, 33, 63))
def test_reads_in_set_when_the_filter_passes_a_stranger(k):
    """absent windows whose word and three bits of the bit filter are all set by members: the table alone refuses them, and one of them
    would lift its read over the threshold; with MC_READS_IN_SET_WEAK_FILTER no filter stands in front of the table"""
    import metacherchant_amd as m
    case = sk.filter_pass(k)
    reads, members, pct = sk.reads_case(case)
    codes, off = _reads_inputs(reads)
    want_hits, want_keep = _reads_want(reads, k, members, pct)
    assert want_hits[0] == 18 and not want_keep[0] and want_keep.any()
    for order, flip in _orders(len(members), True):
        hi, lo = um.pack_kmers(_arranged(members, order, flip))
        for weak in (False, True):
            hits, keep = m.reads_in_set(_ctx(k), codes, off, hi if k > 32 else None, lo, pct=pct, weak=weak)
            assert np.array_equal(hits, want_hits) and np.array_equal(keep, want_keep), (weak, hits, want_hits)


# ---- unitigs

def _check_unitigs(got, want):
    offsets, words = um.pack_unitigs(want["seqs"])
    assert got["n_nodes"] == len(want["deg"]) and got["n_unitigs"] == len(want["first"]) and got["n_irregular"] == len(want["irregular"])
    assert got["deg"].tolist() == want["deg"]
    assert got["nbr"].tolist() == want["nbr"]
    assert got["first"].tolist() == want["first"] and got["last_rc"].tolist() == want["last_rc"]
    assert got["irregular"].tolist() == want["irregular"]
    assert np.array_equal(got["base_offsets"], offsets) and np.array_equal(got["bases"], words)


@pytest.mark.parametrize("name,k,n", _cases(sk.UNITIGS), ids=_ids(sk.UNITIGS))
def test_unitigs(name, k, n):
    case = _make(name, k, sk.UNITIGS, n)
    kmers, cls = sk.unitigs_case(case)
    ctx = _ctx(k)
    for order, flip in _orders(len(kmers), True):
        given, given_cls = _arranged(kmers, order, flip), [cls[i] for i in order]
        want = um.link_analysis(given, given_cls, k)
        at = {s: i for i, s in enumerate(given)}
        find = lambda s: at[s] if s in at else at[sk.rc(s)]
        for e, _, x in case.hit_carriers:   # a carrier's one neighbour on that side is the member it looks up
            p = 2 * find(e) + (0 if e in at else 1)  # the node that spells e; its successors are the neighbours of p ^ 1
            assert want["deg"][p ^ 1] == 1
        for e, _, x in case.miss_carriers:  # ... and a miss is nobody
            p = 2 * find(e) + (0 if e in at else 1)
            assert want["deg"][p ^ 1] == 0
        hi, lo = um.pack_kmers(given)
        _check_unitigs(ctx.unitigs(hi if k > 32 else None, lo, np.array(given_cls, dtype=np.uint8)), want)
    if name == "run_wrap" and k in (32, 63):  # the device form, on the second order
        import torch
        got = ctx.unitigs_dev(_device(hi) if k > 32 else None, _device(lo), torch.from_numpy(np.array(given_cls, dtype=np.uint8)).cuda(), len(lo))
        _check_unitigs(got, want)


# ---- the environment join

def _join_args(entries, graphs, gene, k):
    hi, lo = ejm.pack(entries, k)
    rec_hi, rec_lo, rec_depth, offsets = ejm.records(graphs, k)
    return hi, lo, rec_hi, rec_lo, rec_depth, offsets, ejm.pack_gene(gene) if gene else None, len(gene)


def _check_join(got, want, G):
    assert got["n"] == len(want["member"]) and got["n_graphs"] == G
    assert got["member"].tolist() == want["member"]
    assert got["is_gene"].tolist() == want["is_gene"]
    assert got["kc"].tolist() == want["kc"]
    for which in ("diff", "diff_alt", "uni"):
        assert got[which].tolist() == want[which], which


@pytest.mark.parametrize("name,k,n", _cases(sk.ENV_JOIN), ids=_ids(sk.ENV_JOIN))
def test_env_join(name, k, n):
    import metacherchant_amd as m
    case = _make(name, k, sk.ENV_JOIN, n)
    entries, graphs, gene = sk.join_case(case)
    G = len(graphs)
    ctx = _ctx(k)
    for order, flip in _orders(len(entries), True):
        given = _arranged(entries, order, flip)
        want = ejm.join(given, graphs, gene)
        at = {min(s, sk.rc(s)): i for i, s in enumerate(given)}
        assert [i for i, g in enumerate(want["is_gene"]) if g] == sorted(at[min(s, sk.rc(s))] for s in case.hits)  # the hits, no miss
        args = _join_args(given, graphs, gene, k)
        _check_join(ctx.env_join(*args), want, G)
    if name == "run_wrap":
        if k in (32, 63):  # the device form, on the second order
            hi, lo, rec_hi, rec_lo, rec_depth, offsets, gene_words, gene_len = args
            got = ctx.env_join_dev(_device(hi), _device(lo), len(lo), _device(rec_hi), _device(rec_lo), _device(rec_depth, np.int32), _device(offsets),
                                   G, _device(gene_words), gene_len)
            _check_join(got, want, G)
        # a record that is a designed miss: the look-up walks the run and the wrap, and the call names what it did not find
        bad = [dict(g) for g in graphs]
        bad[0][case.misses[0]] = 5
        with pytest.raises(m.McError) as e:
            ctx.env_join(*_join_args(given, bad, gene, k))
        assert e.value.code == EINVAL and "no entry" in str(e.value)


# ---- the trim

@pytest.mark.parametrize("name,k,n", _cases(sk.TRIM_PATHS), ids=_ids(sk.TRIM_PATHS))
def test_trim_paths(name, k, n):
    case = _make(name, k, sk.TRIM_PATHS, n)
    kmers, last = sk.trim_case(case)
    ctx = _ctx(k)
    for order, flip in _orders(len(kmers), False):
        given, given_last = [kmers[i] for i in order], np.array([last[i] for i in order], dtype=np.uint8)
        at = {s: i for i, s in enumerate(given)}
        hi, lo = tm.pack_kmers(given)
        for d in (-1, 1, 0):
            want = tm.kept_mask(given, given_last.tolist(), d)
            for e, side, _ in case.hit_carriers:   # kept through the member it looks up ...
                assert d == -side or want[at[e]] == 1
            for e, side, _ in case.miss_carriers:  # ... and a miss leads nowhere
                assert d != side or want[at[e]] == 0
            got = ctx.trim_paths(hi if k > 32 else None, lo, given_last, d)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (d, np.nonzero(got != want)[0][:8])
    if name == "run_wrap" and k in (32, 63):  # the device form, on the second order
        import torch
        d_kept = torch.full((len(lo),), 0x55, dtype=torch.uint8, device="cuda")
        ctx.trim_paths_dev(_device(hi) if k > 32 else None, _device(lo), torch.from_numpy(given_last).cuda(), len(lo), 0, d_kept)
        assert np.array_equal(d_kept.cpu().numpy(), want)


# ---- the device form of reads-in-set, and the duplicates

@pytest.mark.parametrize("k", (32, 63))
def test_reads_in_set_device_form(k):
    import torch

    import metacherchant_amd as m
    case = sk.run_wrap(k, sk.READS_IN_SET)
    reads, members, pct = sk.reads_case(case)
    codes, off = _reads_inputs(reads)
    want_hits, want_keep = _reads_want(reads, k, members, pct)
    hi, lo = um.pack_kmers(members)
    words = m.Context._words(codes, off, None)
    for weak in (False, True):
        d_hits = torch.full((len(reads),), 0x55555555, dtype=torch.int32, device="cuda")
        d_keep = torch.full((len(reads),), 0x55, dtype=torch.uint8, device="cuda")
        m.reads_in_set_dev(_ctx(k), _device(words), _device(off), len(reads), _device(hi) if k > 32 else None, _device(lo), len(lo), d_hits, d_keep,
                           pct=pct, weak=weak)
        assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), want_hits) and np.array_equal(d_keep.cpu().numpy().astype(bool), want_keep)


@pytest.mark.parametrize("k", (31, 33, 63))
def test_an_entry_given_twice_inside_the_run(k):
    """a member of the crowd with a late home, given again as the last entry, and (where the strands fold) as its reverse complement"""
    import metacherchant_amd as m
    ctx = _ctx(k)
    # unitigs and the join name the duplicate, in either orientation
    case = (sk.shared_first_word if k > 32 else sk.run_wrap)(k, sk.UNITIGS)
    kmers, cls = sk.unitigs_case(case)
    for again in (case.hits[0], sk.rc(case.hits[0])):
        hi, lo = um.pack_kmers(kmers + [again])
        with pytest.raises(m.McError) as e:
            ctx.unitigs(hi, lo, np.array(cls + [0], dtype=np.uint8))
        assert e.value.code == EINVAL and "same k-mer" in str(e.value)
    case = (sk.shared_first_word if k > 32 else sk.run_wrap)(k, sk.ENV_JOIN)
    entries, graphs, gene = sk.join_case(case)
    for again in (case.hits[0], sk.rc(case.hits[0])):
        with pytest.raises(m.McError) as e:
            ctx.env_join(*_join_args(entries + [again], graphs, gene, k))
        assert e.value.code == EINVAL and "two entries" in str(e.value)
    # the trim names the same oriented k-mer; a reverse complement is another entry
    case = sk.shared_low_word(k) if k > 32 else sk.run_wrap(k, sk.TRIM_PATHS)
    kmers, last = sk.trim_case(case)
    hi, lo = tm.pack_kmers(kmers + [case.hits[0]])
    with pytest.raises(m.McError) as e:
        ctx.trim_paths(hi, lo, np.array(last + [0], dtype=np.uint8), 1)
    assert e.value.code == EINVAL and "same oriented k-mer" in str(e.value)
    twin = sk.rc(case.hits[0])
    assert twin not in set(kmers)
    hi, lo = tm.pack_kmers(kmers + [twin])
    for d in (-1, 1, 0):
        got = ctx.trim_paths(hi, lo, np.array(last + [0], dtype=np.uint8), d)
        assert np.array_equal(got, tm.kept_mask(kmers + [twin], last + [0], d))
    # reads-in-set takes duplicates: the answer is the same
    case = (sk.shared_first_word if k > 32 else sk.run_wrap)(k, sk.READS_IN_SET)
    reads, members, pct = sk.reads_case(case)
    codes, off = _reads_inputs(reads)
    want_hits, want_keep = _reads_want(reads, k, members, pct)
    hi, lo = um.pack_kmers(members + [case.hits[0], sk.rc(case.hits[0]), case.hits[1]])
    for weak in (False, True):
        hits, keep = m.reads_in_set(ctx, codes, off, hi if k > 32 else None, lo, pct=pct, weak=weak)
        assert np.array_equal(hits, want_hits) and np.array_equal(keep, want_keep)
