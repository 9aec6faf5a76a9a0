"""GPU: mc_env_join and mc_env_join_dev through the C ABI against tests/env_join_model.py (mc_env_join's definitions on dicts of
strings, which tests/test_env_join_model.py pins to the oracle and to the host's string function): member, is_gene, kc and the three
matrices must be identical.  The designed graph files of the CPU test, then 64 graphs with every bit of member used, 7 graphs with all
127 subsets, sums that wrap 2^32 more than twice, depths of 0 and 32767, no entries at all, and every error the call names."""
import functools
import random

import numpy as np
import pytest

from tests import env_join_model as M

pytestmark = pytest.mark.gpu

EINVAL = -1  # MC_EINVAL


def _ctx(k):
    import metacherchant_amd as m
    return m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)  # (no reads counted: the table plays no part)


def _inputs(graphs, gene, k, entries=None):
    entries = M.entries_of(graphs) if entries is None else entries
    hi, lo = M.pack(entries, k)
    rec_hi, rec_lo, rec_depth, offsets = M.records(graphs, k)
    return entries, (hi, lo, rec_hi, rec_lo, rec_depth, offsets, M.pack_gene(gene) if gene else None, len(gene))


def _check(got, want, G):
    assert got["n"] == len(want["member"]) and got["n_graphs"] == G
    assert got["member"].tolist() == want["member"]
    assert got["is_gene"].tolist() == want["is_gene"]
    assert got["kc"].tolist() == want["kc"]
    for name in ("diff", "diff_alt", "uni"):
        assert got[name].tolist() == want[name], name


def _dev(ctx, args):
    """the same call through mc_env_join_dev, the inputs in torch tensors on the device"""
    import torch
    hi, lo, rec_hi, rec_lo, rec_depth, offsets, gene, gene_len = args
    up = lambda a, dt: None if a is None else torch.from_numpy(a.astype(dt)).cuda()
    t = [up(hi, np.int64), up(lo, np.int64), up(rec_hi, np.int64), up(rec_lo, np.int64), up(rec_depth, np.int32), up(offsets, np.int64), up(gene, np.int64)]
    return ctx.env_join_dev(t[0], t[1], len(lo), t[2], t[3], t[4], t[5], len(offsets) - 1, t[6], gene_len)


@functools.lru_cache(maxsize=None)
def _designed(k, G):
    files, gene = M.designed_case(k, G)
    graphs = [M.graph_dict(lines) for lines in files]
    entries = M.entries_of(graphs)
    return graphs, gene, entries, M.join(entries, graphs, gene)


@pytest.mark.parametrize("G", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("k", [5, 21, 31, 32, 33, 63])
def test_designed_graphs_match_the_model(k, G):
    graphs, gene, entries, want = _designed(k, G)
    _, args = _inputs(graphs, gene, k, entries)
    ctx = _ctx(k)
    _check(ctx.env_join(*args), want, G)
    _check(_dev(ctx, args), want, G)


def test_entries_in_any_order_and_orientation():
    """entries shuffled and half of them given as reverse complements: member and is_gene do not care, kc counts the records that spell
    the entry as given"""
    k, G = 33, 4
    graphs, gene, entries, _ = _designed(k, G)
    rng = random.Random(1)
    entries = [M.rc(e) if rng.random() < 0.5 else e for e in entries]
    rng.shuffle(entries)
    want = M.join(entries, graphs, gene)
    _, args = _inputs(graphs, gene, k, entries)
    _check(_ctx(k).env_join(*args), want, G)


def _subset_graphs(k, G, subsets, rng, depth):
    """one k-mer a subset of the graphs (a bit mask), held by exactly those, oriented at random in each"""
    graphs = [dict() for _ in range(G)]
    seen = set()
    for s in subsets:
        while True:
            w = M.random_dna(rng, k)
            if M.normalize(w) not in seen and w != M.rc(w):
                break
        seen.add(M.normalize(w))
        for g in range(G):
            if s >> g & 1:
                graphs[g][w if rng.random() < 0.7 else M.rc(w)] = depth(rng)
    return graphs


def test_64_graphs_every_bit_of_member():
    """the 48 KB block of counters; 300 k-mers in random sets of the 64 graphs, the full set and every single graph among them"""
    k, G = 31, 64
    rng = random.Random(64)
    subsets = [(1 << 64) - 1] + [1 << g for g in range(64)] + [rng.getrandbits(64) | 1 << rng.randrange(64) for _ in range(235)]
    graphs = _subset_graphs(k, G, subsets, rng, lambda r: r.choice([0, 1, 5, 300, 32767]))
    entries, args = _inputs(graphs, "", k)
    want = M.join(entries, graphs, "")
    assert (1 << 64) - 1 in want["member"] and all(1 << g in want["member"] for g in range(64))
    ctx = _ctx(k)
    _check(ctx.env_join(*args), want, G)
    _check(_dev(ctx, args), want, G)


@pytest.mark.parametrize("k", [21, 63])
def test_7_graphs_all_127_subsets(k):
    G = 7
    rng = random.Random(7 + k)
    graphs = _subset_graphs(k, G, list(range(1, 128)) * 3, rng, lambda r: r.randrange(0, 1000))
    gene = next(iter(graphs[0]))[:k] + "ACGT"
    entries, args = _inputs(graphs, gene, k)
    want = M.join(entries, graphs, gene)
    assert set(want["member"]) == set(range(1, 128)) and sum(want["is_gene"]) >= 1
    _check(_ctx(k).env_join(*args), want, G)


@pytest.mark.parametrize("G", [2, 9])
def test_sums_wrap_2_32_more_than_twice(G):
    """records of depth 2^30: twelve k-mers that only graph 0 holds (diff and uni of row 0 grow by 2^30 each) and a few shared ones.
    Both kernels' ways of adding: G <= 8 through a wave's sum, above it through LDS atomics."""
    k = 31
    rng = random.Random(230 + G)
    subsets = [1] * 12 + [3] * 3 + [2] * 2 + ([1 << (G - 1)] * 10 if G > 2 else [])
    graphs = _subset_graphs(k, G, subsets, rng, lambda r: 1 << 30)
    for x in list(graphs[1])[:2]:
        graphs[1][x] = (1 << 30) - 7
    entries, args = _inputs(graphs, "", k)
    want = M.join(entries, graphs, "")
    assert want["raw_uni_max"] >= 2 << 32 and want["raw_diff_max"] >= 2 << 32  # (the case cannot silently stop wrapping)
    _check(_ctx(k).env_join(*args), want, G)


def test_depths_0_and_32767_and_negative():
    """graph.txt holds shorts, but the call takes any int: a negative depth is added as the host's uint32 conversion adds it"""
    k, G = 32, 3
    rng = random.Random(32767)
    graphs = _subset_graphs(k, G, [1, 2, 4, 3, 5, 6, 7] * 4, rng, lambda r: r.choice([0, 32767, -1, -32768]))
    entries, args = _inputs(graphs, "", k)
    want = M.join(entries, graphs, "")
    assert {0, 32767} <= {d for g in graphs for d in g.values()}
    _check(_ctx(k).env_join(*args), want, G)


@pytest.mark.parametrize("k", [21, 63])
def test_many_workgroups(k):
    """a few thousand entries cut from overlapping contigs (what the CLI test joins): more rows than one workgroup takes at once"""
    G = 4
    texts, gene = M.contig_environments(k, G, 3000)
    graphs = [dict((l.split()[0], int(l.split()[1])) for l in t.decode().splitlines()) for t in texts]
    entries, args = _inputs(graphs, gene, k)
    want = M.join(entries, graphs, gene)
    assert len(entries) > 3000 and sum(want["is_gene"]) > 100
    _check(_ctx(k).env_join(*args), want, G)


def test_no_entries():
    import metacherchant_amd as m
    ctx = _ctx(21)
    z64 = np.zeros(0, dtype=np.uint64)
    got = ctx.env_join(None, z64, None, z64, np.zeros(0, dtype=np.int32), np.zeros(4, dtype=np.uint64))
    assert got["n"] == 0 and got["n_graphs"] == 3 and len(got["member"]) == 0
    assert not got["diff"].any() and not got["diff_alt"].any() and not got["uni"].any() and got["uni"].shape == (3, 3)
    m.native.load().mc_env_join_free(None)


def test_every_error_and_the_context_still_serves():
    import ctypes as C
    import metacherchant_amd as m
    k, G = 33, 3
    graphs, gene, entries, want = _designed(k, G)
    _, good = _inputs(graphs, gene, k, entries)
    hi, lo, rec_hi, rec_lo, rec_depth, offsets, gene_words, gene_len = good
    ctx = _ctx(k)

    def refused(args, what):
        with pytest.raises(m.McError) as e:
            ctx.env_join(*args)
        assert e.value.code == EINVAL and what in str(e.value), str(e.value)
        _check(ctx.env_join(*good), want, G)  # the context still serves a good call

    # two entries the same k-mer; two entries each other's reverse complement
    for twin in (entries[3], M.rc(entries[3])):
        h2, l2 = M.pack(entries + [twin], k)
        refused((h2, l2) + good[2:], "two entries")
    # a record whose k-mer is no entry
    h2, l2 = M.pack(entries[1:], k)
    refused((h2, l2) + good[2:], "no entry")
    # the same oriented k-mer twice in one graph
    dup = np.concatenate([rec_lo[:1], rec_lo]), np.concatenate([rec_hi[:1], rec_hi]), np.concatenate([rec_depth[:1], rec_depth])
    off2 = offsets.copy()
    off2[1:] += 1
    refused((hi, lo, dup[1], dup[0], dup[2], off2, gene_words, gene_len), "twice")
    # more than 64 graphs; offsets that decrease
    refused((hi, lo, rec_hi, rec_lo, rec_depth, np.concatenate([offsets, np.full(63, offsets[-1], dtype=np.uint64)]), gene_words, gene_len), "graphs")
    bad = offsets.copy()
    bad[1] = bad[-1]
    assert bad[1] > bad[2]
    refused((hi, lo, rec_hi, rec_lo, rec_depth, bad, gene_words, gene_len), "decrease")
    # through the C ABI itself: no graph at all, null pointers, too many entries; *out is zeroed
    L = m.native.load()
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    p32 = rec_depth.ctypes.data_as(C.POINTER(C.c_int32))
    for call in (lambda r: L.mc_env_join(ctx._h, p64(hi), p64(lo), len(lo), p64(rec_hi), p64(rec_lo), p32, p64(offsets), 0, None, 0, r),
                 lambda r: L.mc_env_join(ctx._h, p64(hi), None, len(lo), p64(rec_hi), p64(rec_lo), p32, p64(offsets), G, None, 0, r),
                 lambda r: L.mc_env_join(ctx._h, None, p64(lo), len(lo), p64(rec_hi), p64(rec_lo), p32, p64(offsets), G, None, 0, r),
                 lambda r: L.mc_env_join(ctx._h, p64(hi), p64(lo), len(lo), None, p64(rec_lo), p32, p64(offsets), G, None, 0, r),
                 lambda r: L.mc_env_join(ctx._h, p64(hi), p64(lo), len(lo), p64(rec_hi), p64(rec_lo), None, p64(offsets), G, None, 0, r),
                 lambda r: L.mc_env_join(ctx._h, p64(hi), p64(lo), len(lo), p64(rec_hi), p64(rec_lo), p32, None, G, None, 0, r),
                 lambda r: L.mc_env_join(ctx._h, p64(hi), p64(lo), len(lo), p64(rec_hi), p64(rec_lo), p32, p64(offsets), G, None, 5, r),
                 lambda r: L.mc_env_join(ctx._h, p64(hi), p64(lo), 1 << 30, p64(rec_hi), p64(rec_lo), p32, p64(offsets), G, None, 0, r),
                 lambda r: L.mc_env_join_dev(ctx._h, None, None, len(lo), None, None, None, None, G, None, 0, r)):
        r = m.native._EnvJoin()
        r.n, r.device_ms = 99, 1.5
        assert call(C.byref(r)) == EINVAL
        assert r.n == 0 and not r.member and not r.uni and r.device_ms == 0
        L.mc_env_join_free(C.byref(r))  # (a zeroed result)
        _check(ctx.env_join(*good), want, G)
    assert L.mc_env_join(ctx._h, p64(hi), p64(lo), len(lo), p64(rec_hi), p64(rec_lo), p32, p64(offsets), G, None, 0, None) == EINVAL
