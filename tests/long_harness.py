"""What tests/test_gpu_long_leaves.py and tests/test_gpu_long_crowded_bins.py share (test infrastructure only): contexts of polynomial
keys in minimizer bins under either bin rule, a background of random reads that stays out of the designed bins and is large enough for
the leaf capacity the host plans, the debug line of the merge stage, and the comparisons with the CPU oracle (oracle/pyoracle.py).

The expected table of a run is the oracle's table of the designed reads beside the oracle's table of the background's reads times the
number of times they went in: no key is in both (asserted).  A walk from designed reads is compared with po.bfs on the oracle's table of
the designed reads alone after proving that this is the walk on the whole table: a walk asks the table for nothing but the neighbours of
the k-mers it has reached, and none of those is a key of the background (asserted from the oracle's result)."""
import functools
import math
import re

import numpy as np

from oracle import pyoracle as po
from tests import crowded_tables as ct
from tests import long_loci as ll
from tests import read_pointers as rp
from tests.helpers import assert_bfs_equal, seed_windows

HINT = 800_000            # distinct keys the table is made for: the minimum of 4 M slots, and more keys than any case counts
BG_READS, BG_LEN = 4000, 150
MERGE_LINE = re.compile(r"\[count\] merge: (k_p3_\w+(?:<[^>]*>)?) over (\d+) leaves, lcap (\d+), ptr_tries (\d+), general kernel behind it: (yes|no)")
SWITCHES = ("MC_COUNT_PATH", "MC_LONG_RECORDS", "MC_LONG_BINS", "MC_BFS_DIRECT", "MC_SUPERKMERS", "MC_P3_DEDUP")


def set_switches(mp, rule, **more):
    """the environment of a context that counts reads as long records under this bin rule (read at mc_create)"""
    for n in SWITCHES:
        mp.delenv(n, raising=False)
    mp.setenv("MC_COUNT_PATH", "partition")
    mp.setenv("MC_INGEST_DEBUG", "1")
    if rule == 2:
        mp.setenv("MC_LONG_BINS", "2")
    for n, v in more.items():
        mp.setenv(n, v)


def cap2(n_records, n_leaves):
    """mcgpu.hip pipe_prepare: the capacity of a leaf's stream of records"""
    mean = float(n_records) / float(n_leaves)
    return int(mean * 1.15 + 32.0 * math.sqrt(mean) + 64.0)


def records_expected(k, rule, n_windows, n_reads):
    """mcgpu.hip add_reads_long: the records the host expects of a batch (sk_records_bound, 8 / 5 of it under rule 2)"""
    n = int(float(n_windows) * 2.0 / float(k - ll.SK_M + 2) * 1.5) + 2 * n_reads + 1024
    return n * 8 // 5 if rule == 2 else n


@functools.lru_cache(maxsize=None)
def n_leaves(k, rule):
    import pytest

    import metacherchant_amd as m
    with pytest.MonkeyPatch.context() as mp:
        set_switches(mp, rule)
        with m.Context(k, po.KEY_POLY, 0, HINT) as ctx:
            slots = int(ctx.stats().table_slots)
    assert slots % ct.REGION_SLOTS == 0 and slots // ct.REGION_SLOTS >= 1024  # (a second scatter level exists)
    return slots // ct.REGION_SLOTS


class Background:
    """random reads none of whose windows falls into a designed region (the bins of `words`, and region 0 for poly-A), the oracle's
    table of them, and how many times they go in so that the host plans a leaf capacity of `lcap` records and more"""

    def __init__(self, k, rule, words, lcap):
        self.k, self.rule, self.nl = k, rule, n_leaves(k, rule)
        rng = np.random.default_rng(8400 + 10 * k + rule)
        reads = rng.integers(0, 4, (BG_READS + 300, BG_LEN)).astype(np.uint8)
        region = ll.region_of(ll.bin_words(reads, k, rule), self.nl)
        designed = [0] + [int(ll.region_of(np.array([w], dtype=np.uint64), self.nl)[0]) for w in words]
        bad = np.isin(region, designed).any(axis=1)
        assert 0 < bad.sum() <= 300
        self.reads = reads[~bad][:BG_READS]
        assert len(self.reads) == BG_READS
        t = po.Table()
        t.count_reads(self.reads.reshape(-1), np.arange(BG_READS + 1, dtype=np.uint64) * BG_LEN, k, po.KEY_POLY)
        self.keys, self.counts = t.dump()
        self.counts = self.counts.astype(np.int64)
        windows = BG_READS * (BG_LEN - k + 1)
        self.mult = 1
        while cap2(records_expected(k, rule, self.mult * windows, self.mult * BG_READS), self.nl) < lcap:
            self.mult += 1

    def list(self, mult=None):
        return [self.reads[i % BG_READS] for i in range(BG_READS * (self.mult if mult is None else mult))]


_bg = {}


def background(k, rule, words, lcap):
    key = (k, rule, tuple(words), lcap)
    if key not in _bg:
        _bg[key] = Background(k, rule, words, lcap)
    return _bg[key]


def shuffled(designed, bg_list, seed):
    """(codes, offsets, the offsets of the designed reads, their indices in `designed`): the designed reads shuffled among the others"""
    rng = np.random.default_rng(seed)
    n_bg = len(bg_list)
    order = rng.permutation(n_bg + len(designed))
    mine = np.nonzero(order >= n_bg)[0]
    parts = [bg_list[i] if i < n_bg else designed[i - n_bg] for i in order.tolist()]
    off = np.zeros(len(order) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts).astype(np.uint8), off, off[mine].astype(np.int64), order[mine] - n_bg


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def add_reads(ctx, codes, off):
    ctx.add_reads_packed_dev(dev(po.pack(codes).view(np.int64)), dev(off.view(np.int64)), len(off) - 1, len(codes))


def export(ctx):
    """(keys ascending, counts, hints) of the whole table"""
    import torch
    n = ctx.export_count(0)
    d = torch.device("cuda:0")
    pk = torch.zeros(n, dtype=torch.int64, device=d)
    pc = torch.zeros(n, dtype=torch.int16, device=d)
    ph = torch.zeros(n, dtype=torch.int32, device=d)
    assert ctx.export_dev(0, pk, pc, n, ph) == n
    keys, counts, hints = pk.cpu().numpy(), pc.cpu().numpy().astype(np.int64), ph.cpu().numpy().view(np.uint32).astype(np.int64)
    o = np.argsort(keys, kind="stable")
    return keys[o], counts[o], hints[o]


def merge_lines(capfd):
    return MERGE_LINE.findall(capfd.readouterr().err)


def oracle_of(reads, k):
    """the oracle's table of a list of reads, and its dump"""
    t = po.Table()
    codes, off = ct.store(reads)
    t.count_reads(codes, off, k, po.KEY_POLY)
    keys, counts = t.dump()
    return t, keys, counts.astype(np.int64)


def expected(designed_dump, B, times):
    """(keys ascending, counts) of the designed reads' table beside `times` times the background's"""
    dk, dc = designed_dump
    assert len(np.intersect1d(dk, B.keys)) == 0
    keys = np.concatenate([dk, B.keys])
    counts = np.minimum(np.concatenate([dc, B.counts * times]), 32767)
    o = np.argsort(keys, kind="stable")
    return keys[o], counts[o]


def assert_table(got_keys, got_counts, keys, counts, name):
    assert len(got_keys) == len(keys), (name, len(got_keys), len(keys))
    assert len(np.unique(got_keys)) == len(got_keys), (name, "a key is exported twice")
    assert np.array_equal(got_keys, keys), name
    wrong = np.nonzero(got_counts != counts)[0]
    assert len(wrong) == 0, "%s: %d of %d counts differ, the first (key, got, want): %s" % (
        name, len(wrong), len(keys), [(int(keys[i]), int(got_counts[i]), int(counts[i])) for i in wrong[:5]])


def answers(keys, counts, asked):
    """mc_get's answer by the expected table: the count, or -1"""
    at = np.minimum(np.searchsorted(keys, asked), len(keys) - 1)
    return np.where(keys[at] == asked, counts[at], -1)


def neighbour_keys(hi, lo, k):
    """the keys of the eight neighbours of every oriented k-mer (hi:lo) of a walk's result"""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    c = np.zeros((len(lo), k), dtype=np.uint8)
    for i in range(k):
        sh = 2 * (k - 1 - i)
        c[:, i] = ((hi >> np.uint64(sh - 64)) if sh >= 64 else (lo >> np.uint64(sh))) & np.uint64(3)
    nb = np.zeros((len(lo), 8, k), dtype=np.uint8)
    for b in range(4):
        nb[:, b, :k - 1], nb[:, b, k - 1] = c[:, 1:], b
        nb[:, 4 + b, 1:], nb[:, 4 + b, 0] = c[:, :-1], b
    return ll.window_keys(nb, k).reshape(-1)


def seeds_windows(seeds, k):
    """(hi, lo) of every window of every seed read, as the walk takes them"""
    his, los = zip(*[seed_windows(s, k) for s in seeds])
    return np.concatenate(his), np.concatenate(los)


def assert_walk(ctx, t, k, seeds, B, direction, min_cov, max_kmers=20000, windows=None):
    """ctx's walk from the seed reads against po.bfs on t, the oracle's table of the designed reads, with the proof that the background
    cannot change it: no neighbour of a reached k-mer, and no seed window, is a key of the background.  Returns the oracle's result."""
    want = po.bfs(t, k, po.KEY_POLY, seeds, direction, min_cov, max_kmers, -1)
    hi, lo = seeds_windows(seeds, k) if windows is None else windows
    asked = np.concatenate([ll.window_keys(s, k) for s in seeds] + ([neighbour_keys(want["hi"], want["lo"], k)] if want is not None else []))
    assert not np.isin(asked, B.keys).any()
    assert_bfs_equal(ctx.bfs(hi, lo, direction, min_cov, max_kmers, -1), want)
    return want


def assert_pointers(keys, hints, designed_keys, batches, k, name):
    """tests/read_pointers.py not_found over the designed keys: every hint of one leads to a window with that key.  batches: (store
    position of the batch, its bases, the offsets of the designed reads in it, those reads)"""
    total = batches[-1][0] + batches[-1][1]
    wk = np.full(total, -1, dtype=np.int64)
    for at, _, offs, reads in batches:
        for o, r in zip(offs.tolist(), reads):
            w = ll.window_keys(r, k)
            wk[at + o:at + o + len(w)] = w
    h = hints[np.searchsorted(keys, designed_keys)]
    bad = rp.not_found(designed_keys, h, 0, wk, wk != -1, total)
    assert len(bad) == 0, "%s: %d of %d hints lead nowhere, the first (key, hint): %s" % (
        name, len(bad), int((h != 0).sum()), [(int(designed_keys[i]), int(h[i])) for i in bad[:5]])
    return int((h != 0).sum())
