"""The merge kernel of the counting pipeline (csrc/count_pipeline.h k_p3_dedup) on leaves composed record by record
(tests/dedup_leaves.py; tests/test_dedup_leaves_model.py checks without a GPU that every leaf meets the condition named here), so
that every path the kernel's comments call rare is taken by design, and the table, its read pointers and the kernel that ran are
checked behind each:

  leaf                  what the design's numbers make the kernel do
  quiet                 200 distinct records of 20 loci at different places, 1 .. 5 copies, every window count: one turn of the
                        record table, one round of units, pairs with and without a second window
  second-turn-1025/3000 more than 1024 records, 600 distinct: the records of a later turn join the entries of the first
  units-1976/1977/3953  exactly so many units: one round, two rounds, three rounds (D2_UL_CAP = 1976)
  no-place              1500 distinct records twice: 476 at least find no place among 1024 and go in through add_plain; three rounds and more
  twins                 the quiet leaf and two records with the same fingerprint and home place, 3 and 5 copies
  copies-4000/4096      one record of 16 windows 4000 times beside 96 others, and 4096 times alone: the 13-bit copy field
  counter bound         poly-A, 16 windows of one key, 3000 times (48 000, reads 32767), then 4096 times on top: 32767 + 65 536 in
                        the 17-bit packed counter
  hand-over-4096/4097   the dedup kernel takes the first, the general kernel queued behind it the second; and the leaf of 4096
                        under a leaf capacity of exactly 4096, where no general kernel is queued and the dedup kernel must take it
  crossings             30 records of 16 windows 40 times with a coverage hint of 5: every window crosses the threshold at once,
                        more crossings than a wave has read units, noted from the list's end down

Records form: the leaf's records and a background (super-k-mer records of random reads, those of the designed leaves dropped, repeated to
a mean of 2300 records a leaf so that the leaf capacity passes 4097) go in through add_superkmers_dev, into an empty table
(k_p3_dedup<1, ., .>) and as a second batch onto a table that holds every other record of the leaf once (<0, ., .>); with read
pointers on two records in three (ptr_tries 16: <., 0, 0>) and on all (PTRS_ON_EVERY_RECORD, ptr_tries 1: the ONE_GPU forms
<1, 1, 1> and <0, 1, 0>).  The expected table is the plain expansion of the records (dedup_leaves.table_of).  Reads form: the
records' bases as reads among random reads, MC_COUNT_PATH=partition, k = 31 (<1, 1, 1>) and k = 27, 23 (the generic shifts,
<1, 1, 0>), against the oracle's table.

MC_INGEST_DEBUG's line "[count] merge: ..." names the kernel, the leaf capacity and ptr_tries of every run; stats().spill_keys == 0
says that no record left the merge stage for the direct kernel."""
import functools
import math
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import crowded_tables as ct
from tests import dedup_leaves as dl
from tests import read_pointers as rp
from tests.helpers import oracle_table

gpu = pytest.mark.gpu

HINT = 800_000             # distinct keys the table is made for: 1024 regions, and more keys than any case counts
MEAN_LEAF = 2300           # records a leaf of the records form: cap2 = 1.15 m + 32 sqrt(m) + 64 >= 4243 > 4097
BG_READS, BG_LEN = 5000, 150
READS_BG, READS_MULT = 4200, 22   # reads form: 92 400 background reads, for which the host expects 1900 records a leaf and more
M32 = np.uint64(0xFFFFFFFF)
MERGE_LINE = re.compile(r"\[count\] merge: (k_p3_\w+(?:<[^>]*>)?) over (\d+) leaves, lcap (\d+), ptr_tries (\d+), general kernel behind it: (yes|no)")
RECORD_LEAVES = ["quiet", "second-turn-1025", "second-turn-3000", "units-1976", "units-1977", "units-3953", "no-place", "twins",
                 "copies-4000", "copies-4096", "hand-over-4096", "hand-over-4097", "crossings"]
READ_LEAVES = ["quiet", "second-turn-1025", "second-turn-3000", "units-1976", "units-1977", "units-3953", "no-place"]


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    for n in ("MC_COUNT_PATH", "MC_P3_DEDUP", "MC_SUPERKMERS", "MC_SK_COMPACT", "MC_SK_VLEAF"):
        monkeypatch.delenv(n, raising=False)
    monkeypatch.setenv("MC_INGEST_DEBUG", "1")


def cap2(n_records, n_leaves):
    """mcgpu.hip pipe_prepare: the capacity of a leaf's stream of super-k-mer records"""
    mean = float(n_records) / float(n_leaves)
    return int(mean * 1.15 + 32.0 * math.sqrt(mean) + 64.0)


@functools.lru_cache(maxsize=None)
def n_leaves(k):
    import metacherchant_amd as m
    with m.Context(k, po.KEY_PACKED, 0, HINT) as ctx:
        slots = int(ctx.stats().table_slots)
    assert slots % 4096 == 0 and slots // 4096 >= 1024  # (a second scatter level exists)
    return slots // 4096


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _export(ctx):
    """(keys ascending, counts, hints) of the whole table"""
    import torch
    n = ctx.export_count(0)
    dev = torch.device("cuda:0")
    pk = torch.zeros(n, dtype=torch.int64, device=dev)
    pc = torch.zeros(n, dtype=torch.int16, device=dev)
    ph = torch.zeros(n, dtype=torch.int32, device=dev)
    assert ctx.export_dev(0, pk, pc, n, ph) == n
    keys, counts, hints = pk.cpu().numpy(), pc.cpu().numpy().astype(np.int64), ph.cpu().numpy().view(np.uint32).astype(np.int64)
    o = np.argsort(keys, kind="stable")
    return keys[o], counts[o], hints[o]


def _merge_lines(capfd):
    return MERGE_LINE.findall(capfd.readouterr().err)


# ---------------------------------------------------------------------------------------------------- records form
class Background:
    """super-k-mer records of random reads (the extract kernel is not under test: its records' expansion is held against the oracle's
    table of the reads here), without those of the designed leaves, repeated and shuffled to MEAN_LEAF records a leaf"""

    def __init__(self, k):
        import metacherchant_amd as m
        import torch
        dev = torch.device("cuda:0")
        rng = np.random.default_rng(8100 + k)
        codes = rng.integers(0, 4, BG_READS * BG_LEN).astype(np.uint8)
        off = np.arange(BG_READS + 1, dtype=np.uint64) * BG_LEN
        n_windows = BG_READS * (BG_LEN - k + 1)
        with m.Context(k, po.KEY_PACKED, 0, 0) as sender:
            sender.set_read_pointers(sender.PTRS_STORE_ELSEWHERE | sender.PTRS_ON_EVERY_RECORD)
            cap = sender.superkmer_capacity(n_windows, BG_READS)
            d_recs = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
            d_ptrs = torch.zeros(cap, dtype=torch.int32, device=dev)
            n = int(sender.extract_superkmers_dev(_dev(po.pack(codes).view(np.int64)), _dev(off.view(np.int64)), BG_READS, BG_READS * BG_LEN, 1, d_recs, d_ptrs, cap)[1])
        recs = d_recs[:n].cpu().numpy().view(np.uint64)
        lo, hi, ptrs = recs[:, 0].copy(), recs[:, 1].copy(), d_ptrs[:n].cpu().numpy().view(np.uint32).copy()
        t, nw = oracle_table(codes, off, k, po.KEY_PACKED)
        keys, counts = dl.table_of(lo, hi, np.ones(n, dtype=np.int64), k)
        ok, oc = t.dump()
        assert nw == n_windows and np.array_equal(keys, ok) and np.array_equal(counts, oc) and (ptrs != 0).all()
        self.k, self.nl = k, n_leaves(k)
        leaf = ((lo & M32) * np.uint64(self.nl)) >> np.uint64(32)
        keep = (leaf != dl.leaf_of(dl.bin_of(ct.M_INTERIOR), self.nl)) & (leaf != 0)
        assert 0 < (~keep).sum() < n // 100
        self.lo, self.hi, self.ptrs = lo[keep], hi[keep], ptrs[keep]
        total = MEAN_LEAF * self.nl
        mult = -(-total // len(self.lo))
        self.inst = rng.permutation(np.tile(np.arange(len(self.lo)), mult))[:total]
        self.keys, self.rec, _ = dl.expand(self.lo, self.hi, k)
        self.d_recs = _dev(np.stack([self.lo[self.inst], self.hi[self.inst]], axis=1).view(np.int64))
        p = self.ptrs[self.inst]
        some = p.copy()
        some[np.arange(total) % 3 == 0] = 0
        self.d_ptrs = {"all": _dev(p.view(np.int32)), "some": _dev(some.view(np.int32))}
        self._tables = {}

    def table(self, nb):
        """what the first nb records of the background add"""
        if nb not in self._tables:
            copies = np.bincount(self.inst[:nb], minlength=len(self.lo))
            self._tables[nb] = dl.sum_tables((self.keys, copies[self.rec]))
        return self._tables[nb]


@functools.lru_cache(maxsize=None)
def background(k=31):
    return Background(k)


@functools.lru_cache(maxsize=None)
def region_keys(k):
    """the keys of 400 loci around the designed leaves' 15-mer: all of one region"""
    P = dl.pool_of(k, dl.N_LOCI_TWINS)
    return np.unique(dl.expand(P.lo, P.hi, k)[0])


def pointers_of(n, first, mode):
    """the read pointers of the n records of a batch: record i names store position 2^20 + 64 (first + i), so that no two records'
    windows share a pointer; one in forty lies in the last 16 exact positions (ptr_advance leaves the exact tier), one in forty in
    the 4-base tier (ptr_advance keeps the granule); mode "some": every third record carries none"""
    i = np.arange(n)
    pos = (1 << 20) + 64 * (first + i)
    pos = np.where(i % 40 == 7, rp.EXACT_END - 16 + (i // 40) % 16, pos)
    pos = np.where(i % 40 == 23, rp.T1_POS + 4096 + 64 * (first + i), pos)
    p = rp.ptr_encode(pos)
    if mode == "some":
        p = np.where(i % 3 == 0, 0, p)
    return p


def allowed_pairs(leaf, inst, ptrs):
    """every (key, pointer) a record of the batch may leave: window j of a copy with pointer p leaves ptr_advance(p, j) at its key"""
    keys, rec, win = dl.expand(leaf.lo, leaf.hi, leaf.k)
    keymat = np.zeros((leaf.distinct, dl.SK_MAX_WINDOWS), dtype=np.int64)
    keymat[rec, win] = keys
    has = np.nonzero(ptrs != 0)[0]
    nw = dl.windows_of(leaf.hi)[inst[has]]
    rows = np.repeat(has, nw)
    j = np.arange(len(rows)) - np.repeat(np.cumsum(nw) - nw, nw)
    return set(zip(keymat[inst[rows], j].tolist(), rp.ptr_advance(ptrs[rows], j).tolist()))


def count_records(mc, capfd, batches, mode, nb=None):
    """the leaves of `batches` one after the other into one table, each with the first nb records of the background.  mode: "some"
    (ptr_tries 16) or "all" (ptr_tries 1)"""
    import torch
    B = background(batches[0].k)
    nb = len(B.inst) if nb is None else nb
    out = {"nb": nb, "allowed": set(), "lines": []}
    capfd.readouterr()
    with mc.Context(batches[0].k, po.KEY_PACKED, 0, HINT) as ctx:
        if mode == "all":
            ctx.set_read_pointers(ctx.PTRS_OWN_STORE | ctx.PTRS_ON_EVERY_RECORD)
        if batches[-1].cov_hint:
            ctx.set_coverage_hint(batches[-1].cov_hint)
        first = 0
        for leaf in batches:
            inst = leaf.instances()
            ptrs = pointers_of(len(inst), first, mode)
            first += len(inst)
            out["allowed"] |= allowed_pairs(leaf, inst, ptrs)
            recs = np.stack([leaf.lo[inst], leaf.hi[inst]], axis=1).view(np.int64)
            d_recs = torch.cat([_dev(recs), B.d_recs[:nb]])
            d_ptrs = torch.cat([_dev(ptrs.astype(np.uint32).view(np.int32)), B.d_ptrs[mode][:nb]])
            ctx.add_superkmers_dev(d_recs, d_ptrs, len(inst) + nb)
            out["lines"] += _merge_lines(capfd)
        out["size"] = ctx.finalize()
        out["stats"] = ctx.stats()
        assert ctx.export_count(0) == out["size"]
        out["keys"], out["counts"], out["hints"] = _export(ctx)
        absent = np.setdiff1d(region_keys(batches[0].k), np.concatenate([b.keys for b in batches]))[:2000]  # keys of the leaf's own region that were never counted
        ask = np.concatenate([b.keys for b in batches] + [absent, np.array([1, (1 << 62) - 1, 0x123456789ABCDEF], dtype=np.int64)])
        out["asked"], out["got"] = ask, ctx.get(ask).astype(np.int64)
    return out


def check_records(R, batches, mode, name):
    """every assertion of the records form; returns the share of the designed keys with count >= 4 that have no hint"""
    B = background(batches[0].k)
    nb = R["nb"]
    # the debug line of every run
    assert len(R["lines"]) == len(batches), R["lines"]
    for i, (leaf, (kernel, leaves, lcap, tries, behind)) in enumerate(zip(batches, R["lines"])):
        one = 1 if mode == "all" else 0
        assert kernel == "k_p3_dedup<%d, %d, %d>" % (1 if i == 0 else 0, one, 1 if i == 0 and one and leaf.k == 31 else 0), (name, kernel)
        assert int(leaves) == B.nl and int(tries) == (1 if mode == "all" else 16)
        assert int(lcap) == cap2(leaf.records + nb, B.nl) >= leaf.records, (name, lcap, leaf.records)
        assert behind == ("yes" if int(lcap) > dl.DD_MAX_CAP else "no")
    assert R["stats"].spill_keys == 0, (name, int(R["stats"].spill_keys))
    # the table
    bgk, bgc = B.table(nb)
    keys, counts = dl.sum_tables((bgk, bgc * len(batches)), *[(b.keys, b.counts) for b in batches])
    counts = np.minimum(counts, 32767)
    assert R["size"] == len(keys) == len(R["keys"]), (name, R["size"], len(keys), len(R["keys"]))
    assert np.array_equal(R["keys"], keys), name
    wrong = np.nonzero(R["counts"] != counts)[0]
    assert len(wrong) == 0, "%s: %d of %d counts differ, the first (key, got, want): %s" % (
        name, len(wrong), len(keys), [(int(keys[i]), int(R["counts"][i]), int(counts[i])) for i in wrong[:5]])
    at = np.searchsorted(keys, R["asked"])
    want = np.where((at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == R["asked"]), counts[np.minimum(at, len(keys) - 1)], -1)
    assert np.array_equal(R["got"], want) and (want == -1).sum() >= 1000 and (want > 0).sum() >= 1  # (mc_get: -1 for an absent key)
    # the read pointers of the designed keys
    dk, dc = dl.sum_tables(*[(b.keys, b.counts) for b in batches])
    mine = np.searchsorted(keys, dk)
    hints = R["hints"][mine]
    bad = [(int(a), int(h)) for a, h in zip(dk[hints != 0].tolist(), hints[hints != 0].tolist()) if (a, h) not in R["allowed"]]
    assert not bad, "%s: %d of %d hints are no window's pointer, the first: %s" % (name, len(bad), int((hints != 0).sum()), bad[:5])
    solid = dc >= 4
    return int((hints[solid] == 0).sum()), int(solid.sum())


def _batches(name, second):
    leaf = dl.cases(31)[name]
    return [leaf.half(), leaf] if second else [leaf]


@gpu
@pytest.mark.parametrize("second", [False, True], ids=["first", "second"])
@pytest.mark.parametrize("mode", ["some", "all"])
@pytest.mark.parametrize("name", RECORD_LEAVES)
def test_records(mc, capfd, name, mode, second):
    """a designed leaf through add_superkmers_dev: the kernel named by the debug line, no record spilled, the table equal to the
    plain expansion in every (key, count), look-ups of counted and absent keys, and every hint of a designed key the pointer of one
    of its windows.  In the quiet leaf with a pointer on every record every key counted four times and more has a hint
    (kmer_device.h ptr_pick); elsewhere the share without one is printed (a note that finds no room in the list is a hint less)."""
    batches = _batches(name, second)
    R = count_records(mc, capfd, batches, mode)
    full_name = "%s/%s/%s" % (name, mode, "second" if second else "first")
    missing, solid = check_records(R, batches, mode, full_name)
    print("dedup leaves, hints: %s: %d of %d keys with count >= 4 have none" % (full_name, missing, solid))
    if name == "quiet" and mode == "all":
        assert solid >= 100 and missing == 0, (missing, solid)


@gpu
@pytest.mark.parametrize("mode", ["some", "all"])
def test_hand_over_at_a_leaf_capacity_of_4096(mc, capfd, mode):
    """the leaf of exactly DD_MAX_CAP records under a leaf capacity of exactly DD_MAX_CAP: the host queues no general kernel
    (lcap > DD_MAX_CAP is false), so the dedup kernel must take the leaf (n0 > DD_MAX_CAP is false too)"""
    leaf = dl.cases(31)["hand-over-4096"]
    B = background()
    nb = next(n for n in range(len(B.inst), 0, -B.nl // 4) if cap2(leaf.records + n, B.nl) == dl.DD_MAX_CAP)
    for second in (False, True):
        batches = [leaf.half(), leaf] if second else [leaf]
        R = count_records(mc, capfd, batches, mode, nb)
        assert R["lines"][-1][2:] == (str(dl.DD_MAX_CAP), "1" if mode == "all" else "16", "no")
        check_records(R, batches, mode, "hand-over-4096/lcap-4096/%s/%d" % (mode, second))


@gpu
@pytest.mark.parametrize("mode", ["some", "all"])
def test_counter_bound(mc, capfd, mode):
    """poly-A: 3000 records of 16 windows of the key 0 (48 000: reads 32767), then 4096 more on top of the clamped count:
    32767 + 65 536 = 98 303, the bound of the kernel's static_assert, in the 17 bits of the packed counter; reads 32767"""
    lo, hi = dl.poly_a()
    first = dl.Leaf("poly-a-3000", 31, lo, hi, [3000], 11, bin_word=0)
    again = dl.Leaf("poly-a-4096", 31, lo, hi, [dl.DD_MAX_CAP], 12, bin_word=0)
    assert first.max_count == 48000 and again.max_count == 65536 and again.max_copies == dl.DD_MAX_CAP
    for batches in ([first], [again], [first, again]):
        R = count_records(mc, capfd, batches, mode)
        check_records(R, batches, mode, "counter-bound/%s/%d" % (mode, len(batches)))
        assert R["keys"][0] == 0 and R["counts"][0] == 32767


# ---------------------------------------------------------------------------------------------------- reads form
class ReadsBackground:
    """random reads none of whose windows falls into the designed leaf, and the oracle's table of them"""

    def __init__(self, k):
        self.k, self.nl = k, n_leaves(k)
        rng = np.random.default_rng(8200 + k)
        reads = rng.integers(0, 4, (READS_BG + 200, BG_LEN)).astype(np.uint8)
        flat = reads.reshape(-1)
        _, lo = ct.pack_windows(flat, k)
        leaf = ct.region_of_bin(ct.sk_hmin_of_kmer(lo, k), self.nl)  # (windows astride two reads count for the first: a read too many dropped)
        bad = np.unique(np.nonzero(leaf == np.uint64(dl.leaf_of(dl.bin_of(ct.M_INTERIOR), self.nl)))[0] // BG_LEN)
        assert 0 < len(bad) <= 200
        self.reads = np.delete(reads, bad, axis=0)[:READS_BG]
        assert len(self.reads) == READS_BG
        t, _ = oracle_table(self.reads.reshape(-1), np.arange(READS_BG + 1, dtype=np.uint64) * BG_LEN, k, po.KEY_PACKED)
        self.keys, self.counts = t.dump()
        self.counts = self.counts.astype(np.int64)


@functools.lru_cache(maxsize=None)
def reads_background(k):
    return ReadsBackground(k)


def reads_batch(leaf, seed):
    """the leaf's records as reads (a record's own bases) shuffled among the background's reads, READS_MULT times each: (codes,
    offsets, and for the designed reads their offsets and the index of their record)"""
    B = reads_background(leaf.k)
    rng = np.random.default_rng(seed)
    inst = leaf.instances()
    n_bg = READS_BG * READS_MULT
    order = rng.permutation(n_bg + len(inst))  # order[i] < n_bg: a background read
    mine = np.nonzero(order >= n_bg)[0]
    rec = inst[order[mine] - n_bg]
    parts = [B.reads[i % READS_BG] if i < n_bg else leaf.bases[inst[i - n_bg]] for i in order.tolist()]
    off = np.zeros(len(order) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    codes = np.concatenate(parts).astype(np.uint8)
    return codes, off, off[mine].astype(np.int64), rec


@gpu
@pytest.mark.parametrize("second", [False, True], ids=["first", "second"])
@pytest.mark.parametrize("k,name", [(k, name) for k in (31, 27, 23) for name in READ_LEAVES if name in dl.cases(k)])
def test_reads(mc, capfd, monkeypatch, k, name, second):
    """the ONE_GPU forms: a designed leaf as reads, one record's bases a read, through the partitioned pipeline; the table against the
    oracle's, and no pointer of a designed key that leads nowhere"""
    monkeypatch.setenv("MC_COUNT_PATH", "partition")
    leaf = dl.cases(k)[name]
    batches = [leaf.half(), leaf] if second else [leaf]
    B = reads_background(k)
    tables, lines, at, wk = [], [], [], []
    capfd.readouterr()
    with mc.Context(k, po.KEY_PACKED, 0, HINT) as ctx:
        for n, b in enumerate(batches):
            codes, off, mine, rec = reads_batch(b, 8300 + n)
            t, _ = oracle_table(np.concatenate([b.bases[r] for r in range(b.distinct)]), np.concatenate([[0], np.cumsum([len(x) for x in b.bases])]).astype(np.uint64), k, po.KEY_PACKED)
            dk, dc = t.dump()
            assert np.array_equal(dk, b.keys)  # (one copy of every distinct record: the keys; the counts are table_of's)
            tables += [(b.keys, b.counts), (B.keys, B.counts * READS_MULT)]
            at.append(ctx.read_store_tell())
            ctx.add_reads_packed_dev(_dev(po.pack(codes).view(np.int64)), _dev(off.view(np.int64)), len(off) - 1, len(codes))
            lines += _merge_lines(capfd)
            # the key of every window of the designed reads at its place in the store (elsewhere: no key)
            keys, r_, w_ = dl.expand(b.lo, b.hi, k)
            km = np.full((b.distinct, dl.SK_MAX_WINDOWS), -1, dtype=np.int64)
            km[r_, w_] = keys
            w = np.full(len(codes), -1, dtype=np.int64)
            pos = (mine[:, None] + np.arange(dl.SK_MAX_WINDOWS)[None, :])
            ok = km[rec] >= 0
            w[pos[ok]] = km[rec][ok]
            wk.append(w)
        size = ctx.finalize()
        stats = ctx.stats()
        got_keys, got_counts, got_hints = _export(ctx)
        ask = np.concatenate([leaf.keys, np.array([1, (1 << 62) - 1], dtype=np.int64)])
        got = ctx.get(ask).astype(np.int64)
    assert len(lines) == len(batches), lines
    for i, (kernel, leaves, lcap, tries, behind) in enumerate(lines):
        assert kernel == "k_p3_dedup<%d, 1, %d>" % (1 if i == 0 else 0, 1 if i == 0 and k == 31 else 0), kernel
        assert int(leaves) == B.nl and int(tries) == 1 and int(lcap) >= 1.1 * batches[i].records
    assert stats.spill_keys == 0
    keys, counts = dl.sum_tables(*tables)
    counts = np.minimum(counts, 32767)
    assert size == len(keys) == len(got_keys) and np.array_equal(got_keys, keys)
    wrong = np.nonzero(got_counts != counts)[0]
    assert len(wrong) == 0, "%d of %d counts differ, the first (key, got, want): %s" % (
        len(wrong), len(keys), [(int(keys[i]), int(got_counts[i]), int(counts[i])) for i in wrong[:5]])
    assert np.array_equal(got[:len(leaf.keys)], counts[np.searchsorted(keys, leaf.keys)]) and (got[len(leaf.keys):] == -1).all()
    # pointers: the batches lie one behind the other in the store, each from a word boundary
    assert at[0] == 0
    total = at[-1] + len(wk[-1])
    allw = np.full(total, -1, dtype=np.int64)
    for a, w in zip(at, wk):
        allw[a:a + len(w)] = w
    dk, dc = dl.sum_tables(*[(b.keys, b.counts) for b in batches])
    hints = got_hints[np.searchsorted(keys, dk)]
    bad = rp.not_found(dk, hints, 0, allw, allw >= 0, total)
    assert len(bad) == 0, "%d of %d hints lead nowhere, the first (key, hint): %s" % (
        len(bad), int((hints != 0).sum()), [(int(dk[i]), int(hints[i])) for i in bad[:5]])
    solid = dc >= 4
    print("dedup leaves, hints: reads/k%d/%s/%s: %d of %d keys with count >= 4 have none" % (
        k, name, "second" if second else "first", int((hints[solid] == 0).sum()), int(solid.sum())))
