"""The extract kernel's tile of 62 lanes x 16 positions (csrc/count_pipeline.h k_sk1w_extract<false, ..>, NI = 16) on the smallest
read sets at which it can go wrong, on the GPU: read boundaries at, before and behind the tile edges at multiples of 992 and on
every position of a lane; runs of one minimizer longer than 48 windows that begin on every lane offset and cross a tile edge; a
tile with more than 128 record starts (three passes of the record loop); more than 64 read starts inside one tile's bitmap range
(a second round of the read-start scan); batches whose last window ends at the last base, 992 m + {-1, 0, 1, 30, 31} bases long.
Every case goes through the partitioned pipeline (MC_COUNT_PATH=partition) once with a capacity hint -- compact records -- and
once without -- the two-array form --, at k = 31, 27 and 23, and its (key, count) pairs and window count are the CPU oracle's.
The hinted k = 31 case of the boundary set also has its read pointers checked, as tests/test_gpu_read_pointers.py does at
store position 0: a wrong position inside a compact record would pass a count check."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import crowded_tables as ct
from tests import read_pointers as rp
from tests import seq_cov_model as sm
from tests.helpers import oracle_table
from tests.test_gpu_read_pointers import switches

gpu = pytest.mark.gpu

KS = (31, 27, 23)
TILE = 992  # 62 lanes x 16 positions
MAXW = 16   # SK_MAX_WINDOWS
COV = 3
TAILS = (-1, 0, 1, 30, 31)


def _fill(rng, genome, n):
    """reads of 150 bases and a shorter last one, n bases in all, each a stretch of the genome"""
    reads = []
    while n > 0:
        m = min(150, n)
        a = int(rng.integers(0, len(genome) - m + 1))
        reads.append(genome[a:a + m])
        n -= m
    return reads


def edge_reads():
    """Reads of a 1200-base genome over 8 tiles.  One boundary sits one base before the edge at 992, one on the edge at 2 x 992, one
    behind the edge at 3 x 992; all three sit around 4 x 992 (two reads of one base between them); reads cross the other edges.
    In between the reads are 40 .. 160 bases long, so the boundaries fall on every position of a lane."""
    rng = np.random.default_rng(61)
    genome = rng.integers(0, 4, 1200).astype(np.uint8)
    anchors = [0, TILE - 1, 2 * TILE, 3 * TILE + 1, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1, 8 * TILE + 100]
    cuts = []
    for a, b in zip(anchors[:-1], anchors[1:]):
        at = a
        while b - at > 200:  # (the last read in front of an anchor keeps 40 .. 200 bases)
            cuts.append(at)
            at += int(rng.integers(40, 161))
            for e in (5 * TILE, 6 * TILE, 7 * TILE):  # (no boundary next to these edges: a read crosses them with windows on both sides)
                if abs(at - e) < 35:
                    at = e + 35
        cuts.append(at)
    cuts.append(anchors[-1])
    reads = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        g = int(rng.integers(0, len(genome) - (b - a) + 1))
        reads.append(genome[g:g + b - a])
    return ct.store(reads)


def run_reads():
    """poly-A and (AC)n, 120 bases each (90 windows of 31 bases: more than 48), one a tile: the read begins 48 - p bases in front of a
    tile edge, p = 0 .. 15, so the run's first window falls on every lane offset and the run crosses the edge.  Random reads between."""
    rng = np.random.default_rng(62)
    genome = rng.integers(0, 4, 4000).astype(np.uint8)
    reads, at, m = [], 0, 1
    for unit in (np.array([0]), np.array([0, 1])):
        for p in range(16):
            start = m * TILE - 48 + p
            reads += _fill(rng, genome, start - at)
            reads.append(np.tile(unit, 120)[:120].astype(np.uint8))
            at = start + 120
            m += 1
    reads += _fill(rng, genome, 200)
    return ct.store(reads)


def dense_read():
    """one random read: at k = 23 (windows of 9 hashes) a record starts every 5 windows or so"""
    return ct.store([np.random.default_rng(63).integers(0, 4, 3000).astype(np.uint8)])


def short_reads():
    """ten reads of 150 bases, 200 reads of 0 .. 12 bases, ten reads of 150 bases"""
    rng = np.random.default_rng(64)
    genome = rng.integers(0, 4, 1500).astype(np.uint8)
    short = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(0, 13, 200)]
    return ct.store(_fill(rng, genome, 1500) + short + _fill(rng, genome, 1500))


def tail_reads(d):
    """reads of 150 bases and a last one of 150 .. 299, 2 x 992 + d bases in all: the batch's last window ends at its last base"""
    rng = np.random.default_rng(70 + d)
    total = 2 * TILE + d
    n_full = total // 150 - 1
    return ct.store([rng.integers(0, 4, 150).astype(np.uint8) for _ in range(n_full)] + [rng.integers(0, 4, total - 150 * n_full).astype(np.uint8)])


SETS = {"edges": edge_reads, "runs": run_reads, "dense": dense_read, "short": short_reads}
SETS.update({"tail%+d" % d: functools.partial(tail_reads, d) for d in TAILS})


def record_starts(codes, off, k):
    """The super-k-mer cut stated window by window, for every base position: (is a window, starts a record).  A window breaks the run
    when the position before it holds no window of the same read, their minimizers differ, or it is the first of a tile; a record
    starts at a break and every MAXW windows behind it."""
    off = np.asarray(off).astype(np.int64)
    n = len(codes)
    window = np.zeros(n, dtype=bool)
    hmin = np.zeros(n, dtype=np.uint64)
    for a, b in zip(off[:-1], off[1:]):
        if b - a >= k:
            _, lo = ct.pack_windows(codes[a:b], k)
            hmin[a:a + len(lo)] = ct.sk_hmin_of_kmer(lo, k)
            window[a:a + len(lo)] = True
    start = np.zeros(n, dtype=bool)
    cur = 0
    for p in np.nonzero(window)[0]:
        if p % TILE == 0 or not window[p - 1] or p in off or hmin[p - 1] != hmin[p]:
            cur = p
        start[p] = (p - cur) % MAXW == 0
    return window, start


@functools.lru_cache(maxsize=None)
def case(name, k):
    """the reads of a set, packed, and what the oracle says of them at k"""
    codes, off = SETS[name]()
    t, n = oracle_table(codes, off, k, po.KEY_PACKED)
    keys, counts = t.dump()
    return dict(codes=codes, off=off, words=po.pack(codes), windows=n, keys=keys, counts=counts)


def test_the_read_sets_are_what_the_cases_need():
    """No GPU: the properties the cases above are there for, asserted of the offsets that were generated."""
    # boundaries at, before and behind multiples of 992, on every position of a lane, about 8 tiles, reads across other edges
    codes, off = edge_reads()
    o = off.astype(np.int64)
    assert 8 * TILE <= len(codes) <= 8 * TILE + 250
    assert {TILE - 1, 2 * TILE, 3 * TILE + 1, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1} <= set(o.tolist())
    assert not {TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 3 * TILE - 1, 3 * TILE} & set(o.tolist())
    assert {int(x) % 16 for x in o} == set(range(16))
    for e in (5 * TILE, 6 * TILE, 7 * TILE):  # a read with windows on both sides of the edge
        r = int(np.searchsorted(o, e, side="right")) - 1
        assert o[r] + 31 <= e and o[r + 1] >= e + 31 and o[r] < e
    for k in KS:  # ... and the reads next to the boundaries at the edges hold windows
        window, _ = record_starts(codes, off, k)
        assert all(window[e - 40:e - 1].any() and window[e + 1:e + 40].any() for e in (TILE, 2 * TILE, 3 * TILE, 4 * TILE))
    # runs of more than 48 windows that begin on every lane offset and cross a tile edge
    codes, off = run_reads()
    o = off.astype(np.int64)
    lens = np.diff(o)
    runs = [r for r in range(len(lens)) if lens[r] == 120 and (codes[o[r]:o[r + 1]] <= 1).all() and len(set(codes[o[r]:o[r + 1]:2].tolist())) == 1]
    assert len(runs) == 32 and 120 - 31 + 1 > 48
    for half in (runs[:16], runs[16:]):
        assert {int(o[r]) % 16 for r in half} == set(range(16))
        assert all((o[r] // TILE + 1) * TILE - o[r] == 48 - o[r] % 16 for r in half)  # (windows begin on both sides of the edge)
    window, start = record_starts(codes, off, 31)
    r = runs[3]  # the cut: every 16 windows from the run's first, and again from the tile's first
    edge = (o[r] // TILE + 1) * TILE
    assert np.nonzero(start[o[r]:o[r] + 90])[0].tolist() == sorted(set(range(0, edge - o[r], 16)) | set(range(edge - o[r], 90, 16)))
    # more than 128 record starts in one tile at k = 23, more than 64 at every k
    codes, off = dense_read()
    window, start = record_starts(codes, off, 23)
    per_tile = np.add.reduceat(start.astype(np.int64), np.arange(0, len(codes), TILE))
    assert per_tile.max() > 128, per_tile
    assert all(np.add.reduceat(record_starts(codes, off, k)[1].astype(np.int64), np.arange(0, len(codes), TILE)).max() > 64 for k in KS)
    # more than 64 read starts inside one tile's bitmap range lo - 64 .. lo + 1088
    codes, off = short_reads()
    o = off.astype(np.int64)
    lens = np.diff(o)
    assert ((lens <= 12).sum() == 200) and (lens[10:210] <= 12).all() and (lens[:10] == 150).all() and 0 in lens and 12 in lens
    in_range = [int(((o[:-1] >= lo - 64) & (o[:-1] < lo + 1088)).sum()) for lo in range(0, len(codes), TILE)]
    assert max(in_range) > 128, in_range  # (three rounds of 64 lanes)
    # the tails
    for d in TAILS:
        codes, off = tail_reads(d)
        assert len(codes) == 2 * TILE + d and int(off[-1] - off[-2]) >= 150
    assert {(2 * TILE + d) % 32 for d in TAILS} >= {0, 1, 31}


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


@gpu
@pytest.mark.parametrize("hinted", [True, False], ids=["hint", "nohint"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SETS))
def test_pairs_and_windows_are_the_oracles(mc, name, k, hinted):
    c = case(name, k)
    with switches({"MC_COUNT_PATH": "partition"}):
        ctx = mc.Context(k, mc.KEY_PACKED, 0, max(int(len(c["keys"]) * 1.3), 64) if hinted else 0)
    with ctx:
        ctx.add_reads_packed(c["words"], c["off"])
        assert ctx.finalize() == len(c["keys"])
        assert ctx.stats().windows == c["windows"]
        gk, gc = ctx.export(0)
    assert np.array_equal(gk, c["keys"]) and np.array_equal(gc, c["counts"])


@gpu
def test_the_compact_records_carry_their_positions(mc):
    """the boundary set at k = 31 with a capacity hint, at store position 0: every exported hint names a position where a window
    with that very key starts (below 2^31 a hint is exact), and every key with count >= the coverage hint has one"""
    import torch
    k = 31
    c = case("edges", k)
    codes, off = c["codes"], c["off"].astype(np.int64)
    n_bases, n_reads, n_keys = len(codes), len(off) - 1, len(c["keys"])
    wk = sm.window_keys(codes, k, po.KEY_PACKED)
    read_end = np.repeat(off[1:], np.diff(off))  # the end of the read that holds each position
    valid = (np.arange(n_bases) + k <= read_end)[:len(wk)]
    assert int(valid.sum()) == c["windows"]
    dev = torch.device("cuda:0")
    d_words = torch.from_numpy(c["words"].view(np.int64)).to(dev)
    d_off = torch.from_numpy(off).to(dev)
    with switches({"MC_COUNT_PATH": "partition"}):
        ctx = mc.Context(k, mc.KEY_PACKED, 0, int(n_keys * 1.3))
    with ctx:
        ctx.set_coverage_hint(COV)
        ctx.read_store_seek(0, n_bases + 64)
        ctx.add_reads_packed_dev(d_words, d_off, n_reads, n_bases)
        assert ctx.finalize() == n_keys
        pk = torch.zeros(n_keys, dtype=torch.int64, device=dev)
        pc = torch.zeros(n_keys, dtype=torch.int16, device=dev)
        ph = torch.zeros(n_keys, dtype=torch.int32, device=dev)
        assert ctx.export_dev(0, pk, pc, n_keys, ph) == n_keys
    keys, counts, hints = pk.cpu().numpy(), pc.cpu().numpy(), ph.cpu().numpy().view(np.uint32).astype(np.int64)
    o = np.argsort(keys, kind="stable")
    keys, counts, hints = keys[o], counts[o], hints[o]
    assert np.array_equal(keys, c["keys"]) and np.array_equal(counts, c["counts"])
    solid = counts >= COV
    assert solid.sum() >= 300 and (hints[solid] != 0).all(), "%d of %d solid keys without a hint" % (int((hints[solid] == 0).sum()), int(solid.sum()))
    some = np.nonzero(hints != 0)[0]
    lo, span = rp.ptr_range(hints[some])
    assert (span == 1).all() and (lo >= 0).all() and (lo < len(wk)).all()
    bad = some[~(valid[lo] & (wk[lo] == keys[some]))]
    assert len(bad) == 0, "%d of %d hints lead nowhere, the first: %s" % (len(bad), len(some), [(int(keys[i]), int(hints[i])) for i in bad[:5]])
