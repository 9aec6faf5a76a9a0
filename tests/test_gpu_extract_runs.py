"""The extract kernel's run bookkeeping (csrc/count_pipeline.h k_sk1w_extract: sk_break_bits, sk_start_bits, the tile-edge test) on
read sets made for it, on the GPU: runs of one minimizer many records long that begin on every lane offset, read boundaries on
every position of a lane and on both sides of the tile edges, batches that end with a window.  Every case goes through the
partitioned pipeline (MC_COUNT_PATH=partition, read at mc_create) once with a capacity hint -- compact records -- and once
without -- the two-array form --, at k = 31, 27 and 23 (windows of 17, 13 and 9 SK_M-mers), and its (key, count) pairs and its
window count are the CPU oracle's.  A wrong position inside a compact record would pass that -- it only slows the walk -- so the
hinted k = 31 case of the ragged reads also has its read pointers checked, as tests/test_gpu_read_pointers.py does at store
position 0."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import read_pointers as rp
from tests import seq_cov_model as sm
from tests.helpers import oracle_table, ragged_case
from tests.test_gpu_read_pointers import switches

gpu = pytest.mark.gpu

KS = (31, 27, 23)
TILE = 992  # the read sets are sized for a tile of 62 lanes x 16 positions as well; the kernel's tile is 496 = 62 x 8
COV = 3


def _join(reads):
    lens = [len(r) for r in reads]
    codes = np.concatenate(reads).astype(np.uint8) if sum(lens) else np.zeros(0, dtype=np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return codes, off


def long_runs():
    """poly-A, (AC)n, (ACG)n and a random 40-mer repeated, 150 .. 400 bases each -- every window of such a read has the same
    minimizer or one of a few, in runs of more than 48 windows --, each behind 0 .. 17 random bases and a multiple of 16 long: the run's first window falls on
    every lane offset and its cuts, every 16 windows, on every phase"""
    rng = np.random.default_rng(31)
    units = [np.array([0]), np.array([0, 1]), np.array([0, 1, 2]), rng.integers(0, 4, 40)]
    reads = []
    for u in units:
        for prefix in range(18):
            n = 16 * int(rng.integers(11, 26)) - prefix  # (159 .. 400; every read a multiple of 16 long, so the prefixes alone decide the offset)
            reads.append(np.concatenate([rng.integers(0, 4, prefix), np.tile(u, n // len(u) + 1)[:n]]))
    return _join(reads)


def ragged(k_all=KS):
    """reads of 0 .. 220 bases of a small genome, reads of k - 1 and k bases for every k among them: 700 reads, some 77 000 bases"""
    rng = np.random.default_rng(32)
    genome, codes, off = ragged_case(rng, 700)
    lens = np.diff(off).astype(np.int64)
    reads = [codes[int(a):int(a) + int(n)] for a, n in zip(off[:-1], lens)]
    for i, n in enumerate(x for k in k_all for x in (k - 1, k)):
        reads.insert(50 + 97 * i, genome[100 * i:100 * i + n])
    return _join(reads)


def one_long_read():
    return _join([np.random.default_rng(33).integers(0, 4, 5000)])


def one_window(k):
    return _join([np.random.default_rng(34).integers(0, 4, k)])


def ends_with_a_window(rem):
    """20 reads of 150 bases and a last one of 150 .. 181 that makes n_bases % 32 == rem: the batch's last window ends at its last base"""
    rng = np.random.default_rng(35 + rem)
    last = 150 + (rem - 21 * 150) % 32
    codes, off = _join([rng.integers(0, 4, 150) for _ in range(20)] + [rng.integers(0, 4, last)])
    assert len(codes) % 32 == rem
    return codes, off


SETS = {
    "runs": lambda k: long_runs(),
    "ragged": lambda k: ragged(),
    "long-read": lambda k: one_long_read(),
    "one-window": one_window,
    "tail0": lambda k: ends_with_a_window(0),
    "tail1": lambda k: ends_with_a_window(1),
    "tail31": lambda k: ends_with_a_window(31),
}


@functools.lru_cache(maxsize=None)
def case(name, k):
    """the reads of a set, packed, and what the oracle says of them at k"""
    codes, off = SETS[name](k)
    t, n = oracle_table(codes, off, k, po.KEY_PACKED)
    keys, counts = t.dump()
    return dict(codes=codes, off=off, words=po.pack(codes), windows=n, keys=keys, counts=counts)


def test_the_read_sets_are_what_the_cases_need():
    """No GPU.  Runs longer than 48 windows exist and begin on every position mod 16; the ragged reads span 6 tiles of 992
    positions, their boundaries fall on every position mod 16, next to both sides of the tile edges at multiples of 496, and reads of
    k - 1 and k bases are among them; the last window of the tail batches ends at the last base"""
    codes, off = long_runs()
    lens = np.diff(off).astype(np.int64)
    assert len(lens) == 72 and (lens % 16 == 0).all() and lens.min() >= 176 and lens.max() <= 400
    first = off[:-1].astype(np.int64) + np.tile(np.arange(18), 4)  # where the repeat begins
    assert all({int(x) % 16 for x in first[18 * u:18 * u + 18]} == set(range(16)) for u in range(4))
    poly_a = codes[int(first[0]):int(off[1])]
    assert len(poly_a) - 31 + 1 > 48 and not poly_a.any()
    codes, off = ragged()
    lens = np.diff(off).astype(np.int64)
    assert len(codes) >= 6 * TILE and {int(x) % 16 for x in off} == set(range(16))
    assert {0, 1} | {x for k in KS for x in (k - 1, k)} <= set(lens.tolist())
    edges = np.arange(496, len(codes), 496)
    nearest = np.abs(off.astype(np.int64)[None, :] - edges[:, None])
    assert (nearest.min(axis=1) <= 110).all()  # (a read ends within a read's length of every edge, so windows end on both sides of it)
    for d in (-1, 0, 1):  # ... and some boundaries sit right at, before and behind an edge
        assert np.isin(off.astype(np.int64) % 496, [d % 496]).any(), d
    for rem in (0, 1, 31):
        codes, off = ends_with_a_window(rem)
        assert len(codes) % 32 == rem and int(off[-1] - off[-2]) >= 150
    assert len(one_long_read()[0]) == 5000 and all(len(one_window(k)[0]) == k for k in KS)


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
    """the ragged reads at k = 31 with a capacity hint, at store position 0: every exported hint names a position where a window
    with that very key starts (below 2^31 a hint is exact), and every key with count >= the coverage hint has one"""
    import torch
    k = 31
    c = case("ragged", k)
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
    assert solid.sum() >= 1000 and (hints[solid] != 0).all(), "%d of %d solid keys without a hint" % (int((hints[solid] == 0).sum()), int(solid.sum()))
    some = np.nonzero(hints != 0)[0]
    lo, span = rp.ptr_range(hints[some])
    assert (span == 1).all() and (lo >= 0).all() and (lo < len(wk)).all()
    bad = some[~(valid[lo] & (wk[lo] == keys[some]))]
    assert len(bad) == 0, "%d of %d hints lead nowhere, the first: %s" % (len(bad), len(some), [(int(keys[i]), int(hints[i])) for i in bad[:5]])
