"""Tables for the .kmers.bin tests (tests/test_gpu_kmers_bin*.py): the dense ones -- the reads of synth_case(1, 30000, 4000, 150, 80)
counted at k = 25 packed and k = 40 poly, the latter through the partitioned pipeline with a capacity hint (long records: regions
are minimizer bins, the key join runs) -- with their oracle tables, made once a process; and the designed ones."""
import functools
import os

import numpy as np

from oracle import pyoracle as po
from tests.helpers import oracle_table, synth_case

DENSE = [(25, po.KEY_PACKED), (40, po.KEY_POLY)]
DESIGNED_COUNTS = [1, 2, 255, 256, 257, 32766, 32767]


@functools.lru_cache(maxsize=None)
def dense_case(k, mode):
    """(genome, codes, offsets, oracle table, its keys sorted, their counts)"""
    genome, codes, off = synth_case(1, 30000, 4000, 150, 80)
    t, _ = oracle_table(codes, off, k, mode)
    ok, oc = t.dump()
    return genome, codes, off, t, ok, oc


def dense_context(m, k, mode):
    """a finalized context that counted the dense case's reads (the caller closes it)"""
    _, codes, off, t, _, _ = dense_case(k, mode)
    old = os.environ.get("MC_COUNT_PATH")
    if mode == po.KEY_POLY:
        os.environ["MC_COUNT_PATH"] = "partition"
    try:
        ctx = m.Context(k, mode, 0, int(t.size() * 1.3))
    finally:
        if mode == po.KEY_POLY:
            if old is None:
                del os.environ["MC_COUNT_PATH"]
            else:
                os.environ["MC_COUNT_PATH"] = old
    ctx.add_reads_packed(po.pack(codes), off)
    assert ctx.finalize() == t.size()
    return ctx


def designed_pairs(n, k, mode):
    """n distinct keys -- 0 and 0x0102030405060708 first, in the hash mode then two with the top bit set (never -1, the table's
    free-slot mark), seeded random ones behind -- and the (key, count) pairs to add: the first key twice with 32767, the next ones with
    DESIGNED_COUNTS in turn, the rest mostly with 1 and 2.  Returns (keys int64, counts int16 as added, what the table must read: sorted keys,
    their values)."""
    rng = np.random.default_rng(1000 * k + n)
    special = [0, 0x0102030405060708]
    if mode != po.KEY_PACKED:
        special += [-(1 << 63), -2]
    if mode == po.KEY_PACKED:
        pool = rng.integers(1, 1 << (2 * k), 2 * n + 8, dtype=np.int64)
    else:
        pool = rng.integers(-(1 << 63), (1 << 63) - 1, 2 * n + 8, dtype=np.int64)  # (the high end is exclusive: no -1 + 2^64 either way)
    pool = pool[(pool != -1) & ~np.isin(pool, special)]
    keys = np.concatenate([np.array(special, dtype=np.int64), np.unique(pool)])[:n]
    assert len(np.unique(keys)) == n
    counts = np.array([32767 if i == 0 else DESIGNED_COUNTS[i - 1] if i <= len(DESIGNED_COUNTS) else
                       (1 if rng.random() < 0.7 else 2 if rng.random() < 0.7 else int(rng.integers(3, 1500))) for i in range(n)], dtype=np.int16)
    add_k = np.concatenate([keys, keys[:1]])  # (2 x 32767 reads 32767)
    add_c = np.concatenate([counts, counts[:1]])
    o = np.argsort(keys, kind="stable")
    return add_k, add_c, keys[o], counts[o]


def designed_context(m, n, k, mode):
    """(a finalized context filled through add_pairs_dev, sorted keys, their values)"""
    import torch
    add_k, add_c, keys, values = designed_pairs(n, k, mode)
    ctx = m.Context(k, mode, 0, 0)
    if len(add_k):
        dk = torch.from_numpy(add_k.copy()).to("cuda:0")
        dc = torch.from_numpy(add_c.copy()).to("cuda:0")
        ctx.add_pairs_dev(dk, dc, len(add_k))
    assert ctx.finalize() == n
    return ctx, keys, values
