"""Designed inputs for the walk (csrc/bfs_device.h), test infrastructure only: reads and seeds whose de Bruijn graph has a frontier of
a chosen width at a chosen level, so that k_bfs's decisions at a level boundary -- narrow or wide (le - lb <= flim), speculate or replay,
the 512-candidate chunks of bfs_chunk_wide, the seed chunks, the buckets of the visited index -- are met by design and not by luck.

Codes are the oracle's: A0 G1 C2 T3.  A builder returns a Case: seed sequences, reads, and `facts`, what the case claims about itself.
The widths a case claims are no model of the BFS: they are counts of distinct windows at one offset of the reads (a vertex of level j
is a window j bases behind the seed's), and tests/test_walk_shapes_model.py holds them against the histogram of the oracle's distances
(oracle/pyoracle.py bfs, the restatement of OneSequenceCalculator).  The table counts canonical k-mers, so the same reads serve a walk to
the left: its seeds are the reverse complements (Case.seeds_for), its graph the mirror image, its widths the same.

vis_hash / fmix64 / fmix64_inv restate kmer_hash.h and bfs_device.h in Python integers; the model test pins fmix64 to what
`mc_hosttest placement` prints from the header."""
import itertools
from collections import Counter

import numpy as np

M64 = (1 << 64) - 1
NARROW_CAND = 64      # bfs_device.h: candidates of a replayed level; flim = NARROW_CAND / nb
SCOUT_MAX_F = 8       # walkers that get a scout
CHUNK = 512           # BFS_THREADS: candidates (or seed windows) of one wide chunk
GOLDEN = 0x9e3779b97f4a7c15


def nb_of(direction):
    return 8 if direction == 0 else 4


def flim_of(direction):
    return NARROW_CAND // nb_of(direction)


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[::-1]).astype(np.uint8)


def kmer_int(codes):
    v = 0
    for c in codes:
        v = (v << 2) | int(c)
    return v


def kmer_codes(v, k):
    return np.array([(v >> (2 * (k - 1 - i))) & 3 for i in range(k)], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- the visited index's hash
def fmix64(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


_INV1, _INV2 = pow(0xff51afd7ed558ccd, -1, 1 << 64), pow(0xc4ceb9fe1a85ec53, -1, 1 << 64)


def fmix64_inv(y):
    """x ^= x >> 33 is its own inverse on 64 bits (the second application shifts by 66)"""
    y &= M64
    y ^= y >> 33
    y = (y * _INV2) & M64
    y ^= y >> 33
    y = (y * _INV1) & M64
    y ^= y >> 33
    return y


def vis_salt(hi):
    return fmix64(GOLDEN) if hi == 0 else fmix64(hi + GOLDEN)


def vis_hash(v):
    """bfs_device.h vis_hash of the k-mer v (hi = v >> 64, lo = the low word)"""
    return fmix64((v & M64) ^ vis_salt(v >> 64))


# ---------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, k, seeds, reads, min_cov, facts):
        self.name, self.k, self.min_cov, self.facts = name, k, min_cov, facts
        self.seeds = [np.asarray(s, dtype=np.uint8) for s in seeds]
        self.reads = [np.asarray(r, dtype=np.uint8) for r in reads]

    def seeds_for(self, direction):
        """the seeds of a walk in `direction`: to the left the mirror image (the reverse complements) is walked"""
        return [revcomp(s) for s in self.seeds] if direction == -1 else self.seeds

    def widths(self, direction):
        w = self.facts["widths"]
        return list(w[0 if direction == 0 and 0 in w else 1])

    @property
    def n_seed_windows(self):
        return sum(max(len(s) - self.k + 1, 0) for s in self.seeds)

    def store(self):
        """(codes, offsets) of the reads, as the counting calls take them"""
        off = np.zeros(len(self.reads) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in self.reads])
        return np.concatenate(self.reads).astype(np.uint8), off


def offset_widths(placed, k, min_cov):
    """placed: (offset, codes, copies) with the seed's first base at offset 0.  The number of distinct windows at every offset that
    min_cov copies and more hold, up to the first offset with none"""
    out = []
    for j in itertools.count():
        c = Counter()
        for at, codes, copies in placed:
            if at <= j and j + k <= at + len(codes):
                c[bytes(codes[j - at:j - at + k])] += copies
        w = sum(1 for n in c.values() if n >= min_cov)
        if w == 0:
            return out
        out.append(w)


def words_of(d, m):
    return [np.array(w, dtype=np.uint8) for w in itertools.islice(itertools.product(range(4), repeat=d), m)]


def _build(name, k, S, placed, min_cov, **facts):
    widths = offset_widths(placed, k, min_cov)
    reads = [codes for _, codes, copies in placed for _ in range(copies)]
    facts.update(widths={1: widths}, n=sum(widths))
    return Case(name, k, [S], reads, min_cov, facts)


def fan(rng, k, d, m, tail, cov=1, weak=(), name=None):
    """reads S + w + Y for the first m words w of d bases: m vertices at level d, kept until the words leave the window and the
    vertices with equal rests of a word merge.  weak: indices of words with one copy too few"""
    S, Y = rng.integers(0, 4, k).astype(np.uint8), rng.integers(0, 4, tail).astype(np.uint8)
    placed = [(0, np.concatenate([S, w, Y]), cov - 1 if i in weak else cov) for i, w in enumerate(words_of(d, m))]
    return _build(name or "fan-%d" % m, k, S, placed, cov, d=d, m=m, weak=tuple(weak))


def ragged_fan(rng, k, d, m, lengths, name="ragged"):
    """the fan with a tail of its own and a length of its own for every word: walker i ends at level d + lengths[i], no two merge"""
    S = rng.integers(0, 4, k).astype(np.uint8)
    placed = [(0, np.concatenate([S, w, rng.integers(0, 4, n).astype(np.uint8)]), 1) for w, n in zip(words_of(d, m), lengths)]
    return _build(name, k, S, placed, 1, d=d, m=m, dies=sorted(d + n for n in lengths))


def branch_off(rng, k, p, cov_main=3, cov_side=2, tail=200, side=40, name=None):
    """one path S + Y and a side read that leaves it behind base p of Y: one walker until level p, two from level p + 1 on for
    `side` levels"""
    S, Y, Z = (rng.integers(0, 4, n).astype(np.uint8) for n in (k, tail, side))
    Z[0] = (Y[p] + 1 + Z[0] % 3) % 4
    path = np.concatenate([S, Y])
    placed = [(0, path, cov_main), (p, np.concatenate([path[p:p + k], Z]), cov_side)]
    return _build(name or "branch-%d" % p, k, S, placed, min(cov_main, cov_side), p=p, side=side)


def cycle(rng, k, period, name=None):
    """S + Y + S + Y[:k], len(S + Y) = period: the path comes back to the seed after `period` vertices"""
    S, Y = rng.integers(0, 4, k).astype(np.uint8), rng.integers(0, 4, period - k).astype(np.uint8)
    read = np.concatenate([S, Y, S, Y[:k]])
    both = [1] + [2] * ((period - 1) // 2) + [1] * ((period - 1) % 2)  # (both ways round at once)
    return Case(name or "cycle-%d" % period, k, [S], [read], 1, dict(widths={1: [1] * period, 0: both}, n=period, period=period))


SEED_KINDS = ("dup_in_chunk", "dup_across_chunks", "dup_narrow", "exact_chunk", "exact_chunk_plus", "none_solid_first_chunk")
PATH_WINDOWS, SEED_AT = 1000, 120   # the random path of the seeds cases, and its first window that is a seed


def seeds_case(rng, k, kind):
    """seed sequences over a plain random path G, every k-mer of G twice and more in the reads"""
    G = rng.integers(0, 4, PATH_WINDOWS + k - 1).astype(np.uint8)
    reads = [G[i:i + 200] for i in range(0, len(G) - 200, 100)] + [G[-200:]]
    seg = lambda n: G[SEED_AT:SEED_AT + n + k - 1]  # noqa: E731  (n windows from window SEED_AT on)

    def then(first, n):
        """`first`, one base that continues neither it nor the path in front of window SEED_AT, and the piece of n windows: the
        k windows astride the two are in no read"""
        cont = G[SEED_AT + len(first)] if len(first) < len(G) - SEED_AT else 4
        sep = next(b for b in range(4) if b != cont and b != G[SEED_AT - 1])
        return np.concatenate([first, [sep], seg(n)]).astype(np.uint8)

    if kind == "dup_in_chunk":
        seed, first, dups = then(seg(100), 100), 100, list(range(100, 200))
    elif kind == "dup_across_chunks":
        seed, first, dups = then(seg(700), 100), 700, list(range(700, 800))
    elif kind == "dup_narrow":
        seed, first, dups = then(seg(3), 3), 3, [3, 4, 5]
    elif kind == "exact_chunk":
        seed, first, dups = seg(CHUNK), CHUNK, []
    elif kind == "exact_chunk_plus":
        seed, first, dups = seg(CHUNK + 1), CHUNK + 1, []
    elif kind == "none_solid_first_chunk":
        seed, first, dups = then(rng.integers(0, 4, 600 + k - 1).astype(np.uint8), 50), 50, []
    else:
        raise ValueError(kind)
    after, before = PATH_WINDOWS - SEED_AT - first, SEED_AT
    widths = {1: [first] + [1] * after, 0: [first] + [2] * min(after, before) + [1] * abs(after - before)}
    facts = dict(widths=widths, n=first + after, distinct=first, dup_queue_positions=dups,
                 dup_window=(len(seed) - k + 1 - len(dups)) if dups else None)
    return Case("seeds-" + kind, k, [seed], reads + reads, 2, facts)


def vis_collide(rng, k, n_fill, wide=False):
    """v1, its right neighbour v2, and n_fill k-mers u_j with vis_hash(u_j) == vis_hash(v2) ^ (j << 24): the fingerprint (the high
    32 bits) and the home bucket (the low bits, in every index of up to 2^24 buckets) of v2.  The seeds are u_1 .. u_n_fill, then
    v1; with `wide`, 20 unrelated solid seeds more, so that level 0 is expanded by bfs_chunk_wide (vis_find)."""
    mask = (1 << (2 * k)) - 1
    v1 = kmer_int(rng.integers(0, 4, k))
    b = int(rng.integers(0, 4))
    v2 = ((v1 << 2) | b) & mask
    hi = v2 >> 64
    us = [(hi << 64) | (fmix64_inv(vis_hash(v2) ^ (j << 24)) ^ vis_salt(hi)) for j in range(1, n_fill + 1)]
    assert all(u <= mask for u in us)
    reads = [kmer_codes(u, k) for u in us] + [np.concatenate([kmer_codes(v1, k), [b]]).astype(np.uint8)]
    seeds = [kmer_codes(u, k) for u in us] + [kmer_codes(v1, k)]
    if wide:
        extra = [rng.integers(0, 4, k).astype(np.uint8) for _ in range(20)]
        reads, seeds = reads + extra, seeds + extra
    return Case("collide-%d%s" % (n_fill, "-wide" if wide else ""), k, seeds, reads, 1,
                dict(widths={1: [len(seeds), 1]}, n=len(seeds) + 1, v1=v1, v2=v2, us=us))


# ---------------------------------------------------------------------------------------------------- reading an oracle walk
def kmers_of(res):
    return [(int(h) << 64) | int(lo) for h, lo in zip(res["hi"], res["lo"])]


def histogram(res):
    return np.bincount(res["dist"]).tolist()


def parents_of(res, k, direction, level):
    """for every vertex of `level`, in order: the places, inside level - 1 in its order, of every vertex it is a neighbour of.  (Not
    the walk: one shift and compare on the result.)  The smallest is the parent that inserted it; a chunk holds CHUNK / nb parents."""
    low = (1 << (2 * (k - 1))) - 1
    v = kmers_of(res)
    dist = np.asarray(res["dist"])
    prev, cur = np.nonzero(dist == level - 1)[0], np.nonzero(dist == level)[0]
    right, left = {}, {}
    for place, i in enumerate(prev.tolist()):
        right.setdefault(v[i] & low, []).append(place)   # its right neighbours begin with its last k - 1 bases
        left.setdefault(v[i] >> 2, []).append(place)     # its left neighbours end with its first k - 1
    out = []
    for i in cur.tolist():
        p = []
        if direction >= 0:
            p += right.get(v[i] >> 2, [])
        if direction <= 0:
            p += left.get(v[i] & low, [])
        out.append(sorted(p))
    return out


def first_chunk_accepts(res, k, direction, level):
    """how many vertices of level + 1 the first chunk of level's expansion inserts"""
    per = CHUNK // nb_of(direction)
    return sum(1 for p in parents_of(res, k, direction, level + 1) if p[0] < per)


def chunks_expected(n_seed_windows, widths, direction):
    """chunks_wide of a walk as k_bfs counts it: the seed chunks, and ceil(W nb / 512) for every level wider than flim"""
    nb, flim = nb_of(direction), flim_of(direction)
    return -(-n_seed_windows // CHUNK) + sum(-(-w * nb // CHUNK) for w in widths if w > flim)


# ---------------------------------------------------------------------------------------------------- the cases of the tests
FAN_TABLE = [  # (d, m, directions, the first widths), k = 21, tail 70
    (4, 256, (1, 0), [1, 4, 16, 64, 256]),
    (4, 128, (1,), [1, 2, 8, 32, 128]),
    (4, 129, (1,), [1, 3, 9, 33, 129]),
    (3, 16, (1,), [1, 1, 4, 16]),
    (3, 17, (1,), [1, 2, 5, 17]),
    (2, 8, (1, 0), [1, 2, 8]),
    (3, 9, (1, 0), [1, 1, 3, 9]),
    (3, 64, (0,), [1, 4, 16, 64]),
    (4, 65, (0,), [1, 2, 5, 17, 65]),
]
TAIL = 70
RAGGED_LENGTHS = (20, 64, 65, 100, 130, 150)   # d = 2, six walkers: one ends inside the first predicted stretch, one 64 levels behind
                                               # the fan-out, one a level later
BRANCH_P = (20, 64, 65, 128, 129)
WEAK = (5, 77, 200)


def fans(k, seed=0):
    rng = np.random.default_rng(9000 + 100 * k + seed)
    return [fan(rng, k, d, m, TAIL) for d, m, _, _ in FAN_TABLE]


def fan_directions(m):
    return next(dirs for _, mm, dirs, _ in FAN_TABLE if mm == m)


def others(k):
    rng = np.random.default_rng(9100 + k)
    out = [fan(rng, k, 4, 256, TAIL, cov=3, weak=WEAK, name="fan-256-weak"), ragged_fan(rng, k, 2, 6, RAGGED_LENGTHS)]
    out += [branch_off(rng, k, p) for p in BRANCH_P]
    out += [cycle(rng, k, 150), cycle(rng, k, k + 9)]
    out += [seeds_case(rng, k, kind) for kind in SEED_KINDS]
    return out


def collisions(k):
    rng = np.random.default_rng(9200 + k)
    return [vis_collide(rng, k, n, wide) for n in (1, 2, 3) for wide in (False, True)]
