"""Designed components for mc_walk_order (tests/test_walk_order_model.py, tests/test_gpu_walk_order.py): lists of k-mer strings, the
seed first, as tests/walk_order_model.py takes them, and their packed form as the library takes them."""
import itertools

import numpy as np

from tests import walk_order_model as wm

_CODE = {"A": 0, "G": 1, "C": 2, "T": 3}


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def windows(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def members_of(reads, k, connected=True):
    """The distinct k-mers of the reads, each as its first window spells it (what mc_components gives); the first read's first window
    is the seed.  connected: only what hangs together with the seed, else everything."""
    seen, members = set(), []
    for r in reads:
        for w in windows(r, k):
            if w not in seen:
                seen.add(w)
                seen.add(wm.rc(w))
                members.append(w)
    if not connected:
        return members
    at = {}
    for i, m in enumerate(members):
        at[m] = i
        at[wm.rc(m)] = i
    reach, stack = {0}, [members[0]]
    while stack:
        x = stack.pop()
        for y in wm.neighbours(x):
            t = at.get(y)
            if t is not None and t not in reach:
                reach.add(t)
                stack.append(members[t])
    return [m for i, m in enumerate(members) if i in reach]


def _distinct(kmers):
    both = set(kmers) | {wm.rc(x) for x in kmers}
    return len(both) == 2 * len(kmers) - sum(1 for x in kmers if wm.rc(x) == x) and len(set(kmers)) == len(kmers)


def chain(rng, k, n, seed_at=0):
    """n k-mers in a row, the seed at place seed_at"""
    while True:
        ws = windows(rand_seq(rng, n + k - 1), k)
        if _distinct(ws):
            return [ws[seed_at]] + ws[:seed_at] + ws[seed_at + 1:]


def cycle(rng, k, n):
    """n k-mers around a circular sequence of n bases: the two fronts meet opposite the seed"""
    while True:
        s = rand_seq(rng, n)
        ws = windows((s * (k // n + 2))[:n + k - 1], k)
        if _distinct(ws):
            return ws


def bubble_reads(rng, k, n_bubbles, gap=None, seed_end=True):
    """a genome and its copy with n_bubbles substitutions, gap bases apart: equal arms of k k-mers each, in series"""
    gap = gap or k + 9
    while True:
        g = rand_seq(rng, gap * (n_bubbles + 1) + k)
        v = list(g)
        for b in range(n_bubbles):
            at = gap * (b + 1)
            v[at] = "ACGT"[("ACGT".index(v[at]) + 1 + int(rng.integers(0, 3))) % 4]
        reads = [g, "".join(v)]
        if not seed_end:
            reads = [g[len(g) // 2:], g, "".join(v)]
        members = members_of(reads, k)
        if len(members) == len(members_of(reads, k, connected=False)) and len(members) == len(g) - k + 1 + n_bubbles * k:
            return reads


def bubbles(rng, k, n_bubbles, gap=None, seed_end=True):
    """the k-mers of bubble_reads, seeded at the genome's end or in its middle"""
    return members_of(bubble_reads(rng, k, n_bubbles, gap, seed_end), k)


def unequal_bubble_and_tip(rng, k):
    """a deletion (arms of k - 1 and k k-mers) and a dead side arm of six k-mers"""
    while True:
        g = rand_seq(rng, 5 * k)
        cut = 2 * k
        tip = g[3 * k:4 * k - 1] + rand_seq(rng, 6)
        reads = [g, g[:cut] + g[cut + 1:], tip]
        members = members_of(reads, k)
        if len(members) == len(members_of(reads, k, connected=False)):
            return members


def complete(k, seed=None):
    """every k-mer there is: the widest levels, pushes by many entries at once, self and reverse-complement edges"""
    every = ["".join(p) for p in itertools.product("AGCT", repeat=k)]
    seed = seed or ("AGCTTCGA" * 8)[:k]
    return members_of([seed] + every, k)


def random_reads(rng, k, genome=20000, n_reads=4000, length=100):
    """reads of a random genome, half of them with one substitution (the first one, which holds the seed, has none: at k > length / 2
    its error would be in every window and cut it off), a third reverse-complemented"""
    g = rand_seq(rng, genome)
    reads = []
    for i in range(n_reads):
        a = int(rng.integers(0, genome - length))
        r = list(g[a:a + length])
        if i and rng.random() < 0.5:
            r[int(rng.integers(0, length))] = "ACGT"[int(rng.integers(0, 4))]
        r = "".join(r)
        reads.append(wm.rc(r) if rng.random() < 1 / 3 else r)
    return reads


def pack(members, k, rng=None):
    """(hi, lo): A0 G1 C2 T3, the first base most significant; rng: random bits above the k-mer"""
    hi, lo = np.zeros(len(members), dtype=np.uint64), np.zeros(len(members), dtype=np.uint64)
    for i, m in enumerate(members):
        v = 0
        for ch in m:
            v = (v << 2) | _CODE[ch]
        if rng is not None:
            v |= int(rng.integers(0, 1 << 62)) << (2 * k) & ((1 << 128) - 1)
        hi[i], lo[i] = v >> 64, v & ((1 << 64) - 1)
    return hi, lo
