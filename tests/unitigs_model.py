"""Unitig compaction at string level (no GPU, no library): the reference's initializeStructures + doMerge
(src/algo/OneSequenceCalculator.java:387-451) restated literally -- lists, passes and merges as the reference does them -- and the
link analysis that include/mcgpu.h mc_unitigs defines, which must leave the same nodes.

Entry e (an oriented k-mer string) makes node 2e (the string) and node 2e + 1 (its reverse complement).  A node is a dict
{seq, deleted, rc, nbrs}.  What a deleted node keeps as seq and rc depends on the loop's scan order and is never read: state()
leaves both out."""
import itertools
import random

import numpy as np

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CODE = {"A": 0, "G": 1, "C": 2, "T": 3}


def rc(s):
    return "".join(_COMP[c] for c in reversed(s))


def init_nodes(kmers, k):
    """initializeStructures: nbrs(p) = the nodes whose (k-1)-prefix is the (k-1)-suffix of node p ^ 1, in node order"""
    nodes = []
    for s in kmers:
        assert len(s) == k
        nodes.append({"seq": s, "deleted": False, "rc": len(nodes) + 1, "nbrs": []})
        nodes.append({"seq": rc(s), "deleted": False, "rc": len(nodes) - 1, "nbrs": []})
    by_prefix = {}
    for i, nd in enumerate(nodes):
        by_prefix.setdefault(nd["seq"][:k - 1], []).append(i)
    for i, nd in enumerate(nodes):
        nodes[nd["rc"]]["nbrs"].extend(by_prefix.get(nd["seq"][1:], []))
    return nodes


def _merge_labels(a, b, k):
    assert a[len(a) - (k - 1):] == b[:k - 1], (a, b)
    return a + b[k - 1:]


def merge_nodes(nodes, k, first_plus, second_minus):
    first_minus, second_plus = nodes[first_plus]["rc"], nodes[second_minus]["rc"]
    new_seq = _merge_labels(nodes[second_plus]["seq"], nodes[first_plus]["seq"], k)
    new_seq_rc = _merge_labels(nodes[first_minus]["seq"], nodes[second_minus]["seq"], k)
    nodes[second_plus]["seq"] = new_seq
    nodes[first_minus]["seq"] = new_seq_rc
    nodes[second_plus]["rc"] = first_minus
    nodes[first_minus]["rc"] = second_plus
    nodes[first_plus]["deleted"] = True
    nodes[second_minus]["deleted"] = True


def merge_loop(nodes, k, cls, scan):
    """doMerge over the nodes of `scan` (ascending), pass after pass until nothing merges"""
    while True:
        acted = False
        for i in scan:
            if not nodes[i]["deleted"] and len(nodes[i]["nbrs"]) == 1:
                other = nodes[i]["nbrs"][0]
                if len(nodes[other]["nbrs"]) != 1 or cls[i // 2] != cls[other // 2]:
                    continue
                merge_nodes(nodes, k, i, other)
                acted = True
        if not acted:
            return nodes


def reference_loop(kmers, cls, k):
    nodes = init_nodes(kmers, k)
    return merge_loop(nodes, k, cls, range(len(nodes)))


def link_analysis(kmers, cls, k):
    """mc_unitigs' result with the unitigs as strings: deg, nbr (flat), first, last_rc, seqs, irregular"""
    n = len(kmers)
    canon = [min(s, rc(s)) for s in kmers]
    if len(set(canon)) != n:
        raise ValueError("two entries are the same k-mer or each other's reverse complement")
    nodes = init_nodes(kmers, k)
    nbrs = [nd["nbrs"] for nd in nodes]
    pal = [nd["seq"] == rc(nd["seq"]) for nd in nodes]
    link, mark = [None] * (2 * n), [False] * (2 * n)
    for p in range(2 * n):
        if len(nbrs[p]) == 1:
            q = nbrs[p][0]
            if len(nbrs[q]) == 1 and cls[p // 2] == cls[q // 2]:
                assert nbrs[q][0] == p
                link[p] = q
                mark[p] = q == p or q == p ^ 1 or pal[p] or pal[q]
    seen, irr = [False] * (2 * n), [False] * n
    first, last_rc, seqs = [], [], []
    for h in range(2 * n):
        if link[h] is not None:
            continue
        chain, a, bad = [], h, False
        while True:
            chain.append(a)
            seen[a] = True
            bad = bad or mark[a ^ 1]
            if link[a ^ 1] is None:
                break
            a = link[a ^ 1]
        if bad:
            for a in chain:
                irr[a // 2] = True
        elif len(chain) >= 2 and h < chain[-1] ^ 1:
            first.append(h)
            last_rc.append(chain[-1] ^ 1)
            seqs.append(nodes[h]["seq"] + "".join(nodes[a]["seq"][-1] for a in chain[1:]))
    for a in range(2 * n):
        if not seen[a]:
            irr[a // 2] = True  # on a cycle
    return {"deg": [len(x) for x in nbrs], "nbr": [j for x in nbrs for j in x], "first": first, "last_rc": last_rc, "seqs": seqs,
            "irregular": [e for e in range(n) if irr[e]]}


def from_links(kmers, cls, k, res=None):
    """the nodes built from a link analysis, then the loop over the irregular entries' nodes"""
    res = res or link_analysis(kmers, cls, k)
    nodes = init_nodes(kmers, k)
    for first, last_rc, s in zip(res["first"], res["last_rc"], res["seqs"]):
        a = first
        while a ^ 1 != last_rc:
            nodes[a ^ 1]["deleted"] = True
            a = nodes[a ^ 1]["nbrs"][0]
            nodes[a]["deleted"] = True
        nodes[first]["seq"], nodes[last_rc]["seq"] = s, rc(s)
        nodes[first]["rc"], nodes[last_rc]["rc"] = last_rc, first
    scan = [2 * e + o for e in res["irregular"] for o in (0, 1)]
    return merge_loop(nodes, k, cls, scan)


def state(nodes):
    return [(True, None, None, tuple(nd["nbrs"])) if nd["deleted"] else (False, nd["rc"], nd["seq"], tuple(nd["nbrs"])) for nd in nodes]


# ---- inputs

def windows(seq, k):
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def entries_of(seqs, k):
    """the k-mers of the sequences in order, each canonical k-mer once"""
    out, have = [], set()
    for s in seqs:
        for w in windows(s, k):
            c = min(w, rc(w))
            if c not in have:
                have.add(c)
                out.append(w)
    return out


def random_chain(rng, m, k):
    """a sequence of m windows that is one regular chain on its own: no canonical k-mer twice, no (k-1)-mer twice on either strand"""
    while True:
        s = "".join(rng.choice("ACGT") for _ in range(m + k - 1))
        ends = [w for x in windows(s, k - 1) for w in (x, rc(x))]
        if len(set(ends)) == len(ends) and len(set(min(w, rc(w)) for w in windows(s, k))) == m:
            return s


def shuffled(rng, kmers):
    """node order and orientation shuffled"""
    out = [w if rng.random() < 0.5 else rc(w) for w in kmers]
    rng.shuffle(out)
    return out


def hand_cases():
    """name -> (k, kmers, cls): the shapes the link analysis has to get right"""
    cases = {}
    rng = random.Random(7)
    k = 5
    three = windows(random_chain(rng, 3, k), k)
    for perm in itertools.permutations(range(3)):
        for flips in itertools.product((0, 1), repeat=3):
            kmers = [rc(three[i]) if flips[i] else three[i] for i in perm]
            cases["chain3_%s_%s" % ("".join(map(str, perm)), "".join(map(str, flips)))] = (k, kmers, [0, 0, 0])
    stem = random_chain(rng, 6, 7)
    cases["branch"] = (7, entries_of([stem + "ACCTGA", stem + "CTTGAC", "GGATCA" + stem[:6]], 7), None)
    five = windows(random_chain(rng, 6, k), k)
    cases["class_change"] = (k, five, [0, 0, 0, 1, 1, 1])
    while True:  # a closed chain: the windows of a circular sequence, every (k-1)-mer once on either strand
        ring = "".join(rng.choice("ACGT") for _ in range(9))
        turn = ring + ring[:k - 1]
        ends = [w for x in windows(turn, k - 1)[:9] for w in (x, rc(x))]
        if len(set(ends)) == len(ends):
            break
    cases["cycle"] = (k, windows(turn, k), None)
    cases["poly_a"] = (k, ["AAAAA"], None)
    cases["poly_a_beside_a_chain"] = (k, ["AAAAA"] + three, None)
    x = random_chain(rng, 4, k)
    cases["hairpin"] = (k, entries_of([x + rc(x)], k), None)
    cases["hairpin_shuffled"] = (k, shuffled(rng, entries_of([x + rc(x)], k)), None)
    cases["palindrome_k4"] = (4, entries_of(["GGACGTTT"], 4), None)
    cases["palindrome_k4_alone"] = (4, ["ACGT"], None)
    cases["palindrome_k4_five_neighbours"] = (4, entries_of(["GACGT", "ACGA", "ACGG", "ACGC"], 4), None)
    return {name: (k, kmers, cls if cls is not None else [0] * len(kmers)) for name, (k, kmers, cls) in cases.items()}


def random_set(seed, k, n, n_classes=2):
    """n distinct canonical k-mers drawn at random (dense at small k: branches, cycles, hairpins, and palindromes at even k)"""
    rng = random.Random(seed)
    have, kmers = set(), []
    while len(kmers) < n:
        w = "".join(rng.choice("ACGT") for _ in range(k))
        c = min(w, rc(w))
        if c not in have:
            have.add(c)
            kmers.append(w)
    return kmers, [rng.randrange(n_classes) for _ in kmers]


def mixed_set(seed, k, chain_lengths=(1, 2, 3, 64, 65)):
    """chains of the lengths given beside a class change, a branch, a cycle, a self-loop, a hairpin and (even k) a palindrome, node order
    and orientation shuffled; whatever k-mer would repeat an earlier one is left out"""
    rng = random.Random(seed)
    seqs = [random_chain(rng, m, k) for m in chain_lengths]
    stem = random_chain(rng, k + 3, k)
    seqs += [stem + "A" + random_chain(rng, 1, k), stem + "C" + random_chain(rng, 1, k)]  # a branch
    ring = random_chain(rng, 2 * k, k)
    seqs.append(ring + ring[:k - 1])  # a cycle
    seqs.append("A" * k)  # a self-loop
    x = random_chain(rng, k, k)
    seqs.append(x + rc(x))  # a hairpin (at even k with a palindrome at its centre)
    if k % 2 == 0:
        half = random_chain(rng, 1, k)[:k // 2]
        seqs.append(random_chain(rng, 3, k) + half + rc(half) + random_chain(rng, 3, k))
    kmers = entries_of(seqs, k)
    change = windows(random_chain(rng, 8, k), k)  # a class change in mid-chain
    fresh = [w for w in change if min(w, rc(w)) not in set(min(v, rc(v)) for v in kmers)]
    cls = {min(w, rc(w)): (1 if i >= 4 else 0) for i, w in enumerate(fresh)}
    kmers = shuffled(rng, kmers + fresh)
    return kmers, [cls.get(min(w, rc(w)), 0) for w in kmers]


def disjoint_chains(rng, ms, k):
    """strings of m + k - 1 bases, one for every m of ms: no (k-1)-mer twice on either strand over all of them, so every string is one
    regular chain on its own and no chain touches another (grown base by base; a dead end starts the string again)"""
    used, out = set(), []
    for m in ms:
        for _ in range(2000):
            s = "".join(rng.choice("ACGT") for _ in range(k - 1))
            if s in used or s == rc(s):
                continue
            mine = {s, rc(s)}
            while len(s) < m + k - 1:
                for c in rng.sample("ACGT", 4):
                    e = s[len(s) - (k - 2):] + c if k > 2 else c
                    if e not in used and e not in mine and e != rc(e):
                        s += c
                        mine |= {e, rc(e)}
                        break
                else:
                    break
            if len(s) == m + k - 1:
                used |= mine
                out.append(s)
                break
        else:
            raise AssertionError("no chain of %d entries at k = %d beside the others" % (m, k))
    return out


WORD_EDGE_LENGTHS = (31, 32, 33, 63, 64, 65, 96, 97)


def word_edge_groups(k):
    """The unitig lengths of WORD_EDGE_LENGTHS that exist at this k (a chain has m = length - k + 1 >= 2 entries), in groups that one call
    can hold side by side.  From k = 31 on one group holds them all.  At k = 5 there are 240 4-mers that are not their own reverse
    complement, and a chain of m entries takes m + 1 of them on either strand: 31, 32 and 33 fit together, every longer one stands in
    a call of its own in front of a short neighbour -- 63, 64, 65 before one of 31, 32, 33, and 96 and 97 (186 and 188 4-mers) before
    a chain of two entries."""
    if k > 5:
        return [[n for n in WORD_EDGE_LENGTHS if n - k + 1 >= 2]]
    return [[31, 32, 33], [63, 31], [64, 32], [65, 33], [96, k + 1], [97, k + 1]]


def word_edge_chains(seed, k, odd_head, group=0):
    """Regular chains side by side whose unitigs have the lengths of word_edge_groups(k)[group]: a word of bases, one less, one more.
    A base written a word late lands in the next unitig's first word.  Every chain's entries stand in string order, so it is listed
    from its first entry's node: the entry as given (an even node) or, with odd_head, given as its reverse complement, so that the
    listed head is the odd node.  The other entries are oriented at random.  Returns (kmers, cls, the unitig lengths)."""
    rng = random.Random(seed + 17 * group)
    lengths = word_edge_groups(k)[group]
    kmers = []
    for s in disjoint_chains(rng, [n - k + 1 for n in lengths], k):
        w = windows(s, k)
        kmers += [rc(w[0]) if odd_head else w[0]] + [x if rng.random() < 0.5 else rc(x) for x in w[1:]]
    return kmers, [0] * len(kmers), lengths


# ---- the packed forms

def pack_kmers(kmers):
    """(hi, lo) as include/mcgpu.h takes oriented k-mers"""
    hi, lo = np.zeros(len(kmers), dtype=np.uint64), np.zeros(len(kmers), dtype=np.uint64)
    for i, s in enumerate(kmers):
        v = 0
        for c in s:
            v = (v << 2) | CODE[c]
        hi[i], lo[i] = v >> 64, v & ((1 << 64) - 1)
    return hi, lo


def pack_unitigs(seqs):
    """(base_offsets, bases) as mc_unitigs_result holds the unitigs: every one from a new word on"""
    offsets, words = [0], []
    for s in seqs:
        for i in range(0, len(s), 32):
            v = 0
            for c in s[i:i + 32]:
                v = (v << 2) | CODE[c]
            words.append(v << (2 * (32 - len(s[i:i + 32]))))
        offsets.append(32 * len(words))
    return np.array(offsets, dtype=np.uint64), np.array(words, dtype=np.uint64)


def hosttest_input(k, kmers, cls):
    return "%d %d\n" % (k, len(kmers)) + "".join("%s %d\n" % (s, c) for s, c in zip(kmers, cls))
