"""mc_env_join's definitions (include/mcgpu.h) restated on dicts of strings, the designed graph files that the CPU and the GPU tests of
the environment join share, and what both need to get from strings to packed words and back.  No test of its own: test_env_join_model.py
pins it, test_gpu_env_join.py and test_gpu_cli_multi_join.py use it."""
import random

import numpy as np

COMP = {"A": "T", "G": "C", "C": "G", "T": "A"}
CODE = {"A": 0, "G": 1, "C": 2, "T": 3}
M32 = 0xFFFFFFFF


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def normalize(s):
    r = rc(s)
    return s if s < r else r


def i32_abs_diff(v, w):
    """|v - w| in 32-bit int arithmetic, as an unsigned word"""
    d = (v - w) & M32
    return (-d) & M32 if d >> 31 else d


def join(entries, graphs, gene):
    """entries: oriented k-mer strings; graphs: one dict {oriented k-mer: depth} a graph; gene: a string.  Returns member, is_gene, kc
    (lists, one value an entry) and the matrices diff, diff_alt, uni (lists of rows), from the definitions."""
    G = len(graphs)
    member, is_gene, kc = [], [], []
    for e in entries:
        r = rc(e)
        member.append(sum(1 << g for g in range(G) if e in graphs[g] or r in graphs[g]))
        is_gene.append(1 if (e in gene or r in gene) else 0)
        kc.append(sum(graphs[g][e] for g in range(G) if e in graphs[g]))
    diff = [[0] * G for _ in range(G)]
    diff_alt = [[0] * G for _ in range(G)]
    uni = [[0] * G for _ in range(G)]
    for x in sorted(set().union(*[set(g) for g in graphs])):
        H = [g for g in range(G) if x in graphs[g]]
        for i in range(G):
            for j in range(G):
                if i in H and j in H:
                    di, dj = graphs[i][x], graphs[j][x]
                    diff[i][j] += i32_abs_diff(di, dj)
                    diff_alt[i][j] += i32_abs_diff(di, dj)
                    uni[i][j] += max(di, dj) & M32
                elif i in H:
                    for m in (diff, diff_alt, uni):
                        m[i][j] += graphs[i][x] & M32
                elif j in H:
                    diff[i][j] += graphs[j][x] & M32
                    uni[i][j] += graphs[j][x] & M32
    raw_uni_max = max(max(row) for row in uni) if G else 0
    raw_diff_max = max(max(row) for row in diff) if G else 0
    wrap = lambda m: [[v & M32 for v in row] for row in m]
    return {"member": member, "is_gene": is_gene, "kc": kc, "diff": wrap(diff), "diff_alt": wrap(diff_alt), "uni": wrap(uni),
            "raw_uni_max": raw_uni_max, "raw_diff_max": raw_diff_max}


def entries_of(graphs):
    """one entry a k-mer of the graphs, in normalised form, sorted (any order serves mc_env_join)"""
    return sorted({normalize(x) for g in graphs for x in g})


def pack(kmers, k):
    """(hi, lo) uint64 arrays of k-mer strings; hi is None when k <= 32"""
    vals = []
    for s in kmers:
        v = 0
        for c in s:
            v = (v << 2) | CODE[c]
        vals.append(v)
    lo = np.array([v & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)
    hi = np.array([v >> 64 for v in vals], dtype=np.uint64) if k > 32 else None
    return hi, lo


def pack_gene(gene):
    words = [0] * ((len(gene) + 31) // 32)
    for i, c in enumerate(gene):
        words[i >> 5] |= CODE[c] << (62 - 2 * (i & 31))
    return np.array(words, dtype=np.uint64)


def records(graphs, k):
    """rec_hi, rec_lo, rec_depth, graph_offsets of a list of graph dicts"""
    kmers, depths, offsets = [], [], [0]
    for g in graphs:
        for x, d in g.items():
            kmers.append(x)
            depths.append(d)
        offsets.append(len(kmers))
    hi, lo = pack(kmers, k)
    return hi, lo, np.array(depths, dtype=np.int64).astype(np.int32), np.array(offsets, dtype=np.uint64)


def graph_text(lines):
    return "".join("%s %d\n" % (x, d) for x, d in lines)


def graph_dict(lines):
    """what DeBruijnGraphUtils.loadGraph keeps of a file's lines: the last line of a k-mer wins"""
    return dict(lines)


def random_dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def no_palindrome(seq, k):
    return all(seq[i:i + k] != rc(seq[i:i + k]) for i in range(len(seq) - k + 1))


def windows(seq, k):
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def designed_case(k, G, seed=0):
    """Graph files (lists of (k-mer, depth) lines) and a gene with every feature the join has to tell apart:
      - a stem, then a bubble whose arms are in different graph sets, then the stem again: the arms must not merge with the stem;
      - the gene lies inside the stem, given as the reverse complement of the graphs' strand: the gene barrier cuts the stem;
      - graph 0 spells the stem as it is, the last graph its reverse complement (one orientation in one graph, the other in another);
      - graph 0 also holds BOTH orientations of a few stem k-mers, with different depths;
      - one k-mer is on two lines of graph 0's file (the last line wins);
      - with G >= 3 graph 1 is empty; depths of 0 and 32767 occur.
    Returns (files, gene): files[g] is the list of lines of graph g."""
    rng = random.Random(1000 * k + 10 * G + seed)
    while True:
        left, right = random_dna(rng, k + 12), random_dna(rng, k + 12)
        arm_a, arm_b = random_dna(rng, k + 3), random_dna(rng, k + 3)
        path_a, path_b = left + arm_a + right, left + arm_b + right
        if no_palindrome(path_a, k) and no_palindrome(path_b, k):
            break
    gene = rc(left[3:3 + k + 4])  # k + 4 bases of the stem, on the other strand
    files = [[] for _ in range(G)]
    depth = lambda: rng.choice([0, 1, 2, 7, 100, 32767])
    holders_a = list(range(0, G, 2)) or [0]           # arm a: the even graphs
    holders_b = list(range(1, G, 2)) or [0]           # arm b: the odd ones (G = 1: both in graph 0)
    empty = 1 if G >= 3 else None
    for g in range(G):
        if g == empty:
            continue
        flip = g == G - 1 and G > 1
        seqs = []
        if g in holders_a:
            seqs.append(path_a)
        if g in holders_b or (g not in holders_a):
            seqs.append(path_b)
        seen = set()
        for s in seqs:
            for w in windows(s, k):
                x = rc(w) if flip else w
                if x not in seen:
                    seen.add(x)
                    files[g].append((x, depth()))
    if empty is not None:   # the arm that only the empty graph would have held goes to graph 0 as well, so that it exists at all
        have = {x for x, _ in files[0]}
        for w in windows(path_b, k):
            if w not in have:
                files[0].append((w, depth()))
    stem = windows(left, k)
    for w in stem[:3]:      # both orientations in graph 0
        files[0].append((rc(w), depth() + 1))
    files[0].append((stem[4], 11))   # a second line of one k-mer ...
    files[0].append((stem[4], 13))   # ... and a third: 13 stays
    return files, gene


def java_spread_hash(s):
    """String.hashCode, then HashMap.hash's spread"""
    h = 0
    for ch in s:
        h = (31 * h + ord(ch)) & M32
    return h ^ (h >> 16)


def treeified_case():
    """k = 5 (odd: no palindromes): graph 0 is twelve k-mers that share a bucket of a 64-bucket java.util.HashMap: they come first, so the
    union map of k-mers and reverse complements treeifies that bin when it has 64 buckets.  Graphs 1 and 2 bring 210 others and share a part."""
    rng = random.Random(5)
    every = ["".join(t) for t in __import__("itertools").product("ACGT", repeat=5)]
    buckets = {}
    for w in every:
        buckets.setdefault(java_spread_hash(w) & 63, []).append(w)
    crowd = max(buckets.values(), key=len)[:12]
    assert len(crowd) == 12
    others = [w for w in every if w not in crowd]
    rng.shuffle(others)
    lists = [crowd, others[:100] + crowd[3:5], others[60:210]]
    files = [[(x, 1 + (i + 3 * g) % 9) for i, x in enumerate(l)] for g, l in enumerate(lists)]
    return files, "ACGTTGCATTGACC"


def contig_environments(k, G, n, seed=0, flip=(1,)):
    """G graph files (bytes) cut from one random contig of n + k - 1 bases: graph g holds the windows of a slice of it, the slices
    overlapping widely; the odd graphs read a variant of the contig with a substitution every ~1500 bases (coloured bubbles); the graphs
    of `flip` spell their k-mers on the other strand.  Depths are 10 .. 99 and differ between graphs.  Also returns the gene: 300 bases
    from the middle of the contig (or all of a shorter one).  About n k-mers in the union (a few more for the variant's)."""
    from numpy.lib.stride_tricks import sliding_window_view
    rng = np.random.default_rng(seed + 1000 * k + G)
    base = rng.integers(0, 4, n + k - 1).astype(np.uint8)
    variant = base.copy()
    for pos in range(700, len(base) - k, 1500):
        variant[pos] = (variant[pos] + 1 + pos % 3) & 3
    letters = np.frombuffer(b"ACGT", dtype="S1")
    texts = []
    for g in range(G):
        a, b = g * n // (2 * G), n - (G - 1 - g) * n // (2 * G)   # windows a .. b - 1
        codes = (variant if g % 2 else base)[a:b + k - 1]
        if g in flip:
            codes = (3 - codes[::-1]).astype(np.uint8)              # (ACGT order: the complement is 3 - code)
        win = sliding_window_view(letters[codes], k)
        m = len(win)
        out = np.empty((m, k + 4), dtype="S1")
        out[:, :k] = win
        out[:, k] = b" "
        depth = 10 + (np.arange(m) * (7 + g) + 13 * g) % 90
        out[:, k + 1] = np.frombuffer(b"0123456789", dtype="S1")[depth // 10]
        out[:, k + 2] = np.frombuffer(b"0123456789", dtype="S1")[depth % 10]
        out[:, k + 3] = b"\n"
        texts.append(out.tobytes())
    mid = len(base) // 2
    gene = letters[base[max(0, mid - 150):mid + 150]].tobytes().decode()
    return texts, gene
