"""runTrimPaths (src/algo/OneSequenceCalculator.java:241-262) restated with letters, lists and sets: the model that
mc_trim_paths is tested against (tests/test_gpu_trim_paths.py) and that is itself tested against the oracle
(tests/test_trim_paths_model.py).  Plus the helpers that turn strings into the packed arrays the ABI takes and back."""
import numpy as np

NUCLEOTIDES = "AGCT"  # src/utils/StringUtils.java: the order of the neighbours, and the 2-bit codes of the packing


def left_neighbors(kmer):
    return [c + kmer[:-1] for c in NUCLEOTIDES]


def right_neighbors(kmer):
    return [kmer[1:] + c for c in NUCLEOTIDES]


def all_neighbors(kmer):
    out = []
    for c in NUCLEOTIDES:  # interleaved L(A) R(A) L(G) R(G) ...
        out.append(c + kmer[:-1])
        out.append(kmer[1:] + c)
    return out


def neighbors_by_dir(direction, kmer):
    if direction == -1:
        return left_neighbors(kmer)
    if direction == 1:
        return right_neighbors(kmer)
    assert direction == 0
    return all_neighbors(kmer)


def run_trim_paths(last_kmers, distance_to_kmer, direction):
    """the Java, line for line: returns visitedKmers (what retainAll keeps)"""
    queue = []
    visited = set()
    for kmer in last_kmers:
        queue.append(kmer)
        visited.add(kmer)
    head = 0
    while head < len(queue):
        kmer = queue[head]
        head += 1
        for neighbor in neighbors_by_dir(-direction, kmer):
            if neighbor in distance_to_kmer and neighbor not in visited:
                queue.append(neighbor)
                visited.add(neighbor)
    return visited


def kept_mask(kmers, last, direction):
    """kmers: distinct strings of one length; last: a flag each.  np.uint8[n]: 1 where the walk visits the entry"""
    assert len(set(kmers)) == len(kmers)
    visited = run_trim_paths([s for s, l in zip(kmers, last) if l], set(kmers), direction)
    return np.array([1 if s in visited else 0 for s in kmers], dtype=np.uint8)


def pack_kmers(kmers):
    """strings -> (hi, lo) as mc_bfs_result holds them: 2 bits a base, A0 G1 C2 T3, first base most significant"""
    hi = np.zeros(len(kmers), dtype=np.uint64)
    lo = np.zeros(len(kmers), dtype=np.uint64)
    for i, s in enumerate(kmers):
        v = 0
        for c in s:
            v = (v << 2) | NUCLEOTIDES.index(c)
        hi[i] = v >> 64
        lo[i] = v & 0xFFFFFFFFFFFFFFFF
    return hi, lo


def unpack_kmers(hi, lo, k):
    out = []
    for h, l in zip(hi, lo):
        v = (int(h) << 64) | int(l)
        out.append("".join(NUCLEOTIDES[(v >> (2 * (k - 1 - i))) & 3] for i in range(k)))
    return out


def windows(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def circular_windows(s, k):
    return windows(s + s[:k - 1], k)


def revcomp(s):
    return "".join("TCGA"[NUCLEOTIDES.index(c)] for c in reversed(s))


def repeat_free(rng, length, k):
    """a random string whose k-windows, and whose (k-1)-windows, are all different: its k-windows are one chain"""
    for _ in range(100):
        s = "".join(NUCLEOTIDES[c] for c in rng.integers(0, 4, length))
        w = windows(s, k - 1) if k > 1 else []
        if len(set(w)) == len(w):
            return s
    raise AssertionError("no repeat-free string of %d bases at k = %d" % (length, k))


# ---- designed shapes: (kmers, last) of strings of length k, shared by the model's tests and the GPU's

def _rand(rng, n):
    return "".join(NUCLEOTIDES[c] for c in rng.integers(0, 4, n))


def _other(c, step=1):
    return NUCLEOTIDES[(NUCLEOTIDES.index(c) + step) % 4]


def _flags(kmers, last_kmers):
    assert len(set(kmers)) == len(kmers) and set(last_kmers) <= set(kmers)
    return kmers, [1 if s in set(last_kmers) else 0 for s in kmers]


def chain(rng, k, n, last_at=None):
    """the n windows of a repeat-free string in string order, `last` on window n // 3 alone"""
    w = windows(repeat_free(rng, n + k - 1, k), k)
    return _flags(w, [w[n // 3 if last_at is None else last_at]])


def fork(rng, k, stem=40, arm=30, live=(True, False)):
    """a stem whose last window has two right neighbours, each the start of an arm; live: which arms end in `last`.
    Returns (kmers, last, parts) with parts = the windows of the stem, of arm 0 and of arm 1"""
    s = repeat_free(rng, stem + k - 1, k)
    a = s[-(k - 1):] + _other(s[-1], 1) + _rand(rng, arm - 1) if k > 1 else _rand(rng, arm)
    b = s[-(k - 1):] + _other(s[-1], 2) + _rand(rng, arm - 1) if k > 1 else _rand(rng, arm)
    ws, wa, wb = windows(s, k), windows(a, k), windows(b, k)
    kmers, last = _flags(ws + wa + wb, ([wa[-1]] if live[0] else []) + ([wb[-1]] if live[1] else []))
    return kmers, last, (ws, wa, wb)


def bubble(rng, k, flank=30):
    """two strings that differ in one base: a branch node whose arms rejoin k windows later; `last` on the far end"""
    p, q = _rand(rng, flank + k), _rand(rng, flank + k)
    w = windows(p + "A" + q, k)
    w2 = [s for s in windows(p + "G" + q, k) if s not in set(w)]
    return _flags(w + w2, [w[-1]])


def cycle(rng, k, length=70, n_last=0):
    """the windows of a circular string"""
    w = circular_windows(repeat_free(rng, length, k), k)
    assert len(set(w)) == len(w)
    return _flags(w, w[5:5 + n_last])


def cycle_with_tail_out(rng, k, length=70, tail=25):
    """... and a tail that leaves it by right steps and ends in `last`"""
    c = repeat_free(rng, length, k)
    w = circular_windows(c, k)
    t = w[10][1:] + _other(w[11][-1]) + _rand(rng, tail)
    wt = windows(t, k)
    return _flags(w + wt, [wt[-1]])


def last_into_cycle(rng, k, length=70, head=25):
    """a `last` at the start of a head whose right steps lead into a cycle and nowhere else"""
    c = repeat_free(rng, length, k)
    w = circular_windows(c, k)
    h = _rand(rng, head) + _other(w[19][0]) + w[20][:-1]  # (its last window's right neighbour is w[20])
    wh = windows(h, k)
    return _flags(wh + w, [wh[0]])


def dense(rng, k, genome=3000, density=200):
    """the distinct windows of a random genome, `last` at random"""
    w = list(dict.fromkeys(windows(_rand(rng, genome), k)))
    last = [1 if x == 0 else 0 for x in rng.integers(0, density, len(w))]
    return w, last


# ---- a walk on which the trim bites, for the oracle and for mc_bfs alike

def walk_case(k):
    """Reads and seeds on which a trimmed walk loses something in every direction: a main contig whose walk the radius cap
    stops (`last` there), tips that leave it or join it and die out inside the radius, an island that ends before the cap
    reaches it, and a lone k-mer with no neighbour at all (under dir = 0 every k-mer that has a neighbour in the walk is `last`:
    the neighbour it was reached from is refused).  Every read twice: walk with min_cov = 2.
    Returns (codes, offsets, seeds, max_radius), codes as the oracle's (A0 G1 C2 T3)."""
    rng = np.random.default_rng(100 * k)
    draw = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    text = lambda a: "".join(NUCLEOTIDES[c] for c in a)
    if k > 5:
        main, island = draw(1200), draw(k + 70)
        tips = [np.concatenate([main[p - k:p], draw(25)]) for p in (560, 580, 640, 660)]
        tips += [np.concatenate([draw(25), main[p:p + k]]) for p in (540, 570, 650, 670)]
        L, radius, seeds = k + 20, 60, [main[590:590 + k + 30], island[30:30 + k + 8]]
    else:  # (4^5 k-mers in all: everything is small)
        main, island, tips = draw(60), draw(12), []
        L, radius, seeds = 8, 4, [main[28:36], island[3:9]]
    there = set()
    for s in [main, island] + tips:
        w = windows(text(s), k)
        there.update(w, [revcomp(x) for x in w])
    while True:  # (at k = 5 a random k-mer has a neighbour among the others more often than not: drawn until it has none)
        lone = draw(k)
        s = text(lone)
        if not (there | {s, revcomp(s)}) & set(all_neighbors(s)) and s not in there:  # (nor its own neighbour, on either strand)
            break
    seeds.append(lone)
    reads = []
    for s in [main, island, lone] + tips:
        n = min(L, len(s))
        for i in range(len(s) - n + 1):
            reads += [s[i:i + n], s[i:i + n]]
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), off, seeds, radius
