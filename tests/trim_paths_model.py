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


# ---- deeper shapes: nests of forks, fans, arms that rejoin through PASS pointers, structures that stay OPEN (all by right steps:
# twin() gives the same shape by left steps)

def twin(kmers):
    """the reverse complements: x's right neighbours become the left neighbours of its twin, so dir = -1 on the twins is dir = +1 here"""
    return [revcomp(s) for s in kmers]


def _tip(rng, frm, c, n):
    """n windows that leave k-mer frm by base c and end nowhere"""
    return windows(frm[1:] + c + _rand(rng, n - 1), len(frm))


def _path_to(rng, frm, c, m, target, via=None):
    """the k + m windows that leave frm by base c and whose last one has `target` for its right neighbour; via: that window's first
    base (m >= 1), so that two paths to one target end in different windows"""
    middle = _rand(rng, m) if via is None or m == 0 else _rand(rng, m - 1) + via
    return windows(frm[1:] + c + middle + target[:-1], len(frm))


def _nest(rng, out, lasts, frm, levels, live, arm=3, bases="AG"):
    """a full binary tree of forks below k-mer frm (which becomes its root fork): `levels` levels of forks, every leaf a tip; with
    `live` the tip on the last base of the last fork of every level ends in `last`, every other tip is dead"""
    for side, c in enumerate(bases):
        w = _tip(rng, frm, c, arm)
        out += w
        on = live and side == len(bases) - 1
        if levels > 1:
            _nest(rng, out, lasts, w[-1], levels - 1, on, arm, bases)
        elif on:
            lasts.append(w[-1])


def fork_nest(rng, k, depth):
    """a stem, then `depth` levels of forks, only the deepest arm live: a fork is settled one phase after both its arms are, so the
    root waits depth + 1 phases"""
    out, lasts = windows(repeat_free(rng, 5 + k - 1, k), k), []
    _nest(rng, out, lasts, out[-1], depth, True)
    return _flags(out, lasts)


def fan(rng, k, width):
    """`width` components, each a stem whose last window has `width` right neighbours in the set (bases A, G, C, T in that order), the
    live arm in another position in each.  Returns (kmers, last, parts): parts[p] = (stem, [arm windows by position]) of the component
    whose live arm is p"""
    out, lasts, parts = [], [], []
    for p in range(width):
        stem = windows(repeat_free(rng, 5 + k - 1, k), k)
        arms = [_tip(rng, stem[-1], NUCLEOTIDES[j], 4) for j in range(width)]
        lasts.append(arms[p][-1])
        out += stem + [x for a in arms for x in a]
        parts.append((stem, arms))
    kmers, last = _flags(out, lasts)
    return kmers, last, parts


def rejoin_through_pass(rng, k):
    """One component for every way to give three arms of a node X three of the four bases (24), and for each the next of four
    variants.  Two arms, of k and k + 5 windows, end at one stop S, the third at another stop S2; S and S2 are roots of two-level nests,
    so both are OPEN when X first looks: its first two arms' pointers rest on the same stop (they count once), the third sets a second
    stop and X waits.  Variants: S live, S2 live, neither, and no third arm at all (X then passes to S).
    Returns (kmers, last, xs): xs = [(X, variant)]"""
    import itertools
    out, lasts, xs = [], [], []
    for n, bases in enumerate(itertools.permutations(NUCLEOTIDES, 3)):
        variant = n % 4
        stem = windows(repeat_free(rng, 3 + k - 1, k), k)
        x, s, s2 = stem[-1], _rand(rng, k), _rand(rng, k)
        out += stem + _path_to(rng, x, bases[0], 0, s) + _path_to(rng, x, bases[1], 5, s, _other(bases[0])) + [s]
        _nest(rng, out, lasts, s, 2, variant == 0)
        if variant != 3:
            out += _path_to(rng, x, bases[2], 2, s2) + [s2]
            _nest(rng, out, lasts, s2, 2, variant == 1)
        xs.append((x, variant))
    kmers, last = _flags(out, lasts)
    return kmers, last, xs


def figure_eight(rng, k, with_last):
    """two cycles through one node, a stem in front of it; with_last: a third way out of the node that ends in `last`.  Without it
    both of the node's ways come back to itself: nothing is kept"""
    stem = windows(repeat_free(rng, 4 + k - 1, k), k)
    n = stem[-1]
    out = stem + _path_to(rng, n, "A", 3, n, _other(stem[-2][0], 1)) + _path_to(rng, n, "G", 6, n, _other(stem[-2][0], 2))
    tail = _tip(rng, n, "C", 5) if with_last else []
    return _flags(out + tail, tail[-1:])


def open_triangle(rng, k, with_last):
    """three forks, each with one arm to either of the other two: every one has two OPEN stops for good.  with_last: a third arm of the
    last fork ends in `last`, and everything is kept"""
    f = [_rand(rng, k) for _ in range(3)]
    out = windows(_rand(rng, 3) + "A" + f[0], k) + f[1:]  # a stem into the first
    for i in range(3):
        out += _path_to(rng, f[i], "A", 1 + i, f[(i + 1) % 3], "C") + _path_to(rng, f[i], "G", 4 + i, f[(i + 2) % 3], "T")
    tail = _tip(rng, f[2], "T", 5) if with_last else []
    return _flags(out + tail, tail[-1:])


def dead_beside_cycle(rng, k):
    """a stem to a fork whose arms are a dead tip and a path into a closed cycle of entries with one way on: nothing is kept"""
    stem = windows(repeat_free(rng, 5 + k - 1, k), k)
    ring = circular_windows(repeat_free(rng, 70, k), k)
    assert len(set(ring)) == 70
    out = stem + _tip(rng, stem[-1], "A", 6) + _path_to(rng, stem[-1], "C", 2, ring[7], _other(ring[6][0])) + ring
    return _flags(out, [])


def kept_through_pass(rng, k, length=40):
    """a stem to a fork Q: one arm is a chain of k + `length` windows (more than 2^5) to a fork F with a dead and a live tip, the other
    a dead two-level nest.  F turns KEPT in the second phase, when Q still has two OPEN stops; in the third Q finds the KEPT stop
    where its arm's pointer rests.  Returns (kmers, last, (Q, F))"""
    stem = windows(repeat_free(rng, 5 + k - 1, k), k)
    q, f = stem[-1], _rand(rng, k)
    out, lasts = stem + _path_to(rng, q, "T", length, f) + [f], []
    _nest(rng, out, lasts, f, 1, True, arm=4)
    root = _tip(rng, q, "G", 2)
    out += root
    _nest(rng, out, lasts, root[-1], 2, False)
    kmers, last = _flags(out, lasts)
    return kmers, last, (q, f)


# ---- one phase of csrc/trim_paths.hip (dir = +1 / -1), restated on lists from the unit's header comment

DEAD, KEPT, PASS, OPEN = 0, 1, 2, 3
BRANCHES = ("kept_stop", "kept_through_pass", "rejoin", "second_stop", "itself", "dead_stop", "unrested_pass")


def phase_model(kmers, last, direction):
    """classify, then pointer jumping over ceil(log2 n) rounds, until a classify changes nothing.  Returns (kept mask, the number of
    classify passes, the last one included, and for every entry the set of BRANCHES it took while it was OPEN)"""
    assert direction in (-1, 1)
    n = len(kmers)
    at = {s: i for i, s in enumerate(kmers)}
    succ = [[at.get(x) for x in (right_neighbors(s) if direction > 0 else left_neighbors(s))] for s in kmers]
    kind, rest = [KEPT if l else OPEN for l in last], list(range(n))
    took = [set() for _ in range(n)]
    rounds = 0
    while (1 << rounds) < n:
        rounds += 1
    phases = 0
    for _ in range(n + 1):
        phases += 1
        new_kind, new_rest, changed, passed = list(kind), list(rest), False, False
        for i in range(n):
            if kind[i] != OPEN:
                continue
            kept, a, b = False, None, None
            for j in succ[i]:
                if j is None:
                    continue
                t = rest[j] if kind[j] == PASS else j
                kt = kind[t]
                if kt == KEPT:
                    kept = True
                    took[i].add("kept_through_pass" if t != j else "kept_stop")
                elif kt == OPEN and t != i:
                    if a is None or a == t:
                        if a == t:
                            took[i].add("rejoin")
                        a = t
                    else:
                        b = t
                        took[i].add("second_stop")
                else:
                    took[i].add("itself" if kt == OPEN else "dead_stop" if kt == DEAD else "unrested_pass")
            if kept:
                new_kind[i] = KEPT
            elif a is None:
                new_kind[i] = DEAD
            elif b is None:
                new_kind[i], new_rest[i] = PASS, a
                passed = True
            changed = changed or new_kind[i] != OPEN
        kind, rest = new_kind, new_rest
        if not changed:
            break
        if passed:
            for _ in range(rounds):
                rest = [rest[rest[i]] if kind[i] == PASS and kind[rest[i]] == PASS else rest[i] for i in range(n)]
    kept = [1 if kind[i] == KEPT or (kind[i] == PASS and kind[rest[i]] == KEPT) else 0 for i in range(n)]
    return np.array(kept, dtype=np.uint8), phases, took


SHAPES = ("chain", "fork", "fork_dead", "bubble", "cycle", "cycle_last", "cycle_with_tail_out", "last_into_cycle", "dense",
          "fork_nest_2", "fork_nest_3", "fork_nest_6", "fan_3", "fan_4", "rejoin_through_pass", "figure_eight", "figure_eight_last",
          "open_triangle", "open_triangle_last", "dead_beside_cycle", "kept_through_pass")
NEW_SHAPES = SHAPES[SHAPES.index("fork_nest_2"):]


def shape(name, k):
    """(kmers, last) of a named shape, by right steps; the same every time"""
    rng = np.random.default_rng(1000 * SHAPES.index(name) + k)
    if name.startswith("fork_nest_"):
        return fork_nest(rng, k, int(name[-1]))
    if name.startswith("fan_"):
        return fan(rng, k, int(name[-1]))[:2]
    made = {"chain": lambda: chain(rng, k, 100), "fork": lambda: fork(rng, k)[:2], "fork_dead": lambda: fork(rng, k, live=(False, False))[:2],
            "bubble": lambda: bubble(rng, k), "cycle": lambda: cycle(rng, k, 70, 0), "cycle_last": lambda: cycle(rng, k, 70, 1),
            "cycle_with_tail_out": lambda: cycle_with_tail_out(rng, k), "last_into_cycle": lambda: last_into_cycle(rng, k),
            "dense": lambda: dense(rng, 7 if k < 32 else k), "rejoin_through_pass": lambda: rejoin_through_pass(rng, k)[:2],
            "figure_eight": lambda: figure_eight(rng, k, False), "figure_eight_last": lambda: figure_eight(rng, k, True),
            "open_triangle": lambda: open_triangle(rng, k, False), "open_triangle_last": lambda: open_triangle(rng, k, True),
            "dead_beside_cycle": lambda: dead_beside_cycle(rng, k), "kept_through_pass": lambda: kept_through_pass(rng, k)[:2]}
    return made[name]()


# what every shape is named for: (the least number of classify passes, the branches of k_tp_classify that some entry must take)
SHAPE_MEETS = {
    "fork_nest_2": (4, {"dead_stop", "kept_through_pass", "second_stop"}), "fork_nest_3": (5, {"dead_stop", "kept_through_pass", "second_stop"}),
    "fork_nest_6": (8, {"dead_stop", "kept_through_pass", "second_stop"}), "fan_3": (3, {"dead_stop", "kept_through_pass", "second_stop"}),
    "fan_4": (3, {"dead_stop", "kept_through_pass", "second_stop"}), "rejoin_through_pass": (5, {"rejoin", "second_stop", "kept_through_pass", "dead_stop"}),
    "figure_eight": (3, {"itself", "second_stop"}), "figure_eight_last": (3, {"itself", "kept_through_pass"}),
    "open_triangle": (2, {"second_stop"}), "open_triangle_last": (3, {"second_stop", "kept_stop"}),
    "dead_beside_cycle": (3, {"dead_stop", "unrested_pass"}), "kept_through_pass": (4, {"kept_through_pass", "second_stop", "dead_stop"}),
}


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
