"""The walk of KmerEnvCalculator.runBfs (src/algo/KmerEnvCalculator.java:60-76) over one component, on strings: the exact replay with
its whole queue, and the bounded form that mc_walk_order computes.

A component is a list of distinct k-mers as strings, no two of them reverse complements of each other; member 0 is the seed as the
read spells it.  Both functions answer with member numbers:
  order   the members in the order of their first pops (the order of the subgraph's first puts), the seed first;
  twice   per member, whether it is popped more than once (its put value then ends as 0).
Neighbours are StringUtils.allNeighbors': for A, G, C, T in turn the left neighbour (base + x[:-1]) before the right one (x[1:] + base)."""

BASES = "AGCT"  # the reference's NUCLEOTIDES, codes 0..3
_COMP = str.maketrans("ACGT", "TGCA")


def rc(x):
    return x.translate(_COMP)[::-1]


def neighbours(x):
    out = []
    for c in BASES:
        out.append(c + x[:-1])
        out.append(x[1:] + c)
    return out


def _index(members):
    """k-mer string in either orientation -> member number"""
    at = {}
    for i, m in enumerate(members):
        assert m not in at, "two members are the same k-mer or each other's reverse complement"
        at[m] = i
        at[rc(m)] = i
    return at


def exact_replay(members, cap=None):
    """The reference's loop as it is: a FIFO without a visited set over the component's own counts.  Returns (order, twice, queue
    length), or None when the queue passes `cap` entries."""
    at = _index(members)
    live = [True] * len(members)  # count > 0
    pops = [0] * len(members)
    order = []
    queue = [members[0]]
    head = 0
    while head < len(queue):
        if cap is not None and len(queue) > cap:
            return None
        x = queue[head]
        head += 1
        for y in neighbours(x):
            t = at.get(y)
            if t is not None and live[t]:
                queue.append(y)
        m = at[x]
        if pops[m] == 0:
            order.append(m)
        pops[m] += 1
        live[m] = False
    return order, [p > 1 for p in pops], len(queue)


def bounded_walk(members):
    """The same order and the same `twice` from a queue of at most two entries a member, level by level.  Returns (order, twice, stats)
    with stats = {"queue": entries, "levels": levels, "widest": entries of the widest level}."""
    at = _index(members)
    n = len(members)
    INF = 1 << 62
    first = [INF] * n
    cnt = [0] * n
    queue = [members[0]]
    first[0], cnt[0] = 0, 1
    order = [0]
    s, levels, widest = 0, 0, 1
    while s < len(queue):
        e = len(queue)
        levels += 1
        widest = max(widest, e - s)
        cand = []  # (key, k-mer, target) in key order
        for p in range(s, e):
            for j, y in enumerate(neighbours(queue[p])):
                t = at.get(y)
                if t is not None and first[t] >= p:
                    cand.append((8 * (p - s) + j, y, t))
        m1, m2 = {}, {}
        for key, _, t in cand:
            m1[t] = min(m1.get(t, INF), key)
        for key, _, t in cand:
            if key != m1[t]:
                m2[t] = min(m2.get(t, INF), key)
        had = {t: cnt[t] for t in m1}
        for key, y, t in cand:
            room = 2 - had[t]
            if (room >= 1 and key == m1[t]) or (room >= 2 and key == m2.get(t, INF)):
                if cnt[t] == 0:
                    first[t] = len(queue)
                    order.append(t)
                cnt[t] += 1
                queue.append(y)
        s = e
    return order, [c == 2 for c in cnt], {"queue": len(queue), "levels": levels, "widest": widest}
