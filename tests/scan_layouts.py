"""Designed sequence stores for the kernels that cut their work by base positions of the flattened store, not by sequences:
k_seq_cov (csrc/seq_cov.hip), k_cc_first (csrc/components.hip) and k_rs_count (csrc/reads_in_set.hip).  The cut is restated here in
plain Python from the constants below (tests/test_scan_layouts_model.py pins them to the sources):

    tile t starts at first + t * TILE, first = seq_offsets[0]; thread i of a tile at the tile's start + i * ITEMS; a wave is 64
    threads; "the sequence of p" is the greatest s with offsets[s] <= p; a sequence's index in a tile is j = s - s0, s0 the
    sequence of the tile's first position.

A layout is a list of sequence lengths behind a lead (the bases of the store in front of the first sequence that is handed over:
a sliced form drops the first m sequences from the offsets and keeps the store).  Every named layout is built for a cut, a k and a
shift = first % TILE (0: whole; 1, 7, 8, TILE - 1: sliced), its designed places relative to `first`, so the whole and the sliced
forms hold the same edges.  tests/test_scan_layouts_model.py checks that each layout holds what its name says,
tests/test_gpu_scan_edges.py holds the kernels to them.

Background: a genome of regions of 200 bases; table t counts region r mult(t, r) times (as reads that run k - 1 bases into the next
region, so a window's count is the multiplicity of the region it starts in).  Sequences with a window are drawn from regions in
turn, 37 apart: neighbours differ in multiplicity in every table and in membership of the reads-in-set set (the k-mers that start
in even regions)."""
import collections
import functools

import numpy as np

Cut = collections.namedtuple("Cut", "kernel tile items segs grid_cap")
LANES = 64
SEQ_COV = Cut("k_seq_cov", 2048, 8, 256, None)      # csrc/seq_cov.hip SC_THREADS * SC_ITEMS, SC_ITEMS, SC_SEGS
COMPONENTS = Cut("k_cc_first", 2048, 8, None, None)  # csrc/components.hip CC_THREADS * CC_ITEMS, CC_ITEMS
READS_IN_SET = Cut("k_rs_count", 32768, 32, None, 512)  # csrc/reads_in_set.hip RS_THREADS * RS_ITEMS, RS_ITEMS, grid_for(n_tiles, 1, 512)

SHIFTS = (0, 1, 7, 8, -1)  # first % TILE of the forms a layout is offered in (-1: TILE - 1); none but 0 is a multiple of 32
EMPTY_RUNS = (1, 2, 63, 64, 65, 300)
SEARCH_SEQS = (1, 2, 64, 65, 4096, 4097, 64 ** 3 + 1)

REGION = 200
N_REGIONS = 1800
DRAWN = 1100        # sequences are drawn from regions below this one (an even number: the turn's parity is the region's)
FRESH = 1700        # regions no drawn sequence reaches: content that occurs nowhere else
N_TABLES = 4
SEED = 20241107


# ---------------------------------------------------------------------------------------------------------------- the background

@functools.lru_cache(None)
def genome():
    return np.random.default_rng(SEED).integers(0, 4, N_REGIONS * REGION).astype(np.uint8)


def mult(t, r):
    """how often table t counts region r: four patterns, two of them with zeros"""
    return ((r % 13) + 1, (5 * r + 2) % 13, (7 * r + 4) % 11 + 1, (3 * r + 1) % 7)[t]


def table_reads(t, k):
    """(codes, offsets) of the reads table t counts: region r, k - 1 bases into the next, mult(t, r) times"""
    g = genome()
    reads = []
    for r in range(N_REGIONS):
        reads += [g[r * REGION:min((r + 1) * REGION + k - 1, len(g))]] * mult(t, r)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in reads])
    return np.concatenate(reads), off


class DumpedTable:
    """an oracle table for tests/seq_cov_model.store_coverage, its sorted dump made once"""

    def __init__(self, table):
        self.table, self._dump = table, table.dump()

    def dump(self):
        return self._dump


def pack_words(codes, pad=3):
    """base codes as 2-bit packed words, the first base in the top bits, `pad` zero words behind"""
    codes = np.asarray(codes, dtype=np.uint8)
    n = (len(codes) + 31) // 32
    c = np.zeros(n * 32, dtype=np.uint64)
    c[:len(codes)] = codes & 3
    sh = np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)
    words = np.zeros(n + pad, dtype=np.uint64)
    words[:n] = np.bitwise_or.reduce(c.reshape(-1, 32) << sh, axis=1)
    return words


def _extract(words, p, k):
    """(hi, lo) of the k-mers that start at the positions p of a packed store: 2k bits right-aligned in 128"""
    p = np.asarray(p, dtype=np.int64)
    q, r = p >> 5, ((p & 31) * 2).astype(np.uint64)
    a, b, c = words[q], words[q + 1], words[q + 2]
    inv = np.uint64(63) - r  # (x >> 1) >> (63 - r) is x >> (64 - r), and 0 at r = 0
    xh = (a << r) | ((b >> np.uint64(1)) >> inv)
    xl = (b << r) | ((c >> np.uint64(1)) >> inv)
    sh = 128 - 2 * k
    if sh >= 64:
        return np.zeros(len(p), dtype=np.uint64), xh >> np.uint64(sh - 64)
    return xh >> np.uint64(sh), (xh << np.uint64(64 - sh)) | (xl >> np.uint64(sh))


def oriented_windows(codes, k, starts=None):
    """(hi, lo) of the windows of one array of codes as they are read, at every start 0 .. len - k or at the given ones"""
    n = len(codes) - k + 1
    if starts is None:
        starts = np.arange(max(n, 0), dtype=np.int64)
    return _extract(pack_words(codes), starts, k)


def canonical_windows(codes, k):
    """(hi, lo) of every window's canonical form: the smaller of the k-mer and its reverse complement as 2k-bit numbers"""
    codes = np.asarray(codes, dtype=np.uint8)
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    p = np.arange(n, dtype=np.int64)
    fh, fl = _extract(pack_words(codes), p, k)
    rh, rl = _extract(pack_words(3 - codes[::-1]), len(codes) - k - p, k)
    fw = (fh < rh) | ((fh == rh) & (fl <= rl))
    return np.where(fw, fh, rh), np.where(fw, fl, rl)


@functools.lru_cache(None)
def member_set(k):
    """the reads-in-set set: the k-mers that start in even regions, as the library takes them (oriented hi, lo) and canonical"""
    g = genome()
    p = np.arange(len(g) - k + 1, dtype=np.int64)
    p = p[(p // REGION) % 2 == 0]
    hi, lo = oriented_windows(g, k, p)
    ch, cl = canonical_windows(g, k)
    return hi, lo, ch[p], cl[p]


@functools.lru_cache(None)
def _member_pairs(k):
    _, _, sh, sl = member_set(k)
    return set(zip(sh.tolist(), sl.tolist()))


def window_members(codes, k):
    """for every window of one array of codes: is it in member_set(k)?  Canonical and packed, looked up with np.isin; above
    k = 32 the few windows whose low word is in the set are compared in full"""
    _, _, sh, sl = member_set(k)
    ch, cl = canonical_windows(codes, k)
    sieve = np.zeros(1 << 24, dtype=bool)  # (most windows of a large store miss: a sieve on 24 low bits comes before np.isin)
    sieve[(sl & np.uint64(0xFFFFFF)).astype(np.int64)] = True
    member = sieve[(cl & np.uint64(0xFFFFFF)).astype(np.int64)]
    at = np.nonzero(member)[0]
    member[at] = np.isin(cl[at], sl)
    if k > 32:
        full = _member_pairs(k)
        at = np.nonzero(member)[0]
        member[at] = [x in full for x in zip(ch[at].tolist(), cl[at].tolist())]
    return member


def reads_in_set_hits(codes, offsets, k, member=None):
    """the vectorised model of mc_reads_in_set's hits over member_set(k): windows 0 .. L - k - 1 of every read (ReadsFilter never
    tests the last one)"""
    offsets = np.asarray(offsets).astype(np.int64)
    member = window_members(codes, k) if member is None else member
    csum = np.zeros(len(codes) + 1, dtype=np.int64)
    csum[1:len(member) + 1] = np.cumsum(member)
    csum[len(member) + 1:] = csum[len(member)]
    b, e = offsets[:-1], offsets[1:]
    return (csum[np.maximum(e - k, b)] - csum[b]).astype(np.uint32)


def reads_in_set_keep(hits, offsets, k, pct):
    """kmersFiltration: a read longer than k with hits >= max(1, (L - k + 1) * pct / 100)"""
    n = np.diff(np.asarray(offsets).astype(np.int64))
    return (n > k) & (hits.astype(np.int64) >= np.maximum(1, (n - k + 1) * pct // 100))


# ------------------------------------------------------------------------------------------------------------------- a layout

class Layout:
    """lengths: every sequence of the store, the m dropped ones first.  offsets: what the kernel is handed (absolute positions)."""

    def __init__(self, name, purpose, cut, k, lengths, m, given):
        self.name, self.purpose, self.cut, self.k, self.m = name, purpose, cut, k, m
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.all_offsets = np.zeros(len(lengths) + 1, dtype=np.uint64)
        self.all_offsets[1:] = np.cumsum(self.lengths)
        self.offsets = self.all_offsets[m:]
        self.first, self.end = int(self.offsets[0]), int(self.offsets[-1])  # the lead, and the store's end
        self.n_seqs = len(self.offsets) - 1
        self.n_tiles = -(-(self.end - self.first) // cut.tile)
        self._given = given
        self._ioff = self.offsets.astype(np.int64)

    # -- the cut
    def tile_start(self, t):
        return self.first + t * self.cut.tile

    def tile_of(self, p):
        return (p - self.first) // self.cut.tile

    def thread_of(self, p):
        return (p - self.first) % self.cut.tile // self.cut.items

    def lane_of(self, p):
        return self.thread_of(p) % LANES

    def wave_of(self, p):
        return self.thread_of(p) // LANES

    def seq_of(self, p):
        """the greatest s with offsets[s] <= p (p in first .. end - 1), counted from the first sequence handed over"""
        return int(np.searchsorted(self._ioff[:-1], p, side="right")) - 1

    def s0(self, t):
        return self.seq_of(self.tile_start(t))

    def j_of(self, s, t):
        return s - self.s0(t)

    def starts(self):
        """the start positions of the sequences handed over"""
        return self._ioff[:-1]

    def lens(self):
        return self.lengths[self.m:]

    # -- the content
    @functools.cached_property
    def codes(self):
        """the whole store: sequences with a window from regions in turn (37 apart), shorter ones from turns of their own"""
        g = genome()
        out = np.zeros(int(self.all_offsets[-1]), dtype=np.uint8)
        turn = short = 0
        for i, n in enumerate(self.lengths.tolist()):
            if n == 0:
                continue
            b = int(self.all_offsets[i])
            if i in self._given:
                out[b:b + n] = self._given[i]
                continue
            if i < self.m:  # (the dropped sequences take no turn: every form of a layout holds the same sequences behind them)
                at = (700 + 2 * i) * REGION + 20
            elif n >= self.k:
                r = (turn * 37 + 11) % DRAWN
                at = r * REGION + (turn * 13) % 50
                turn += 1
            else:
                at = ((short * 53 + 7) % DRAWN) * REGION + (short * 29) % 150
                short += 1
            out[b:b + n] = g[at:at + n]
        return out

    def sequences(self):
        """the sequences handed over, as code arrays"""
        o = self._ioff
        return [self.codes[o[i]:o[i + 1]] for i in range(self.n_seqs)]


class _Builder:
    """positions are counted from `first`: the lead (the dropped sequences) is laid down before anything else"""

    def __init__(self, cut, k, shift):
        self.cut, self.k = cut, k
        shift = shift % cut.tile
        lead = {0: [], 1: [1], 7: [3, 4], 8: [8]}.get(shift, [k + 5, shift - (k + 5)])
        assert sum(lead) == shift
        self.lens, self.m, self.given, self.pos, self._fill = list(lead), len(lead), {}, 0, 0
        self.span = min(max(cut.tile // 50, 8), 147 - k)  # (a filler stays inside the region it is drawn from: k + 3 .. 149 bases)

    def seq(self, n=None, codes=None):
        """one sequence; returns its number among the sequences handed over"""
        if codes is not None:
            self.given[len(self.lens)], n = codes, len(codes)
        self.lens.append(n)
        self.pos += n
        return len(self.lens) - 1 - self.m

    def empties(self, n):
        self.lens += [0] * n

    def ones(self, n):
        for _ in range(n):
            self.seq(1)

    def pad_to(self, target):
        """sequences of k + 3 bases and more up to `target`: the last one takes what is left (it is short when the gap is)"""
        gap, lo = target - self.pos, self.k + 3
        assert gap >= 0, (target, self.pos)
        while gap > 0:
            n = lo + (self._fill * 7) % self.span
            self._fill += 1
            if gap - n < lo:
                n = gap
            self.seq(n)
            gap -= n

    def burn(self, count, span):
        """exactly `count` sequences over exactly `span` positions: a covered one, then empty and one-base ones"""
        assert count >= 1 and span >= self.k + 3, (count, span)
        ones = min(count - 1, 200, span - (self.k + 3))
        rest = count - 1 - ones
        self.seq(span - ones)
        self.empties(rest // 2)
        self.ones(ones)
        self.empties(rest - rest // 2)


def _covered(b):
    return b.seq(2 * b.k + 7)


def _edge_at_tile(b):
    T, k = b.cut.tile, b.k
    for at in (T, 2 * T - 1, 3 * T + 1):      # a boundary on a tile's start, one base before it, one after
        b.pad_to(at)
        _covered(b)
    for at in (4 * T - (k - 1), 5 * T - k, 6 * T - 1):  # windows that start in one tile and read the next
        b.pad_to(at)
        _covered(b)                            # (and the last sequence ends on the store's last position)


def _edge_at_unit(b, unit):
    """boundaries on the first position of a thread (unit = ITEMS) or a wave (64 * ITEMS) and beside it; a thread of ITEMS one-base
    sequences; a thread whose run touches three sequences"""
    T, I, k = b.cut.tile, b.cut.items, b.k
    first_unit = 5 if unit == I else 1
    gap = -(-(4 * k + 20) // unit)
    for n, d in ((0, 0), (1, -1), (2, 1)):
        b.pad_to(T + (first_unit + n * max(gap, 1)) * unit + d)
        _covered(b)
    b.pad_to(2 * T + 9 * I)
    b.ones(I)
    pt = 2 * T + 77 * I
    b.pad_to(pt + 1 - (2 * k + 7))
    _covered(b)                     # ends on the thread's first position
    if k <= I - 2:
        b.seq(k)                    # wholly inside the thread's run
    else:
        b.seq(I - 2)                # (k bases do not fit a run: the middle one has no window ...
    _covered(b)
    for _ in range(3):              # ... and three sequences of exactly k bases follow, one window each)
        b.seq(k)
    b.pad_to(3 * T)


def _empties(b, run):
    T, I = b.cut.tile, b.cut.items
    b.empties(run)                  # at position 0 of what is handed over
    _covered(b)
    b.pad_to(T)
    b.empties(run)                  # at a tile's first position
    _covered(b)
    b.pad_to(2 * T + 11 * I + I // 2)
    b.empties(run)                  # in the middle of a thread's run
    _covered(b)
    b.pad_to(3 * T - 5)
    _covered(b)
    b.empties(run)                  # behind the last base


def _long_over_tiles(b):
    T = b.cut.tile
    b.pad_to(T // 2 + 3)
    b.seq(3 * T + T // 2)
    b.pad_to(4 * T + T // 2 + 3)


def _lds_entries(b, form):
    T, k = b.cut.tile, b.k
    b.pad_to(T)
    if form == "ones":
        b.ones(255)                 # j = 0 .. 254
    else:
        b.seq(1)                    # j = 0, and 254 empty sequences behind it: j = 1 .. 254
        b.empties(254)
    for _ in range(3):
        b.seq(100)                  # j = 255, 256, 257
    b.pad_to(2 * T)
    b.seq(1)                        # j = 0 .. 252 on one position
    b.empties(252)
    for _ in range(8):
        b.seq(k + 3)                # j = 253 .. 260, a few threads each: one wave holds last runs on both sides of the 256th
    b.pad_to(3 * T - 20)
    b.seq(2 * k + 27)               # runs on into the next tile: j = 0 there


def search_step(n):
    return -(-n // 64)


def search_marks(n):
    """the numbers of the two sequences on both sides of a multiple of the search's first step (n >= 64)"""
    step = search_step(n)
    a = 16 * step - 1 if step > 1 else n // 2 - 1
    return a, a + 1


def _search_rounds(b, n):
    T, k = b.cut.tile, b.k
    if n == 1:
        b.seq(2 * T + T // 2)
    elif n == 2:
        b.seq(T + T // 2)
        b.seq(T + T // 2)
    else:
        a, _ = search_marks(n)
        b.seq(T + T // 2)                        # number 0: tiles 0 and 1 start in it
        b.burn(a - 1, 2 * T - 5 - b.pos)
        assert b.seq(T - 2) == a                 # tile 2 starts in it
        b.seq(k + 16)                            # number a + 1: tile 3 starts in it
        b.burn(n - 2 - (a + 1), 4 * T - 9 - b.pos)
        assert b.seq(T // 2) == n - 1            # the last sequence: tile 4 starts in it


def _tails(b, kind):
    T, I, k = b.cut.tile, b.cut.items, b.k
    if kind in ("tiles", "tiles_plus1", "tiles_minus1"):
        b.pad_to(2 * T + {"tiles": 0, "tiles_plus1": 1, "tiles_minus1": -1}[kind])
    elif kind == "few":
        b.seq(2)
        b.empties(1)
        b.seq(I - 3)                # fewer than ITEMS positions
    else:
        b.seq({"lt_k": k - 1, "k": k, "k_plus1": k + 1}[kind])


def _fresh(region, n):
    return genome()[region * REGION:region * REGION + n]


def _repeats(b):
    T, I, k = b.cut.tile, b.cut.items, b.k
    unit = _fresh(FRESH, 7)
    rep = np.concatenate([unit] * (k // 7 + 4))[:k + 14]  # period 7: the window at 0 is the window at 7
    for t, i in ((1, 3), (3, 5), (5, 7)):                  # in three tiles, on a thread's first position
        b.pad_to(t * T + i * I)
        b.seq(codes=rep)
    b.pad_to(7 * T - 3)
    b.seq(codes=_fresh(FRESH + 10, 2 * k + 7))            # a component whose first window straddles a tile edge
    b.pad_to(7 * T + 40 * I)
    b.empties(3)
    b.seq(codes=_fresh(FRESH + 20, 2 * k))                # a seed behind empty sequences
    b.pad_to(7 * T + 80 * I)
    b.seq(codes=_fresh(FRESH + 30, 2 * k))                # a seed in the last sequence that has bases
    b.empties(3)


PURPOSES = {
    "edge_at_tile": "sequence boundaries on a tile's start and one base off it; sequences that start k - 1, k and 1 bases before a tile's end",
    "edge_at_thread": "boundaries on a thread's first position and one base off it; ITEMS one-base sequences in one thread; three sequences in one thread's run",
    "edge_at_wave": "the same boundaries on a wave's first position",
    "long_over_tiles": "one sequence over 3.5 tiles: whole tiles and waves inside it, short sequences behind",
    "lds_entries": "sequences 255, 256 and 257 of a tile covered side by side; one wave with last runs on both sides of the 256th",
    "lds_entries_empties": "the same behind 254 empty sequences on one position",
    "repeats": "one k-mer in three tiles and twice in a thread's run; a component whose first window straddles a tile edge; seeds beside empty sequences",
}
PURPOSES.update({"empties_%d" % r: "runs of %d empty sequences at position 0, at a tile's start, inside a thread's run and behind the last base" % r
                 for r in EMPTY_RUNS})
PURPOSES.update({"search_rounds_%d" % n: "%d sequences: tiles start in the first, the last and on both sides of a step of the 64-ary search" % n
                 for n in SEARCH_SEQS})
PURPOSES.update({"tails_" + t: "a store of " + d for t, d in (
    ("tiles", "two whole tiles"), ("tiles_plus1", "two tiles and one position"), ("tiles_minus1", "two tiles less one position"),
    ("few", "fewer than ITEMS positions"), ("lt_k", "k - 1 positions"), ("k", "k positions"), ("k_plus1", "k + 1 positions"))})

SMALL = tuple(PURPOSES)                 # every layout but many_tiles
SEQ_COV_LAYOUTS = tuple(n for n in SMALL if n != "repeats")
COMPONENTS_LAYOUTS = tuple(n for n in SMALL if not n.startswith("lds_entries"))
READS_IN_SET_LAYOUTS = SMALL


@functools.lru_cache(None)
def layout(name, cut, k, shift=0):
    b = _Builder(cut, k, shift)
    if name == "edge_at_tile":
        _edge_at_tile(b)
    elif name == "edge_at_thread":
        _edge_at_unit(b, cut.items)
    elif name == "edge_at_wave":
        _edge_at_unit(b, cut.items * LANES)
    elif name.startswith("empties_"):
        _empties(b, int(name[8:]))
    elif name == "long_over_tiles":
        _long_over_tiles(b)
    elif name.startswith("lds_entries"):
        _lds_entries(b, "empties" if name.endswith("_empties") else "ones")
    elif name.startswith("search_rounds_"):
        _search_rounds(b, int(name[14:]))
    elif name.startswith("tails_"):
        _tails(b, name[6:])
    elif name == "repeats":
        _repeats(b)
    else:
        raise KeyError(name)
    return Layout(name, PURPOSES[name], cut, k, b.lens, b.m, b.given)


def forms(name, cut, k):
    """the layout whole and in its four sliced forms"""
    return [layout(name, cut, k, s) for s in SHIFTS]


# ------------------------------------------------------------------------------------------------------------------ many_tiles

ManyTiles = collections.namedtuple("ManyTiles", "codes offsets planted")  # planted: {what: (read, position of the window)}


@functools.lru_cache(2)
def many_tiles(k):
    """reads-in-set only: more tiles than the grid's 512 workgroups, so the grid-stride loop runs twice in some of them.  Random
    bases (no member among them), a few long reads and many short ones, and members of the set planted at chosen places."""
    cut = READS_IN_SET
    T, I = cut.tile, cut.items
    rng = np.random.default_rng(SEED + k)
    short = lambda n: rng.integers(k + 2, 301, n)  # noqa: E731
    lengths = np.concatenate([[3 * T + 17], short(30000), [150 * T + 555], short(20000), [5 * T + 1234], short(20000), [2 * T + 99], short(3000)]).astype(np.int64)
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    o = off.astype(np.int64)
    n_tiles = -(-int(o[-1]) // T)
    assert n_tiles > cut.grid_cap + 2
    codes = rng.integers(0, 4, int(o[-1])).astype(np.uint8)
    g = genome()
    planted = {}

    def plant(what, p, region):
        """the k bases of a member (region is even) at p .. p + k - 1"""
        src = region * REGION + 50
        codes[p:p + k] = g[src:src + k]
        codes[p - 1], codes[p + k] = (g[src - 1] + 1) & 3, (g[src + k] + 1) & 3  # (the windows beside it are no members)
        planted[what] = (int(np.searchsorted(o[:-1], p, side="right")) - 1, p)

    def room(p):
        """the first position at or behind p whose window lies inside one read with a base to spare"""
        while True:
            s = int(np.searchsorted(o[:-1], p, side="right")) - 1
            if p + k < o[s + 1]:
                return p
            p = int(o[s + 1])
    plant("tile 0", room(1000), 2)
    plant("tile 511", room(511 * T + 77), 4)
    plant("tile 512", room(512 * T + 5), 6)
    p = room((n_tiles - 1) * T + 3)
    assert p + k < o[-1] - 400
    plant("last tile", p, 8)
    plant("a thread's last position", room(200 * T) // I * I + I - 1, 10)
    s = int(np.searchsorted(o[:-1], 515 * T, side="right"))
    plant("straddling a boundary", int(o[s + 1]) - k // 2, 12)   # must not count
    plant("a read's last window", int(o[s + 4]) - k, 14)         # must not count
    return ManyTiles(codes, off, planted)
