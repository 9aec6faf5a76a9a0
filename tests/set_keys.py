"""Designed key sets for the four units that build an exact open-addressing set of k-mers for one call and probe it: reads_in_set.hip
(k_rs_build / rs_in_table), unitigs.hip (k_ut_build / ut_find), env_join.hip (k_ej_build / ej_row) and trim_paths.hip (k_tp_build /
tp_find).  Test infrastructure only, with no test of its own: tests/test_set_keys_model.py pins the restatements below to
csrc/kmer_set.h (compiled as host C++) and holds every named set to its name, tests/test_gpu_set_keys.py sends the sets through the C ABI.

Restated here over numpy arrays (uint64 words, 32-bit arithmetic masked): rs_key, rs_hash, rs_home, the trim's tp_home, the reverse
complement and the smaller-of-two rule, the size rule lg_cap(n), reads-in-set's filter word and bits.  Base codes A 0, G 1, C 2, T 3,
the first base most significant, as everywhere in tests/.

A named set is a crowd of isolated k-mers whose homes lie in the last slots of the table, so that linear probing makes ONE run of
occupied slots that passes slot cap - 1 and goes on at slot 0, beside the unit's own shapes (some of whose entries fall into the run)
and with designed look-ups: present members of the crowd, and absent keys whose home is the run's first slot, which a look-up can
refuse only after it has walked the whole run and the wrap.  Each look-up arrives the way its unit looks keys up: a window of a read
(reads-in-set), a gene window or a record (join), a neighbour string of a `carrier` entry (unitigs, trim)."""
import functools
import random
import types

import numpy as np

from tests import env_join_model as ejm
from tests import trim_paths_model as tm
from tests import unitigs_model as um

READS_IN_SET, UNITIGS, ENV_JOIN, TRIM_PATHS = UNITS = ("reads_in_set", "unitigs", "env_join", "trim_paths")
LETTERS = "AGCT"
LG_CAP_MIN = 6                 # every unit: int lg_cap = 6; while ((1ull << lg_cap) < 2 * n) lg_cap++;
RS_FILTER_WORDS_LG = 14        # reads_in_set.hip

_U = np.uint64
_M32 = _U(0xFFFFFFFF)
_LUT = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate(LETTERS):
    _LUT[ord(_c)] = _i
_BYTES = np.frombuffer(LETTERS.encode(), dtype=np.uint8)


# ---- strings, codes, words

def codes_of(strings, k):
    """(n, k) uint8 codes of n strings of k letters"""
    if not len(strings):
        return np.zeros((0, k), dtype=np.uint8)
    assert all(len(s) == k for s in strings)
    return _LUT[np.frombuffer("".join(strings).encode(), dtype=np.uint8).reshape(-1, k)]


def text_of(codes):
    return [row.tobytes().decode() for row in _BYTES[codes]]


def rc_codes(codes):
    return (3 - codes[:, ::-1]).astype(np.uint8)


_COMPLEMENT = str.maketrans("AGCT", "TCGA")


def rc(s):
    return s.translate(_COMPLEMENT)[::-1]


def pack(codes):
    """(hi, lo) of (n, k) codes: 2k bits right-aligned in 128"""
    n, k = codes.shape
    hi, lo = np.zeros(n, dtype=_U), np.zeros(n, dtype=_U)
    for j in range(k):
        if j < k - 32:
            hi = (hi << _U(2)) | codes[:, j]
        else:
            lo = (lo << _U(2)) | codes[:, j]
    return hi, lo


def smaller_is_forward(fhi, flo, rhi, rlo):
    """rs_key's rule (and ut_le / ej_le): the forward k-mer stands for both when it is not the larger 2k-bit number"""
    return (fhi < rhi) | ((fhi == rhi) & (flo <= rlo))


def _rev_pairs(x):
    """the 32 two-bit groups of every word in reverse order"""
    x = ((x >> _U(2)) & _U(0x3333333333333333)) | ((x & _U(0x3333333333333333)) << _U(2))
    x = ((x >> _U(4)) & _U(0x0F0F0F0F0F0F0F0F)) | ((x & _U(0x0F0F0F0F0F0F0F0F)) << _U(4))
    return x.byteswap()


def rc_words(hi, lo, k):
    """the reverse complement of packed k-mers: the complemented 128 bits with their base order turned, moved down to 2k bits"""
    rhi, rlo = _rev_pairs(~lo), _rev_pairs(~hi)
    sh = 128 - 2 * k
    if sh >= 64:
        return np.zeros(len(lo), dtype=_U), (rhi >> _U(sh - 64)) if sh < 128 else np.zeros(len(lo), dtype=_U)
    if sh == 0:
        return rhi, rlo
    return rhi >> _U(sh), (rlo >> _U(sh)) | (rhi << _U(64 - sh))


def random_words(rng, n, k):
    """n random packed k-mers"""
    lo = rng.integers(0, 1 << 63, n, dtype=np.uint64) * _U(2) + rng.integers(0, 2, n, dtype=np.uint64)
    hi = rng.integers(0, 1 << 63, n, dtype=np.uint64) * _U(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if k <= 32:
        return np.zeros(n, dtype=_U), lo >> _U(64 - 2 * k)
    return hi >> _U(128 - 2 * k), lo


def unpack(hi, lo, k):
    """packed k-mers as strings"""
    out = []
    for h, l in zip(hi.tolist(), lo.tolist()):
        v = (h << 64) | l
        out.append("".join(LETTERS[(v >> (2 * (k - 1 - i))) & 3] for i in range(k)))
    return out


# ---- csrc/kmer_set.h

def rs_key(k, fhi, flo, rhi, rlo):
    """(a, b) of the canonical k-mer"""
    if k <= 32:
        return np.minimum(flo, rlo), np.zeros(len(flo), dtype=_U)
    f = smaller_is_forward(fhi, flo, rhi, rlo)
    hi, lo = np.where(f, fhi, rhi), np.where(f, flo, rlo)
    return (hi << _U(1)) | (lo >> _U(63)), lo & _U(0x7FFFFFFFFFFFFFFF)


def rs_hash(a, b, wide):
    a, b = np.asarray(a, dtype=_U), np.asarray(b, dtype=_U)
    h = (a & _M32) ^ (((a >> _U(32)) * _U(0x85ebca6b)) & _M32)
    if wide:
        h = h ^ (((b & _M32) * _U(0xc2b2ae35)) & _M32) ^ (((b >> _U(32)) * _U(0x27d4eb2f)) & _M32)
    h = h ^ (h >> _U(16))
    h = (h * _U(0x7feb352d)) & _M32
    h = h ^ (h >> _U(15))
    h = (h * _U(0x846ca68b)) & _M32
    return h ^ (h >> _U(16))


def rs_home(h, lg_cap):
    return ((np.asarray(h, dtype=_U) * _U(0x9e3779b1)) & _M32) >> _U(32 - lg_cap)


def tp_home(k, hi, lo, lg_cap):
    """trim_paths.hip: rs_home(rs_hash<WIDE>(RsKey{v.lo, v.hi}), lg_cap) on the ORIENTED words, WIDE from k = 33 on"""
    return rs_home(rs_hash(lo, hi, k >= 33), lg_cap)


def lg_cap(n):
    lg = LG_CAP_MIN
    while (1 << lg) < 2 * n:
        lg += 1
    return lg


def rs_filter_word(h):
    return np.asarray(h, dtype=_U) >> _U(32 - RS_FILTER_WORDS_LG)


def rs_filter_bits(h):
    h = np.asarray(h, dtype=_U)
    one = _U(1)
    return (one << (h & _U(63))) | (one << ((h >> _U(6)) & _U(63))) | (one << ((h >> _U(12)) & _U(63)))


def key_of_codes(codes):
    """(a, b, forward is canonical) of (n, k) codes"""
    k = codes.shape[1]
    fhi, flo = pack(codes)
    rhi, rlo = pack(rc_codes(codes))
    a, b = rs_key(k, fhi, flo, rhi, rlo)
    return a, b, smaller_is_forward(fhi, flo, rhi, rlo)


def hash_of_codes(codes, unit):
    k = codes.shape[1]
    if unit == TRIM_PATHS:
        hi, lo = pack(codes)
        return rs_hash(lo, hi, k >= 33)
    a, b, _ = key_of_codes(codes)
    return rs_hash(a, b, k > 32)


def homes_of_codes(codes, unit, lg):
    return rs_home(hash_of_codes(codes, unit), lg).astype(np.int64)


def homes(strings, k, unit, lg):
    return homes_of_codes(codes_of(strings, k), unit, lg)


# ---- the slot model

def occupied(home_list, lg):
    """Linear probing of 2^lg slots: which slots hold a key after keys with these homes went in -- the same set in whatever order they
    went (as tests/crowded_tables.py says of its table).  Returns slots (bool a slot), runs [(first slot, length)] with a run that
    passes cap - 1 -> 0 counted once, longest, wraps (such a run exists), run_of(slot) and visits(home): the number of slots that a
    look-up of an ABSENT key of that home reads, the free slot that ends it included."""
    cap = 1 << lg
    mask = cap - 1
    occ = np.zeros(cap, dtype=bool)
    for h in home_list:
        s = int(h)
        while occ[s]:
            s = (s + 1) & mask
        occ[s] = True
    assert not occ.all()
    free = int(np.nonzero(~occ)[0][0])
    runs, at, i = [], None, 1
    while i <= cap:  # one turn from a free slot on
        s = (free + i) & mask
        if occ[s]:
            if at is None:
                at = [s, 0]
            at[1] += 1
        elif at is not None:
            runs.append(tuple(at))
            at = None
        i += 1
    assert at is None

    def run_of(slot):
        for first, length in runs:
            if (slot - first) & mask < length:
                return first, length
        return None

    def visits(home):
        r = run_of(home)
        return 1 if r is None else r[1] - ((home - r[0]) & mask) + 1

    wrapping = [r for r in runs if r[0] + r[1] > cap]
    return types.SimpleNamespace(lg=lg, cap=cap, slots=occ, runs=runs, longest=max([r[1] for r in runs] or [0]), wraps=bool(wrapping),
                                 wrapping=wrapping[0] if wrapping else None, run_of=run_of, visits=visits)


# ---- neighbours on both strands

def neighbour_map(strings, k):
    """entry -> the set of other entries that follow or precede it on either strand (share k - 1 bases end to start)"""
    by_prefix = {}
    for i, s in enumerate(strings):
        for t in (s, rc(s)):
            by_prefix.setdefault(t[:k - 1], set()).add(i)
    out = {}
    for i, s in enumerate(strings):
        near = set()
        for t in (s, rc(s)):
            near |= by_prefix.get(t[1:], set())
        out[i] = near - {i}
    return out


# ---- candidates

def _family_codes(rng, n, k, family):
    """n random k-mers; family = ("first", prefix codes, top bit) fixes the first 2k - 63 bits, the first base A and the last not T
    (the forward strand is then the canonical one); ("low", suffix codes) fixes the last 32 bases"""
    c = rng.integers(0, 4, (n, k), dtype=np.uint8)
    if family is None:
        return c
    if family[0] == "first":
        c[:, :k - 32] = family[1]
        c[:, k - 32] = 2 * family[2] + (c[:, k - 32] & 1)
        c[:, -1] = rng.integers(0, 3, n, dtype=np.uint8)
    else:
        c[:, k - 32:] = family[1]
    return c


def _with_home(rng, k, unit, lg, family, lo_slot, width, want, taken):
    """`want` distinct candidate strings whose home lies in [lo_slot, lo_slot + width), none of them in `taken`"""
    cap = 1 << lg
    out, seen = [], set(taken)
    space = None if family is None else (4 ** 31 if family[0] == "first" else 4 ** (k - 32))
    for _ in range(60):
        n = min(max(4 * want * cap // width, 4096), 400000)
        c = _family_codes(rng, n, k, family)
        h = homes_of_codes(c, unit, lg)
        for s in text_of(c[(h >= lo_slot) & (h < lo_slot + width)]):
            key = s if unit == TRIM_PATHS else min(s, rc(s))
            if key not in seen and s != rc(s):
                seen.add(key)
                out.append(s)
                if len(out) == want:
                    return out
        if space is not None and space <= 4096:
            break  # (a family of a handful of k-mers: every one has been seen)
    return out


def _low_word_at_k_33(rng, lg, w0, width):
    """32 bases S such that, of the four 33-mers that end in S, one has its home at w0 and two others theirs from w0 on (by tp_home)"""
    for _ in range(20):
        s = rng.integers(0, 4, (200000, 32), dtype=np.uint8)
        h = np.stack([homes_of_codes(np.concatenate([np.full((len(s), 1), c, dtype=np.uint8), s], axis=1), TRIM_PATHS, lg) for c in range(4)])
        good = np.nonzero(((h == w0).sum(axis=0) == 1) & ((h > w0).sum(axis=0) >= 2))[0]
        if len(good):
            return s[good[0]]
    raise AssertionError("no shared low word at k = 33")


# ---- the units' shapes

def _shape(unit, k, seed, big, exact):
    """the unit's own shapes: entries (oriented strings) and what the unit needs beside them"""
    if exact is not None:  # a chain of exactly that many entries
        text = um.random_chain(random.Random(seed), exact, k)
        w = um.windows(text, k)
        if unit == TRIM_PATHS:
            return types.SimpleNamespace(entries=w, last=[1 if i == exact // 3 else 0 for i in range(exact)])
        if unit == UNITIGS:
            return types.SimpleNamespace(entries=w, cls=[0] * exact)
        if unit == ENV_JOIN:
            return types.SimpleNamespace(entries=w, graphs=[{x: 3 + i % 5 for i, x in enumerate(w)}, {}, {rc(x): 9 for x in w[::2]}])
        return types.SimpleNamespace(entries=w, reads=[text])
    if unit == TRIM_PATHS:
        rng = np.random.default_rng(seed)
        kmers, last, _ = tm.fork(rng, k, stem=20, arm=15)
        if big:
            more, more_last = tm.chain(rng, k, 2400)
            kmers, last = kmers + more, last + more_last
        return types.SimpleNamespace(entries=kmers, last=last)
    if unit == UNITIGS:
        kmers, cls = um.mixed_set(seed, k, (1, 2, 3, 64, 65) if big else (1, 2, 3))
        if big:  # ... beside one chain of 2200 entries, as tests/test_gpu_unitigs.py puts its long chain beside the mixed set
            rng = random.Random(seed + 1)
            have = {min(w, rc(w)) for w in kmers}
            more = [w for w in um.shuffled(rng, um.windows(um.random_chain(rng, 2200, k), k)) if min(w, rc(w)) not in have]
            kmers, cls = kmers + more, cls + [0] * len(more)
        return types.SimpleNamespace(entries=kmers, cls=cls)
    if unit == ENV_JOIN:
        if big:
            texts, _ = ejm.contig_environments(k, 3, 2400, seed=seed)
            graphs = [dict((l.split()[0], int(l.split()[1])) for l in t.decode().splitlines()) for t in texts]
        else:
            files, _ = ejm.designed_case(k, 3, seed)
            graphs = [ejm.graph_dict(lines) for lines in files]
        return types.SimpleNamespace(entries=ejm.entries_of(graphs), graphs=graphs)
    rng = random.Random(seed)  # reads-in-set: the windows of a few reads
    seqs = [um.random_chain(rng, 30, k) for _ in range(70 if big else 1)]
    return types.SimpleNamespace(entries=[w for s in seqs for w in um.windows(s, k)], reads=seqs)


def _canon(unit, s):
    """what makes two entries the same one: the oriented k-mer for the trim, the smaller strand for the units that fold the strands"""
    return s if unit == TRIM_PATHS else min(s, rc(s))


def _family(rng, kind, k):
    """what a family shares: None; ("first", the first k - 32 bases with A in front, the top bit of the next); ("low", the last 32 bases)"""
    if kind == "first":
        prefix = rng.integers(0, 4, k - 32, dtype=np.uint8)
        prefix[0] = 0
        return ("first", prefix, int(rng.integers(0, 2)))
    if kind == "low":
        return ("low", rng.integers(0, 4, 32, dtype=np.uint8))
    return None


def _choose_slots(shape, k, unit, m, n_total):
    """The table's size and the crowd's window [w0, cap): the last cap/16 slots, or fewer, so that m members make one run.  start: the
    run's first slot, w0 unless entries of the shape sit just in front of it.  Returns (lg, w0, width, start)"""
    lg = lg_cap(n_total)
    cap = 1 << lg
    width = min(cap >> 4, max(4, m // 4))
    w0 = cap - width
    start, there = w0, occupied(homes(shape.entries, k, unit, lg), lg).slots
    while there[(start - 1) & (cap - 1)] and w0 - start < width:
        start -= 1
    return lg, w0, width, start


def _draw(rng, k, unit, lg, family, w0, width, start, m, n_miss, taken):
    """(misses, crowd): absent k-mers at home in slot `start`, and m members at home in [w0, w0 + width) with one in w0 itself; both
    of the family where there is one.  None when this table does not give them.  The misses come first: a small family has few to give.
    (A low word at k = 33 is shared by four k-mers only: one miss serves, and k-mers outside the family fill the crowd.)"""
    tiny = family is not None and family[0] == "low" and k == 33
    misses = _with_home(rng, k, unit, lg, family, start, 1, n_miss + 2, taken)
    if len(misses) < (1 if tiny else n_miss):
        return None
    reserved = taken | {_canon(unit, s) for s in misses}
    crowd = _with_home(rng, k, unit, lg, family, w0, width, m, reserved)
    if tiny:
        crowd += _with_home(rng, k, unit, lg, None, w0, width, m - len(crowd), reserved | {_canon(unit, s) for s in crowd})
    assert len(crowd) == m, (k, unit, len(crowd))
    if not (homes(crowd, k, unit, lg) == w0).any():
        return None
    return misses, crowd


def _carriers(rng, sides, looked_up, k, unit, lg, guard, taken):
    """[(entry, side, the k-mer it looks up)] for every side and every k-mer x of looked_up: an entry whose right (side = +1) or left
    (-1) neighbour string is x, with its own home outside the guarded slots; None when one cannot be had"""
    out = []
    for side in sides:
        four = [[c + x[:-1] if side > 0 else x[1:] + c for c in LETTERS] for x in looked_up]
        at_home = homes([e for es in four for e in es], k, unit, lg).reshape(-1, 4) if four else []
        for x, es, hs in zip(looked_up, four, at_home):
            ok = [e for j in rng.permutation(4) for e in [es[j]]
                  if _canon(unit, e) not in taken and e != rc(e) and e != x and not guard(int(hs[j]))]
            if not ok:
                return None
            taken.add(_canon(unit, ok[0]))
            out.append((ok[0], side, x))
    return out


def _attempt(rng, name, k, unit, shape, family, m, exact_n, n_miss, n_hit, sides):
    """one shape, one table: the case, or None when a designed place does not come out (the caller takes another shape)"""
    designed_reads = unit == READS_IN_SET and exact_n is None  # (two reads around a designed miss each, see _reads_around)
    n_total = len(shape.entries) + m + len(sides) * (n_miss + n_hit) + (2 * 18 if designed_reads else 0)
    taken = {_canon(unit, s) for s in shape.entries}
    if len(taken) != len(shape.entries):
        return None
    lg, w0, width, start = _choose_slots(shape, k, unit, m, n_total)
    mask = (1 << lg) - 1
    if family is not None and family[0] == "low" and k == 33:
        if start != w0:
            return None
        family = ("low", _low_word_at_k_33(rng, lg, w0, width))
    drawn = _draw(rng, k, unit, lg, family, w0, width, start, m, n_miss, taken)
    if drawn is None:
        return None
    misses, crowd = drawn
    taken |= {_canon(unit, s) for s in misses + crowd}
    extra = []
    if designed_reads:
        extra, reads = _reads_around(rng, misses[:2], k)
        keys = {_canon(unit, s) for s in extra}
        if len(misses) < 3 or keys & taken or len(keys) != len(extra):
            return None
        shape.reads = shape.reads + reads
        taken |= keys
    # the run, by the slot model: it begins at `start`, and the unit's own entries reach into it
    own = shape.entries + extra
    run = occupied(homes(own + crowd, k, unit, lg), lg).run_of(w0)
    if run is None or run[0] != start:
        return None
    in_run = [s for s, h in zip(own, homes(own, k, unit, lg)) if (h - start) & mask < run[1]]
    if exact_n is None and len(in_run) < 3:
        return None
    # the look-ups: the members with the latest homes first; carriers keep clear of the run and of the slots beside it
    hc = homes(crowd, k, unit, lg)
    hits = [crowd[i] for i in np.argsort(-((hc - w0) & mask), kind="stable")[:n_hit]]
    guard = lambda h: (h - (start - 1)) & mask <= run[1] + 1
    miss_carriers = _carriers(rng, sides, (misses * n_miss)[:n_miss], k, unit, lg, guard, taken)
    hit_carriers = None if miss_carriers is None else _carriers(rng, sides, hits, k, unit, lg, guard, taken)
    if hit_carriers is None:
        return None
    entries = own + crowd + [e for e, _, _ in miss_carriers + hit_carriers]
    assert len(entries) == n_total and (exact_n is None or n_total == exact_n), (len(entries), n_total, exact_n)
    if occupied(homes(entries, k, unit, lg), lg).run_of(w0) != run:
        return None
    return types.SimpleNamespace(name=name, k=k, unit=unit, lg=lg, entries=entries, crowd=crowd, shape=shape, extra=extra, in_run=in_run,
                                 misses=misses, hits=hits, miss_carriers=miss_carriers, hit_carriers=hit_carriers, run=run, family=family)


def _build(name, k, unit, seed, m, kind=None, big=False, exact_n=None, n_miss=4, n_hit=None):
    """See the module's docstring.  kind: None, "first" or "low" (what the crowd and the misses share).  Returns a namespace:
      k, unit, name, lg, entries (oriented strings: shape, then crowd, then carriers), crowd, shape (the namespace of _shape),
      misses: absent k-mers whose home is the run's first slot (family sets: of the family), hits: crowd members that are looked up
      (all of them; two in half_full), the latest homes first,
      miss_carriers / hit_carriers: [(entry, side, the k-mer it looks up)] for unitigs and the trim,
      run: (first slot, length) of the crowd's run in the whole set's table, and the unit's inputs (see the unit's maker below).
    Every member is looked up unless the set's size is given: wherever the entries went in, the member in the run's last slot lies
    len(crowd) - width slots behind its home, so some look-up that must succeed probes that far."""
    rng = np.random.default_rng(seed)
    n_hit = m if n_hit is None else n_hit
    # carriers: none where reads, records and the gene bring the look-ups; right neighbours for unitigs; both sides for the trim
    # (at k = 33 a left carrier of a low-word family would follow all four of its k-mers)
    sides = () if unit in (READS_IN_SET, ENV_JOIN) else (1,) if unit == UNITIGS or (kind == "low" and k == 33) else (1, -1)
    family = _family(rng, kind, k)
    for attempt in range(200):
        n_shape = None if exact_n is None else exact_n - m - len(sides) * (n_miss + n_hit)
        shape = _shape(unit, k, 1000 * seed + attempt, big, n_shape)
        case = _attempt(rng, name, k, unit, shape, family, m, exact_n, n_miss, n_hit, sides)
        if case is not None:
            return case
    raise AssertionError("no %s at k = %d for %s" % (name, k, unit))


def _reads_around(rng, misses, k):
    """two reads of k + 19 bases (20 windows, 19 of them tested) with a designed miss as window 9: the other 18 tested windows become
    members, so the miss is its read's only member-free window, and at pct = 95 (threshold 19) it alone keeps the read out"""
    extra, reads = [], []
    for x in misses:
        left = "".join(LETTERS[c] for c in rng.integers(0, 4, 9))
        right = "".join(LETTERS[c] for c in rng.integers(0, 4, 10))
        read = left + x + right
        w = um.windows(read, k)
        assert len(w) == 20 and w[9] == x
        extra += w[:9] + w[10:19]
        reads.append(read)
    return extra, reads


# ---- the named sets

def _seed(name, k, unit, n=0):
    return 1 + ["run_wrap", "run_big", "shared_first_word", "shared_low_word", "half_full"].index(name) * 100003 + k * 101 + UNITS.index(unit) * 7 + n * 13


@functools.lru_cache(maxsize=None)
def run_wrap(k, unit):
    """45 isolated k-mers in the last slots: a run of at least 40 slots with at least 8 on each side of cap - 1 -> 0"""
    return _build("run_wrap", k, unit, _seed("run_wrap", k, unit), 45)


@functools.lru_cache(maxsize=None)
def run_big(k, unit):
    """the same at about 3000 entries (8192 slots) with a run of at least 300: no probe loop may have a small hidden bound"""
    return _build("run_big", k, unit, _seed("run_big", k, unit), 320, big=True)


@functools.lru_cache(maxsize=None)
def shared_first_word(k, unit):
    """45 canonical k-mers (k > 32) with one `a` and different `b` in one run; the absent keys are of the family too"""
    assert k > 32 and unit != TRIM_PATHS
    return _build("shared_first_word", k, unit, _seed("shared_first_word", k, unit), 45, kind="first")


@functools.lru_cache(maxsize=None)
def shared_low_word(k):
    """the trim's twin: oriented k-mers with one `lo` (their last 32 bases) and different `hi`, homes by tp_home.  At k = 33 only four
    k-mers end in one word: three (or fewer) are in the set beside a crowd of others, one is the absent key"""
    assert k > 32
    return _build("shared_low_word", k, TRIM_PATHS, _seed("shared_low_word", k, TRIM_PATHS), 45, kind="low")


HALF_FULL_N = (32, 33, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def half_full(k, unit, n):
    """exactly n entries, half of them a crowd at the wrap: load exactly 0.5 at n = 32, 64, 128 and the doubled table one entry on"""
    return _build("half_full", k, unit, _seed("half_full", k, unit, n), n // 2, exact_n=n, n_miss=2, n_hit=2)


@functools.lru_cache(maxsize=None)
def filter_pass(k):
    """reads-in-set's bit filter made to pass what the table must refuse.  members: 16 k-mers whose hashes name ONE of the filter's 2^14
    words, then the 18 windows around passers[0] (reads_case's designed read: at pct = 95 that window alone keeps its read out);
    passers: absent k-mers of that word whose three bits are all set by members; near: absent k-mers of that word with exactly one of
    their three bits not set.  Returns a namespace with entries, crowd (the 16), misses (passers, then near), word, bits (what the
    members set in that word), reads and pct."""
    rng = np.random.default_rng(4000 + k)
    hi, lo = random_words(rng, 3000000, k)
    rhi, rlo = rc_words(hi, lo, k)
    a, b = rs_key(k, hi, lo, rhi, rlo)
    h = rs_hash(a, b, k > 32)
    word = int(rs_filter_word(h[0]))
    at = np.nonzero((rs_filter_word(h) == _U(word)) & ((hi != rhi) | (lo != rlo)))[0]
    texts = list(dict.fromkeys(unpack(hi[at], lo[at], k)))
    assert len(texts) >= 100
    crowd, rest = texts[:16], texts[16:]
    own_bits = lambda xs: rs_filter_bits(hash_of_codes(codes_of(xs, k), READS_IN_SET))
    union = int(np.bitwise_or.reduce(own_bits(crowd)))
    missing = [bin(int(x) & ~union).count("1") for x in own_bits(rest)]
    passers = [s for s, m in zip(rest, missing) if m == 0][:8]
    near = [s for s, m in zip(rest, missing) if m == 1][:8]
    assert len(passers) >= 4 and len(near) >= 4
    extra, reads = _reads_around(rng, passers[:1], k)
    entries = crowd + extra
    assert len({min(s, rc(s)) for s in entries + passers + near}) == len(entries + passers + near)
    for i, s in enumerate(crowd + passers[1:] + near):
        reads.append((rc(s) if i % 3 == 1 else s) + LETTERS[i % 4])
    return types.SimpleNamespace(name="filter_pass", k=k, unit=READS_IN_SET, lg=lg_cap(len(entries)), entries=entries, crowd=crowd, extra=extra,
                                 misses=passers + near, passers=passers, near=near, hits=crowd, word=word, bits=union, reads=reads, pct=95)


# ---- what each unit is given

def reads_case(case, dup=None):
    """reads-in-set: (reads, members, pct).  The shape's reads (all their tested windows members, two of them with a designed miss as
    their only member-free window), one read a crowd member (every third on the other strand) and one a miss: k + 1 bases, one tested
    window, so `keep` at the threshold of 1 is the look-up's answer"""
    if case.name == "filter_pass":
        return list(case.reads), list(case.entries), case.pct
    reads = list(getattr(case.shape, "reads", []))
    for i, s in enumerate(case.crowd):
        reads.append((rc(s) if i % 3 == 1 else s) + LETTERS[i % 4])
    for i, s in enumerate(case.misses):
        reads.append((rc(s) if i % 2 else s) + LETTERS[i % 4])
    return reads, list(case.entries), 95


def join_case(case):
    """the join: (entries, graphs, gene).  The crowd goes into graphs 0 and 2 (there on the other strand), the gene is hits and misses
    in turn: every miss arrives as a gene window"""
    graphs = [dict(g) for g in case.shape.graphs]
    of_shape = set(case.shape.entries)
    own = [e for e in case.entries if e not in of_shape]
    for i, s in enumerate(own):
        if i % 3 != 1:
            graphs[0][s] = 1 + i % 7
        if i % 2 == 0 or i % 3 == 1:
            graphs[2][rc(s)] = 2 + i % 5
    gene = "".join(h + x for h, x in zip(case.hits, (case.misses * len(case.hits))[:len(case.hits)]))
    return list(case.entries), graphs, gene


def trim_case(case):
    """the trim: (kmers, last).  Every crowd member is `last`: a carrier is kept (dir = +1 for side +1, -1 for side -1) iff the look-up
    of its neighbour finds a member"""
    crowd = set(case.crowd)
    shape_last = dict(zip(case.shape.entries, case.shape.last))
    return list(case.entries), [1 if s in crowd else shape_last.get(s, 0) for s in case.entries]


def unitigs_case(case):
    """unitigs: (kmers, cls)"""
    cls = dict(zip(case.shape.entries, case.shape.cls))
    return list(case.entries), [cls.get(s, 0) for s in case.entries]
