"""Leaves composed record by record for the merge kernel of the counting pipeline (csrc/count_pipeline.h k_p3_dedup), so that each of
the paths its comments call rare is taken by design and not by luck (test infrastructure only; tests/test_gpu_dedup_leaves.py runs
the leaves, tests/test_dedup_leaves_model.py pins this file to the C code and checks that every leaf meets its condition).

A record is a run of 1 to 16 consecutive windows of a locus of tests/crowded_tables.py: k - 15 random bases, the 15-mer M_INTERIOR,
k - 15 random bases, every window of which has that 15-mer for its minimizer.  Its bin word is sk_bin(sk_order(M)), so all records of
all loci fall into one leaf whatever the table's size, and a look-up finds their keys in that leaf's region.  The layout of a record
and the key of its window j are restated from the comment above SK_MAX_WINDOWS and from sk_window_key; dd_hash, the tag and the home
place in the kernel's record table from csrc/kmer_hash.h and the kernel's phase A.

What the kernel does with a leaf follows from numbers this file computes from the design alone:
  records     how many the leaf holds: above DD_MAX_CAP the general kernel takes it; above D2_SLOTS phase A takes several turns
  distinct    records that differ: above D2_SLOTS some find no place in the record table (add_plain)
  units       pairs of windows of the distinct records that have a place: above D2_UL_CAP phase B takes several rounds
  max_copies  the greatest number of copies of one record (the 13-bit field of the tag word)
  max_count   the greatest count a key reaches (the 17-bit packed counter)
"""
import numpy as np

from tests import crowded_tables as ct

SK_MAX_WINDOWS = 16
D2_SLOTS = 1024      # places of the record table
D2_UL_CAP = 1976     # units of one round
DD_MAX_CAP = 4096    # records of a leaf the dedup kernel takes
DD_PROBES = 8
K_FROM, K_TO = 23, 31

_U64 = np.uint64
_M32 = _U64(0xFFFFFFFF)


def bin_of(m):
    """the bin word of the records whose minimizer is the 15-mer m"""
    canon = min(int(m), int(ct.rc_mmer(np.array([m]))[0]))
    return int(ct.sk_bin(ct.sk_order(np.array([canon])))[0])


def leaf_of(bin_word, n_leaves):
    return (int(bin_word) * int(n_leaves)) >> 32


# ---------------------------------------------------------------------------------------------------- records
def records(codes, n_windows, bin_word, k):
    """codes: uint8 [n, 46], the bases of n records left-aligned (a record of w windows holds w + k - 1 bases, the tail is cleared
    here); n_windows [n]; -> (lo, hi) uint64 arrays"""
    c = np.array(codes, dtype=np.uint64).reshape(-1, SK_MAX_WINDOWS + 30)
    nw = np.asarray(n_windows, dtype=np.uint64).reshape(-1)
    assert (nw >= 1).all() and (nw <= SK_MAX_WINDOWS).all() and K_FROM <= k <= K_TO
    c[np.arange(c.shape[1])[None, :] >= (nw[:, None] + _U64(k - 1))] = 0
    hi = (nw - _U64(1)) << _U64(60)
    for i in range(30):
        hi |= c[:, i] << _U64(2 * (29 - i))
    lo = np.full(len(nw), int(bin_word), dtype=np.uint64)
    for i in range(30, 46):
        lo |= c[:, i] << _U64(32 + 2 * (45 - i))
    return lo, hi


def record(codes, n_windows, bin_word, k=31):
    """one record from its n_windows + k - 1 bases: (lo, hi) as ints"""
    codes = np.asarray(codes, dtype=np.uint8)
    assert len(codes) == n_windows + k - 1
    padded = np.zeros((1, SK_MAX_WINDOWS + 30), dtype=np.uint8)
    padded[0, :len(codes)] = codes
    lo, hi = records(padded, [n_windows], bin_word, k)
    return int(lo[0]), int(hi[0])


def windows_of(hi):
    return (np.asarray(hi, dtype=np.uint64) >> _U64(60)).astype(np.int64) + 1


def units_of(hi):
    """pairs of windows: ceil(windows / 2)"""
    return (windows_of(hi) + 1) // 2


def rc_packed(x, k):
    """kmer_hash.h rc_packed on uint64 arrays"""
    r = np.asarray(x, dtype=np.uint64).copy()
    for sh, m in ((2, 0x3333333333333333), (4, 0x0f0f0f0f0f0f0f0f), (8, 0x00ff00ff00ff00ff), (16, 0x0000ffff0000ffff)):
        r = ((r & _U64(m)) << _U64(sh)) | ((r >> _U64(sh)) & _U64(m))
    r = (r << _U64(32)) | (r >> _U64(32))
    return (~r) >> _U64(64 - 2 * k)


def expand(lo, hi, k):
    """the canonical key of every window of every record: (keys int64, index of the record, window number), record by record"""
    lo, hi = np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64)
    nw = windows_of(hi)
    t_hi = (hi << _U64(4)) | (lo >> _U64(60))
    t_lo = (lo >> _U64(32)) << _U64(36)
    keys, rec, win = [], [], []
    for j in range(SK_MAX_WINDOWS):
        at = np.nonzero(nw > j)[0]
        if not len(at):
            break
        top = t_hi[at] << _U64(2 * j)
        if j:
            top |= t_lo[at] >> _U64(64 - 2 * j)
        fw = top >> _U64(64 - 2 * k)
        keys.append(np.minimum(fw, rc_packed(fw, k)))
        rec.append(at)
        win.append(np.full(len(at), j))
    keys, rec, win = np.concatenate(keys), np.concatenate(rec), np.concatenate(win)
    o = np.lexsort((win, rec))
    return keys[o].astype(np.int64), rec[o], win[o]


def sum_tables(*tables):
    """(keys, counts) of the sum of some (keys, counts): keys ascending, counts int64 and not clamped"""
    keys = np.concatenate([np.asarray(t[0], dtype=np.int64) for t in tables] + [np.zeros(0, dtype=np.int64)])
    counts = np.concatenate([np.asarray(t[1], dtype=np.int64) for t in tables] + [np.zeros(0, dtype=np.int64)])
    uk, inv = np.unique(keys, return_inverse=True)
    out = np.zeros(len(uk), dtype=np.int64)
    np.add.at(out, inv, counts)
    return uk, out


def table_of(lo, hi, copies, k, before=None):
    """the table the records make, by the plain rule: every window of every copy adds one to its key.  (keys ascending, counts; not
    clamped: compare np.minimum(counts, 32767)); before = the (keys, counts) the table held"""
    keys, rec, _ = expand(lo, hi, k)
    t = (keys, np.asarray(copies, dtype=np.int64)[rec])
    return sum_tables(t, before) if before is not None else sum_tables(t)


# ---------------------------------------------------------------------------------------------------- the record table
def dd_hash(lo, hi):
    """kmer_hash.h dd_hash(rec.y, rec.z, rec.w): uint32 arithmetic in uint64 words"""
    lo, hi = np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64)
    y, z, w = lo >> _U64(32), hi & _M32, hi >> _U64(32)
    h = y ^ ((z * _U64(0x9E3779B1)) & _M32)
    h = ((h ^ (h >> _U64(15))) * _U64(0x85EBCA6B)) & _M32
    h ^= (w * _U64(0xC2B2AE35)) & _M32
    h = ((h ^ (h >> _U64(13))) * _U64(0x27D4EB2F)) & _M32
    return h ^ (h >> _U64(16))


def tag(lo, hi):
    return (dd_hash(lo, hi) & _U64(0xFFFF0000)) | _U64(0x8000)


def home_place(lo, hi):
    return (dd_hash(lo, hi) & _U64(D2_SLOTS - 1)).astype(np.int64)


def pick_distinct_places(lo, hi, order, n=None, units=None):
    """indices of records, taken in `order`, with pairwise different home places: each then claims its home place whatever the order
    of arrival, all have a place and the leaf's units are the sum of theirs.  n: that many records; units: as many as make exactly
    that many units (a record that would overshoot is passed over)"""
    place, u = home_place(lo, hi), units_of(hi)
    taken, out, total = set(), [], 0
    for i in order:
        if (n is not None and len(out) == n) or (units is not None and total == units):
            break
        p = int(place[i])
        if p in taken or (units is not None and total + int(u[i]) > units):
            continue
        taken.add(p)
        out.append(int(i))
        total += int(u[i])
    assert (n is None or len(out) == n) and (units is None or total == units), (len(out), total)
    return np.array(out)


def twins(lo, hi):
    """pairs (i, j) of different records with the same tag and the same home place: the second to arrive finds the first one's
    fingerprint in its home place, is compared with it word for word, and stays on its own"""
    h = dd_hash(lo, hi)
    sig = ((h >> _U64(16)) << _U64(10)) | (h & _U64(D2_SLOTS - 1))
    o = np.argsort(sig, kind="stable")
    same = np.nonzero(sig[o][1:] == sig[o][:-1])[0]
    return [(int(o[a]), int(o[a + 1])) for a in same if (lo[o[a]], hi[o[a]]) != (lo[o[a + 1]], hi[o[a + 1]])]


# ---------------------------------------------------------------------------------------------------- candidate records of loci
class Pool:
    """every record a set of loci can give: a run of w = 1 .. min(16, k - 14) windows from window s on, of the locus or of its reverse
    complement.  lo, hi, and for each record its locus, strand, first window; codes[i] = the record's bases"""

    def __init__(self, loci, k, m=ct.M_INTERIOR):
        self.k, self.bin = k, bin_of(m)
        n_loc, length = loci.shape
        windows = length - k + 1
        rows, meta = [], []
        for strand in (0, 1):
            src = loci if strand == 0 else (3 - loci[:, ::-1]).astype(np.uint8)
            for w in range(1, min(SK_MAX_WINDOWS, windows) + 1):
                for s in range(windows - w + 1):
                    block = np.zeros((n_loc, SK_MAX_WINDOWS + 30), dtype=np.uint8)
                    block[:, :w + k - 1] = src[:, s:s + w + k - 1]
                    rows.append(block)
                    meta.append(np.stack([np.arange(n_loc), np.full(n_loc, strand), np.full(n_loc, s), np.full(n_loc, w)], axis=1))
        self.codes = np.concatenate(rows)
        meta = np.concatenate(meta)
        self.locus, self.strand, self.first, self.nw = meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3]
        self.lo, self.hi = records(self.codes, self.nw, self.bin, k)

    def __len__(self):
        return len(self.lo)

    def bases(self, i):
        return self.codes[i, :int(self.nw[i]) + self.k - 1]


class Leaf:
    """one designed leaf: its distinct records, the copies of each, and the numbers the kernel's path follows from"""

    def __init__(self, name, k, lo, hi, copies, seed, bases=None, bin_word=None, cov_hint=0):
        self.name, self.k, self.cov_hint = name, k, cov_hint
        self.lo, self.hi = np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64)
        self.copies = np.asarray(copies, dtype=np.int64)
        self.bases = bases  # the records' own bases (the reads of the reads form), where the design kept them
        assert len(self.lo) == len(self.hi) == len(self.copies) and (self.copies >= 1).all()
        assert len(set(zip(self.lo.tolist(), self.hi.tolist()))) == len(self.lo), "the records listed differ from each other"
        self.bin = int(self.lo[0] & _M32) if bin_word is None else bin_word
        assert ((self.lo & _M32) == _U64(self.bin)).all()
        self.seed = seed
        # the design's numbers
        self.records = int(self.copies.sum())
        self.distinct = len(self.lo)
        place = home_place(self.lo, self.hi)
        self.distinct_places = len(np.unique(place))
        self.all_placed = self.distinct_places == self.distinct
        self.units = int(units_of(self.hi).sum())  # (exact when all_placed)
        # every home place some record names ends up taken: at least so many records have a place, each with a unit or more
        self.units_at_least = int(np.sort(units_of(self.hi))[:self.distinct_places].sum()) if not self.all_placed else self.units
        self.max_copies = int(self.copies.max())
        self.keys, self.counts = table_of(self.lo, self.hi, self.copies, k)
        self.max_count = int(self.counts.max())

    def instances(self):
        """the index of the distinct record of every record of the leaf, in the shuffled order they are handed in"""
        return np.random.default_rng(self.seed).permutation(np.repeat(np.arange(self.distinct), self.copies))

    def half(self):
        """what a first batch holds of it: every other distinct record, once"""
        idx = np.arange(0, self.distinct, 2)
        return Leaf(self.name + "/half", self.k, self.lo[idx], self.hi[idx], np.ones(len(idx), dtype=np.int64), self.seed + 1,
                    [self.bases[i] for i in idx] if self.bases is not None else None, self.bin)

    def rounds(self):
        """rounds of phase B when every record has a place"""
        return -(-self.units // D2_UL_CAP)


def _leaf(name, pool, idx, copies, seed, cov_hint=0):
    idx = np.asarray(idx)
    return Leaf(name, pool.k, pool.lo[idx], pool.hi[idx], copies, seed, [pool.bases(i) for i in idx], pool.bin, cov_hint)


N_LOCI = 100        # 1700 keys at k = 31: the leaf's region of 4096 slots stays half empty
N_LOCI_TWINS = 400  # 121 600 candidate records at k = 31: some hundred pairs agree in the 26 bits of tag and place

_cache = {}


def pool_of(k, n_loci=N_LOCI):
    if (k, n_loci) not in _cache:
        loci = ct.loci(np.random.default_rng(7100 + k), ct.M_INTERIOR, n_loci, k)
        _cache[(k, n_loci)] = Pool(loci, k)
    return _cache[(k, n_loci)]


def poly_a(k=31):
    """the record of 16 windows of poly-A: one key, 0; its minimizer is the 15-mer 0, of order 0 and bin 0: leaf 0 of any table"""
    return records(np.zeros((1, 46), dtype=np.uint8), [SK_MAX_WINDOWS], 0, k)


def cases(k=31):
    """name -> Leaf, every leaf of the table in tests/test_gpu_dedup_leaves.py that lies in M_INTERIOR's leaf, at this k (the
    counter bound's poly-A batches are poly_a)"""
    if ("cases", k) in _cache:
        return _cache[("cases", k)]
    P = pool_of(k)
    rng = np.random.default_rng(7200 + k)
    wmax = int(P.nw.max())
    out = {}
    # quiet: 20 loci, ten records of each (what a leaf of real reads holds), every window count present
    few = np.nonzero(P.locus < 20)[0]
    order = list(rng.permutation(few))
    first = [next(i for i in order if P.nw[i] == w) for w in range(1, wmax + 1)]  # one record of every window count in front
    idx = pick_distinct_places(P.lo, P.hi, first + order, n=200)
    out["quiet"] = _leaf("quiet", P, idx, 1 + np.arange(200) % 5, 1)
    # second turn: more than 1024 records, at most 600 distinct ones, all with a place
    idx = pick_distinct_places(P.lo, P.hi, rng.permutation(len(P)), n=600)
    for total in (1025, 3000):
        copies = np.full(600, total // 600)
        copies[:total - int(copies.sum())] += 1
        out["second-turn-%d" % total] = _leaf("second-turn-%d" % total, P, idx, copies, 2)
    # unit boundary: exactly so many units, one copy of each record
    # (three rounds at k = 31 alone: shorter k-mers give a locus fewer windows, and 1024 places too few units)
    for units in (D2_UL_CAP, D2_UL_CAP + 1) + ((2 * D2_UL_CAP + 1,) if k == 31 else ()):
        order = rng.permutation(len(P))
        if units > D2_UL_CAP + 1:  # the records of many windows first: 1024 records at most have a place
            order = order[np.argsort(-units_of(P.hi[order]), kind="stable")]
        idx = pick_distinct_places(P.lo, P.hi, order, units=units)
        out["units-%d" % units] = _leaf("units-%d" % units, P, idx, np.ones(len(idx), dtype=np.int64), 3)
    # no place: 1500 distinct records of many windows for 1024 places
    many = np.nonzero(P.nw >= wmax - 3)[0]
    idx = rng.choice(many, 1500, replace=False)
    out["no-place"] = _leaf("no-place", P, idx, np.full(1500, 2), 4)
    if k == 31:
        # twins: the quiet leaf and one pair with the same tag and place
        big = pool_of(k, N_LOCI_TWINS)
        far = [(i, j) for i, j in twins(big.lo, big.hi) if big.locus[i] >= N_LOCI and big.locus[j] >= N_LOCI]
        q = out["quiet"]
        i, j = next((i, j) for i, j in far if int(home_place(big.lo[[i]], big.hi[[i]])[0]) not in set(home_place(q.lo, q.hi).tolist()))
        out["twins"] = Leaf("twins", k, np.concatenate([q.lo, big.lo[[i, j]]]), np.concatenate([q.hi, big.hi[[i, j]]]),
                            np.concatenate([q.copies, [3, 5]]), 5, q.bases + [big.bases(i), big.bases(j)], P.bin)
        # many copies: one record of 16 windows 4000 times and 96 others; and 4096 times, all the copy field takes, alone
        full = np.nonzero(P.nw == SK_MAX_WINDOWS)[0]
        idx = pick_distinct_places(P.lo, P.hi, list(full[:1]) + list(rng.permutation(len(P))), n=97)
        out["copies-4000"] = _leaf("copies-4000", P, idx, np.array([4000] + [1] * 96), 6)
        out["copies-4096"] = _leaf("copies-4096", P, full[:1], np.array([DD_MAX_CAP]), 7)
        # hand-over: 4096 records the dedup kernel still takes, 4097 it leaves to the general kernel
        idx = pick_distinct_places(P.lo, P.hi, rng.permutation(len(P)), n=500)
        for total in (DD_MAX_CAP, DD_MAX_CAP + 1):
            copies = np.full(500, total // 500)
            copies[:total - int(copies.sum())] += 1
            out["hand-over-%d" % total] = _leaf("hand-over-%d" % total, P, idx, copies, 8)
        # crossings: 30 records of 16 windows of 30 loci, 40 copies each: every key reaches the threshold with its first addition
        idx = pick_distinct_places(P.lo, P.hi, [i for i in full if P.strand[i] == 0 and P.first[i] == 0], n=30)
        out["crossings"] = _leaf("crossings", P, idx, np.full(30, 40), 9, cov_hint=5)
    _cache[("cases", k)] = out
    return out
