"""Loci, records and leaves composed base by base for the long-record form of the counting pipeline (csrc/count_long.h: polynomial
keys of 33 .. 63 bases in minimizer bins), so that crowded bins and the paths the comments of k_p3_long call rare are entered by design
(test infrastructure only, numpy only; tests/test_gpu_long_leaves.py and tests/test_gpu_long_crowded_bins.py run what it designs,
tests/test_long_loci_model.py pins it to the C code through `mc_hosttest placement <k> poly` and `mc_hosttest long-tags` and checks
that every case meets the condition in its name).

A locus forces all its windows to one bin word, whatever the table's size:
  rule 1 (smallest hash)    k - 15 random bases, the 15-mer M, k - 15 random bases: k - 14 windows that all hold M, whose sk_order is
                            smaller than that of every other 15-mer of the locus
  rule 2 (two smallest)     k - 30 random bases, M1 = M_INTERIOR and M2 back to back, k - 30 random bases: k - 29 windows that all hold
                            both, the two smallest of every window as a multiset (count_long.h "TWO SMALLEST")
A read that is windows s .. s + w - 1 of a locus, or of its reverse complement, is one run of the extract kernel, cut every 32 windows:
one record when w <= 32.  The record's words, the hash of k_p3_long's table of equal records (kmer_hash.h skl_rec_hash), its 16-bit tag
and its home slot are restated here, as are skl_bin, skl_word2, sk_hmin_of_kmer2 for both rules, sk_home and the region of a bin word.
"""
import numpy as np

from tests import crowded_tables as ct

SK_M = ct.SK_M
SKL_MAX_WINDOWS = 32   # windows of a record
SKL_ROUND = 512        # records k_p3_long has at hand at a time
SKL_DTAB = 1024        # slots of its table of equal records
SKL_PROBES = 4         # slots a record tries there
SKL_CHUNK = 8          # windows a lane takes of a record
K_FROM, K_TO = 33, 63
M_INTERIOR, M_LAST = ct.M_INTERIOR, ct.M_LAST

_U64 = np.uint64
_M32 = _U64(0xFFFFFFFF)
_NONE = 0xFFFFFFFF


def _canon(m):
    return min(int(m), int(ct.rc_mmer(np.array([m]))[0]))


def order_of(m):
    """sk_order of the canonical form of one 15-mer"""
    return int(ct.sk_order(np.array([_canon(m)]))[0])


# ---------------------------------------------------------------------------------------------------- placement over base codes
def mmer_orders(codes):
    """sk_order of the canonical 15-mer that starts at every position of the last axis: [..., L] codes -> [..., L - 14] uint64"""
    c = np.asarray(codes).astype(np.uint64)
    n = c.shape[-1] - SK_M + 1
    f = np.zeros(c.shape[:-1] + (n,), dtype=np.uint64)
    r = f.copy()
    for i in range(SK_M):
        b = c[..., i:i + n]
        f = (f << _U64(2)) | b
        r |= (_U64(3) - b) << _U64(2 * i)
    return ct.sk_order(np.minimum(f, r))


def two_smallest(orders, k):
    """(lo, hi): the two smallest, as a multiset, of the k - 14 orders of every window of k bases (count_long.h skl_merge2)"""
    w = k - SK_M + 1
    n = orders.shape[-1] - w + 1
    lo = orders[..., 0:n].copy()
    hi = np.full_like(lo, _NONE)
    for i in range(1, w):
        b = orders[..., i:i + n]
        t = np.maximum(lo, b)
        lo = np.minimum(lo, b)
        hi = np.minimum(t, hi)
    return lo, hi


def skl_word2(lo, hi):
    return ct._u64(lo) ^ ((ct._u64(hi) * _U64(0x85EBCA6B)) & _M32)


def skl_bin(word):
    return ct.sk_bin(word) & _U64(0xFFFFFF00)


def bin_words(codes, k, rule):
    """sk_hmin_of_kmer2(window, k, rule == 2) of every window of k bases along the last axis"""
    lo, hi = two_smallest(mmer_orders(codes), k)
    return lo if rule == 1 else skl_word2(lo, hi)


def region_of(word, n_regions):
    """the region of a key whose k-mer has this bin word: (skl_bin(word) * n_regions) >> 32"""
    return ((skl_bin(word) * _U64(n_regions)) >> _U64(32)).astype(np.int64)


def sk_home(keys):
    """kmer_hash.h sk_home: the key's home slot inside its region"""
    k = ct._u64(keys)
    x = ((k & _M32) * _U64(0x9E3779B1) + (k >> _U64(32)) * _U64(0x85EBCA6B)) & _M32
    x ^= x >> _U64(15)
    x = (x * _U64(0xC2B2AE35)) & _M32
    return (x >> _U64(32 - ct.REGION_LG)).astype(np.int64)


def window_keys(codes, k):
    """the polynomial key (src/utils/PolynomialHash.java:19-28) of every window of k bases along the last axis: int64"""
    c = np.asarray(codes).astype(np.uint64)
    n = c.shape[-1] - k + 1
    fw = np.ones(c.shape[:-1] + (max(n, 0),), dtype=np.uint64)
    rc = fw.copy()
    if n <= 0:
        return fw.view(np.int64)
    with np.errstate(over="ignore"):
        for i in range(k):
            fw = fw * _U64(5) + c[..., i:i + n]
            rc = rc * _U64(5) + (_U64(3) ^ c[..., k - 1 - i:k - 1 - i + n])
    return np.minimum(fw.view(np.int64), rc.view(np.int64))


def kmer_words(codes):
    """(hi, lo) as ints of one k-mer of up to 64 bases, right-aligned, first base on top (kmer_hash.h Kmer)"""
    v = 0
    for c in np.asarray(codes).tolist():
        v = (v << 2) | int(c)
    return v >> 64, v & 0xFFFFFFFFFFFFFFFF


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[..., ::-1]).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- loci
_ORDER_MUL_INV = pow(0x9E3779B1, -1, 1 << 32)


def mmer_of_order(t):
    """the 32-bit word whose sk_order is t (sk_order is a bijection of 32-bit words)"""
    x = t ^ (t >> 15) ^ (t >> 30)
    return (x * _ORDER_MUL_INV) & 0xFFFFFFFF


def pick_m2(n_regions=(1024, 1085, 2048, 4096, 1 << 20)):
    """The second 15-mer of a rule-2 locus: the canonical 15-mer of the smallest sk_order above M_INTERIOR's such that, set right behind
    M_INTERIOR, none of the 14 15-mers across the junction orders below it on either strand (mmer_orders takes the canonical form), and
    the bin of the pair is an interior region of tables of these sizes."""
    if "m2" in _cache:
        return _cache["m2"]
    o1 = order_of(M_INTERIOR)
    for t in range(o1 + 1, 1 << 20):
        m = mmer_of_order(t)
        if m >= 1 << 30 or _canon(m) != m or m == M_INTERIOR:
            continue
        o = mmer_orders(np.concatenate([ct.mmer_codes(M_INTERIOR), ct.mmer_codes(m)]))
        if int(o[0]) != o1 or int(o[-1]) != t or not (o[1:-1] > _U64(t)).all():
            continue
        word = skl_word2(np.array([o1], dtype=np.uint64), np.array([t], dtype=np.uint64))
        if all(0 < int(region_of(word, n)[0]) < n - 1 for n in n_regions):
            _cache["m2"] = m
            return m
    raise AssertionError("no second 15-mer found")


def core_of(rule, m=M_INTERIOR):
    """the forced bases of a locus and the bin word of all its windows"""
    if rule == 1:
        return ct.mmer_codes(m), order_of(m)
    assert m == M_INTERIOR
    m2 = pick_m2()
    o1, o2 = order_of(m), order_of(m2)
    word = int(skl_word2(np.array([min(o1, o2)], dtype=np.uint64), np.array([max(o1, o2)], dtype=np.uint64))[0])
    return np.concatenate([ct.mmer_codes(m), ct.mmer_codes(m2)]), word


def locus_windows(k, rule):
    return k - (SK_M if rule == 1 else 2 * SK_M) + 1


def loci(rng, k, rule, n, m=M_INTERIOR, seen=None):
    """n loci of k-mers of k bases whose windows all have one bin word under the rule: uint8 [n, 2 flank + core].  A locus whose flanks
    hold a 15-mer that changes a window's word is dropped and another drawn; no two loci share a canonical k-mer, nor does any with the
    keys in `seen` (a set that is extended)."""
    assert K_FROM <= k <= K_TO and rule in (1, 2)
    core, word = core_of(rule, m)
    flank = k - len(core)
    length, windows = 2 * flank + len(core), flank + 1
    seen = set() if seen is None else seen
    out = []
    while len(out) < n:
        cand = rng.integers(0, 4, (n, length)).astype(np.uint8)
        cand[:, flank:flank + len(core)] = core
        ok = (bin_words(cand, k, rule) == _U64(word)).all(axis=1)
        keys = window_keys(cand, k)
        for i in np.nonzero(ok)[0]:
            ks = set(keys[i].tolist())
            if len(ks) == windows and not (ks & seen) and len(out) < n:
                seen |= ks
                out.append(cand[i])
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------- records
def pack96(codes):
    """the three words of bases of records: [n, L <= 96] codes, first base on top of X0, the tail zero"""
    c = np.asarray(codes).astype(np.uint64)
    assert c.ndim == 2 and c.shape[1] <= 96
    X = [np.zeros(c.shape[0], dtype=np.uint64) for _ in range(3)]
    for i in range(c.shape[1]):
        X[i >> 5] |= c[:, i] << _U64(62 - 2 * (i & 31))
    return X[0], X[1], X[2]


def _keep_bases(X0, X1, X2, length):
    """the words with everything behind the first `length` bases (33 .. 95) cleared"""
    full = _U64(0xFFFFFFFFFFFFFFFF)
    if length < 64:
        return X0, X1 & (full << _U64(2 * (64 - length))), np.zeros_like(X2)
    if length == 64:
        return X0, X1, np.zeros_like(X2)
    return X0, X1, X2 & (full << _U64(2 * (96 - length)))


def cuts(n_windows):
    """(first window, windows) of every record of a read of n_windows windows of one bin word: cut every 32 windows"""
    return [(a, min(SKL_MAX_WINDOWS, n_windows - a)) for a in range(0, n_windows, SKL_MAX_WINDOWS)]


def records_of_read(codes, k):
    """(X0, X1, X2, windows) as ints of every record of one read whose windows share their bin word"""
    codes = np.asarray(codes, dtype=np.uint8)
    out = []
    for a, w in cuts(len(codes) - k + 1):
        X0, X1, X2 = pack96(codes[None, a:a + w + k - 1])
        out.append((int(X0[0]), int(X1[0]), int(X2[0]), w))
    return out


def rec_hash(X0, X1, X2, nw):
    """kmer_hash.h skl_rec_hash(q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, windows): uint32 arithmetic in uint64 words"""
    X0, X1, X2, nw = (np.asarray(a, dtype=np.uint64) for a in (X0, X1, X2, nw))
    h = (((X0 & _M32) * _U64(0x9E3779B1)) & _M32) ^ (X0 >> _U64(32))
    h = (((h ^ (h >> _U64(15))) * _U64(0x85EBCA6B)) & _M32) ^ (X1 & _M32)
    h = (((h ^ (h >> _U64(13))) * _U64(0xC2B2AE35)) & _M32) ^ (X1 >> _U64(32))
    h = (((h ^ (h >> _U64(16))) * _U64(0x27D4EB2F)) & _M32) ^ (X2 & _M32)
    h = (((h ^ (h >> _U64(15))) * _U64(0x165667B1)) & _M32) ^ (X2 >> _U64(32)) ^ nw
    return h ^ (h >> _U64(16))


def tag_of(h):
    return (np.asarray(h, dtype=np.uint64) >> _U64(16)).astype(np.int64)


def slot_of(h):
    return (np.asarray(h, dtype=np.uint64) & _U64(SKL_DTAB - 1)).astype(np.int64)


class Pool:
    """every single record a set of loci can give: windows s .. s + w - 1, w = 1 .. min(32, windows of a locus), of the locus or of its
    reverse complement.  X0, X1, X2, nw, and for each record its locus, strand and first window; read(i) = the record's bases"""

    def __init__(self, loci_, k, rule):
        self.k, self.rule, self.loci = k, rule, loci_
        n_loc, length = loci_.shape
        windows = length - k + 1
        assert windows == locus_windows(k, rule)
        X, meta = [[], [], []], []
        self.src = [loci_, revcomp(loci_)]
        for strand in (0, 1):
            for s in range(windows):
                P = pack96(self.src[strand][:, s:s + 96])
                for w in range(1, min(SKL_MAX_WINDOWS, windows - s) + 1):
                    for a, x in zip(X, _keep_bases(P[0], P[1], P[2], w + k - 1)):
                        a.append(x)
                    meta.append(np.stack([np.arange(n_loc), np.full(n_loc, strand), np.full(n_loc, s), np.full(n_loc, w)], axis=1))
        self.X0, self.X1, self.X2 = (np.concatenate(a) for a in X)
        meta = np.concatenate(meta)
        self.locus, self.strand, self.first, self.nw = meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3]
        self.hash = rec_hash(self.X0, self.X1, self.X2, self.nw)
        self.tag, self.slot = tag_of(self.hash), slot_of(self.hash)

    def __len__(self):
        return len(self.X0)

    def read(self, i):
        s, w = int(self.first[i]), int(self.nw[i])
        return self.src[int(self.strand[i])][int(self.locus[i]), s:s + w + self.k - 1]

    def words(self, i):
        return int(self.X0[i]), int(self.X1[i]), int(self.X2[i]), int(self.nw[i])

    # --- searches, in the manner of tests/dedup_leaves.py
    def twins(self):
        """pairs (i, j) of different records with the same tag and the same home slot: the second to arrive finds the first one's
        fingerprint, is compared with it word for word, and stays on its own"""
        sig = self.hash & _U64(0xFFFF03FF)
        o = np.argsort(sig, kind="stable")
        same = np.nonzero(sig[o][1:] == sig[o][:-1])[0]
        return [(int(o[a]), int(o[a + 1])) for a in same if self.words(o[a]) != self.words(o[a + 1])]

    def same_home(self, n):
        """n records of one home slot with n different tags (the first such slot in slot order)"""
        o = np.argsort(self.slot, kind="stable")
        bounds = np.nonzero(np.diff(self.slot[o]))[0] + 1
        for grp in np.split(o, bounds):
            _, first = np.unique(self.tag[grp], return_index=True)
            if len(first) >= n:
                return grp[np.sort(first)[:n]]
        raise AssertionError("no home slot with %d tags" % n)

    def pick_distinct_slots(self, order, n, avoid=()):
        """n records taken in `order` with pairwise different home slots, none in `avoid`"""
        taken, out = set(avoid), []
        for i in order:
            if len(out) == n:
                break
            if int(self.slot[i]) not in taken:
                taken.add(int(self.slot[i]))
                out.append(int(i))
        assert len(out) == n, len(out)
        return np.array(out)


class Leaf:
    """one designed leaf: distinct reads of one record each, the copies of each, and the numbers the kernel's path follows from"""

    def __init__(self, name, k, rule, reads, copies, seed, cov_hint=0, word=None):
        self.name, self.k, self.rule, self.seed, self.cov_hint = name, k, rule, seed, cov_hint
        self.reads = [np.asarray(r, dtype=np.uint8) for r in reads]
        self.copies = np.asarray(copies, dtype=np.int64)
        assert len(self.reads) == len(self.copies) and (self.copies >= 1).all()
        recs = [records_of_read(r, k) for r in self.reads]
        assert all(len(r) == 1 for r in recs), "a read of a leaf is one record"
        self.words = [r[0] for r in recs]
        assert len(set(self.words)) == len(self.words), "the records listed differ from each other"
        self.X0, self.X1, self.X2, self.nw = (np.array([w[i] for w in self.words], dtype=np.uint64) for i in range(4))
        self.hash = rec_hash(self.X0, self.X1, self.X2, self.nw)
        self.tag, self.slot = tag_of(self.hash), slot_of(self.hash)
        wk = [window_keys(r, k) for r in self.reads]
        self.word = int(bin_words(self.reads[0], k, rule)[0]) if word is None else word
        # the design's numbers
        self.records = int(self.copies.sum())
        self.distinct = len(self.reads)
        self.rounds = -(-self.records // SKL_ROUND)
        self.window_counts = sorted(set(self.nw.astype(np.int64).tolist()))
        self.max_copies = int(self.copies.max())
        keys = np.concatenate(wk)
        self.keys, inv = np.unique(keys, return_inverse=True)
        self.counts = np.zeros(len(self.keys), dtype=np.int64)
        np.add.at(self.counts, inv, np.repeat(self.copies, [len(x) for x in wk]))
        self.max_count = int(self.counts.max())

    def one_bin(self):
        """do all windows of all reads have the leaf's bin word?"""
        return all((bin_words(r, self.k, self.rule) == _U64(self.word)).all() for r in self.reads)

    def instances(self):
        """the index of the distinct read of every read of the leaf, in the shuffled order they are handed in"""
        return np.random.default_rng(self.seed).permutation(np.repeat(np.arange(self.distinct), self.copies))

    def half(self):
        """what a first batch holds of it: every other distinct record, once"""
        idx = np.arange(0, self.distinct, 2)
        return Leaf(self.name + "/half", self.k, self.rule, [self.reads[i] for i in idx], np.ones(len(idx), dtype=np.int64), self.seed + 1, 0, self.word)

    def unmerged_at_least(self):
        """Distinct records that go in unmerged whatever the order of arrival.  The records of one home slot try the same four slots; a
        slot holds one record, and only a record with the same tag as a slot's stops there.  Of the groups of records that share a
        home slot AND have pairwise different tags, four at most find a slot; different records of equal tag and home: all but one stay
        on their own.  (Records of other home slots can only take slots away.)"""
        n = 0
        for s in np.unique(self.slot):
            tags = self.tag[self.slot == s]
            n += max(len(np.unique(tags)) - SKL_PROBES, 0) + (len(tags) - len(np.unique(tags)))
        return n


def _leaf(name, pool, idx, copies, seed, cov_hint=0):
    return Leaf(name, pool.k, pool.rule, [pool.read(i) for i in idx], copies, seed, cov_hint)


N_LOCI = 40         # the leaves' own loci: 1960 keys at k = 63, so the leaf's region of 4096 slots stays half empty
N_LOCI_BIG = 400    # k = 41: 302 400 candidate records, some hundred twin pairs and about 300 records a home slot

_cache = {}


def all_loci(k, rule=1):
    """the loci of (k, rule): N_LOCI_BIG under rule 1, N_LOCI + 10 under rule 2 (where the quiet leaf alone is designed)"""
    key = ("loci", k, rule)
    if key not in _cache:
        _cache[key] = loci(np.random.default_rng(7300 + 10 * k + rule), k, rule, N_LOCI_BIG if rule == 1 else N_LOCI + 10)
    return _cache[key]


def pool_of(k, rule=1, n_loci=N_LOCI):
    """the pool of the first n_loci loci of (k, rule)"""
    if ("pool", k, rule, n_loci) not in _cache:
        _cache[("pool", k, rule, n_loci)] = Pool(all_loci(k, rule)[:n_loci], k, rule)
    return _cache[("pool", k, rule, n_loci)]


def poly_a(k):
    """the read of 32 windows of poly-A: one record, one key; its 15-mers have sk_order 0, bin word 0: leaf 0 of any table"""
    return np.zeros(k + SKL_MAX_WINDOWS - 1, dtype=np.uint8)


def cases(k, rule=1):
    """name -> Leaf: the leaves of the table in tests/test_gpu_long_leaves.py that lie in M_INTERIOR's bin, at this k under this rule
    (rule 2: the quiet leaf alone; the counter's poly-A reads are poly_a)"""
    if ("cases", k, rule) in _cache:
        return _cache[("cases", k, rule)]
    P = pool_of(k, rule)
    rng = np.random.default_rng(7400 + 10 * k + rule)
    wmax = int(P.nw.max())
    out = {}
    # quiet: 20 loci, every window count in front, both strands, 1 .. 5 copies: 130 distinct records, 390 in all, at different home slots
    few = np.nonzero(P.locus < 20)[0]
    order = list(rng.permutation(few))
    first = [next(i for i in order if P.nw[i] == w and P.strand[i] == w % 2) for w in range(1, wmax + 1)]
    idx = P.pick_distinct_slots(first + order, 130)
    out["quiet"] = _leaf("quiet", P, idx, 1 + np.arange(130) % 5, 1)
    out["quiet"].strands = set(P.strand[idx].tolist())
    if rule == 2:
        _cache[("cases", k, rule)] = out
        return out
    # rounds: 300 distinct records at different home slots in 513 and in 1500 records
    idx = P.pick_distinct_slots(rng.permutation(len(P)), 300)
    for total in (513, 1500):
        copies = np.full(300, total // 300)
        copies[:total - int(copies.sum())] += 1
        out["rounds-%d" % total] = _leaf("rounds-%d" % total, P, idx, copies, 2)
    # copies: one record of the most windows fills a round; 511 of it and one other
    full = np.nonzero((P.nw == wmax) & (P.strand == 0))[0]
    out["copies-512"] = _leaf("copies-512", P, full[:1], [SKL_ROUND], 3)
    out["copies-511+1"] = _leaf("copies-511+1", P, full[:2], [SKL_ROUND - 1, 1], 4)
    # twins: the quiet leaf and two different records of one tag and home, at a home slot no quiet record has
    big = pool_of(k, 1, N_LOCI_BIG)
    q = out["quiet"]
    busy = set()
    for s in q.slot.tolist():
        busy |= {(s + d) % SKL_DTAB for d in range(-SKL_PROBES + 1, SKL_PROBES)}
    i, j = next((i, j) for i, j in big.twins() if big.locus[i] >= N_LOCI and big.locus[j] >= N_LOCI and int(big.slot[i]) not in busy)
    out["twins"] = Leaf("twins", k, 1, q.reads + [big.read(i), big.read(j)], np.concatenate([q.copies, [3, 5]]), 5)
    # same home: six records of one home slot and six tags, 4 copies each
    idx = big.same_home(6)
    out["same-home"] = _leaf("same-home", big, idx, np.full(6, 4), 6)
    # crossings: 30 records of the most windows of 30 loci, 40 copies each: every key reaches the threshold in one addition
    idx = [i for i in full if P.first[i] == 0][:30]
    out["crossings"] = _leaf("crossings", P, idx, np.full(30, 40), 7, cov_hint=5)
    _cache[("cases", k, rule)] = out
    return out


# ---------------------------------------------------------------------------------------------------- crowded bins
N_FULL, N_NEARLY, N_BEYOND, N_ABSENT = ct.N_FULL, ct.N_NEARLY, 22000, ct.N_ABSENT


class Crowded:
    """Whole loci as reads for one (k, rule): units[name] = the loci of the tables full (N_FULL keys of one interior region), nearly
    (N_NEARLY), last (rule 1, around M_LAST: the last region) and beyond (N_BEYOND, more than the five regions of the chain have slots);
    absent[name] = loci of the same bin that the table does not count."""

    def __init__(self, k, rule, names=("full", "nearly")):
        self.k, self.rule = k, rule
        W = self.windows = locus_windows(k, rule)
        rng = np.random.default_rng(9300 + 10 * k + rule)
        need = {"full": N_FULL, "nearly": N_NEARLY, "last": N_FULL, "beyond": N_BEYOND}
        n_absent = -(-N_ABSENT // W)
        self.units, self.absent, self.word = {}, {}, {}
        seen = set()
        if "full" in names or "nearly" in names or "beyond" in names:
            n_top = max(-(-need[n] // W) for n in names if n != "last")
            a = loci(rng, k, rule, n_top + n_absent, M_INTERIOR, seen)
            for n in names:
                if n != "last":
                    self.units[n] = list(a[:-(-need[n] // W)])  # (nearly and full are the first loci of one list)
                    self.absent[n] = list(a[n_top:])
                    self.word[n] = core_of(rule)[1]
        if "last" in names:
            assert rule == 1
            b = loci(rng, k, 1, -(-N_FULL // W) + n_absent, M_LAST, seen)
            self.units["last"], self.absent["last"] = list(b[:-(-N_FULL // W)]), list(b[-(-N_FULL // W):])
            self.word["last"] = order_of(M_LAST)

    def keys_in_home(self, name):
        """the designer's count of keys whose home region is the crowded one: every window of every unit has the region's bin word"""
        units = np.stack(self.units[name])
        assert (bin_words(units, self.k, self.rule) == _U64(self.word[name])).all()
        return len(np.unique(window_keys(units, self.k)))
