"""Key sets designed for the join by key (csrc/dup_check.h): k-mers composed for chosen 64-bit PolynomialHash keys, so that the rare
paths of k_dup_find, the fix-up and the walk's check by key are entered by design (test infrastructure only, numpy and plain Python;
tests/test_join_keys_model.py checks every family against the condition in its name, tests/test_gpu_join_keys.py runs them).

PolynomialHash (src/utils/PolynomialHash.java:19-28) is fw(s) = 5^k + sum b_i 5^(k-1-i) mod 2^64, the key the smaller (as int64) of
fw(s) and fw(rc(s)).  For k >= 41 a k-mer of any key is found by drawing its upper k - 28 digits and solving for the lower 28: the at
most three v < 5^28 with v = key - upper (mod 2^64) are candidates, one is kept when none of its base-5 digits is 4 and the forward
strand is the canonical one ((4/5)^28 = 1.9e-3 a candidate: some 500 draws a k-mer, drawn 4096 at a time).

The placement functions of the join are restated here from their definitions (kmer_hash.h sk_home_mix, fmix64; dup_check.h dup_b1,
dup_f2, dup_sub, dup_mix3, dup_fp; mcgpu.hip ensure_dups for f2_lg).  The table is the project's minimum (long_harness.HINT: 4 M slots,
REGIONS regions); a key set that shares the top nine bits of sk_home_mix lies in one sub-bucket under f2_lg 0 and 1 alike, so the keys
of a family do not depend on f2_lg -- the size of the background does."""
import functools

import numpy as np

from tests import long_loci as ll

REGIONS = 1024           # of a table made for long_harness.HINT keys (asserted on the GPU: long_harness.n_leaves)
DUP_MAX_CAND = 32
SUB_MAX_KEYS = 1800      # mcgpu.hip ensure_dups: keys a sub-bucket is planned for
FLANK = 3                # random bases on either side of a designed k-mer
BG_LEN = 150
COV_HINT = 12
_U64 = np.uint64
_M32 = _U64(0xFFFFFFFF)
_FULL = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the join's placement, restated
def _u64(keys):
    return np.asarray(keys).astype(np.int64).view(np.uint64) if np.asarray(keys).dtype != np.uint64 else np.asarray(keys)


def sk_home_mix(keys):
    k = _u64(keys)
    x = ((k & _M32) * _U64(0x9E3779B1) + (k >> _U64(32)) * _U64(0x85EBCA6B)) & _M32
    x ^= x >> _U64(15)
    return (x * _U64(0xC2B2AE35)) & _M32


def dup_b1(keys):
    return (sk_home_mix(keys) >> _U64(24)).astype(np.int64)


def dup_f2(keys, f2_lg):
    if not f2_lg:
        return np.zeros(np.shape(keys), dtype=np.int64)
    return (((sk_home_mix(keys) << _U64(8)) & _M32) >> _U64(32 - f2_lg)).astype(np.int64)


def dup_sub(keys, f2_lg):
    return (dup_b1(keys) << f2_lg) | dup_f2(keys, f2_lg)


def dup_mix3(keys):
    k = _u64(keys)
    x = (((k >> _U64(32)) * _U64(0x9E3779B1)) & _M32) ^ (((k & _M32) * _U64(0xC2B2AE35)) & _M32)
    x ^= x >> _U64(16)
    x = (x * _U64(0x7FEB352D)) & _M32
    x ^= x >> _U64(15)
    return x


def _fp_first(keys):
    """dup_fp's first step: linear in the key's two words"""
    k = _u64(keys)
    return ((k & _M32) * _U64(0x85EBCA6B) + (k >> _U64(32)) * _U64(0x27D4EB2F)) & _M32


def dup_fp(keys):
    x = _fp_first(keys)
    x ^= x >> _U64(13)
    x = (x * _U64(0x165667B1)) & _M32
    x ^= x >> _U64(16)
    return x | _U64(1)


def fmix64(keys):
    x = _u64(keys).copy()
    with np.errstate(over="ignore"):
        x ^= x >> _U64(33)
        x *= _U64(0xff51afd7ed558ccd)
        x ^= x >> _U64(33)
        x *= _U64(0xc4ceb9fe1a85ec53)
        x ^= x >> _U64(33)
    return x


def f2_lg_for(n_used):
    """the host's rule: the smallest f2_lg with n_used / (256 << f2_lg) <= 1800, 10 at most"""
    f2_lg = 0
    while f2_lg < 10 and float(n_used) / float(256 << f2_lg) > float(SUB_MAX_KEYS):
        f2_lg += 1
    return f2_lg


def sub9(keys):
    """the sub-bucket under f2_lg = 1: keys that agree here share their sub-bucket under f2_lg 0 and 1"""
    return dup_sub(keys, 1)


def signed(key):
    key &= _FULL
    return key - (1 << 64) if key >> 63 else key


# ------------------------------------------------------------------------------------------------ k-mers of a chosen key
_P14 = 5 ** 14
_Q0, _M0 = divmod(1 << 64, _P14)
_POW28 = _U64(5 ** 28 & _FULL)
_BATCH = 4096


def _no_digit_4(x):
    """do the 14 base-5 digits of every x < 5^14 stay below 4?"""
    ok = np.ones(x.shape, dtype=bool)
    x = x.copy()
    for _ in range(14):
        ok &= (x % _U64(5)) != _U64(4)
        x //= _U64(5)
    return ok


def region_of_kmer(codes, k, rule, n_regions=REGIONS):
    return int(ll.region_of(ll.bin_words(np.asarray(codes, dtype=np.uint8), k, rule), n_regions)[0])


def preimages(k, key, rng, n=1, accept=None):
    """n distinct k-mers (uint8 codes) whose forward strand is canonical and has this key (an int, taken mod 2^64); accept(codes): a
    further condition, asked of every find in the order of the draws"""
    assert k >= 41
    key &= _FULL
    out, seen = [], set()
    while len(out) < n:
        upper = rng.integers(0, 4, (_BATCH, k - 28)).astype(np.uint64)
        with np.errstate(over="ignore"):
            h = np.ones(_BATCH, dtype=np.uint64)
            for i in range(k - 28):
                h = h * _U64(5) + upper[:, i]
            r = _U64(key) - h * _POW28
        qr, mr = r // _U64(_P14), r % _U64(_P14)
        for c in range(3):  # v = r + c 2^64 = Q 5^14 + R
            R = mr + _U64(c * _M0)
            Q = qr + _U64(c * _Q0) + R // _U64(_P14)
            R = R % _U64(_P14)
            good = (Q < _U64(_P14)) & _no_digit_4(np.minimum(Q, _U64(_P14 - 1))) & _no_digit_4(R)
            for i in np.nonzero(good)[0].tolist():
                v = int(Q[i]) * _P14 + int(R[i])
                low = np.zeros(28, dtype=np.uint8)
                for j in range(27, -1, -1):
                    v, low[j] = divmod(v, 5)
                codes = np.concatenate([upper[i].astype(np.uint8), low])
                if int(ll.window_keys(codes, k)[0]) != signed(key) or bytes(codes) in seen:
                    continue  # (the reverse strand has the smaller hash)
                if accept is not None and not accept(codes):
                    continue
                seen.add(bytes(codes))
                out.append(codes)
    return out[:n]


def preimage(k, key, rng):
    return preimages(k, key, rng, 1)[0]


def preimages_in_regions(k, key, rng, n, rule, n_regions=REGIONS, avoid=()):
    """n k-mers of one key in pairwise different regions under the bin rule, none in `avoid` (region 0 is poly-A's: never taken)"""
    taken = set(avoid) | {0}

    def accept(codes):
        r = region_of_kmer(codes, k, rule, n_regions)
        if r in taken:
            return False
        taken.add(r)
        return True
    return preimages(k, key, rng, n, accept)


# ------------------------------------------------------------------------------------------------ the plain answer
def join_model(keys, regions, counts):
    """What a join by key must find in a table that files (key, region) in a slot of its own.  keys, regions, counts: one entry an
    occurrence (a window, times its read's copies).  Returns slots (distinct (key, region)), listed (the keys that sit in two regions
    or more, ascending), sums (their counters added up), dup_keys, and regions_of (listed key -> its regions)"""
    keys, regions, counts = np.asarray(keys, dtype=np.int64), np.asarray(regions, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    o = np.lexsort((regions, keys))
    k, r, c = keys[o], regions[o], counts[o]
    new_slot = np.ones(len(k), dtype=bool)
    new_slot[1:] = (k[1:] != k[:-1]) | (r[1:] != r[:-1])
    sk, sr = k[new_slot], r[new_slot]
    sc = np.add.reduceat(c, np.nonzero(new_slot)[0])
    uk, first, per_key = np.unique(sk, return_index=True, return_counts=True)
    sel = per_key >= 2
    sums = np.add.reduceat(sc, first)[sel]
    listed = uk[sel]
    regions_of = {int(kk): sr[a:a + n].tolist() for kk, a, n in zip(listed.tolist(), first[sel].tolist(), per_key[sel].tolist())}
    own = {int(kk): sc[a:a + n].tolist() for kk, a, n in zip(listed.tolist(), first[sel].tolist(), per_key[sel].tolist())}
    return {"slots": len(sk), "keys": len(uk), "listed": listed, "sums": sums, "dup_keys": int(sel.sum()), "regions_of": regions_of, "own": own}


def occurrences(reads, copies, k, rule, n_regions=REGIONS):
    """(keys, regions, counts) of every window of reads of one length, each read `copies` times"""
    keys, regions, counts = [], [], []
    by_len = {}
    for r, c in zip(reads, copies):
        by_len.setdefault(len(r), []).append((r, c))
    for group in by_len.values():
        a = np.stack([g[0] for g in group])
        wk = ll.window_keys(a, k)
        keys.append(wk.reshape(-1))
        regions.append(ll.region_of(ll.bin_words(a, k, rule), n_regions).reshape(-1))
        counts.append(np.repeat(np.array([g[1] for g in group], dtype=np.int64), wk.shape[1]))
    return np.concatenate(keys), np.concatenate(regions), np.concatenate(counts)


# ------------------------------------------------------------------------------------------------ the background
class Background:
    """random reads of BG_LEN bases with the attributes long_harness.expected / assert_walk ask of a background (keys, counts, mult,
    list); size 0: 4000 reads, the table stays at f2_lg 0 (at most 460 800 keys with any family beside it); size 1: as many reads as
    give 484 000 windows, f2_lg 1.  (long_harness.Background keeps whole regions free for a designed leaf and asks a GPU for the
    table's size: here the designed k-mers lie wherever their bases put them, and the model has to run without a GPU.)"""

    def __init__(self, k, rule, size):
        from oracle import pyoracle as po
        self.k, self.rule, self.size, self.nl, self.mult = k, rule, size, REGIONS, 1
        n = 4000 if size == 0 else -(-484000 // (BG_LEN - k + 1))
        self.reads = np.random.default_rng(8800 + 100 * size + 10 * k + rule).integers(0, 4, (n, BG_LEN)).astype(np.uint8)
        t = po.Table()
        t.count_reads(self.reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * BG_LEN, k, po.KEY_POLY)
        self.keys, self.counts = t.dump()
        self.counts = self.counts.astype(np.int64)

    def list(self, mult=None):
        return list(self.reads) * (self.mult if mult is None else mult)

    @functools.lru_cache(maxsize=None)
    def model(self):
        """join_model of the background alone"""
        return join_model(*occurrences(list(self.reads), [1] * len(self.reads), self.k, self.rule))


@functools.lru_cache(maxsize=None)
def background(k, rule, size):
    return Background(k, rule, size)


# ------------------------------------------------------------------------------------------------ families
def _draw_keys(rng, n, want_sub9=None, distinct_sub9=False, avoid=()):
    """n random keys (ints mod 2^64, never the free-slot mark, pairwise different, of pairwise different dup_fp within a sub-bucket):
    all in sub-bucket want_sub9, or in pairwise different ones under f2_lg 0 and 1 alike (different level-1 buckets)"""
    out, subs, fps = [], set(), set(int(x) for x in avoid)
    while len(out) < n:
        cand = rng.integers(0, 1 << 63, 1 << 16, dtype=np.uint64) << _U64(1) | rng.integers(0, 2, 1 << 16, dtype=np.uint64)
        s9, fp = sub9(cand), dup_fp(cand)
        for i in (np.nonzero(s9 == want_sub9)[0] if want_sub9 is not None else range(len(cand))):
            key = int(cand[i])
            if key == _FULL or (int(s9[i]), int(fp[i])) in fps or (distinct_sub9 and int(s9[i]) >> 1 in subs) or len(out) == n:
                continue
            subs.add(int(s9[i]) >> 1)
            fps.add((int(s9[i]), int(fp[i])))
            out.append(key)
    return out


_FP_A_INV = pow(0x85EBCA6B, -1, 1 << 32)


def fp_twin(key, rng):
    """another key with the sub-bucket (nine bits), the dup_fp and the low 13 bits of dup_mix3 of `key`: the low word follows from a
    free high word through dup_fp's linear first step, and the high word is searched for the 9 + 13 remaining bits"""
    a = np.array([key], dtype=np.uint64)
    x1, s, m = _fp_first(a)[0], int(sub9(a)[0]), int(dup_mix3(a)[0]) & 8191
    while True:
        hi = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64)
        lo = (((x1 - hi * _U64(0x27D4EB2F)) & _M32) * _U64(_FP_A_INV)) & _M32
        cand = (hi << _U64(32)) | lo
        hit = np.nonzero((sub9(cand) == s) & ((dup_mix3(cand) & _U64(8191)) == _U64(m)) & (cand != _U64(key)) & (cand != _U64(_FULL)))[0]
        if len(hit):
            return int(cand[hit[0]])


class Family:
    """reads (each one designed k-mer between FLANK random bases), their copies, and what the design says of them.
    kmers: (key as int64, codes, region, copies, index of its read) of every designed k-mer"""

    def __init__(self, name, k, rule, f2_lg):
        self.name, self.k, self.rule, self.f2_lg = name, k, rule, f2_lg
        self.rng = np.random.default_rng(9100 + 1000 * sorted(FAMILIES).index(name) + 10 * k + rule)
        self.reads, self.copies, self.kmers = [], [], []
        self.designed = {}     # key -> regions, of the keys meant to sit in two regions or more
        self.single = []       # designed keys meant to sit in one slot
        self.seeds = []        # reads a walk starts from
        self.extra = {}
        self.window_keys = set()

    def place(self, codes, copies, left=FLANK, right=FLANK):
        key = int(ll.window_keys(codes, self.k)[0])
        while True:  # (flanks whose windows share no key with anything placed so far: next to k-mers of one key the rolling hash would
            # go on colliding wherever the same bases leave and enter)
            read = np.concatenate([self.rng.integers(0, 4, left), codes, self.rng.integers(0, 4, right)]).astype(np.uint8)
            others = ll.window_keys(read, self.k).tolist()
            others.remove(key)
            if len(set(others)) == len(others) and key not in others and not set(others) & self.window_keys:
                break
        self.window_keys |= set(others) | {key}
        self.kmers.append((key, codes, region_of_kmer(codes, self.k, self.rule), copies, len(self.reads)))
        self.reads.append(read)
        self.copies.append(copies)
        return len(self.reads) - 1

    def add_key(self, key, copies, avoid=()):
        """k-mers of `key` in len(copies) pairwise different regions"""
        if len(copies) == 1:
            ks = preimages(self.k, key, self.rng, 1, lambda c: region_of_kmer(c, self.k, self.rule) not in (set(avoid) | {0}))
        else:
            ks = preimages_in_regions(self.k, key, self.rng, len(copies), self.rule, REGIONS, avoid)
        # (more than four k-mers of one key: bare k-mers -- with sixteen pairs of an end base and the flank's base beside it, some two
        # of them would have neighbours of one key again)
        flank = FLANK if len(copies) <= 4 else 0
        at = [self.place(c, n, flank, flank) for c, n in zip(ks, copies)]
        regions = [self.kmers[-len(ks) + i][2] for i in range(len(ks))]
        if len(copies) > 1:
            self.designed[signed(key)] = regions
        else:
            self.single.append(signed(key))
        return at

    def read_list(self):
        return [r for r, c in zip(self.reads, self.copies) for _ in range(c)]

    def background(self):
        return background(self.k, self.rule, self.f2_lg)

    @functools.lru_cache(maxsize=None)
    def model(self):
        """join_model over the family's reads and the background's: the two share no key (asserted), so their models add up"""
        a = occurrences(self.reads, self.copies, self.k, self.rule)
        m, b = join_model(*a), self.background().model()
        assert not np.isin(np.unique(a[0]), self.background().keys).any()
        o = np.argsort(np.concatenate([m["listed"], b["listed"]]), kind="stable")
        return {"slots": m["slots"] + b["slots"], "keys": m["keys"] + b["keys"], "dup_keys": m["dup_keys"] + b["dup_keys"],
                "listed": np.concatenate([m["listed"], b["listed"]])[o], "sums": np.concatenate([m["sums"], b["sums"]])[o],
                "regions_of": {**m["regions_of"], **b["regions_of"]}, "own": {**m["own"], **b["own"]}}

    def noted(self, sub):
        """how often k_dup_find notes a key of this sub-bucket (nine bits): every slot of a key beyond its first"""
        return sum(len(r) - 1 for key, r in self.designed.items() if int(sub9(np.array([key]))[0]) == sub)


def ks_of(F, at):
    """the designed k-mer of read `at`"""
    return next(codes for _, codes, _, _, i in F.kmers if i == at)


def _pairs(F):
    for key in _draw_keys(F.rng, 64, distinct_sub9=True):
        F.add_key(key, (3, 5))


def _multi(F):
    plan = {"three": (1, 7, 20), "four": (2, 1, 9, 30), "five": (1, 1, 3, 7, 20), "nine": (1, 2, 3, 4, 5, 6, 7, 8, 40),
            "sum-only": (5, 4, 6), "saturated": (300,) * 110}
    # (saturated: 33 000 > 32 767 must read 32 767.  Two counters of 20 000 would do, but 20 000 equal records overflow the stream of
    # their leaf -- some 400 records at this table size -- and under bin rule 2 the batch then loses records, is counted by the direct
    # kernel and the table leaves its bins before any join: 300 records a leaf stay inside it)
    for (what, copies), key in zip(plan.items(), _draw_keys(F.rng, len(plan), distinct_sub9=True)):
        at = F.add_key(key, copies)
        F.extra[what] = signed(key)
        F.seeds.append((ks_of(F, at[0]), signed(key), copies))
    assert max(plan["sum-only"]) < COV_HINT <= sum(plan["sum-only"])


def _noted(n, three=0):
    def make(F):
        sub = int(F.rng.integers(0, 512))
        F.extra["sub9"] = sub
        keys = _draw_keys(F.rng, n + three, want_sub9=sub)
        for key in keys[:n]:
            F.add_key(key, (2, 3))
        for key in keys[n:]:
            F.add_key(key, (2, 3, 4))
    return make


def _fp_twins(F):
    firsts = _draw_keys(F.rng, 10, distinct_sub9=True)
    F.extra["twins"] = []
    for i, a in enumerate(firsts):
        b = fp_twin(a, F.rng)
        F.add_key(a, (3,) if i < 8 else (3, 5))
        F.add_key(b, (4,) if i < 9 else (4, 6))
        F.extra["twins"].append((signed(a), signed(b)))


def _many_slots(F):
    F.add_key(_draw_keys(F.rng, 1)[0], (1,) * 73)


def _retreat(F):
    for key in _draw_keys(F.rng, 3, distinct_sub9=True):
        F.add_key(key, (1,) * (DUP_MAX_CAND + 1))


def _phantoms(F):
    """70 strings w nobody counts, each the right neighbour of a counted read end v, whose keys lie in one sub-bucket and are held
    by counted k-mers u elsewhere; the last four w have a second predecessor.  u and w (forward strands, both canonical) differ in
    their first and in their last base: the rolling hash then stops colliding, no neighbour of w shares its key with a neighbour of u,
    and one repetition of the walk finds everything."""
    k, rng = F.k, F.rng
    sub = int(rng.integers(0, 512))
    F.extra.update(sub9=sub, w=[], w_keys=[], regions={})
    ws = []
    while len(ws) < 70:
        cand = rng.integers(0, 4, (1 << 15, k)).astype(np.uint8)
        keys = ll.window_keys(cand, k).reshape(-1)
        for i in np.nonzero(sub9(keys) == sub)[0].tolist():
            if len(ws) < 70 and int(keys[i]) not in [x[0] for x in ws] and int(keys[i]) != -1 and _forward_is_canonical(cand[i], k):
                ws.append((int(keys[i]), cand[i]))
    for n, (key, w) in enumerate(ws):
        w_region = region_of_kmer(w, k, F.rule)
        u = preimages(k, key, rng, 1, lambda c: c[0] != w[0] and c[-1] != w[-1] and region_of_kmer(c, k, F.rule) not in (0, w_region))[0]
        F.place(u, 4)
        F.extra["regions"][key] = (w_region, F.kmers[-1][2])  # (where w asks, where u lives)
        F.single.append(key)
        for first in ([0] if n < 66 else [0, 1]):
            v = np.concatenate([[(int(w[0]) + 1 + first) % 4], w[:-1]]).astype(np.uint8)  # (any first base: v[1:] = w[:-1])
            while True:
                read = np.concatenate([rng.integers(0, 4, 2 * FLANK), v]).astype(np.uint8)
                wk = ll.window_keys(read, k).tolist()
                if len(set(wk)) == len(wk) and not set(wk) & F.window_keys and key not in wk:
                    break
            F.window_keys |= set(wk)
            F.reads.append(read)
            F.copies.append(4)
            F.seeds.append(read)
        F.extra["w"].append(w)
        F.extra["w_keys"].append(key)


def _forward_is_canonical(codes, k):
    c = np.asarray(codes).astype(object)
    fw = rc = 1
    for i in range(k):
        fw = (fw * 5 + int(c[i])) & _FULL
        rc = (rc * 5 + (3 ^ int(c[k - 1 - i]))) & _FULL
    return signed(fw) < signed(rc)


FAMILIES = {"pairs": _pairs, "multi": _multi, "noted-32": _noted(32), "noted-33": _noted(33), "noted-40": _noted(40, 1),
            "fp-twins": _fp_twins, "many-slots": _many_slots, "retreat": _retreat, "phantoms": _phantoms}
PARAMS = [(k, rule, f2_lg) for k in (41, 63) for rule in (1, 2) for f2_lg in (0, 1)]


@functools.lru_cache(maxsize=None)
def family(name, k, rule, f2_lg):
    F = Family(name, k, rule, f2_lg)
    FAMILIES[name](F)
    return F
