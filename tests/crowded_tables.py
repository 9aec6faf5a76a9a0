"""Reads whose k-mers all have one home region of the counting table, so that the region holds more keys than it has slots and every
look-up path must follow the probing rule of csrc/kmer_device.h past the home stretch: 128 slots that wrap inside the 4096-slot region,
then the same stretch of the next region, through 4 regions, the last region followed by region 0 (test infrastructure only;
tests/test_gpu_crowded_lookups.py uses it, tests/test_crowded_tables_model.py pins it to the C code through `mc_hosttest placement`).

The placement functions of csrc/kmer_hash.h and the region of slot_of (csrc/kmer_device.h) are restated here over numpy arrays.

Two ways to one region:
  - minimizer bins (packed keys, k = 31): every k-mer that holds a 15-mer M of very small sk_order has M for its minimizer, and the bin
    is a function of the minimizer alone, whatever the table's size.  A locus is 16 random bases + M + 16 random bases: 17 windows that
    all hold M, a chain of 17 neighbouring k-mers.
  - hash prefixes (packed k < 23, hash keys): the region is the top bits of fmix64(key).  Of a pool of random windows the ones whose
    top 10 bits have a chosen value are kept: they share a region of a table of 4 M slots (1024 regions).
"""
import numpy as np

from tests import seq_cov_model as sm

REGION_LG = 12          # MC_REGION_LG: 4096 slots a region
REGION_SLOTS = 1 << REGION_LG
TABLE_MAX_PROBES = 128
TABLE_CHAIN = 4
SK_M = 15
SK_MMASK = (1 << (2 * SK_M)) - 1

# canonical 15-mers of very small sk_order (the one of order 0 is poly-A: not used)
M_INTERIOR = 0x0e8b2f51  # sk_order 1, sk_bin 0x688990c0: an interior region
M_LAST = 0x356ca2e4      # sk_order 1467272, sk_bin 0xfffff483: the last region for every n_regions up to 2^20
LOCUS_FLANK = 16         # (k = 31; loci() takes any k from 23 on: locus_flank)
LOCUS_LEN = 2 * LOCUS_FLANK + SK_M   # 47 bases
LOCUS_WINDOWS = LOCUS_LEN - 31 + 1   # 17 windows at k = 31

N_FULL, N_NEARLY, N_ABSENT, N_ELSEWHERE, N_BACKGROUND = 5600, 3900, 1500, 2000, 100000
HASH_BITS = 10                 # regions of a table of 4 M slots
HASH_INTERIOR = 0x155          # the chosen interior region
HASH_LAST = (1 << HASH_BITS) - 1
# A region's share of the pool is 1 / 1024 of it: 5600 counted keys and 1500 that never are need 7100, so the pool is 8 M windows
# (7800 a region, give or take 90), not the 6 M that 5800 keys a region would take.
POOL_WINDOWS = 8 << 20

_U64 = np.uint64
_M32 = _U64(0xFFFFFFFF)


def _u64(x):
    a = np.asarray(x)
    return a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)


def fmix64(x):
    x = _u64(x).copy()
    with np.errstate(over="ignore"):
        x ^= x >> _U64(33)
        x *= _U64(0xff51afd7ed558ccd)
        x ^= x >> _U64(33)
        x *= _U64(0xc4ceb9fe1a85ec53)
        x ^= x >> _U64(33)
    return x


def sk_order(canon_mmer):
    """uint32 arithmetic in uint64 words"""
    x = (_u64(canon_mmer) * _U64(0x9E3779B1)) & _M32
    return x ^ (x >> _U64(15))


def sk_bin(hmin):
    x = _u64(hmin) & _M32
    x = x ^ (x >> _U64(16))
    x = (x * _U64(0x7FEB352D)) & _M32
    x = x ^ (x >> _U64(15))
    x = (x * _U64(0x846CA68B)) & _M32
    return x ^ (x >> _U64(16))


def rc_mmer(x):
    """reverse complement of a packed 15-mer (sk_rc_mmer)"""
    x = _u64(x)
    r = np.zeros_like(x)
    for _ in range(SK_M):
        r = (r << _U64(2)) | (_U64(3) - (x & _U64(3)))
        x = x >> _U64(2)
    return r


def sk_hmin_of_kmer(fw, k):
    """smallest sk_order over the canonical 15-mers of the packed k-mers fw (k <= 32)"""
    fw = _u64(fw)
    best = np.full(fw.shape, 0xFFFFFFFF, dtype=np.uint64)
    for i in range(k - SK_M + 1):
        f = (fw >> _U64(2 * (k - SK_M - i))) & _U64(SK_MMASK)
        best = np.minimum(best, sk_order(np.minimum(f, rc_mmer(f))))
    return best


def region_of_hash(keys, n_regions):
    """slot_of's region in a table whose regions are hash prefixes: fmix64(key) >> (shift + 12); n_regions is a power of two"""
    lg = int(n_regions).bit_length() - 1
    assert 1 << lg == n_regions
    return fmix64(keys) >> _U64(64 - lg) if lg else np.zeros(len(keys), dtype=np.uint64)


def region_of_bin(hmin, n_regions):
    """... and in one whose regions are minimizer bins: (sk_bin(hmin) * n_regions) >> 32"""
    return (sk_bin(hmin) * _U64(n_regions)) >> _U64(32)


def pack_windows(codes, k):
    """every window of one array of codes as an oriented packed k-mer: (hi, lo) uint64 arrays (hi = 0 for k <= 32)"""
    c = np.asarray(codes, dtype=np.uint64)
    n = len(c) - k + 1
    hi, lo = np.zeros(max(n, 0), dtype=np.uint64), np.zeros(max(n, 0), dtype=np.uint64)
    for i in range(k if n > 0 else 0):
        if i < k - 32:
            hi = (hi << _U64(2)) | c[i:i + n]
        else:
            lo = (lo << _U64(2)) | c[i:i + n]
    return hi, lo


def mmer_codes(m):
    return np.array([(m >> (2 * (SK_M - 1 - i))) & 3 for i in range(SK_M)], dtype=np.uint8)


def revcomp(codes):
    return (3 - np.asarray(codes, dtype=np.uint8)[::-1]).astype(np.uint8)


def store(reads):
    """(codes, offsets) of a list of code arrays"""
    codes = np.concatenate(list(reads) + [np.zeros(0, dtype=np.uint8)]).astype(np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return codes, off


def store_windows(codes, off, k):
    """start positions of the windows of a store that lie inside one sequence, and the sequence of each"""
    lens = np.diff(off.astype(np.int64))
    n = np.maximum(lens - k + 1, 0)
    seq = np.repeat(np.arange(len(lens)), n)
    first = np.repeat(off[:-1].astype(np.int64), n)
    within = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    return first + within, seq


# ---------------------------------------------------------------------------------------------------- minimizer bins, k = 31
def locus_flank(k):
    """bases either side of the 15-mer of a locus: k - 15, so that every one of its k - 14 windows holds the 15-mer"""
    return k - SK_M


def loci(rng, m, n, k=31):
    """n loci around the 15-mer m, every window of which has m for its minimizer (a locus with a still smaller 15-mer in a flank is
    dropped and another drawn), no two sharing a canonical k-mer: uint8 [n, 2 (k - 15) + 15], k - 14 windows a locus (k = 31: 47
    bases, 17 windows)"""
    flank = locus_flank(k)
    length, windows = 2 * flank + SK_M, flank + 1
    target = int(sk_order(np.array([min(m, int(rc_mmer(np.array([m]))[0]))]))[0])
    core = mmer_codes(m)
    out, seen = [], set()
    while len(out) < n:
        cand = rng.integers(0, 4, (n, length)).astype(np.uint8)
        cand[:, flank:flank + SK_M] = core
        flat = cand.reshape(-1)
        _, lo = pack_windows(flat, k)
        starts = (np.arange(n)[:, None] * length + np.arange(windows)[None, :])
        ok = (sk_hmin_of_kmer(lo[starts.reshape(-1)], k).reshape(n, windows) == target).all(axis=1)
        keys = sm.window_keys(flat, k, 0)[starts]
        for i in np.nonzero(ok)[0]:
            ks = set(keys[i].tolist())
            if len(ks) == windows and not (ks & seen) and len(out) < n:
                seen |= ks
                out.append(cand[i])
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------- hash prefixes
def pool(seed, k, mode, n_windows=POOL_WINDOWS):
    """one random sequence and its windows' keys, the first window of every key only: (codes, keys int64, fmix64 of the keys,
    positions)"""
    codes = np.random.default_rng(seed).integers(0, 4, n_windows + k - 1).astype(np.uint8)
    keys = sm.window_keys(codes, k, mode)
    _, first = np.unique(keys, return_index=True)
    first.sort()
    return codes, keys[first], fmix64(keys[first]), first


def pool_region(p, prefix, k, bits=HASH_BITS):
    """the pool's k-mers whose fmix64(key) has `prefix` for its top bits, as code arrays in pool order, with their keys"""
    codes, keys, mix, pos = p
    pick = np.nonzero(mix >> _U64(64 - bits) == _U64(prefix))[0]
    return [codes[int(a):int(a) + k] for a in pos[pick]], keys[pick]


# ---------------------------------------------------------------------------------------------------- the walk's solid copy
SOLID_REGION_LG = 11  # mcgpu.hip SOLID_SB: regions of 2048 slots, by the key's own hash whatever the counting table's regions are


def solid_layout(keys):
    """Where the builder of the solid copy (mcgpu.hip solid_build, k_solid_from_leaves) puts n solid keys: a table of the first power of
    two of at least 4 n slots (4096 at least), region and home slot from the top bits of fmix64(key), linear probing over
    TABLE_MAX_PROBES slots that wraps inside the region, no chain.  Returns (longest run of occupied slots, greatest displacement when
    the keys come in the order of their home slots).  The set of occupied slots of linear probing does not depend on the order of
    insertion: a longest run under 128 means that no key ever finds 128 occupied slots before it, so the copy builds.  A key whose
    displacement in home order is d has d + 1 keys before and with it whose homes lie in a window that ends at its own home, all of
    which must sit within 127 slots behind that window: d >= 128 means that one of them cannot, whatever the order, so the builder must
    refuse."""
    n = len(keys)
    lg = REGION_LG
    while (1 << lg) < 4 * n:
        lg += 1
    lg = max(lg, SOLID_REGION_LG + 1)
    size = 1 << SOLID_REGION_LG
    slot = np.sort((fmix64(keys) >> _U64(64 - lg)).astype(np.int64))
    region, home = slot >> SOLID_REGION_LG, slot & (size - 1)
    longest = displaced = 0
    for r in np.unique(region):
        h = home[region == r]
        if len(h) >= size:  # more keys than slots
            return size, len(h) - size + TABLE_MAX_PROBES
        h2 = np.concatenate([h, h + size])  # two turns round the region: the second meets what the first pushed over the end
        i = np.arange(len(h2))
        at = i + np.maximum.accumulate(h2 - i)  # the slot of every key: its home, or the slot behind the key before it
        occupied = np.zeros(size, dtype=bool)
        occupied[at[len(h):] % size] = True
        free = np.nonzero(~occupied)[0]
        gaps = np.diff(np.append(free, free[0] + size)) - 1  # occupied slots between one free slot and the next, round the region
        longest = max(longest, int(gaps.max()))
        displaced = max(displaced, int((at - h2)[len(h):].max()))
    return longest, displaced


# ---------------------------------------------------------------------------------------------------- a case
class Case:
    """What one (k, key mode) builds.  reads[name] = (codes, offsets) of the tables full, nearly, last and roomy; units[name] = the
    crowded reads of a table, one a key (hash prefixes) or a locus; absent[name] = reads of the same region that no table counts
    (name: full, last); queries = (codes, offsets) of everything shuffled; seeds[name] = the walk's seed reads (full, nearly, last)."""

    def __init__(self, k, mode):
        self.k, self.mode, self.bins = k, mode, mode == 0 and k >= 23
        rng = np.random.default_rng(9000 + 10 * k + mode)
        self.units, self.absent = {}, {}
        if self.bins:
            n_full = -(-N_FULL // LOCUS_WINDOWS)      # 330 loci, 5610 keys
            n_nearly = -(-N_NEARLY // LOCUS_WINDOWS)  # 230 loci, 3910 keys
            n_absent = -(-N_ABSENT // LOCUS_WINDOWS)  # 89 loci, 1513 keys
            a = loci(rng, M_INTERIOR, 2 * n_full + n_absent - 100)
            self.units["full"] = list(a[:n_full])
            self.units["nearly"] = list(a[n_full - 100:n_full - 100 + n_nearly])  # (100 loci of full's, the others its own)
            self.absent["full"] = list(a[2 * n_full - 100:])
            assert n_full - 100 + n_nearly <= 2 * n_full - 100
            b = loci(rng, M_LAST, n_full + n_absent)
            self.units["last"], self.absent["last"] = list(b[:n_full]), list(b[n_full:])
        else:
            p = pool(77 + 10 * k + mode, k, mode)
            for name, prefix in (("full", HASH_INTERIOR), ("last", HASH_LAST)):
                kmers, _ = pool_region(p, prefix, k)
                assert len(kmers) >= N_FULL + N_ABSENT, (name, len(kmers))
                self.units[name], self.absent[name] = kmers[:N_FULL], kmers[N_FULL:N_FULL + N_ABSENT]
                if name == "full":  # nearly: 2700 keys that full counts too, 1200 that it does not (absent from full, present here)
                    self.units["nearly"] = kmers[N_FULL - 2700:N_FULL - 2700 + N_NEARLY]
        per_read = 100
        bg = [rng.integers(0, 4, (N_BACKGROUND // per_read, k + per_read - 1)).astype(np.uint8) for _ in range(2)]
        mult = {"full": lambda i: 1 + i % 5, "nearly": lambda i: 1 + i % 3, "last": lambda i: 1 + (i + 2) % 5, "roomy": lambda i: 1 + (3 * i + 1) % 5}
        self.reads = {}
        for name in ("full", "nearly", "last", "roomy"):
            units = self.units["full" if name == "roomy" else name]
            reads = [u for i, u in enumerate(units) for _ in range(mult[name](i))]
            if name != "nearly":
                reads += list(bg[name == "roomy"])
            self.reads[name] = store([reads[i] for i in rng.permutation(len(reads))])
        # queries
        q = []
        for name in ("full", "nearly", "last"):
            q += self.units[name] + [revcomp(u) for u in self.units[name]]
        q += self.absent["full"] + self.absent["last"]
        q += list(rng.integers(0, 4, (N_ELSEWHERE, k)).astype(np.uint8))
        q += [np.zeros(0, dtype=np.uint8)] * 20 + [u[:n] for u in self.units["full"][:20] for n in (1, k - 1)]
        self.query_reads = [q[i] for i in rng.permutation(len(q))]
        self.queries = store(self.query_reads)
        # the walks' seeds: 40 counted reads of a table and 10 of its region that it does not count (nearly counts the first 1200 of the
        # hash-prefix cases' absent["full"], and none of the bin case's)
        uncounted = {"full": self.absent["full"][:10], "last": self.absent["last"][:10],
                     "nearly": self.absent["full"][:10] if self.bins else self.absent["full"][N_ABSENT - 10:]}
        self.seeds = {name: [self.units[name][i] for i in rng.choice(len(self.units[name]), 40, replace=False)] + uncounted[name]
                      for name in ("full", "nearly", "last")}

    def keys_of(self, reads):
        """the distinct keys of a list of reads (the crowded units: no window spans two of them)"""
        codes, off = store(reads)
        at, _ = store_windows(codes, off, self.k)
        return np.unique(sm.window_keys(codes, self.k, self.mode)[at])

    def regions(self, keys, n_regions, bins=None, kmers_lo=None):
        """the home region of each key in a table of n_regions regions: by minimizer bin (packed keys are their own k-mers) or by hash"""
        if self.bins if bins is None else bins:
            return region_of_bin(sk_hmin_of_kmer(keys if kmers_lo is None else kmers_lo, self.k), n_regions)
        return region_of_hash(keys, n_regions)
