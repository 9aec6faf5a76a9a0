"""CPU: tests/set_keys.py, the designer of key sets for the per-call k-mer sets of reads_in_set.hip, unitigs.hip, env_join.hip and
trim_paths.hip.  Its restatement of csrc/kmer_set.h is held to the header itself, compiled as host C++ into a small program; what a
compile cannot reach (the size rule, the filter's functions, tp_home's argument order) is pinned by regular expression; and every
named set is held to its name by the slot model alone: run length, the wrap with its slots on both sides, the shape entries inside
the run, the slots each designed miss reads, the shared and the differing words of a family, isolation, no duplicates, the load."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import reads_filter_model as rf
from tests import set_keys as sk

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metacherchant_amd", "csrc")
U = np.uint64

RUN_KS = (31, 32, 33, 47, 63)
HALF_K = {32: 31, 33: 33, 64: 32, 65: 47, 128: 63, 129: 33}
CASES = [("run_wrap", k, u, 0) for u in sk.UNITS for k in RUN_KS] + [("run_big", k, u, 0) for u in sk.UNITS for k in (31, 63)]
CASES += [("shared_first_word", k, u, 0) for u in sk.UNITS[:3] for k in (33, 47, 63)]
CASES += [("shared_low_word", k, sk.TRIM_PATHS, 0) for k in (33, 41, 63)]
CASES += [("half_full", HALF_K[n], u, n) for u in sk.UNITS for n in sk.HALF_FULL_N]
IDS = ["%s-k%d-%s%s" % (name, k, u, "-n%d" % n if n else "") for name, k, u, n in CASES]


def make(name, k, unit, n):
    if name == "half_full":
        return sk.half_full(k, unit, n)
    if name == "shared_low_word":
        return sk.shared_low_word(k)
    return getattr(sk, name)(k, unit)


# ---- the restatement against the header, compiled

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
using std::min;
#include "kmer_set.h"
int main()
{
    char what;
    int k, lg;
    unsigned long long w[4];
    while (scanf(" %c %d %d %llx %llx %llx %llx", &what, &k, &lg, &w[0], &w[1], &w[2], &w[3]) == 7) {
        RsKey key{w[0], w[1]};  // 'h': a key as given (the trim hands rs_hash its oriented words)
        if (what == 'k') key = k > 32 ? rs_key<true>(w[0], w[1], w[2], w[3]) : rs_key<false>(w[0], w[1], w[2], w[3]);
        const uint32_t h0 = rs_hash<false>(key), h1 = rs_hash<true>(key);
        printf("%llx %llx %x %x %llx %llx %d\n", (unsigned long long)key.a, (unsigned long long)key.b, h0, h1, (unsigned long long)rs_home(h0, lg),
               (unsigned long long)rs_home(h1, lg), key.a == RS_EMPTY || (k > 32 && key.b == RS_EMPTY));
    }
    return 0;
}
"""


def _compiler():
    """(clang++, the ROCm include directory) or None"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    roots = [os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))] if os.path.exists(hipcc) else []
    roots += [os.environ.get("ROCM_PATH") or "/opt/rocm"]
    for root in roots:
        cxx, inc = os.path.join(root, "lib", "llvm", "bin", "clang++"), os.path.join(root, "include")
        if os.path.exists(cxx) and os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
            return cxx, inc
    return None


def _candidates():
    """(k, lg, codes) of a few thousand k-mers: random ones at every k of the tests, both sides of the word edge, and the designed ones"""
    rng = np.random.default_rng(5)
    out = [(k, lg, rng.integers(0, 4, (200, k), dtype=np.uint8)) for k in (1, 5, 16, 31, 32, 33, 34, 47, 48, 62, 63) for lg in (6, 13, 31)]
    for k in (32, 33, 63):  # words of all ones and all zeros on either strand
        out.append((k, 8, np.array([[0] * k, [3] * k, [0] * (k - 1) + [3], [3] + [0] * (k - 1), [2] * k], dtype=np.uint8)))
    for name, k, unit in (("run_wrap", 31, sk.UNITIGS), ("run_wrap", 33, sk.ENV_JOIN), ("shared_first_word", 63, sk.READS_IN_SET),
                          ("shared_first_word", 47, sk.UNITIGS), ("shared_low_word", 41, sk.TRIM_PATHS), ("run_wrap", 32, sk.TRIM_PATHS)):
        case = make(name, k, unit, 0)
        out.append((k, case.lg, sk.codes_of(case.entries + case.misses, k)))
    return out


def test_the_restatement_is_the_header_compiled(tmp_path):
    found = _compiler()
    if found is None:
        pytest.skip("no clang++ of a ROCm installation to compile csrc/kmer_set.h with")
    cxx, inc = found
    src, exe = tmp_path / "set_keys_pin.cpp", tmp_path / "set_keys_pin"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", CSRC, "-o", str(exe), str(src)], check=True)
    lines, want = [], []
    for k, lg, codes in _candidates():
        fhi, flo = sk.pack(codes)
        rhi, rlo = sk.pack(sk.rc_codes(codes))
        a, b = sk.rs_key(k, fhi, flo, rhi, rlo)
        for what, w in (("k", (fhi, flo, rhi, rlo)), ("h", (flo, fhi, rhi, rlo))):
            ka, kb = (a, b) if what == "k" else (flo, fhi)
            h0, h1 = sk.rs_hash(ka, kb, False), sk.rs_hash(ka, kb, True)
            for i in range(len(codes)):
                lines.append("%s %d %d %x %x %x %x" % (what, k, lg, int(w[0][i]), int(w[1][i]), int(w[2][i]), int(w[3][i])))
            want += list(zip(ka.tolist(), kb.tolist(), h0.tolist(), h1.tolist(), sk.rs_home(h0, lg).tolist(), sk.rs_home(h1, lg).tolist()))
            if what == "h":  # the trim's home is this hash of its oriented words
                assert np.array_equal(sk.tp_home(k, fhi, flo, lg), sk.rs_home(h1 if k >= 33 else h0, lg))
                assert np.array_equal(sk.homes_of_codes(codes, sk.TRIM_PATHS, lg), sk.tp_home(k, fhi, flo, lg).astype(np.int64))
            else:
                assert np.array_equal(sk.homes_of_codes(codes, sk.UNITIGS, lg), sk.rs_home(h1 if k > 32 else h0, lg).astype(np.int64))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(want) > 4000 and len(out) == len(want) + 1
    for line, row, given in zip(out, want, lines):
        got = line.split()
        assert tuple(int(x, 16) for x in got[:6]) == row, (given, line, row)
        assert given[0] == "h" or got[6] == "0", given  # no canonical k-mer's word is the free-slot mark


def test_smaller_of_two_and_the_reverse_complement():
    rng = np.random.default_rng(9)
    for k in (5, 31, 32, 33, 63):
        codes = rng.integers(0, 4, (300, k), dtype=np.uint8)
        texts = sk.text_of(codes)
        assert sk.text_of(sk.rc_codes(codes)) == [sk.rc(s) for s in texts] and [sk.rc(sk.rc(s)) for s in texts] == texts
        assert np.array_equal(sk.codes_of(texts, k), codes)
        num = lambda s: int("".join(str(sk.LETTERS.index(c)) for c in s), 4)
        fhi, flo = sk.pack(codes)
        assert [(int(h) << 64) | int(l) for h, l in zip(fhi, flo)] == [num(s) for s in texts]
        a, b, fw = sk.key_of_codes(codes)
        for s, ai, bi, f in zip(texts, a.tolist(), b.tolist(), fw.tolist()):
            v = min(num(s), num(sk.rc(s)))
            assert f == (num(s) <= num(sk.rc(s)))
            assert (ai, bi) == ((v, 0) if k <= 32 else (v >> 63, v & (2 ** 63 - 1)))


# ---- what a compile cannot reach

def test_the_size_rule_the_filter_and_the_trims_key_are_the_kernels():
    src = {f: open(os.path.join(CSRC, f + ".hip")).read() for f in ("reads_in_set", "unitigs", "env_join", "trim_paths")}
    for name, text in src.items():
        rule = re.findall(r"int lg_cap = (\d+);\s*while \(\(1ull << lg_cap\) < 2 \* (?:\(uint64_t\))?(\w+)\) lg_cap\+\+;", text)
        assert rule == [(str(sk.LG_CAP_MIN), "n_set" if name == "reads_in_set" else "n")], (name, rule)
        assert len(re.findall(r"s = \(s \+ 1\) & mask\)", text)) == 2, name  # the build's probing and the look-up's
    assert [sk.lg_cap(n) for n in (1, 32, 33, 64, 65, 128, 129, 4096, 4097)] == [6, 6, 7, 7, 8, 8, 9, 13, 14]
    rs = src["reads_in_set"]
    assert re.search(r"constexpr int RS_FILTER_WORDS_LG = %d;" % sk.RS_FILTER_WORDS_LG, rs)
    assert "uint64_t rs_filter_bits(uint32_t h) { return (1ull << (h & 63)) | (1ull << ((h >> 6) & 63)) | (1ull << ((h >> 12) & 63)); }" in rs
    assert "uint32_t rs_filter_word(uint32_t h) { return h >> (32 - RS_FILTER_WORDS_LG); }" in rs
    h = np.array([0, 1, 0xFFFFFFFF, 0x12345678, 0x80000000], dtype=U)
    assert sk.rs_filter_word(h).tolist() == [int(x) >> 18 for x in h]
    assert sk.rs_filter_bits(h).tolist() == [(1 << (int(x) & 63)) | (1 << ((int(x) >> 6) & 63)) | (1 << ((int(x) >> 12) & 63)) for x in h]
    tp = src["trim_paths"]
    assert "return rs_home(rs_hash<WIDE>(RsKey{v.lo, v.hi}), lg_cap);" in tp
    assert re.search(r"constexpr int TP_WIDE_K = 33;", tp) and "const bool wide = c->cfg.k >= TP_WIDE_K;" in tp
    for name in ("reads_in_set", "unitigs", "env_join"):
        assert re.search(r"wide = (c->cfg\.)?k > 32;", src[name]), name


# ---- the slot model

def test_the_slot_model_on_tables_by_hand():
    m = sk.occupied([5, 5, 5, 62, 63, 63, 63, 20], 6)
    assert sorted(np.nonzero(m.slots)[0].tolist()) == [0, 1, 5, 6, 7, 20, 62, 63]
    assert sorted(m.runs) == [(5, 3), (20, 1), (62, 4)] and m.longest == 4 and m.wraps and m.wrapping == (62, 4)
    assert m.run_of(1) == (62, 4) and m.run_of(2) is None and m.run_of(7) == (5, 3)
    assert [m.visits(h) for h in (62, 63, 0, 1, 2, 5, 7, 20)] == [5, 4, 3, 2, 1, 4, 2, 2]
    rng = np.random.default_rng(3)
    homes = rng.integers(40, 64, 30)
    a, b = sk.occupied(homes, 6), sk.occupied(rng.permutation(homes), 6)
    assert np.array_equal(a.slots, b.slots) and a.runs == b.runs  # whatever the order
    assert not sk.occupied([3, 4], 6).wraps


# ---- every named set is what it is called

def _canon(case, s):
    return s if case.unit == sk.TRIM_PATHS else min(s, sk.rc(s))


@pytest.mark.parametrize("name,k,unit,n", CASES, ids=IDS)
def test_a_named_set_is_what_it_is_called(name, k, unit, n):
    case = make(name, k, unit, n)
    entries, cap = case.entries, 1 << case.lg
    mask = cap - 1
    keys = [_canon(case, s) for s in entries]
    assert len(set(keys)) == len(entries)  # no entry twice, none beside its reverse complement where the strands fold
    assert case.lg == sk.lg_cap(len(entries))
    model = sk.occupied(sk.homes(entries, k, unit, case.lg), case.lg)
    first, length = model.wrapping
    assert model.wraps and (first, length) == case.run and length == model.longest
    before, behind = cap - first, first + length - cap
    crowd_homes = sk.homes(case.crowd, k, unit, case.lg)
    assert (crowd_homes >= cap - (cap >> 4)).all() and set(case.crowd) <= set(entries)
    if name == "run_big":
        assert 2048 < len(entries) <= 4096 and cap == 8192 and length >= 300 and before >= 8 and behind >= 8
    elif name == "half_full":
        assert len(entries) == n and len(case.crowd) == n // 2 and length >= n // 2
        assert (2 * n == cap) if n % 2 == 0 else (cap == 4 * (n - 1))  # load exactly 0.5, or the doubled table one entry on
        # run_wrap's crowd has 8 slots and more in front of the wrap; the last cap/16 slots of 64 are 4, and 16 members (n = 32, 33)
        # make one run only from 4 slots: there the run begins 4 slots before the wrap, from n = 64 on 8 and more
        assert before >= (8 if n >= 64 else 4) and behind >= 8
    else:
        assert length >= 40 and before >= 8 and behind >= 8
    # the unit's own entries inside the run: they are displaced, or displace a member of the crowd
    own = case.shape.entries + case.extra
    inside = [s for s, h in zip(own, sk.homes(own, k, unit, case.lg)) if (int(h) - first) & mask < length]
    assert sorted(inside) == sorted(case.in_run) and (name == "half_full" or len(inside) >= 3)
    # the designed misses: absent, at home in the run's first slot, refused only after the whole run and the wrap
    have = set(keys)
    assert len(case.misses) >= (1 if (name, k) == ("shared_low_word", 33) else 2)
    for x in case.misses:
        h = int(sk.homes([x], k, unit, case.lg)[0])
        assert _canon(case, x) not in have and h == first and model.visits(h) == length + 1
    # the crowd is isolated: a member's only neighbours are the carriers that look it up
    near = sk.neighbour_map(entries, k)
    at = {s: i for i, s in enumerate(entries)}
    carriers_of = {}
    for e, side, x in case.hit_carriers:
        carriers_of.setdefault(x, set()).add(at[e])
    for s in case.crowd:
        assert near[at[s]] == carriers_of.get(s, set()), s
    assert {x for _, _, x in case.hit_carriers} <= set(case.crowd) and set(case.hits) <= set(case.crowd)
    if name != "half_full":
        # every member is looked up, and wherever the entries went in, the one in the crowd's last slot lies more than 32 slots behind
        # its home: a look-up that gives up after 32 probes misses a member
        span = int(crowd_homes.max() - crowd_homes.min()) + 1  # (the members go to slots from their first home on)
        assert set(case.hits) == set(case.crowd) and len(case.crowd) - span >= 33
        assert unit in (sk.READS_IN_SET, sk.ENV_JOIN) or {x for _, _, x in case.hit_carriers} == set(case.crowd)
    if unit in (sk.UNITIGS, sk.TRIM_PATHS):
        assert len(case.miss_carriers) >= 2 and len(case.hit_carriers) >= 2
    for e, side, x in case.miss_carriers:  # the carrier's four strings on that side: the miss, and three more that are absent
        assert (e[1:] == x[:-1]) if side > 0 else (e[:-1] == x[1:])
        four = [e[1:] + c for c in sk.LETTERS] if side > 0 else [c + e[:-1] for c in sk.LETTERS]
        assert x in four and x in case.misses and not {_canon(case, y) for y in four} & have
    for e, side, x in case.hit_carriers:
        four = [e[1:] + c for c in sk.LETTERS] if side > 0 else [c + e[:-1] for c in sk.LETTERS]
        assert x in four and len({_canon(case, y) for y in four} & have) == 1
    # the families
    if name == "shared_first_word":
        fam = case.crowd + case.misses
        a, b, fw = sk.key_of_codes(sk.codes_of(fam, k))
        assert len(case.crowd) >= 40 and len(set(a.tolist())) == 1 and len(set(b.tolist())) == len(fam) and fw.all()
        assert all(s[0] == "A" and s[-1] != "T" for s in fam)
        shared = 2 * k - 63
        bits = ["".join(format(sk.LETTERS.index(c), "02b") for c in s) for s in fam]
        assert len({x[:shared] for x in bits}) == 1 and (k == 33 or len({x[:shared + 6] for x in bits}) > 1)
    if name == "shared_low_word":
        hi, lo = sk.pack(sk.codes_of(case.crowd + case.misses, k))
        n_fam = int((lo == lo[-1]).sum())  # (the misses are of the family)
        assert n_fam == (len(lo) if k > 33 else n_fam) and n_fam >= (3 if k == 33 else 40 + len(case.misses))
        fam = lo == lo[-1]
        assert len(set(hi[fam].tolist())) == n_fam and (lo[len(case.crowd):] == lo[-1]).all()
    # reads-in-set: the designed reads
    if unit == sk.READS_IN_SET:
        reads, members, pct = sk.reads_case(case)
        mem = rf.make_set(members)
        got = [rf.hits_and_keep(r, k, mem, pct) for r in reads]
        n_shape = len(case.shape.reads)
        assert all(g == (1, True) for g in got[n_shape:n_shape + len(case.crowd)])
        assert all(g == (0, False) for g in got[n_shape + len(case.crowd):])
        if name != "half_full":  # the two reads whose only member-free window is a miss, one hit short of the threshold
            for r, x in zip(reads[n_shape - 2:n_shape], case.misses[:2]):
                w = [r[i:i + k] for i in range(len(r) - k)]
                assert [y for y in w if rf.normalize_dna(y) not in mem] == [x]
                assert rf.hits_and_keep(r, k, mem, pct) == (18, False) and rf.threshold(len(r), k, pct) == 19
                assert rf.hits_and_keep(r, k, mem | {rf.normalize_dna(x)}, pct) == (19, True)


@pytest.mark.parametrize("k", (31, 33, 63))
def test_filter_pass_is_what_it_is_called(k):
    case = sk.filter_pass(k)
    hashes = lambda xs: sk.hash_of_codes(sk.codes_of(xs, k), sk.READS_IN_SET)
    everyone = case.entries + case.misses
    assert len({min(s, sk.rc(s)) for s in everyone}) == len(everyone) and case.lg == sk.lg_cap(len(case.entries))
    assert len(case.crowd) >= 8 and set(sk.rs_filter_word(hashes(case.crowd)).tolist()) == {case.word}
    h = hashes(case.entries)
    there = sk.rs_filter_word(h) == U(case.word)
    union = int(np.bitwise_or.reduce(sk.rs_filter_bits(h[there])))  # what the whole set writes into that word of the filter
    assert union == case.bits and there.sum() == len(case.crowd)
    for group, short in ((case.passers, 0), (case.near, 1)):
        hg = hashes(group)
        assert len(group) >= 4 and set(sk.rs_filter_word(hg).tolist()) == {case.word}
        assert [bin(int(b) & ~union).count("1") for b in sk.rs_filter_bits(hg)] == [short] * len(group)
    reads, members, pct = sk.reads_case(case)
    mem = rf.make_set(members)
    got = [rf.hits_and_keep(r, k, mem, pct) for r in reads]
    assert got == [(18, False)] + [(1, True)] * len(case.crowd) + [(0, False)] * (len(case.misses) - 1)
    x, r = case.passers[0], reads[0]  # the window the filter passes is its read's only member-free one, one hit short of the threshold
    assert [y for y in (r[i:i + k] for i in range(len(r) - k)) if rf.normalize_dna(y) not in mem] == [x]
    assert rf.threshold(len(r), k, pct) == 19 and rf.hits_and_keep(r, k, mem | {rf.normalize_dna(x)}, pct) == (19, True)


def test_the_word_level_reverse_complement():
    rng = np.random.default_rng(11)
    for k in (1, 5, 31, 32, 33, 47, 63):
        hi, lo = sk.random_words(rng, 300, k)
        codes = sk.codes_of(sk.unpack(hi, lo, k), k)
        assert np.array_equal(np.stack(sk.pack(codes)), np.stack([hi, lo]))
        assert np.array_equal(np.stack(sk.rc_words(hi, lo, k)), np.stack(sk.pack(sk.rc_codes(codes))))
