"""The designer of tests/join_keys.py without a GPU: k-mers composed for chosen keys have those keys by the oracle's own key function,
and every family meets the condition its name states, for every (k, bin rule, f2_lg) tests/test_gpu_join_keys.py runs.

Wall time of the module: 54 s for its 76 cases on one CPU core, most of it the oracle's tables of the sixteen backgrounds (the searches are drawn 4096 k-mers at a time in numpy, the designs are cached)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import join_keys as jk
from tests import long_loci as ll

CASES = [(name,) + p for name in jk.FAMILIES for p in jk.PARAMS]
IDS = ["%s-k%d-rule%d-f2lg%d" % c for c in CASES]


def test_preimage_has_the_key_it_was_composed_for():
    rng = np.random.default_rng(4100)
    seen = 0
    for k in (41, 47, 63):
        for key in rng.integers(0, 1 << 63, 67, dtype=np.uint64).tolist():
            key = (key << 1 | int(rng.integers(0, 2))) & ((1 << 64) - 1)  # (all 64 bits drawn)
            kmers = jk.preimages(k, key, rng, 3)
            assert len({bytes(c) for c in kmers}) == 3 and all(len(c) == k and c.max() <= 3 for c in kmers)
            for c in kmers:
                assert po.key(c, k, po.KEY_POLY) == jk.signed(key)
                assert po.key(ll.revcomp(c), k, po.KEY_POLY) == jk.signed(key)
            seen += 1
    assert seen >= 200


def test_preimages_in_regions_differ_in_their_regions():
    rng = np.random.default_rng(4101)
    for k, rule in ((41, 1), (63, 2)):
        kmers = jk.preimages_in_regions(k, 0x0123456789ABCDEF, rng, 12, rule, jk.REGIONS, avoid=(5, 6))
        regions = [jk.region_of_kmer(c, k, rule) for c in kmers]
        assert len(set(regions)) == 12 and not set(regions) & {0, 5, 6}


def test_placement_functions_on_known_words():
    """the restated mixers against their definitions worked out with Python integers"""
    M = (1 << 32) - 1
    for key in (0, 1, 0xFFFFFFFFFFFFFFFE, 0x0123456789ABCDEF, 0x8000000000000000, 0xDEADBEEFCAFEF00D):
        lo, hi = key & M, key >> 32
        x = (lo * 0x9E3779B1 + hi * 0x85EBCA6B) & M
        x ^= x >> 15
        x = x * 0xC2B2AE35 & M
        a = np.array([key], dtype=np.uint64)
        assert int(jk.sk_home_mix(a)[0]) == x
        assert int(jk.dup_b1(a)[0]) == x >> 24 and int(jk.dup_f2(a, 0)[0]) == 0
        for f2_lg in (1, 2, 10):
            assert int(jk.dup_f2(a, f2_lg)[0]) == ((x << 8) & M) >> (32 - f2_lg)
            assert int(jk.dup_sub(a, f2_lg)[0]) == x >> (24 - f2_lg)
        y = (hi * 0x9E3779B1 & M) ^ (lo * 0xC2B2AE35 & M)
        y ^= y >> 16
        y = y * 0x7FEB352D & M
        y ^= y >> 15
        assert int(jk.dup_mix3(a)[0]) == y
        z = (lo * 0x85EBCA6B + hi * 0x27D4EB2F) & M
        z ^= z >> 13
        z = z * 0x165667B1 & M
        z ^= z >> 16
        assert int(jk.dup_fp(a)[0]) == z | 1
        f = key
        f ^= f >> 33
        f = f * 0xff51afd7ed558ccd & ((1 << 64) - 1)
        f ^= f >> 33
        f = f * 0xc4ceb9fe1a85ec53 & ((1 << 64) - 1)
        f ^= f >> 33
        assert int(jk.fmix64(a)[0]) == f
        assert int(ll.sk_home(a)[0]) == x >> 20  # (the join cuts by the bits the table's home slot starts with)
    assert [jk.f2_lg_for(n) for n in (1, 460800, 460801, 921600, 921601, 1 << 40)] == [0, 0, 1, 1, 2, 10]


def test_join_model_on_a_table_written_out():
    keys = [7, 7, 7, 9, 9, 5, 5, 5, -3]
    regions = [1, 1, 2, 4, 4, 3, 2, 1, 8]
    counts = [2, 3, 10, 1, 1, 1, 1, 1, 6]
    m = jk.join_model(keys, regions, counts)
    assert m["slots"] == 7 and m["keys"] == 4 and m["dup_keys"] == 2
    assert m["listed"].tolist() == [5, 7] and m["sums"].tolist() == [3, 15]
    assert m["regions_of"] == {5: [1, 2, 3], 7: [1, 2]} and m["own"] == {5: [1, 1, 1], 7: [5, 10]}


@pytest.mark.parametrize("name,k,rule,f2_lg", CASES, ids=IDS)
def test_family_is_what_its_name_says(name, k, rule, f2_lg):
    F = jk.family(name, k, rule, f2_lg)
    B = F.background()
    m = F.model()
    # every designed k-mer has its key, sits where the design says, and a key's k-mers lie in pairwise different regions
    per_key = {}
    for key, codes, region, copies, at in F.kmers:
        assert po.key(codes, k, po.KEY_POLY) == key != -1 and region == jk.region_of_kmer(codes, k, rule) != 0
        assert bytes(codes) in bytes(F.reads[at]) and len(F.reads[at]) in (k, k + 2 * jk.FLANK) and F.copies[at] == copies
        per_key.setdefault(key, []).append(region)
    for key, regions in per_key.items():
        assert len(set(regions)) == len(regions)
        assert (key in F.designed) == (len(regions) >= 2) and (key in F.single) == (len(regions) == 1)
    # no designed window falls into a background read, and the reverse (Family.model asserts the same of every window);
    # the listed set is the designed one: neither the flanks nor the background add an equal key in two regions
    wk = np.unique(np.concatenate([ll.window_keys(r, k) for r in F.reads]))
    assert not np.isin(wk, B.keys).any() and not np.isin(B.keys, wk).any() and -1 not in wk
    assert m["listed"].tolist() == sorted(F.designed) and m["dup_keys"] == len(F.designed)
    assert {key: sorted(r) for key, r in F.designed.items()} == m["regions_of"]
    assert m["keys"] == len(wk) + len(B.keys) and m["slots"] == m["keys"] + sum(len(r) - 1 for r in F.designed.values())
    # the table's size puts the join at the f2_lg the case is named for, by its keys and by its slots
    assert jk.f2_lg_for(m["keys"]) == jk.f2_lg_for(m["slots"]) == f2_lg
    assert (m["slots"] <= 460800) if f2_lg == 0 else (460801 <= m["keys"] and m["slots"] <= 921600)
    all_keys = np.concatenate([wk, B.keys])
    sub = jk.dup_sub(all_keys, f2_lg)
    listed_sub = jk.dup_sub(np.array(sorted(F.designed), dtype=np.int64), f2_lg) if F.designed else np.zeros(0, dtype=np.int64)

    def no_accidental_twin(s):
        """no two different keys of sub-bucket s share their dup_fp: k_dup_find notes nothing there but slots of equal keys"""
        fp = jk.dup_fp(all_keys[sub == s])
        return len(np.unique(fp)) == len(fp)

    if name in ("pairs", "multi"):
        assert len(set(listed_sub.tolist())) == len(F.designed)  # (all sub-buckets distinct)
    if name == "pairs":
        assert len(F.designed) == 64 and all(m["own"][key] in ([3, 5], [5, 3]) for key in F.designed)
    if name == "multi":
        assert sorted(len(r) for r in F.designed.values()) == [3, 3, 4, 5, 9, 110]
        own = m["own"][F.extra["sum-only"]]
        assert max(own) < jk.COV_HINT <= sum(own)
        assert m["own"][F.extra["saturated"]] == [300] * 110 and 110 * 300 > 32767
        assert len({tuple(sorted(v)) for v in m["own"].values()}) == 6 and all(len(set(v)) > 1 for key, v in m["own"].items() if key != F.extra["saturated"])
    if name.startswith("noted-"):
        n = int(name[6:])
        s = F.extra["sub9"] >> (1 - f2_lg)
        assert (listed_sub == s).all() and len(F.designed) == n + (name == "noted-40")
        assert F.noted(F.extra["sub9"]) == {32: 32, 33: 33, 40: 42}[n]  # (the note takes DUP_MAX_CAND = 32)
        assert sorted(len(r) for r in F.designed.values()) == [2] * n + [3] * (name == "noted-40")
        assert no_accidental_twin(s)
    if name == "fp-twins":
        assert len(F.extra["twins"]) == 10 and len(F.designed) == 3 and len(F.single) == 17
        for i, (a, b) in enumerate(F.extra["twins"]):
            ab = np.array([a, b], dtype=np.int64)
            assert a != b and jk.dup_sub(ab, f2_lg)[0] == jk.dup_sub(ab, f2_lg)[1] and jk.sub9(ab)[0] == jk.sub9(ab)[1]
            assert jk.dup_fp(ab)[0] == jk.dup_fp(ab)[1] and (int(jk.dup_mix3(ab)[0]) ^ int(jk.dup_mix3(ab)[1])) & 8191 == 0
            assert ((a in F.designed), (b in F.designed)) == ((False, False) if i < 8 else (True, False) if i == 8 else (True, True))
            fp = jk.dup_fp(all_keys[sub == jk.dup_sub(ab, f2_lg)[0]])
            assert len(fp) - len(np.unique(fp)) == 1  # (the twins and nobody else)
        assert len({int(jk.sub9(np.array([a]))[0]) for a, _ in F.extra["twins"]}) == 10
    if name == "many-slots":
        assert [len(r) for r in F.designed.values()] == [73]
    if name == "retreat":
        # three keys, 33 slots each: every key is noted 32 times, which the note just takes, and is listed once: the fix-up plans for
        # 8 * 3 + 64 = 88 slots and finds 99
        assert [len(r) for r in F.designed.values()] == [33] * 3 and len(set(listed_sub.tolist())) == 3
        assert all(F.noted(int(jk.sub9(np.array([key]))[0])) == jk.DUP_MAX_CAND for key in F.designed)
        assert m["slots"] - m["keys"] + 3 == 99 > 8 * 3 + 64
        assert all(no_accidental_twin(s) for s in listed_sub.tolist())
    if name == "phantoms":
        assert not F.designed and len(F.extra["w"]) == len(set(F.extra["w_keys"])) == 70 and len(F.seeds) == 74
        s = F.extra["sub9"] >> (1 - f2_lg)
        counted = {bytes(r[i:i + k]) for r in F.reads for i in range(len(r) - k + 1)}
        counted |= {bytes(ll.revcomp(np.frombuffer(c, dtype=np.uint8))) for c in counted}
        ends = {}
        for read in F.seeds:
            ends.setdefault(bytes(read[-k + 1:]), set()).add(bytes(read[-k:]))
        by_key = {key: codes for key, codes, _, _, _ in F.kmers}
        for key, w in zip(F.extra["w_keys"], F.extra["w"]):
            u = by_key[key]
            assert po.key(w, k, po.KEY_POLY) == key and int(jk.dup_sub(np.array([key]), f2_lg)[0]) == s
            assert bytes(w) not in counted and bytes(w[:-1]) in ends
            assert u[0] != w[0] and u[-1] != w[-1] and jk._forward_is_canonical(w, k) and jk._forward_is_canonical(u, k)
            assert F.extra["regions"][key] == (jk.region_of_kmer(w, k, rule), jk.region_of_kmer(u, k, rule)) and len(set(F.extra["regions"][key])) == 2
        assert sorted(len(ends[bytes(w[:-1])]) for w in F.extra["w"]) == [1] * 66 + [2] * 4
        assert len(ends) == 70 > 64  # (k_pq_match takes the queries of a sub-bucket 64 at a time)
