"""tests/dedup_leaves.py against the C code and against its own claims (no GPU): its dd_hash, tag and home place equal what
`mc_hosttest dedup-tags` prints from csrc/kmer_hash.h, a record's windows have the keys of the record's own bases, every record of
a pool has the locus's 15-mer for the minimizer of all its windows, and every designed leaf meets the condition that makes the merge
kernel take the path tests/test_gpu_dedup_leaves.py names for it.  The conditions are checked here, from the design alone: the GPU
test then needs no luck."""
import subprocess

import numpy as np
import pytest

from tests import crowded_tables as ct
from tests import dedup_leaves as dl
from tests import seq_cov_model as sm

KS = (31, 27, 23)


@pytest.fixture(scope="module")
def hosttest():
    from metacherchant_amd import build
    build.build_host()
    return build.HOSTTEST


def test_hash_tag_and_place_are_the_header_s(hosttest, tmp_path):
    rng = np.random.default_rng(5)
    P = dl.pool_of(31)
    pick = rng.choice(len(P), 3000, replace=False)
    lo = np.concatenate([P.lo[pick], rng.integers(0, 1 << 63, 1000, dtype=np.uint64) * np.uint64(2) + np.uint64(1), np.array([0, 0, 2 ** 64 - 1], dtype=np.uint64)])
    hi = np.concatenate([P.hi[pick], rng.integers(0, 1 << 63, 1000, dtype=np.uint64) * np.uint64(2), np.array([0, 0xF << 60, 2 ** 64 - 1], dtype=np.uint64)])
    path = tmp_path / "records.txt"
    path.write_text("".join("%x %x\n" % (int(a), int(b)) for a, b in zip(lo, hi)))
    out = subprocess.run([hosttest, "dedup-tags", str(path)], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == 3 * len(lo)
    got = np.array([[int(out[i], 16), int(out[i + 1], 16), int(out[i + 2])] for i in range(0, len(out), 3)], dtype=np.uint64)
    assert np.array_equal(got[:, 0], dl.dd_hash(lo, hi))
    assert np.array_equal(got[:, 1], dl.tag(lo, hi))
    assert np.array_equal(got[:, 2].astype(np.int64), dl.home_place(lo, hi))
    assert ((got[:, 1] & np.uint64(0xFFFF)) == 0x8000).all() and (got[:, 2] < dl.D2_SLOTS).all()
    # the bin word is no part of the hash
    assert np.array_equal(dl.dd_hash(lo ^ np.uint64(0x1234), hi), dl.dd_hash(lo, hi))


@pytest.mark.parametrize("k", KS)
def test_a_record_s_windows_are_those_of_its_bases(k):
    P = dl.pool_of(k)
    rng = np.random.default_rng(k)
    pick = np.sort(rng.choice(len(P), 2000, replace=False))
    keys, rec, win = dl.expand(P.lo[pick], P.hi[pick], k)
    assert len(keys) == int(P.nw[pick].sum())
    at = 0
    for n, i in enumerate(pick):
        want = sm.window_keys(P.bases(i), k, 0)
        w = int(P.nw[i])
        assert len(want) == w and np.array_equal(keys[at:at + w], want) and (rec[at:at + w] == n).all() and win[at:at + w].tolist() == list(range(w))
        at += w
    # one record, packed by hand: 30 bases in hi under windows - 1, the rest on top of lo, the bin word below
    i = int(pick[-1])
    lo, hi = dl.record(P.bases(i), int(P.nw[i]), P.bin, k)
    assert (lo, hi) == (int(P.lo[i]), int(P.hi[i])) and hi >> 60 == P.nw[i] - 1 and lo & 0xFFFFFFFF == P.bin
    b = [int(x) for x in P.bases(i)] + [0] * 46
    assert [(hi >> (2 * (29 - j))) & 3 for j in range(30)] == b[:30] and [(lo >> (32 + 2 * (45 - j))) & 3 for j in range(30, 46)] == b[30:46]


@pytest.mark.parametrize("k", KS)
def test_the_records_are_truthful(k):
    """every window of every record of a pool has M_INTERIOR for its minimizer, so the record's bin word is its windows' bin and all
    records share a leaf whatever the table's size; window counts 1 .. min(16, k - 14) are all there, on both strands"""
    P = dl.pool_of(k)
    assert P.bin == 0x688990c0 == dl.bin_of(ct.M_INTERIOR)
    keys, _, _ = dl.expand(P.lo, P.hi, k)
    assert (ct.sk_hmin_of_kmer(keys, k) == 1).all()
    assert sorted(set(P.nw.tolist())) == list(range(1, min(16, k - 14) + 1)) and set(P.strand.tolist()) == {0, 1}
    assert len(np.unique(keys)) == dl.N_LOCI * (k - 14)  # (the two strands of a locus give the same keys)
    for n in (1024, 1085, 4096, 1 << 20):
        assert 0 < dl.leaf_of(P.bin, n) < n - 1
    assert len(set(zip(P.lo.tolist(), P.hi.tolist()))) == len(P)


def test_table_of_is_the_plain_sum():
    P = dl.pool_of(31)
    idx = np.array([0, 5, 5000, 20000])
    copies = np.array([3, 1, 40000, 2])
    want = {}
    for i, c in zip(idx, copies):
        for key in sm.window_keys(P.bases(i), 31, 0).tolist():
            want[key] = want.get(key, 0) + int(c)
    keys, counts = dl.table_of(P.lo[idx], P.hi[idx], copies, 31)
    assert dict(zip(keys.tolist(), counts.tolist())) == want and (np.diff(keys) > 0).all()
    k2, c2 = dl.table_of(P.lo[idx[:2]], P.hi[idx[:2]], copies[:2], 31, before=(keys, counts))
    for i, c in zip(idx[:2], copies[:2]):
        for key in sm.window_keys(P.bases(i), 31, 0).tolist():
            want[key] += int(c)
    assert dict(zip(k2.tolist(), c2.tolist())) == want


def test_pick_distinct_places_and_twins():
    P = dl.pool_of(31)
    idx = dl.pick_distinct_places(P.lo, P.hi, np.arange(len(P)), n=1024)
    assert sorted(dl.home_place(P.lo[idx], P.hi[idx]).tolist()) == list(range(1024))
    idx = dl.pick_distinct_places(P.lo, P.hi, np.arange(len(P))[::-1], units=777)
    assert int(dl.units_of(P.hi[idx]).sum()) == 777 and len(set(dl.home_place(P.lo[idx], P.hi[idx]).tolist())) == len(idx)
    big = dl.pool_of(31, dl.N_LOCI_TWINS)
    pairs = dl.twins(big.lo, big.hi)
    assert len(pairs) >= 20
    for i, j in pairs:
        assert (big.lo[i], big.hi[i]) != (big.lo[j], big.hi[j])
        assert dl.tag(big.lo[[i]], big.hi[[i]])[0] == dl.tag(big.lo[[j]], big.hi[[j]])[0]
        assert dl.home_place(big.lo[[i]], big.hi[[i]])[0] == dl.home_place(big.lo[[j]], big.hi[[j]])[0]


def _common(L, k):
    """what holds for every leaf: one leaf, a region that stays roomy, the table equal to the expansion copy by copy"""
    assert ((L.lo & np.uint64(0xFFFFFFFF)) == np.uint64(0x688990c0)).all()
    assert len(L.keys) <= 1800 and L.records == len(L.instances()) and np.array_equal(np.bincount(L.instances()), L.copies)
    assert int(L.counts.sum()) == int((dl.windows_of(L.hi) * L.copies).sum())
    if L.bases is not None:
        for i in (0, L.distinct // 2, L.distinct - 1):
            assert dl.record(L.bases[i], len(L.bases[i]) - k + 1, L.bin, k) == (int(L.lo[i]), int(L.hi[i]))


@pytest.mark.parametrize("k", KS)
def test_every_leaf_meets_its_condition(k):
    C = dl.cases(k)
    wmax = min(16, k - 14)
    for L in C.values():
        _common(L, k)
    # quiet: one turn, one round, every window count (odd ones leave a pair's second window empty), 1 to 5 copies
    L = C["quiet"]
    assert L.distinct == 200 and L.all_placed and L.records <= dl.D2_SLOTS and L.units <= dl.D2_UL_CAP
    assert sorted(set(dl.windows_of(L.hi).tolist())) == list(range(1, wmax + 1)) and sorted(set(L.copies.tolist())) == [1, 2, 3, 4, 5]
    assert (L.counts >= 4).sum() >= 100 and L.max_count < 200
    # second turn: the records of the second turn find the entries of the first (every distinct record has a copy in both)
    for total in (1025, 3000):
        L = C["second-turn-%d" % total]
        assert L.records == total > dl.D2_SLOTS and L.distinct == 600 and L.all_placed and L.records <= dl.DD_MAX_CAP
        inst = L.instances()
        assert len(set(inst[:dl.D2_SLOTS].tolist()) & set(inst[dl.D2_SLOTS:].tolist())) >= (1 if total == 1025 else 500)
    # unit boundary
    for units, rounds in ((1976, 1), (1977, 2)) + (((3953, 3),) if k == 31 else ()):
        L = C["units-%d" % units]
        assert L.all_placed and L.units == units and L.rounds() == rounds and L.records == L.distinct <= dl.D2_SLOTS
    # no place: at least 476 distinct records without one, and units for three rounds (two where k < 31) among those that have one
    L = C["no-place"]
    assert L.distinct == 1500 and L.records == 3000 and L.distinct - dl.D2_SLOTS >= 476 and (dl.windows_of(L.hi) >= wmax - 3).all()
    assert L.units_at_least > 2 * dl.D2_UL_CAP if k == 31 else L.units_at_least > dl.D2_UL_CAP
    if k != 31:
        assert set(C) == {"quiet", "second-turn-1025", "second-turn-3000", "units-1976", "units-1977", "no-place"}
        return
    # twins: the quiet leaf, and two records that differ but share tag and place, at a place no other record has
    L, Q = C["twins"], C["quiet"]
    assert L.distinct == Q.distinct + 2 and L.copies[-2:].tolist() == [3, 5] and L.records <= dl.D2_SLOTS and L.units <= dl.D2_UL_CAP
    a, b = L.distinct - 2, L.distinct - 1
    assert (L.lo[a], L.hi[a]) != (L.lo[b], L.hi[b])
    assert dl.tag(L.lo[[a]], L.hi[[a]])[0] == dl.tag(L.lo[[b]], L.hi[[b]])[0]
    place = dl.home_place(L.lo, L.hi)
    assert place[a] == place[b] and L.distinct_places == L.distinct - 1 and (place[:a] != place[a]).all()
    # many copies: the 13-bit copy field near its mask and at DD_MAX_CAP, all it must hold
    L = C["copies-4000"]
    assert L.distinct == 97 and L.max_copies == 4000 and L.records == 4096 and dl.windows_of(L.hi)[0] == 16 and L.all_placed
    assert 0x7FF < L.max_copies <= 0x1FFF and L.max_count >= 4000  # (twelve bits in use)
    L = C["copies-4096"]
    assert L.distinct == 1 and L.max_copies == L.records == dl.DD_MAX_CAP == 0x1000 > 0xFFF  # (the thirteenth bit) and dl.windows_of(L.hi)[0] == 16 and L.max_count == 4096
    # hand-over
    for total in (4096, 4097):
        L = C["hand-over-%d" % total]
        assert L.records == total and L.distinct == 500 and L.all_placed
    # crossings: one round, every window a key of its own that reaches the threshold (and the latest pick, 4) at once:
    # two crossings a unit, where a wave has half a word of the list a unit to note them in
    L = C["crossings"]
    assert L.distinct == 30 and L.cov_hint == 5 and L.units == 240 <= dl.D2_UL_CAP and len(L.keys) == 2 * L.units and (L.counts == 40).all()
    # the counter bound's record: one key, 0, sixteen times a record
    lo, hi = dl.poly_a()
    keys, counts = dl.table_of(lo, hi, [3000], 31)
    assert keys.tolist() == [0] and counts.tolist() == [48000] and dl.leaf_of(int(lo[0]) & 0xFFFFFFFF, 1085) == 0
    assert min(48000, 32767) + 4096 * 16 == 98303 < 1 << 17
