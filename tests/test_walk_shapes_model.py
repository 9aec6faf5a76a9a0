"""tests/walk_shapes.py without a GPU: every designed input has the shape it claims.  The histogram of the distances of the oracle's
walk (oracle/pyoracle.py bfs) equals the widths the case states for itself, in every direction it is walked; the named edges -- a
frontier of flim and of flim + 1 vertices for either number of neighbours, 8 and 9 walkers, 128 and 129 parents (512 and 516
candidates), the level of a branch, the level a walker ends at, the duplicates of the seeds -- are where the GPU test aims them; the
merging parents of the full fan lie in the chunks claimed; and the restatement of the visited index's hash equals the header's.
No case is skipped or filtered: one whose walk has another shape fails here, not on the GPU."""
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import walk_shapes as ws

MODES = {21: po.KEY_PACKED, 31: po.KEY_PACKED, 32: po.KEY_POLY, 40: po.KEY_POLY, 41: po.KEY_POLY, 63: po.KEY_POLY}


def table_of(case, mode):
    t = po.Table()
    codes, off = case.store()
    t.count_reads(codes, off, case.k, mode)
    return t


def walk(case, direction, mode=None, max_kmers=-1, max_radius=10000):
    mode = MODES[case.k] if mode is None else mode
    return po.bfs(table_of(case, mode), case.k, mode, case.seeds_for(direction), direction, case.min_cov, max_kmers, max_radius)


def assert_shape(case, direction, mode=None):
    res = walk(case, direction, mode)
    assert res is not None, case.name
    assert ws.histogram(res) == case.widths(direction), (case.name, direction)
    assert len(res["lo"]) == sum(case.widths(direction)) and res["levels"] == len(case.widths(direction)) - 1
    return res


# ---------------------------------------------------------------------------------------------------- the hash
@pytest.fixture(scope="module")
def hosttest():
    from metacherchant_amd import build
    build.build_host()
    return build.HOSTTEST


def test_fmix64_is_the_headers_and_its_inverse_inverts_it(hosttest):
    rng = np.random.default_rng(1)
    words = [0, 1, ws.M64, ws.GOLDEN] + [int(x) for x in rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * 2 + rng.integers(0, 2, 2000, dtype=np.uint64)]
    out = subprocess.run([hosttest, "placement", "32"], input="".join("%x\n" % w for w in words), check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == 4 * len(words)
    assert [int(x, 16) for x in out[0::4]] == [ws.fmix64(w) for w in words]
    assert all(ws.fmix64_inv(ws.fmix64(w)) == w and ws.fmix64(ws.fmix64_inv(w)) == w for w in words)


@pytest.mark.parametrize("k,mode", [(32, po.KEY_POLY), (32, po.KEY_FNV1A), (40, po.KEY_POLY), (63, po.KEY_POLY)])
def test_collisions_share_fingerprint_and_bucket_and_the_oracle_reaches_v2(k, mode):
    for case in ws.collisions(k):
        f = case.facts
        h2 = ws.vis_hash(f["v2"])
        assert len(f["us"]) in (1, 2, 3) and len(set(f["us"] + [f["v1"], f["v2"]])) == len(f["us"]) + 2   # different k-mers
        for u in f["us"]:
            h = ws.vis_hash(u)
            assert h >> 32 == h2 >> 32 and h & 0xFFFFFF == h2 & 0xFFFFFF and u >> 64 == f["v2"] >> 64
        res = assert_shape(case, 1, mode)
        v = ws.kmers_of(res)
        assert v[:len(f["us"])] == f["us"] and v[len(f["us"])] == f["v1"]
        assert v[-1] == f["v2"] and res["dist"][-1] == 1 and (res["dist"][:-1] == 0).all()
        assert (len(case.seeds) > ws.flim_of(1)) == case.name.endswith("-wide")


# ---------------------------------------------------------------------------------------------------- the fans
def test_fans_have_the_widths_of_the_table():
    for case, (d, m, dirs, first) in zip(ws.fans(21), ws.FAN_TABLE):
        for direction in dirs + (-1,):
            res = assert_shape(case, direction)
            assert ws.histogram(res)[:d + 1] == first and case.facts["m"] == m == first[-1]
        w = case.widths(1)
        assert w[d:21 + 1] == [m] * (21 - d + 1) and w[21 + d] == 1 and w[-1] == 1 and len(w) == d + ws.TAIL + 1


def test_the_named_widths_lie_on_either_side_of_each_threshold():
    """flim and flim + 1 for 4 and for 8 neighbours, the scouts' 8 and 9, a level of exactly 512 candidates and one of 516 / 520"""
    by_m = {c.facts["m"]: c for c in ws.fans(21)}
    assert ws.flim_of(1) == 16 and ws.flim_of(0) == 8 and ws.SCOUT_MAX_F == 8
    for narrow, wide, direction in ((16, 17, 1), (8, 9, 0)):
        assert max(by_m[narrow].widths(direction)) == ws.flim_of(direction) and max(by_m[wide].widths(direction)) == ws.flim_of(direction) + 1
        assert direction in ws.fan_directions(narrow) and direction in ws.fan_directions(wide)
    assert max(by_m[8].widths(1)) == ws.SCOUT_MAX_F and max(by_m[9].widths(1)) == ws.SCOUT_MAX_F + 1 <= ws.flim_of(1)
    for m, direction, cands in ((128, 1, 512), (129, 1, 516), (64, 0, 512), (65, 0, 520)):
        assert max(by_m[m].widths(direction)) * ws.nb_of(direction) == cands and direction in ws.fan_directions(m)
    # what the table's widths mean for the chunks: 128 parents one chunk, 129 two
    assert ws.chunks_expected(1, [128], 1) == 2 and ws.chunks_expected(1, [129], 1) == 3 and ws.chunks_expected(1, [16, 17], 1) == 2


@pytest.mark.parametrize("k", [21, 31, 32, 63])
def test_full_fan_profile_and_the_chunks_of_its_merging_parents(k):
    case = ws.fans(k)[0]
    w = case.widths(1)
    assert w[:5] == [1, 4, 16, 64, 256] and w[4:k + 1] == [256] * (k - 3) and w[k + 1:k + 5] == [64, 16, 4, 1]
    for direction in (1, 0, -1):
        res = assert_shape(case, direction)
        # level k + 1: every vertex has four parents, 64 places apart.  4 neighbours: two in the first chunk of 128 parents (lds_set_min),
        # two in the second (vis_find of what the first chunk inserted).  8 neighbours: 64 parents a chunk, one in each of four chunks
        per = ws.CHUNK // ws.nb_of(direction)
        parents = ws.parents_of(res, k, direction, k + 1)
        assert len(parents) == 64
        for p in parents:
            assert len(p) == 4 and [x - p[0] for x in p] == [0, 64, 128, 192]
            assert [x // per for x in p] == ([0, 0, 1, 1] if direction else [0, 1, 2, 3])
        assert ws.first_chunk_accepts(res, k, direction, k) == 64
        assert ws.first_chunk_accepts(res, k, direction, 5) == per   # on the plateau every parent has one child


# ---------------------------------------------------------------------------------------------------- the other shapes
@pytest.mark.parametrize("k", [31, 41])
def test_other_shapes(k):
    cases = {c.name: c for c in ws.others(k)}
    assert len(cases) == 2 + len(ws.BRANCH_P) + 2 + len(ws.SEED_KINDS)
    for case in cases.values():
        for direction in (1, -1, 0):
            assert_shape(case, direction)
    # coverage: the weak words are one copy under the threshold and the fan is that much narrower
    weak = cases["fan-256-weak"]
    assert weak.min_cov == 3 and weak.widths(1)[4] == 256 - len(ws.WEAK) and len(weak.reads) == 3 * 256 - len(ws.WEAK)
    # walkers that end one at a time: inside the first stretch of 64 levels, 64 levels behind the fan-out, and a level later
    ragged = cases["ragged"]
    w, d = ragged.widths(1), ragged.facts["d"]
    assert w[d] == 6 <= ws.SCOUT_MAX_F and ragged.facts["dies"] == [d + n for n in ws.RAGGED_LENGTHS]
    for i, level in enumerate(ragged.facts["dies"]):
        assert w[level] == 6 - i and (w + [0])[level + 1] == 5 - i
    assert ragged.facts["dies"][0] < d + 64 == ragged.facts["dies"][1] == ragged.facts["dies"][2] - 1
    # the branch: one walker up to level p, two behind it
    for p in ws.BRANCH_P:
        w = cases["branch-%d" % p].widths(1)
        assert w[:p + 1] == [1] * (p + 1) and w[p + 1:p + 1 + 40] == [2] * 40 and w[p + 41] == 1
    assert {20, 64, 65, 128, 129} == set(ws.BRANCH_P)
    # the cycles
    assert cases["cycle-150"].widths(1) == [1] * 150 and cases["cycle-%d" % (k + 9)].facts["period"] < 64


@pytest.mark.parametrize("k", [31, 41])
def test_seeds_cases(k):
    cases = {c.name[6:]: c for c in ws.others(k) if c.name.startswith("seeds-")}
    assert tuple(cases) == ws.SEED_KINDS
    for kind, case in cases.items():
        f = case.facts
        t = table_of(case, MODES[k])
        seed = case.seeds[0]
        solid = [i for i in range(len(seed) - k + 1) if t.get(po.key(seed[i:i + k], k, MODES[k])) >= case.min_cov]
        seen, dup_places = set(), []
        for place, i in enumerate(solid):
            w = bytes(seed[i:i + k])
            if w in seen:
                dup_places.append(place)
            seen.add(w)
        assert len(seen) == f["distinct"] == case.widths(1)[0] and dup_places == f["dup_queue_positions"], kind
        res = walk(case, 1)
        assert res["queue_len"] == len(res["lo"]) + len(dup_places)   # (the oracle queues a duplicate again)
        assert solid[0] >= (ws.CHUNK if kind == "none_solid_first_chunk" else 0)
        if dup_places:
            assert solid[dup_places[0]] == f["dup_window"]
    n_windows = {kind: c.n_seed_windows for kind, c in cases.items()}
    assert n_windows["exact_chunk"] == ws.CHUNK and n_windows["exact_chunk_plus"] == ws.CHUNK + 1
    assert cases["dup_in_chunk"].facts["dup_window"] + 100 <= ws.CHUNK           # the duplicates lie in the chunk of the first copies
    assert cases["dup_across_chunks"].facts["dup_window"] >= ws.CHUNK + 100       # a chunk later, and 700 windows and more away
    assert cases["dup_narrow"].widths(1)[0] == 3 <= ws.SCOUT_MAX_F and n_windows["dup_narrow"] <= ws.CHUNK
    assert cases["none_solid_first_chunk"].widths(1)[0] == 50  # (and nothing solid among the first 512 windows: above)
