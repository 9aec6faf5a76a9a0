"""CPU: the designed layouts of tests/scan_layouts.py hold what their names say, by the restated cut and the offsets alone (whole
and sliced); the designer's constants are the kernels'; neighbouring sequences differ in the models' rows; the vectorised
reads-in-set model is tests/reads_filter_model.py's on every small layout."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from oracle.host_oracle import normalize_dna
from tests import components_model as cm
from tests import reads_filter_model as rf
from tests import scan_layouts as sl
from tests import seq_cov_model as sm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metacherchant_amd", "csrc")
BUILDS = [(sl.SEQ_COV, 21), (sl.SEQ_COV, 63), (sl.COMPONENTS, 5), (sl.COMPONENTS, 31), (sl.READS_IN_SET, 31), (sl.READS_IN_SET, 63)]
BUILD_IDS = ["%s-k%d" % (c.kernel, k) for c, k in BUILDS]


def _const(text, name):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, text)
    assert m, name
    return int(eval(m.group(1), {}))  # (a literal, or a product of literals)


def test_the_designers_constants_are_the_kernels():
    src = {f: open(os.path.join(CSRC, f + ".hip")).read() for f in ("seq_cov", "components", "reads_in_set")}
    sc, cc, rs = src["seq_cov"], src["components"], src["reads_in_set"]
    assert _const(sc, "SC_ITEMS") == sl.SEQ_COV.items and _const(sc, "SC_THREADS") * _const(sc, "SC_ITEMS") == sl.SEQ_COV.tile
    assert _const(sc, "SC_SEGS") == sl.SEQ_COV.segs
    assert re.search(r"constexpr int SC_TILE = SC_THREADS \* SC_ITEMS;", sc)
    assert _const(cc, "CC_ITEMS") == sl.COMPONENTS.items and _const(cc, "CC_THREADS") * _const(cc, "CC_ITEMS") == sl.COMPONENTS.tile
    assert re.search(r"constexpr int CC_TILE = CC_THREADS \* CC_ITEMS;", cc)
    assert _const(rs, "RS_ITEMS") == sl.READS_IN_SET.items and _const(rs, "RS_THREADS") * _const(rs, "RS_ITEMS") == sl.READS_IN_SET.tile
    assert re.search(r"constexpr int RS_TILE = RS_THREADS \* RS_ITEMS;", rs)
    caps = re.findall(r"grid_for\(n_tiles, 1, (\d+)\)", rs)
    assert caps == [str(sl.READS_IN_SET.grid_cap)], caps
    for cut in (sl.SEQ_COV, sl.COMPONENTS, sl.READS_IN_SET):  # a wave is 64 threads of ITEMS positions
        assert cut.tile % (sl.LANES * cut.items) == 0
    for s in sl.SHIFTS[1:]:
        assert (s % sl.READS_IN_SET.tile) % 32 != 0 and (s % sl.SEQ_COV.tile) % 32 != 0


# ---- what a layout is for, from its offsets and the cut

def _inner_bounds(L):
    """the positions, counted from `first`, where one sequence with bases ends and the next begins"""
    st = L.starts()[L.lens() > 0] - L.first
    return st[1:]


def _runs_of_empties(L):
    """[(position, run length, number of the sequence behind the run or None)]"""
    lens, out, i = L.lens(), [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0:
                j += 1
            out.append((int(L.starts()[i]), j - i, j if j < len(lens) else None))
            i = j
        else:
            i += 1
    return out


def _edges_at(L, unit):
    """boundaries on a unit's first position (not a greater unit's), one before and one behind"""
    T, k = L.cut.tile, L.k
    b = _inner_bounds(L)
    outer = T if unit * sl.LANES > T or unit == sl.LANES * L.cut.items else sl.LANES * unit
    long_enough = {int(s) - L.first for s, n in zip(L.starts(), L.lens()) if n >= k}
    for d in (0, -1, 1):
        hit = [int(x) for x in b if (x - d) % unit == 0 and (x - d) % outer != 0 and int(x) in long_enough]
        assert hit, (L.name, unit, d)


def _check_edge_at_tile(L):
    T, k = L.cut.tile, L.k
    b = _inner_bounds(L)
    for r in (0, T - 1, 1):
        assert (b % T == r).any(), r
    for before in (k - 1, k, 1):
        ok = [(s, n) for s, n in zip(L.starts(), L.lens()) if (s - L.first) % T == T - before and n >= 2 * k]
        assert ok, before
        s, n = ok[0]
        assert L.tile_of(int(s)) + 1 == L.tile_of(int(s) + k - 1 if before < k else int(s) + k)  # its windows read the next tile
    assert L.lens()[-1] >= k and L.end == int(L.starts()[-1] + L.lens()[-1])


def _check_edge_unit(L, unit):
    I, k = L.cut.items, L.k
    _edges_at(L, unit)
    one = {int(s) for s, n in zip(L.starts(), L.lens()) if n == 1}
    assert any(all(p + i in one for i in range(I)) for p in one if (p - L.first) % I == 0)
    # a thread whose run touches three sequences, the outer two with windows; where k bases fit a run, the middle one too
    found = False
    for p in L.starts()[L.lens() > 0]:
        pt = int(p) - (int(p) - L.first) % I
        a, c = L.seq_of(pt), L.seq_of(pt + I - 1)
        if pt >= L.first and pt + I <= L.end and c - a >= 2:
            inner = [n for n in L.lens()[a + 1:c] if n > 0]
            if L.lens()[a] >= k and L.lens()[c] >= k and inner and (k > I - 2 or inner[0] >= k):
                found = True
    assert found
    lens = L.lens().tolist()
    assert any(lens[i:i + 3] == [k, k, k] for i in range(len(lens) - 2))


def _check_empties(L, run):
    I, k = L.cut.items, L.k
    runs = _runs_of_empties(L)
    assert all(r[1] == run for r in runs) and len(runs) == 4
    (p0, _, s0), (p1, _, s1), (p2, _, s2), (p3, _, s3) = runs
    assert p0 == L.first and L.s0(0) == s0 == run           # the search lands behind the run
    assert (p1 - L.first) % L.cut.tile == 0 and p1 > L.first and L.s0(L.tile_of(p1)) == s1
    assert int((L.starts() == p1).sum()) == run + 1         # (with the sequence behind them)
    assert (p2 - L.first) % I not in (0, I - 1)
    assert s3 is None and p3 == L.end and L.lens()[-run - 1] >= k
    for s in (s0, s1, s2):
        assert L.lens()[s] >= k


def _check_long_over_tiles(L):
    T = L.cut.tile
    s = int(np.argmax(L.lens()))
    assert L.lens()[s] == 3 * T + T // 2
    t0, t1 = L.tile_of(int(L.starts()[s])), L.tile_of(int(L.starts()[s] + L.lens()[s]) - 1)
    inside = [t for t in range(t0 + 1, t1) if L.s0(t) == s and L.s0(t + 1) == s]
    assert len(inside) >= 2 and t1 - t0 == 4
    assert L.n_seqs - 1 - s >= 5 and L.end - int(L.starts()[s] + L.lens()[s]) >= T // 2 - 8


def _check_lds_entries(L):
    T, I, k, segs = L.cut.tile, L.cut.items, L.k, sl.SEQ_COV.segs
    # a tile whose sequences 255, 256 and 257 hold 100 bases each
    t = 1
    s0 = L.s0(t)
    assert (L.lens()[s0 + segs - 1:s0 + segs + 2] == 100).all() and L.tile_of(int(L.starts()[s0 + segs + 1]) + 99) == t
    if L.name.endswith("_empties"):
        assert L.lens()[s0] == 1 and (L.lens()[s0 + 1:s0 + segs - 1] == 0).all()
    else:
        assert (L.lens()[s0:s0 + segs - 1] == 1).all()
    assert (int(L.starts()[s0 + segs]) - L.first) % I != 0  # one thread's run crosses from the 255th to the 256th
    # a wave that holds last runs on both sides of the 256th
    ok = False
    for t in range(L.n_tiles):
        for w in range(T // (sl.LANES * I)):
            lasts = {L.j_of(L.seq_of(min(L.tile_start(t) + (w * sl.LANES + i) * I + I - 1, L.end - 1)), t) for i in range(sl.LANES)}
            ok |= {segs - 2, segs - 1, segs, segs + 1} <= lasts
    assert ok
    a, e = int(L.starts()[-1]), L.end
    assert L.tile_of(a) + 1 == L.tile_of(e - 1) and L.j_of(L.n_seqs - 1, L.tile_of(e - 1)) == 0 and L.lens()[-1] >= 2 * k


def _check_search_rounds(L, n):
    assert L.n_seqs == n
    if n == 1:
        assert L.n_tiles == 3 and L.s0(2) == 0
    elif n == 2:
        assert [L.s0(t) for t in range(L.n_tiles)] == [0, 0, 1]
    else:
        a, b = sl.search_marks(n)
        assert b % sl.search_step(n) == 0
        assert [L.s0(t) for t in range(L.n_tiles)] == [0, 0, a, b, n - 1]
        assert (L.lens() == 0).any() or n < 100
    rounds, width = 0, n
    while width > 1:
        width, rounds = -(-width // 64), rounds + 1
    assert rounds == {1: 0, 2: 1, 64: 1, 65: 2, 4096: 2, 4097: 3, 64 ** 3 + 1: 4}[n]


def _check_tails(L, kind):
    T, I, k = L.cut.tile, L.cut.items, L.k
    want = {"tiles": 2 * T, "tiles_plus1": 2 * T + 1, "tiles_minus1": 2 * T - 1, "lt_k": k - 1, "k": k, "k_plus1": k + 1}
    if kind == "few":
        assert 0 < L.end - L.first < I and (L.lens() == 0).any()
    else:
        assert L.end - L.first == want[kind]


def _check_repeats(L):
    I, k = L.cut.items, L.k
    c = L.codes
    rep = [int(s) for s, n in zip(L.starts(), L.lens()) if n == k + 14 and np.array_equal(c[s:s + k], c[s + 7:s + 7 + k])]  # (period 7)
    assert len(rep) == 3 and len({L.tile_of(p) for p in rep}) == 3
    for p in rep:
        assert (p - L.first) % I == 0 and L.thread_of(p) == L.thread_of(p + 7)
        assert np.array_equal(c[p:p + k], c[rep[0]:rep[0] + k]) and np.array_equal(c[p:p + k], c[p + 7:p + 7 + k])
    assert any(L.tile_of(int(s)) + 1 == L.tile_of(int(s) + k - 1) and n >= k for s, n in zip(L.starts(), L.lens()))
    runs = _runs_of_empties(L)
    assert len(runs) == 2 and runs[0][2] is not None and L.lens()[runs[0][2]] >= k and runs[1][2] is None


def _check(L):
    name = L.name
    assert L.first % L.cut.tile in [s % L.cut.tile for s in sl.SHIFTS] and len(L.codes) == L.end
    if name == "edge_at_tile":
        _check_edge_at_tile(L)
    elif name == "edge_at_thread":
        _check_edge_unit(L, L.cut.items)
    elif name == "edge_at_wave":
        _check_edge_unit(L, L.cut.items * sl.LANES)
    elif name.startswith("empties_"):
        _check_empties(L, int(name[8:]))
    elif name == "long_over_tiles":
        _check_long_over_tiles(L)
    elif name.startswith("lds_entries"):
        _check_lds_entries(L)
    elif name.startswith("search_rounds_"):
        _check_search_rounds(L, int(name[14:]))
    elif name.startswith("tails_"):
        _check_tails(L, name[6:])
    else:
        assert name == "repeats"
        _check_repeats(L)


@pytest.mark.parametrize("cut,k", BUILDS, ids=BUILD_IDS)
def test_every_layout_holds_what_its_name_says(cut, k):
    assert set(sl.EMPTY_RUNS) == {1, 2, 63, 64, 65, 300} and set(sl.SEARCH_SEQS) == {1, 2, 64, 65, 4096, 4097, 64 ** 3 + 1}
    for name in sl.SMALL:
        forms = sl.forms(name, cut, k)
        assert [L.first % cut.tile for L in forms] == [0, 1, 7, 8, cut.tile - 1] and [L.m > 0 for L in forms] == [False] + [True] * 4
        for L in forms:
            _check(L)
            assert L.end - L.first <= 300000 and L.purpose


# ---- the models on the layouts

@pytest.fixture(scope="module")
def tables(oracle):
    """the four tables at k = 21, packed keys"""
    out = []
    for t in range(sl.N_TABLES):
        tab = oracle.Table()
        tab.count_reads(*sl.table_reads(t, 21), 21, 0)
        out.append(sl.DumpedTable(tab))
    return out


def _cov_rows(L, tables):
    wk = sm.window_keys(L.codes, L.k, 0)
    return np.stack([sm.store_coverage(L.codes, L.offsets, L.k, 0, t, wk) for t in tables], axis=1)


def test_a_windows_count_is_its_regions_multiplicity(tables, oracle):
    g, k = sl.genome(), 21
    for t, tab in enumerate(tables):
        for r in (0, 1, 12, 13, 500, sl.N_REGIONS - 1):
            for p in (r * sl.REGION, r * sl.REGION + sl.REGION - 1):
                if p + k <= len(g):
                    assert max(tab.table.get(oracle.key(g[p:p + k], k, 0)), 0) == sl.mult(t, r), (t, r, p)


def test_neighbouring_sequences_differ_in_the_models_rows(tables):
    for name in sl.SEQ_COV_LAYOUTS:
        for L in sl.forms(name, sl.SEQ_COV, 21):
            rows = _cov_rows(L, tables)
            with_windows = np.nonzero(L.lens() >= L.k)[0]
            for a, b in zip(with_windows, with_windows[1:]):
                assert not np.array_equal(rows[a], rows[b]), (name, L.first, a, b)
                assert rows[a, 0, 0] * (L.lens()[b] - L.k + 1) != rows[b, 0, 0] * (L.lens()[a] - L.k + 1), (name, L.first, a, b)  # table 0, a window
    for name in sl.READS_IN_SET_LAYOUTS:
        if name == "repeats":  # (components' own layout: its designed sequences come from regions of no table and no set)
            continue
        for L in sl.forms(name, sl.READS_IN_SET, 31):
            hits = sl.reads_in_set_hits(L.codes, L.offsets, 31)
            tested = np.nonzero(L.lens() > L.k)[0]
            for a, b in zip(tested, tested[1:]):
                assert hits[a] != hits[b], (name, L.first, a, b)


def test_lds_entries_are_covered_from_their_own_tile(tables):
    for name in ("lds_entries", "lds_entries_empties"):
        for L in sl.forms(name, sl.SEQ_COV, 21):
            rows, s0 = _cov_rows(L, tables), L.s0(1)
            for j in (255, 256, 257):
                assert L.j_of(s0 + j, 1) == j and L.tile_of(int(L.starts()[s0 + j])) == 1, j
                assert (rows[s0 + j][[0, 2], 0] > 0).all(), j  # (tables 1 and 3 count some regions 0 times)
            s0 = L.s0(2)
            for j in range(253, 261):
                assert (rows[s0 + j, 0] > 0).all() and L.lens()[s0 + j] == L.k + 3


def _strings(L):
    return [bytes(np.frombuffer(b"AGCT", dtype=np.uint8)[s]).decode() for s in L.sequences()]


@pytest.mark.parametrize("k", (31, 33))
def test_the_vectorised_reads_in_set_model_is_the_string_models(k):
    g = bytes(np.frombuffer(b"AGCT", dtype=np.uint8)[sl.genome()]).decode()
    members = rf.make_set(g[p:p + k] for r in range(0, sl.N_REGIONS, 2) for p in range(r * sl.REGION, min((r + 1) * sl.REGION, len(g) - k + 1)))
    hi, lo, _, _ = sl.member_set(k)
    assert len(lo) == sum(1 for r in range(0, sl.N_REGIONS, 2) for p in range(r * sl.REGION, min((r + 1) * sl.REGION, len(g) - k + 1)))
    assert (hi != 0).any() == (k > 32)
    some = 0
    for cut in (sl.COMPONENTS, sl.READS_IN_SET):
        for name in sl.SMALL:
            for L in sl.forms(name, cut, k) if cut is sl.COMPONENTS else [sl.layout(name, cut, k, 0), sl.layout(name, cut, k, 7)]:
                if cut is sl.READS_IN_SET and L.end > 70000 and not name.startswith("edge_at_tile"):
                    continue  # (the string model is slow: the large builds of two layouts stand for the rest)
                got = sl.reads_in_set_hits(L.codes, L.offsets, k)
                want = [sum(1 for w in rf.tested_windows(r, k) if w in members) for r in _strings(L)]
                assert got.tolist() == want, (name, L.first)
                for pct in (1, 50):
                    keep = sl.reads_in_set_keep(got, L.offsets, k, pct)
                    assert keep.tolist() == [n > k and h >= rf.threshold(int(n), k, pct) for h, n in zip(want, L.lens())]
                some += sum(want)
    assert some > 10000


def test_many_tiles_holds_its_planted_windows():
    cut = sl.READS_IN_SET
    for k in (31, 33):
        mt = sl.many_tiles(k)
        o = mt.offsets.astype(np.int64)
        n_tiles = -(-int(o[-1]) // cut.tile)
        assert int(o[0]) == 0 and n_tiles > cut.grid_cap + 2 and (np.diff(o) > 5 * cut.tile).sum() >= 2 and (np.diff(o) <= 300).sum() > 50000
        tiles = {w: p // cut.tile for w, (r, p) in mt.planted.items()}
        assert (tiles["tile 0"], tiles["tile 511"], tiles["tile 512"], tiles["last tile"]) == (0, 511, 512, n_tiles - 1)
        assert mt.planted["a thread's last position"][1] % cut.items == cut.items - 1
        for what, (r, p) in mt.planted.items():
            assert o[r] <= p < o[r + 1]
            around = sl.window_members(mt.codes[p - 100:p + k + 100], k)
            assert np.nonzero(around)[0].tolist() == [100], what  # one member, at p
            if what == "straddling a boundary":
                assert p < o[r + 1] < p + k
            elif what == "a read's last window":
                assert p + k == o[r + 1]
            else:
                assert p + k < o[r + 1]  # a window that is tested


def test_repeats_seeds_are_where_the_layout_puts_them():
    """on the model: the repeated k-mer's component is seeded at its first occurrence, a seed's window straddles a tile edge, seeds
    lie behind and before empty sequences"""
    k, mode = 31, 0
    for L in sl.forms("repeats", sl.COMPONENTS, k):
        scanned = [po.decode(s) for s in L.sequences()]
        want = cm.phase(k, mode, cm.count_table(scanned, k, mode), None, scanned, pictures=False)[1]
        seeds = {(s, p) for s, p, _ in want}
        lens = L.lens()
        rep = [i for i in range(L.n_seqs) if lens[i] == k + 14 and scanned[i][:k] == scanned[i][7:7 + k]]
        assert len(rep) == 3 and (rep[0], 0) in seeds and not any((r, p) in seeds for r in rep[1:] for p in range(14))
        first = next(w for w in want if w[:2] == (rep[0], 0))
        assert first[2][normalize_dna(scanned[rep[0]][:k])] == 9  # at 0, 7 and 14 of each of the three: twice in one thread's run
        straddle = [s for s, p in seeds if p == 0 and L.tile_of(int(L.starts()[s])) + 1 == L.tile_of(int(L.starts()[s]) + k - 1)]
        assert straddle
        assert any(p == 0 and s > 0 and lens[s - 1] == 0 for s, p in seeds)
        last = max(i for i in range(L.n_seqs) if lens[i] > 0)
        assert last < L.n_seqs - 1 and any(s == last for s, _ in seeds)
