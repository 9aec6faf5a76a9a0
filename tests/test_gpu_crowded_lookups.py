"""GPU: every table look-up path over regions that hold more keys than they have slots (tests/crowded_tables.py builds the cases).

The probing rule of the counting table (csrc/kmer_device.h TABLE_MAX_PROBES, TABLE_CHAIN) is written out in table_get (mc_get, the
reads-classifier), table_locate (mc_components), multi_table.h probe_behind_home (mc_seq_coverage, mc_kmer_presence), solid_probe_from
(the walk) and the builder of the walk's solid copy (MC_BFS_DIRECT=0); table_add_at and the merge kernel place the keys.  Each is
compared here with its plain reference over tables of which one region is the home of 5600 keys: at least 1504 of them live in a later
region of the chain, whatever the order of insertion, and a look-up of an absent key of that region has to pass a full stretch and hop
before it may say so.  Every test first proves that premise by counting, from mc_get_stats and the restated placement functions."""
import numpy as np
import pytest

from oracle import pyoracle as po
from oracle.host_oracle import normalize_dna
from tests import classifier_model as clm
from tests import components_model as cpm
from tests import crowded_tables as ct
from tests import seq_cov_model as sm
from tests.helpers import assert_bfs_equal

pytestmark = pytest.mark.gpu

CASES = [(31, 0), (21, 0), (41, 1), (41, 2)]  # (k, key mode): packed in minimizer bins; packed, polynomial and FNV-1a in hash-prefix regions
CROWDED = ("full", "nearly", "last")
SOLID = ("full_solid", "nearly_solid", "last_solid")  # the same reads in contexts that walk on a solid copy (MC_BFS_DIRECT=0)
TABLE_LISTS = (["full"], ["full", "roomy"], ["roomy", "last", "full"], ["full", "last", "roomy", "nearly"], ["full"] * 4)
ROOMY_HINT = 10_000_000  # 16 M slots in hash-prefix regions: what is one region of 4 M slots is four of these
MC_EOVERFLOW = -5
SOLID_REFUSAL = "a region of the solid k-mer table filled up (hash skew)"


class _Case(ct.Case):
    """the reads with the oracle's tables and every reference, computed once and shared by both count paths"""

    def __init__(self, k, mode):
        ct.Case.__init__(self, k, mode)
        self.table, self.dump, self.ref = {}, {}, {}
        for name, (codes, off) in self.reads.items():
            self.table[name] = po.Table()
            self.table[name].count_reads(codes, off, k, mode)
            self.dump[name] = self.table[name].dump()
        codes, off = self.queries
        self.q_at, self.q_seq = ct.store_windows(codes, off, k)
        self.q_wk = sm.window_keys(codes, k, mode)      # by start position in the store
        self.q_keys = self.q_wk[self.q_at]              # of the windows that lie inside a sequence
        hi, lo = ct.pack_windows(codes, k)
        self.q_hi, self.q_lo = hi[self.q_at], lo[self.q_at]

    def get(self, name, keys):
        """the oracle table's answer for every key: the count, or -1"""
        tk, tc = self.dump[name]
        at = np.minimum(np.searchsorted(tk, keys), len(tk) - 1)
        return np.where(tk[at] == keys, tc[at], -1).astype(np.int16)

    def cached(self, what, f):
        if what not in self.ref:
            self.ref[what] = f()
        return self.ref[what]


class _Tables:
    pass


def _context(m, env, k, mode, reads, hint=0):
    with pytest.MonkeyPatch.context() as mp:  # (the switches are read once per context, by mc_create)
        for name in ("MC_COUNT_PATH", "MC_BFS_DIRECT", "MC_SUPERKMERS", "MC_LONG_RECORDS"):
            mp.delenv(name, raising=False)
        for name, value in env.items():
            mp.setenv(name, value)
        ctx = m.Context(k, mode, 0, hint)
    try:
        ctx.add_reads_packed(po.pack(reads[0]), reads[1])
        ctx.finalize()
    except m.McError:
        ctx.close()
        raise
    return ctx


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "k%d-mode%d" % c)
def case(request):
    po.lib()
    return _Case(*request.param)


@pytest.fixture(scope="module", params=["direct", "partition"])
def tabs(request, case):
    """The case's tables counted on one path: full, nearly and last, the three again for a walk on the solid copy, and roomy (the
    same keys homed normally: hash-prefix regions of a table four times the size, on the default path)."""
    import metacherchant_amd as m
    m.native.load()
    t = _Tables()
    t.path, t.ctx = request.param, {}
    # A polynomial table of 33 .. 63 bases is created in minimizer bins and moves to hash-prefix regions of the same size when the first
    # batch comes without a capacity hint, which mc_stats.grows counts as a rebuild: these start in hash-prefix regions, as they end.
    base_env = {"MC_LONG_RECORDS": "0"} if case.mode == po.KEY_POLY else {}
    try:
        for name in CROWDED + SOLID:
            env = dict(base_env, MC_COUNT_PATH=t.path, **({"MC_BFS_DIRECT": "0"} if name.endswith("_solid") else {}))
            t.ctx[name] = _context(m, env, case.k, case.mode, case.reads[name.split("_")[0]])
        t.ctx["roomy"] = _context(m, {"MC_SUPERKMERS": "0", "MC_LONG_RECORDS": "0"}, case.k, case.mode, case.reads["roomy"], ROOMY_HINT)
        t.stats = {name: c.stats() for name, c in t.ctx.items()}
        yield t
    finally:
        for c in t.ctx.values():
            c.close()


def _premise(case, t):
    """More than 4096 of the table's keys have one home region (the last one in `last`), so at least that many less 4096 live in a later
    region of the chain; the queries hold present and absent k-mers of that region; roomy homes the same keys normally."""
    for name in ("full", "last", "full_solid", "last_solid"):  # (no premise is claimed for nearly)
        st, base = t.stats[name], name.split("_")[0]
        n_regions = int(st.table_slots) >> ct.REGION_LG
        if case.bins:
            assert t.ctx[name].superkmer_capacity(100000, 700) > 0  # (super-k-mer records: the table's regions are minimizer bins)
        else:
            assert st.table_slots == 1 << 22 and st.grows == 0, (name, st.table_slots, st.grows)

        def count():
            tk = case.dump[base][0]
            reg = case.regions(tk, n_regions)
            home = int(case.regions(case.keys_of(case.units[base][:1]), n_regions)[0])
            q_in = case.regions(case.q_keys, n_regions) == home
            return home, int((reg == home).sum()), case.get(base, case.q_keys[q_in])
        home, n_home, answers = case.cached(("premise", base, n_regions), count)
        assert n_home > ct.REGION_SLOTS, (name, n_home)
        assert base != "last" or home == n_regions - 1, (home, n_regions)
        assert base != "full" or 0 < home < n_regions - 1, (home, n_regions)
        assert (answers > 0).sum() >= ct.N_FULL and (answers == -1).sum() >= ct.N_ABSENT, (name, (answers > 0).sum(), (answers == -1).sum())
    st = t.stats["roomy"]
    assert t.ctx["roomy"].superkmer_capacity(100000, 700) == 0  # (counted window by window: its regions are hash prefixes, at k = 31 too)
    n_regions = int(st.table_slots) >> ct.REGION_LG
    assert st.table_slots >= 1 << 24 and n_regions & (n_regions - 1) == 0, st.table_slots
    most = case.cached(("roomy", n_regions), lambda: int(np.bincount(case.regions(case.dump["roomy"][0], n_regions, bins=False).astype(np.int64)).max()))
    assert most < ct.REGION_SLOTS // 2, most


def test_tables_are_the_oracles(case, tabs):
    """first of all the tables must be the oracle's, key for key and count for count, on either path: the merge kernel places keys by
    a loop of its own.  (Neither path refuses the overfull region, a single minimizer bin included: both fill the chain.)"""
    _premise(case, tabs)
    for name, ctx in tabs.ctx.items():
        base = name.split("_")[0]
        gk, gc = ctx.export(0)
        ok, oc = case.dump[base]
        assert len(gk) == len(ok) == case.table[base].size(), name
        assert np.array_equal(gk, ok) and np.array_equal(gc, oc), name


def test_get(case, tabs):
    """mc_get (table_get): the count or -1 for every query window's key -- counted, absent from the crowded region, from elsewhere"""
    _premise(case, tabs)
    for name in CROWDED + ("roomy",):
        got, want = tabs.ctx[name].get(case.q_keys), case.get(name, case.q_keys)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (name, len(bad), case.q_keys[bad[:5]], got[bad[:5]], want[bad[:5]])
        tk, tc = case.dump[name]
        assert np.array_equal(tabs.ctx[name].get(tk), tc), name  # ... and every key of the table, the background among them


def _classify_reference(case, name):
    get = clm.table_getter(case.table[name], case.k, case.mode)
    reads = []
    for i, r in enumerate(case.query_reads):
        q = np.full(len(r), 35, dtype=np.uint8)
        if len(r) and i % 3 == 0:
            q[(7 * i) % len(r)] = 5          # one low-quality position: the correction tries four bases there
        if len(r) > 1 and i % 11 == 0:
            q[[0, len(r) - 1]] = 2           # several: no correction
        reads.append((r, q))
    numbers = [clm.numbers(r, case.k, get) for r, _ in reads]
    verdicts = {(found, z, corr): [clm.classify(rd, case.k, get, found, z, corr) for rd in reads]
                for found, z, corr in ((90, 1.0, False), (50, 1.96, True))}
    bad = np.array([clm.bad_pos(q) for _, q in reads], dtype=np.int32)
    return numbers, verdicts, bad


def test_classify_reads(case, tabs):
    """mc_classify_reads (k_classify's use of table_get) against tests/classifier_model.py, as tests/test_gpu_classify.py compares"""
    _premise(case, tabs)
    codes, off = case.queries
    for name in CROWDED:
        numbers, verdicts, bad = case.cached(("classify", name), lambda: _classify_reference(case, name))
        assert any(w[1] > 0 for w in numbers) and any(w[1] == 0 for w in numbers) and (bad >= 0).any() and (bad == -2).any()
        for (found, z, corr), want in verdicts.items():
            s, c, last, f = tabs.ctx[name].classify_reads(codes, off, bad if corr else None, found=found, z=z, correction=corr)
            got = list(zip(s.tolist(), c.tolist(), last.tolist()))
            assert got == numbers, (name, [i for i in range(len(got)) if got[i] != numbers[i]][:5])
            wrong = [i for i in range(len(want)) if bool(f[i]) != want[i]]
            assert not wrong, (name, found, z, corr, wrong[:5])
            assert any(want) and not all(want)


def _coverage_reference(case):
    codes, off = case.queries
    return {name: sm.store_coverage(codes, off, case.k, case.mode, case.table[name], case.q_wk) for name in CROWDED + ("roomy",)}


def test_seq_coverage(case, tabs):
    """mc_seq_coverage and its device form (home_slots + get_behind_home<true>), one to four tables a call: lanes that hit at home in
    roomy beside lanes that probe through the chain in full, nearly and last"""
    import torch

    import metacherchant_amd as m
    _premise(case, tabs)
    want = case.cached("coverage", lambda: _coverage_reference(case))
    for name in CROWDED + ("roomy",):
        assert (want[name][:, 1] == 0).any() and (want[name][:, 1] != 0).any(), name
    codes, off = case.queries
    dev = torch.device("cuda", 0)
    d_words = torch.from_numpy(po.pack(codes).view(np.int64)).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    for names in TABLE_LISTS:
        w = np.stack([want[n] for n in names], axis=1)
        ctxs = [tabs.ctx[n] for n in names]
        got = m.seq_coverage(ctxs, codes, off)
        bad = np.argwhere(got != w)
        assert len(bad) == 0, (names, len(bad), bad[:5], got[bad[0][0]], w[bad[0][0]])
        d_out = torch.full((len(off) - 1, len(names), 2), -1, dtype=torch.int64, device=dev)
        m.seq_coverage_dev(ctxs, d_words, d_off, len(off) - 1, d_out)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), w), names


def test_kmer_presence(case, tabs):
    """mc_kmer_presence and its device form (home_slots + get_behind_home<false>) over every query window, the same lists of tables"""
    import torch

    import metacherchant_amd as m
    _premise(case, tabs)
    there = case.cached("presence", lambda: {name: (case.get(name, case.q_keys) != -1).astype(np.uint8) for name in CROWDED + ("roomy",)})
    hi, lo = case.q_hi, case.q_lo
    dev = torch.device("cuda", 0)
    d_hi = torch.from_numpy(hi.view(np.int64)).to(dev)
    d_lo = torch.from_numpy(lo.view(np.int64)).to(dev)
    for names in TABLE_LISTS:
        want = np.zeros(len(lo), dtype=np.uint8)
        for j, n in enumerate(names):
            want |= there[n] << j
        # the masks are mixed: roomy holds what full holds, last shares no key with it, nearly has some of full's and some of its own
        assert len(set(want.tolist())) >= (5 if len(set(names)) == 4 else max(len(set(names)), 2)), names
        ctxs = [tabs.ctx[n] for n in names]
        got = m.kmer_presence(ctxs, hi, lo)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (names, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
        if case.k <= 32:
            assert not hi.any() and np.array_equal(m.kmer_presence(ctxs, None, lo), want)
        d_mask = torch.full((len(lo),), 0xEE, dtype=torch.uint8, device=dev)
        m.kmer_presence_dev(ctxs, d_hi, d_lo, len(lo), d_mask)
        assert np.array_equal(d_mask.cpu().numpy(), want), names


def _components_reference(case, name):
    tk, tc = case.dump[name]
    scanned = [po.decode(r) for r in case.query_reads]
    return cpm.phase(case.k, case.mode, dict(zip(tk.tolist(), tc.tolist())), None, scanned, pictures=False)[1], scanned


def test_components(case, tabs):
    """mc_components and its device form (table_locate in k_cc_first, k_cc_union and k_cc_scatter) against tests/components_model.py,
    as tests/test_gpu_components.py compares; the scan is the whole query set"""
    import torch

    import metacherchant_amd as m
    _premise(case, tabs)
    k = case.k
    codes, off = case.queries
    dev = torch.device("cuda", 0)
    d_words = torch.from_numpy(m.Context._words(codes, off, None).view(np.int64)).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    for name in CROWDED:
        want, scanned = case.cached(("components", name), lambda: _components_reference(case, name))
        if case.bins:  # every counted locus is one component of its 17 k-mers, numbered in scan order; the uncounted loci are in none
            assert len(want) == len(case.units[name]) and all(len(w[2]) == ct.LOCUS_WINDOWS for w in want)
            assert [w[:2] for w in want] == sorted(w[:2] for w in want) and all(w[1] == 0 for w in want)
            inside = set().union(*[set(w[2]) for w in want])
            for u in case.absent["full"] + case.absent["last"] + case.units["full" if name == "last" else "last"]:
                s = po.decode(u)
                assert not any(normalize_dna(s[i:i + k]) in inside for i in range(len(s) - k + 1))
        else:
            assert sum(len(w[2]) for w in want) >= len(case.units[name])  # (every counted k-mer of the region is in a component; pool neighbours share one)
        for got in (m.components(tabs.ctx[name], codes, off), m.components_dev(tabs.ctx[name], d_words, d_off, len(off) - 1)):
            assert got["n_components"] == len(want), (name, got["n_components"], len(want))
            assert got["seed_seq"].tolist() == [w[0] for w in want] and got["seed_pos"].tolist() == [w[1] for w in want], name
            co = got["comp_offsets"]
            assert len(co) == len(want) + 1 and int(co[0]) == 0 and int(co[-1]) == got["n_kmers"] == sum(len(w[2]) for w in want)
            assert k > 32 or not got["hi"].any()
            for ci, (s, p, members) in enumerate(want):
                a, b = int(co[ci]), int(co[ci + 1])
                assert po.kmer_string(int(got["hi"][a]), int(got["lo"][a]), k) == scanned[s][p:p + k], (name, ci)
                have = {(normalize_dna(po.kmer_string(int(got["hi"][i]), int(got["lo"][i]), k)), int(got["cov"][i])) for i in range(a, b)}
                assert len(have) == b - a and have == set(members.items()), (name, ci, sorted(have ^ set(members.items()))[:6])


@pytest.mark.parametrize("solid", [False, True], ids=["counting_table", "solid_copy"])
def test_bfs(case, tabs, solid):
    """mc_bfs (solid_probe_from and its entry points; with MC_BFS_DIRECT=0 the builder of the solid copy and solid_probe_from on it) in
    all directions from 40 counted reads and 10 uncounted ones of the crowded region, at coverage 1 and 3.

    The solid copy has no chain, and its home slots are the next bits of the hash whose top bits are the counting table's region: the keys
    that crowd a hash-prefix region clump into a few slots of one solid region, and the builder must refuse (MC_EOVERFLOW).  Whether it
    must build or must refuse is worked out from the oracle's keys (crowded_tables.solid_layout), never taken from what it does."""
    import metacherchant_amd as m
    _premise(case, tabs)
    for name in CROWDED:
        seeds = case.seeds[name]
        codes, off = ct.store(seeds)
        at, _ = ct.store_windows(codes, off, case.k)
        hi, lo = ct.pack_windows(codes, case.k)
        ctx = tabs.ctx[name + "_solid" if solid else name]
        tk, tc = case.dump[name]
        some = 0
        for cov in (1, 3):
            refuses = False
            if solid:
                longest, displaced = case.cached(("solid", name, cov), lambda: ct.solid_layout(tk[tc >= cov]))
                assert longest < ct.TABLE_MAX_PROBES or displaced >= ct.TABLE_MAX_PROBES, (name, cov, longest, displaced)  # one or the other is certain
                refuses = displaced >= ct.TABLE_MAX_PROBES
                assert refuses == (not case.bins), (name, cov, longest, displaced)
            for d in (-1, 1, 0):
                if refuses:
                    with pytest.raises(m.McError) as e:
                        ctx.bfs(hi[at], lo[at], d, cov, 200000, -1)
                    assert e.value.code == MC_EOVERFLOW and SOLID_REFUSAL in str(e.value), (name, d, cov, str(e.value))
                    continue
                want = case.cached(("bfs", name, d, cov), lambda: po.bfs(case.table[name], case.k, case.mode, seeds, d, cov, 200000, -1))
                assert_bfs_equal(ctx.bfs(hi[at], lo[at], d, cov, 200000, -1), want)
                some += want is not None and len(want["lo"])
        assert solid and not case.bins or some >= 3 * 40  # (the walks are not empty: every counted seed reaches coverage 1)
