"""GPU: the kernels that cut their work by base positions -- k_seq_cov, k_cc_first (with k_cc_number's bisect) and k_rs_count --
through the C ABI on the designed layouts of tests/scan_layouts.py, whole and sliced (seq_offsets[0] != 0), against
tests/seq_cov_model.py, tests/components_model.py and the vectorised reads-in-set model (held to tests/reads_filter_model.py by
tests/test_scan_layouts_model.py); and k_classify's correction path on one designed family of reads against
tests/classifier_model.py."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from oracle.host_oracle import normalize_dna
from tests import classifier_model as clm
from tests import components_model as cm
from tests import scan_layouts as sl
from tests import seq_cov_model as sm

pytestmark = pytest.mark.gpu

SEQ_COV_CASES = [(21, 0), (41, 1), (63, 2)]      # (k, key mode): packed, polynomial, FNV-1a
COMPONENTS_CASES = [(31, 0), (5, 0), (41, 1)]
READS_IN_SET_KS = (31, 32, 33, 63)
CLASSIFY_CASES = [(31, 0), (63, 1)]


@pytest.fixture(scope="module")
def tables(oracle):
    """(k, mode, t) -> (context, oracle table with its dump) of the background's table t, counted once"""
    import metacherchant_amd as m
    cache = {}

    def get(k, mode, t):
        if (k, mode, t) not in cache:
            codes, off = sl.table_reads(t, k)
            tab = oracle.Table()
            tab.count_reads(codes, off, k, mode)
            ctx = m.Context(k, mode, 0, 0)
            ctx.add_reads_packed(oracle.pack(codes), off)
            ctx.finalize()
            cache[(k, mode, t)] = (ctx, sl.DumpedTable(tab))
        return cache[(k, mode, t)]
    yield get
    for ctx, _ in cache.values():
        ctx.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


# ---------------------------------------------------------------------------------------------------------------------- seq-cov

@pytest.mark.parametrize("name", sl.SEQ_COV_LAYOUTS)
@pytest.mark.parametrize("k,mode", SEQ_COV_CASES)
def test_seq_cov_on_a_layout(k, mode, name, tables):
    import torch

    import metacherchant_amd as m
    tabs = [tables(k, mode, t) for t in range(sl.N_TABLES)]
    picks = [[0], [0, 1, 2, 3]] + ([[2, 1], [3, 0, 2]] if name.startswith("lds_entries") else [])
    covered = 0
    for L in sl.forms(name, sl.SEQ_COV, k):
        wk = sm.window_keys(L.codes, k, mode)
        want = np.stack([sm.store_coverage(L.codes, L.offsets, k, mode, t, wk) for _, t in tabs], axis=1)  # [n_seqs, 4, 2]
        covered += int((want[:, 0, 0] > 0).sum())
        d_words, d_off = _dev(m.Context._words(L.codes, L.all_offsets, None)), _dev(L.offsets)
        for pick in picks:
            ctxs = [tabs[t][0] for t in pick]
            got = m.seq_coverage(ctxs, L.codes, L.offsets)
            bad = np.argwhere(got != want[:, pick, :])
            assert len(bad) == 0, ("host", L.first, pick, bad[:5].tolist(), got[bad[0][0]].tolist(), want[bad[0][0], pick].tolist())
            d_out = torch.ones((L.n_seqs, len(pick), 2), dtype=torch.int64, device="cuda")  # (the call zeroes it)
            m.seq_coverage_dev(ctxs, d_words, d_off, L.n_seqs, d_out)
            got = d_out.cpu().numpy().view(np.uint64)
            bad = np.argwhere(got != want[:, pick, :])
            assert len(bad) == 0, ("device", L.first, pick, bad[:5].tolist(), got[bad[0][0]].tolist(), want[bad[0][0], pick].tolist())
    assert covered > 0 or name in ("tails_few", "tails_lt_k")


# ------------------------------------------------------------------------------------------------------------------- components

@pytest.fixture(scope="module")
def cached_keys():
    """the model's kmer_key remembers what it computed: the forms of a layout hold the same sequences"""
    plain = cm.kmer_key
    cm.kmer_key = functools.lru_cache(None)(plain)
    yield
    cm.kmer_key = plain


def _text(codes):
    return po.decode(np.asarray(codes, dtype=np.uint8))


def _components_equal(got, want, scanned, k, tag):
    assert got["n_components"] == len(want), (tag, got["n_components"], len(want))
    assert got["seed_seq"].tolist() == [w[0] for w in want], (tag, "seed_seq")
    assert got["seed_pos"].tolist() == [w[1] for w in want], (tag, "seed_pos")
    co = got["comp_offsets"]
    assert len(co) == len(want) + 1 and int(co[0]) == 0 and int(co[-1]) == got["n_kmers"] == sum(len(w[2]) for w in want), tag
    for ci, (s, p, members) in enumerate(want):
        a, b = int(co[ci]), int(co[ci + 1])
        assert po.kmer_string(int(got["hi"][a]), int(got["lo"][a]), k) == scanned[s][p:p + k], (tag, ci)  # member 0: the seed window
        have = {(normalize_dna(po.kmer_string(int(got["hi"][i]), int(got["lo"][i]), k)), int(got["cov"][i])) for i in range(a, b)}
        assert len(have) == b - a and have == set(members.items()), (tag, ci, sorted(have ^ set(members.items()))[:6])


@pytest.mark.parametrize("name", sl.COMPONENTS_LAYOUTS)
@pytest.mark.parametrize("k,mode", COMPONENTS_CASES)
def test_components_on_a_layout(k, mode, name, cached_keys):
    import metacherchant_amd as m
    most = 0
    for L in sl.forms(name, sl.COMPONENTS, k):
        # the table counts what is scanned (the model walks every key of the table, mc_components the scanned ones): in a slice the
        # remaining sequences, so seed_seq counts from the slice's first sequence and the dropped ones hold no vertex of their own
        scanned = [_text(s) for s in L.sequences()]
        want = cm.phase(k, mode, cm.count_table(scanned, k, mode), None, scanned, pictures=False)[1]
        most = max(most, len(want))
        counted = np.concatenate([s for s in L.sequences()] + [np.zeros(0, dtype=np.uint8)])
        off = np.zeros(L.n_seqs + 1, dtype=np.uint64)
        off[1:] = np.cumsum(L.lens())
        with m.Context(k, mode, 0, 0) as c:
            c.add_reads_packed(po.pack(counted), off)
            c.finalize()
            _components_equal(m.components(c, L.codes, L.offsets), want, scanned, k, ("host", L.first))
            d_words, d_off = _dev(m.Context._words(L.codes, L.all_offsets, None)), _dev(L.offsets)
            _components_equal(m.components_dev(c, d_words, d_off, L.n_seqs), want, scanned, k, ("device", L.first))
    if k >= 23 and not name.startswith("tails_") and name not in ("search_rounds_1", "search_rounds_2"):
        assert most >= 2, most  # several components (4^5 k-mers hang together, and so does a store of one or two sequences)


# ----------------------------------------------------------------------------------------------------------------- reads-in-set

def _rs_context(k):
    import metacherchant_amd as m
    return m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)  # (no reads counted: none is needed)


@pytest.mark.parametrize("name", sl.READS_IN_SET_LAYOUTS)
@pytest.mark.parametrize("k", READS_IN_SET_KS)
def test_reads_in_set_on_a_layout(k, name):
    import metacherchant_amd as m
    hi, lo, _, _ = sl.member_set(k)
    hit = 0
    with _rs_context(k) as ctx:
        for L in sl.forms(name, sl.READS_IN_SET, k):
            want = sl.reads_in_set_hits(L.codes, L.offsets, k)
            hit += int(want.sum())
            for weak, pct in ((False, 50), (True, 1)):
                hits, keep = m.reads_in_set(ctx, L.codes, L.offsets, hi if k > 32 else None, lo, pct=pct, weak=weak)
                bad = np.nonzero(hits != want)[0]
                assert len(bad) == 0, (L.first, weak, len(bad), bad[:8].tolist(), hits[bad[:8]].tolist(), want[bad[:8]].tolist())
                assert np.array_equal(keep, sl.reads_in_set_keep(want, L.offsets, k, pct)), (L.first, weak)
    assert hit > 0 or name in ("tails_few", "tails_lt_k", "tails_k", "tails_k_plus1", "repeats") or k == 63


@pytest.mark.parametrize("k", (31, 33))
def test_reads_in_set_over_more_tiles_than_workgroups(k):
    import torch

    import metacherchant_amd as m
    mt = sl.many_tiles(k)
    hi, lo, _, _ = sl.member_set(k)
    member = sl.window_members(mt.codes, k)
    want = sl.reads_in_set_hits(mt.codes, mt.offsets, k, member)
    for what, (r, p) in mt.planted.items():
        assert int(want[r]) == (0 if what in ("straddling a boundary", "a read's last window") else 1), what
    assert int(want.sum()) == len(mt.planted) - 2
    n = len(mt.offsets) - 1
    d_words, d_off, d_hi, d_lo = _dev(m.Context._words(mt.codes, mt.offsets, None)), _dev(mt.offsets), _dev(hi), _dev(lo)
    with _rs_context(k) as ctx:
        # whole with the filter, whole without it, and without its first read (3 tiles and 17 positions) with the filter
        for weak, drop in ((False, 0), (True, 0), (False, 1)):
            d_hits = torch.full((n - drop,), 0x55555555, dtype=torch.int32, device="cuda")
            d_keep = torch.full((n - drop,), 0x55, dtype=torch.uint8, device="cuda")
            m.reads_in_set_dev(ctx, d_words, d_off[drop:], n - drop, d_hi if k > 32 else None, d_lo, len(lo), d_hits, d_keep, pct=1, weak=weak)
            hits = d_hits.cpu().numpy().view(np.uint32)
            bad = np.nonzero(hits != want[drop:])[0]
            assert len(bad) == 0, (weak, drop, bad[:8].tolist(), hits[bad[:8]].tolist(), want[drop:][bad[:8]].tolist())
            assert np.array_equal(d_keep.cpu().numpy().astype(bool), sl.reads_in_set_keep(want[drop:], mt.offsets[drop:], k, 1))


# --------------------------------------------------------------------------------------------------------------------- classify

def _classify_family(k):
    """[(codes, phred, bad_pos handed to the kernel)]: one wrong base at p under the only low quality, the true base each of
    A, G, C, T (the substitution that passes is step 0 .. 3); per length one read with a second wrong base (no step passes), one whose
    bad_pos is its length and one with several low qualities (-2)"""
    g, reads, n = sl.genome(), [], 0
    for length in (k, k + 1, 2 * k - 1, 2 * k, k + 63, k + 64, k + 65, 150):
        places = sorted({p for p in (0, 1, k - 2, k - 1, k, length - k - 1, length - k, length - k + 1, length - 2, length - 1) if 0 <= p < length})

        def wrong(p, true_base):
            nonlocal n
            start = (n * 2111) % (len(g) - 400)
            n += 1
            while g[start + p] != true_base:
                start += 1
            r = g[start:start + length].copy()
            r[p] = (true_base + 1 + p % 3) & 3
            q = np.full(length, 35, dtype=np.uint8)
            q[p] = 5
            return r, q
        for p in places:
            for true_base in range(4):
                r, q = wrong(p, true_base)
                reads.append((r, q, p))
        p = places[len(places) // 2]
        r, q = wrong(p, 2)
        other = (p + length // 2) % length
        r[other] = (r[other] + 1) & 3
        reads.append((r, q, p))                      # a second wrong base that no quality names
        r, q = wrong(p, 1)
        reads.append((r, np.full(length, 35, dtype=np.uint8), length))  # bad_pos = len: read as none
        r, q = wrong(p, 3)
        q[(p + 1) % length] = 3
        reads.append((r, q, -2))                     # several low qualities
    return reads


@pytest.mark.parametrize("k,mode", CLASSIFY_CASES)
def test_classify_corrects_at_every_place_of_a_read(k, mode, tables):
    ctx, tab = tables(k, mode, 0)
    get = clm.table_getter(tab.table, k, mode)
    reads = _classify_family(k)
    codes = np.concatenate([r for r, _, _ in reads])
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r, _, _ in reads])
    bad = np.array([b for _, _, b in reads], dtype=np.int32)
    assert all(b == clm.bad_pos(q) or b == len(r) for r, q, b in reads)
    want = [clm.numbers(r, k, get) for r, _, _ in reads]
    plain = [clm.find_read(r, k, get, 0.9, 1.0) for r, _, _ in reads]
    fixed = [clm.classify((r, q), k, get, 90, 1.0, True) for r, q, _ in reads]
    for length in sorted({len(r) for r, _, _ in reads}):  # the correction decides at least one read of every length
        assert any(a != b for (r, _, _), a, b in zip(reads, plain, fixed) if len(r) == length), length
    assert not all(fixed) and any(fixed)
    for corr, exp in ((True, fixed), (False, plain)):
        s, c, last, f = ctx.classify_reads(codes, off, bad, found=90, z=1.0, correction=corr)
        got = list(zip(s.tolist(), c.tolist(), last.tolist()))
        assert got == want, [i for i in range(len(want)) if got[i] != want[i]][:5]
        wrong = [(i, len(reads[i][0]), int(bad[i])) for i in range(len(exp)) if bool(f[i]) != exp[i]]
        assert not wrong, (corr, wrong[:8])
