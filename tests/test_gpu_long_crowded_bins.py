"""A table of polynomial keys in minimizer bins (csrc/count_long.h) of which one bin is the home of more keys than a region has slots
(tests/long_loci.py Crowded designs the reads; tests/test_long_loci_model.py checks its counts without a GPU).  Such a table is the one
where a bare key does not say where it lives: a key the merge kernel hands on is placed by its leaf (k_add_parked), the walk finds it by
its bases (solid_locate_kmer, sk_hmin_of_kmer2), a look-up by key sweeps the table; and when even the chain of regions is full the table
must leave its bins under the run (pipe_drain_handed_on, table_grow, to_hash_regions).

  full     5 600 keys homed in one interior region R: 1 504 at least live in R + 1 .. R + 4, whatever the order
  last     the same around M_LAST (rule 1, k = 41): R is the last region and the chain wraps to region 0
  nearly   3 900 keys, fewer than R has slots: a few tens of keys still find the 128 slots of their stretch taken and are handed on
           (18 .. 84 seen), the table stays as it is
  beyond   22 000 keys in R (rule 1, k = 41), more than the five regions of the chain have slots: the table leaves its bins

The reads are whole loci, 1 .. 5 times each, shuffled among a background that stays out of R and is large enough for the leaf capacity
the host plans to pass R's records (asserted from MC_INGEST_DEBUG's merge line).  Every expected value is the CPU oracle's."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import crowded_tables as ct
from tests import long_harness as lh
from tests import long_loci as ll

gpu = pytest.mark.gpu

CASES = [(k, rule, name) for k in (41, 46, 63) for rule in (1, 2) for name in ("full", "nearly")] + [(41, 1, "last")]
CHAIN_SLOTS = (ct.TABLE_CHAIN + 1) * ct.REGION_SLOTS
_designs = {}


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


def design(k, rule, name):
    """the case's loci, their reads (every locus 1 .. 5 times), the oracle's table of them once and twice, the records R's leaf gets"""
    key = (k, rule, name)
    if key not in _designs:
        C = ll.Crowded(k, rule, (name,))
        D = {"C": C, "units": C.units[name], "absent": C.absent[name], "word": C.word[name], "in_home": C.keys_in_home(name)}
        D["reads"] = [u for i, u in enumerate(D["units"]) for _ in range(1 + i % 5)]
        D["records"] = sum(len(ll.cuts(len(r) - k + 1)) for r in D["reads"])
        D["once"] = lh.oracle_of(D["reads"], k)
        D["twice"] = lh.oracle_of(D["reads"] + D["reads"], k)
        rng = np.random.default_rng(k + rule)
        D["seeds"] = [D["units"][i] for i in rng.choice(len(D["units"]), 40, replace=False)] + D["absent"][:10]
        D["absent_keys"] = np.unique(ll.window_keys(np.stack(D["absent"]), k))
        D["windows"] = lh.seeds_windows(D["seeds"], k)
        _designs[key] = D
    return _designs[key]


def count(mc, capfd, monkeypatch, D, k, rule, times=1, **env):
    """a hinted context with the case's reads counted `times` times; (context, background, merge lines)"""
    lh.set_switches(monkeypatch, rule, **env)
    B = lh.background(k, rule, (D["word"],), D["records"] + 100)
    capfd.readouterr()
    ctx = mc.Context(k, po.KEY_POLY, 0, lh.HINT)
    lines = []
    try:
        for n in range(times):
            codes, off, _, _ = lh.shuffled(D["reads"], B.list(), 9500 + n)
            lh.add_reads(ctx, codes, off)
            lines += lh.merge_lines(capfd)
        ctx.finalize()
    except Exception:
        ctx.close()
        raise
    return ctx, B, lines


def check_table(ctx, D, B, oracle, times, name, extra=None):
    """export, the size, and look-ups by key of counted keys, absent keys of R and keys from elsewhere against the oracle"""
    t, dk, dc = oracle
    if extra is not None:
        dc = np.minimum(dc + np.isin(dk, extra), 32767)
    keys, counts = lh.expected((dk, dc), B, times * B.mult)
    got = lh.export(ctx)
    lh.assert_table(got[0], got[1], keys, counts, name)
    elsewhere = np.concatenate([B.keys[::50], np.array([1, (1 << 62) - 1, 0x123456789ABCDEF], dtype=np.int64)])
    ask = np.concatenate([dk, D["absent_keys"], elsewhere])
    want = lh.answers(keys, counts, ask)
    assert (want[:len(dk)] > 0).all() and (want[len(dk):len(dk) + len(D["absent_keys"])] == -1).all() and len(D["absent_keys"]) >= ll.N_ABSENT
    got_counts = ctx.get(ask).astype(np.int64)
    bad = np.nonzero(got_counts != want)[0]
    assert len(bad) == 0, (name, len(bad), ask[bad[:5]], got_counts[bad[:5]], want[bad[:5]])


def check_walks(ctx, t, D, B, k, covs=(1, 2)):
    """walks from 40 counted and 10 uncounted loci in every direction against po.bfs.  While the table is in its bins every look-up of
    a walk that came back absent is asked again by key (mcgpu.hip phantom_verify), and a key that turns up after all is given a slot
    in the bin of the k-mer that asked, which the join by key then reports as a key in several regions: results are right either
    way, so the walk itself cannot show a key that was handed on to the wrong region.  mc_stats does: no k-mer of the design shares its
    key with another (tests/test_long_loci_model.py), so a walk must leave dup_keys at 0 and must not make the join run again."""
    before = ctx.stats()
    assert before.dup_keys == 0, before.dup_keys
    some = 0
    for cov in covs:
        for d in (0, 1, -1):
            w = lh.assert_walk(ctx, t, k, D["seeds"], B, d, cov, 200000, D["windows"])
            some += w is not None and len(w["lo"])
    assert some >= 3 * 40  # (the walks are not empty: every counted seed reaches coverage 1)
    after = ctx.stats()
    assert after.dup_keys == 0 and after.dup_checks == before.dup_checks, (after.dup_keys, before.dup_checks, after.dup_checks)


def premise(D, B, name):
    """the designer's count of keys in R, and where R lies"""
    R = int(ll.region_of(np.array([D["word"]], dtype=np.uint64), B.nl)[0])
    if name == "last":
        assert R == B.nl - 1
    else:
        assert 0 < R < B.nl - ct.TABLE_CHAIN - 1
    if name in ("full", "last"):
        assert D["in_home"] >= ll.N_FULL > ct.REGION_SLOTS
    elif name == "nearly":
        assert ll.N_NEARLY <= D["in_home"] < ct.REGION_SLOTS
    else:
        assert D["in_home"] >= ll.N_BEYOND > CHAIN_SLOTS
    assert len(D["once"][1]) == D["in_home"]
    return R


@gpu
@pytest.mark.parametrize("k,rule,name", CASES, ids=["k%d-rule%d-%s" % c for c in CASES])
def test_crowded_bin(mc, capfd, monkeypatch, k, rule, name):
    D = design(k, rule, name)
    # the reads once, then a second time, then a stream of bare keys
    ctx, B, lines = count(mc, capfd, monkeypatch, D, k, rule)
    try:
        premise(D, B, name)
        st = ctx.stats()
        assert [l[0] for l in lines] == ["k_p3_long"] and int(lines[0][2]) >= D["records"], (lines, D["records"])
        assert st.long_runs == 1 and st.grows == 0 and st.left_bins == 0, (st.long_runs, st.grows, st.left_bins)
        if name != "nearly":
            assert st.spill_keys >= ll.N_FULL - ct.REGION_SLOTS, st.spill_keys
        with capfd.disabled():
            print("long crowded bins: k%d rule %d %s: keys in R %d, records %d, lcap %s, spill_keys %d" % (k, rule, name, D["in_home"], D["records"], lines[0][2], int(st.spill_keys)))
        check_table(ctx, D, B, D["once"], 1, name)
        check_walks(ctx, D["once"][0], D, B, k)
        codes, off, _, _ = lh.shuffled(D["reads"], B.list(), 9501)
        capfd.readouterr()
        lh.add_reads(ctx, codes, off)
        lines = lh.merge_lines(capfd)
        ctx.finalize()
        st = ctx.stats()
        assert [l[0] for l in lines] == ["k_p3_long"] and st.long_runs == 2 and st.grows == 0 and st.left_bins == 0, (lines, st.long_runs, st.grows, st.left_bins)
        check_table(ctx, D, B, D["twice"], 2, name + "/twice")  # (no key twice in the export, every count doubled)
        extra = D["once"][1][::3]
        ctx.add_keys_dev(lh.dev(extra), len(extra))
        ctx.finalize()
        assert ctx.stats().left_bins == 1
        check_table(ctx, D, B, D["twice"], 2, name + "/keys", extra)
        t = D["twice"][0]
        for key in extra.tolist():
            t.add(key, 1)
        try:
            check_walks(ctx, t, D, B, k, (2, 3))
        finally:
            D["twice"] = lh.oracle_of(D["reads"] + D["reads"], k)
    finally:
        ctx.close()
    # The same reads into a context that walks on a copy of the solid k-mers.  The copy is built by key from a sweep of the table, and
    # the set-up (mcgpu.hip ensure_solid) moves the table out of its bins for it only when some key sits in several regions because
    # different k-mers share it (mc_stats.dup_keys): none does here -- the designer's keys are as many as its k-mers -- so the table
    # stays where it is.
    ctx, B, _ = count(mc, capfd, monkeypatch, D, k, rule, MC_BFS_DIRECT="0")
    try:
        st = ctx.stats()
        assert st.left_bins == 0 and st.dup_keys == 0, (st.left_bins, st.dup_keys)
        check_walks(ctx, D["once"][0], D, B, k)
        assert ctx.stats().left_bins == (1 if st.dup_keys else 0)
    finally:
        ctx.close()


@gpu
def test_beyond_the_chain(mc, capfd, monkeypatch):
    """22 000 keys of one bin, more than the five regions of its chain have slots: overflow is certain by counting, and a table of hash
    keys in minimizer bins cannot grow: it leaves its bins under the run (left_bins 4) and nothing is lost or counted twice"""
    k, rule, name = 41, 1, "beyond"
    D = design(k, rule, name)
    ctx, B, lines = count(mc, capfd, monkeypatch, D, k, rule)
    try:
        premise(D, B, name)
        st = ctx.stats()
        assert lines and lines[0][0] == "k_p3_long" and int(lines[0][2]) >= D["records"], (lines, D["records"])
        assert ctx.finalize() == ctx.export_count(0) == D["once"][0].size() + len(B.keys)
        assert st.left_bins == 4 and st.grows >= 1, (st.left_bins, st.grows)
        with capfd.disabled():
            print("long crowded bins: k%d rule %d %s: keys in R %d, records %d, lcap %s, spill_keys %d, grows %d" % (
                k, rule, name, D["in_home"], D["records"], lines[0][2], int(st.spill_keys), int(st.grows)))
        check_table(ctx, D, B, D["once"], 1, name)
        lh.assert_walk(ctx, D["once"][0], k, D["seeds"], B, 0, 1, 200000, D["windows"])
    finally:
        ctx.close()
