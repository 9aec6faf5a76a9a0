"""The merge kernel of the long-record form (csrc/count_long.h k_p3_long) on leaves composed record by record (tests/long_loci.py;
tests/test_long_loci_model.py checks without a GPU that every leaf meets the condition named here), so that the paths the kernel's
comments call rare are entered by design, and the table, its look-ups, its read pointers and a walk are checked behind each:

  leaf                    what the design makes the kernel do
  quiet                   130 distinct records of 20 loci at different home slots, every window count 1 .. min(32, k - 14), both
                          strands, 1 .. 5 copies, 390 records: one round, chunks of 1 .. 8 windows at every j0 (both bin rules)
  rounds-513/rounds-1500  300 distinct records in more than 512: two rounds, the second of one record; and three rounds, where by
                          counting some record has copies in two rounds; the table of equal records is rewritten between rounds
  copies-512/copies-511+1 one record fills a round: 512 (511) copies in a 16-bit counter, two to a word; whether the record that
                          stands for the others sits at an even or at an odd place is the scatter's choice
  twins                   the quiet leaf and two different records of one tag and home slot, 3 and 5 copies: compared word for word
  same-home               six records of one home slot and six tags, 4 copies each: two at least find no slot in four probes
  counter                 poly-A reads of k + 31 bases, 32 windows of one key, 1100 times (35 200: reads 32767), then 1100 more; leaf 0
  crossings               30 records x 40 copies with set_coverage_hint(5): every key crosses the threshold in one addition of 40
  second batch            quiet, rounds-1500 and twins onto a table that holds every other record once (virgin == 0)
  stream-spill            rounds-1500 among so few other reads that the leaf capacity is below its 1500 records: the surplus goes
                          through k_skl_add_records, each record to its bin

k = 41, 47, 55, 63 are the forms built for one k, 33, 40, 46, 62 take the generic one; at k <= 46 a whole locus is one record.  Reads go
in through add_reads_packed_dev under MC_COUNT_PATH=partition with a capacity hint; MC_INGEST_DEBUG's line "[count] merge: k_p3_long
... lcap N" gives the leaf capacity, which passes every designed leaf but stream-spill's."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import long_harness as lh
from tests import long_loci as ll

gpu = pytest.mark.gpu

KS = (41, 47, 55, 63, 33, 40, 46, 62)
LEAVES = ["quiet", "rounds-513", "rounds-1500", "copies-512", "copies-511+1", "twins", "same-home", "crossings"]
SECOND = ["quiet", "rounds-1500", "twins"]
LCAP = 1600  # records: more than the largest designed leaf holds in one run (1500)


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


def _words(k, rule):
    return (ll.core_of(rule)[1],)


def run(mc, capfd, monkeypatch, batches, k, rule, lcap=LCAP, mult=None, cov_hint=0):
    """the leaves of `batches` one after the other into one context, each among the background's reads; everything the checks need"""
    # (with a coverage hint the walk runs on a copy of the solid k-mers, whose set-up reports how many there are)
    lh.set_switches(monkeypatch, rule, **({"MC_BFS_DIRECT": "0"} if cov_hint else {}))
    B = lh.background(k, rule, _words(k, rule), lcap)
    R = {"B": B, "lines": [], "placed": []}
    capfd.readouterr()
    with mc.Context(k, po.KEY_POLY, 0, lh.HINT) as ctx:
        if cov_hint:
            ctx.set_coverage_hint(cov_hint)
        everything = []
        for n, leaf in enumerate(batches):
            designed = [leaf.reads[i] for i in leaf.instances()]
            everything += designed
            codes, off, mine, which = lh.shuffled(designed, B.list(mult), 8500 + n)
            at = ctx.read_store_tell()
            lh.add_reads(ctx, codes, off)
            R["lines"] += lh.merge_lines(capfd)
            R["placed"].append((at, len(codes), mine, [designed[i] for i in which]))
        R["size"] = ctx.finalize()
        R["stats"] = ctx.stats()
        t, dk, dc = lh.oracle_of(everything, k)
        R["keys"], R["counts"] = lh.expected((dk, dc), B, len(batches) * (B.mult if mult is None else mult))
        got = lh.export(ctx)
        assert ctx.export_count(0) == R["size"] == t.size() + len(B.keys)
        lh.assert_table(got[0], got[1], R["keys"], R["counts"], batches[-1].name)
        # look-ups by key (a sweep of the table): every designed key, keys of the same bin that were never counted, a few others
        if batches[-1].word == _words(k, rule)[0]:
            absent = np.setdiff1d(np.unique(ll.window_keys(ll.all_loci(k, rule)[:140], k)), dk)[:2000]
            assert len(absent) >= 30
        else:
            absent = np.zeros(0, dtype=np.int64)
        ask = np.concatenate([dk, absent, B.keys[:500], np.array([1, (1 << 62) - 1, 0x123456789ABCDEF], dtype=np.int64)])
        want = lh.answers(R["keys"], R["counts"], ask)
        assert np.array_equal(ctx.get(ask).astype(np.int64), want) and (want[-3:] == -1).all() and (want[:len(dk)] > 0).all()
        R["hinted"] = lh.assert_pointers(got[0], got[2], dk, R["placed"], k, batches[-1].name)
        # one walk from a read of the leaf (at the hinted coverage first: its set-up takes the number of solid k-mers the merge
        # kernel kept, without a sweep of the table)
        seed = max(batches[-1].reads, key=len)
        if cov_hint:
            ctx.reset_stats()
            lh.assert_walk(ctx, t, k, [seed], B, 1, cov_hint)
            st = ctx.stats()
            R["solid"] = (int(st.solid_kmers), int((R["counts"] >= cov_hint).sum()), int(st.solid_sweeps))
        w = lh.assert_walk(ctx, t, k, [seed], B, 0, 1)
        assert w is not None and len(w["lo"]) >= len(np.unique(ll.window_keys(seed, k)))  # (the read's own k-mers at least)
    return R


def check_run(R, batches, k, rule, name):
    """the debug line of every run: the long merge kernel, a leaf capacity that passes the designed leaf; the table stayed in its bins"""
    assert len(R["lines"]) == len(batches), (name, R["lines"])
    for leaf, (kernel, leaves, lcap, _, _) in zip(batches, R["lines"]):
        assert kernel == "k_p3_long" and int(leaves) == R["B"].nl, (name, kernel, leaves)
        assert int(lcap) >= leaf.records, (name, lcap, leaf.records)
    st = R["stats"]
    assert st.long_runs == len(batches) and st.left_bins == 0 and st.grows == 0 and st.spill_keys == 0, (name, st.long_runs, st.left_bins, st.grows, st.spill_keys)
    print("long leaves: %s k%d rule %d: lcap %s, records %s, keys with a hint %d" % (name, k, rule, [l[2] for l in R["lines"]], [b.records for b in batches], R["hinted"]))


@gpu
@pytest.mark.parametrize("rule", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_quiet(mc, capfd, monkeypatch, k, rule):
    leaf = ll.cases(k, rule)["quiet"]
    check_run(run(mc, capfd, monkeypatch, [leaf], k, rule), [leaf], k, rule, "quiet")


@gpu
@pytest.mark.parametrize("name", LEAVES[1:])
@pytest.mark.parametrize("k", KS)
def test_leaf(mc, capfd, monkeypatch, k, name):
    """a designed leaf into an empty table: export, look-ups, pointers and a walk as the oracle's; for crossings the number of solid
    k-mers the merge kernel tracked (no sweep) against the oracle's"""
    leaf = ll.cases(k)[name]
    R = run(mc, capfd, monkeypatch, [leaf], k, 1, cov_hint=leaf.cov_hint)
    check_run(R, [leaf], k, 1, name)
    if leaf.cov_hint:
        assert R["solid"][0] == R["solid"][1] >= len(leaf.keys) and R["solid"][2] == 0, R["solid"]


@gpu
@pytest.mark.parametrize("name", SECOND)
@pytest.mark.parametrize("k", KS)
def test_second_batch(mc, capfd, monkeypatch, k, name):
    """... onto a table that already holds every other record of the leaf once: the kernel reads the region first (virgin == 0)"""
    leaf = ll.cases(k)[name]
    batches = [leaf.half(), leaf]
    check_run(run(mc, capfd, monkeypatch, batches, k, 1), batches, k, 1, name + "/second")


@gpu
@pytest.mark.parametrize("k", KS)
def test_counter(mc, capfd, monkeypatch, k):
    """poly-A: 1100 reads of 32 windows of one key, 35 200 occurrences: reads 32767; then 1100 more on top of the clamped count"""
    a = ll.Leaf("poly-a", k, 1, [ll.poly_a(k)], [1100], 11, word=0)
    b = ll.Leaf("poly-a-again", k, 1, [ll.poly_a(k)], [1100], 12, word=0)
    assert a.max_count == 35200 and len(a.keys) == 1 and a.window_counts == [32] and a.rounds == 3
    for batches in ([a], [a, b]):
        R = run(mc, capfd, monkeypatch, batches, k, 1)
        check_run(R, batches, k, 1, "counter/%d" % len(batches))
        assert R["counts"][np.searchsorted(R["keys"], a.keys[0])] == 32767
        assert int(ll.region_of(np.array([0], dtype=np.uint64), R["B"].nl)[0]) == 0


@gpu
@pytest.mark.parametrize("k", KS)
def test_stream_spill(mc, capfd, monkeypatch, k):
    """the leaf of 1500 records among the background's reads once: the host plans a leaf capacity below 1500, the surplus leaves the
    second scatter level for the spill list and goes in through k_skl_add_records, each record to its bin: the table stays in its bins"""
    leaf = ll.cases(k)["rounds-1500"]
    R = run(mc, capfd, monkeypatch, [leaf], k, 1, mult=1)
    assert len(R["lines"]) == 1 and R["lines"][0][0] == "k_p3_long"
    lcap, st = int(R["lines"][0][2]), R["stats"]
    assert lcap < leaf.records, (lcap, leaf.records)
    assert st.long_runs == 1 and st.left_bins == 0 and st.grows == 0 and st.spill_keys >= leaf.records - lcap, (st.long_runs, st.left_bins, st.grows, st.spill_keys)
    print("long leaves: stream-spill k%d: lcap %d, records %d, spill_keys %d" % (k, lcap, leaf.records, int(st.spill_keys)))
