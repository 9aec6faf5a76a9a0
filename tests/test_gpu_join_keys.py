"""The join by key (csrc/dup_check.h) on key sets designed for its rare paths (tests/join_keys.py composes k-mers for chosen 64-bit
PolynomialHash keys; tests/test_join_keys_model.py checks the designs without a GPU): keys held by 3 .. 73 slots, 32 / 33 / 42 noted
keys in one sub-bucket of k_dup_find (DUP_MAX_CAND = 32), different keys of one fingerprint on one probe path of its LDS set, more
slots than the fix-up planned for (the table leaves its bins), sums past 32767 and across the coverage hint, f2_lg 0 and 1, level 1
from the merge kernel's streams and from a sweep; and the walk's check by key with 74 queries in one sub-bucket, several of one key,
by the join's streams and by a sweep of the table.  Every expected value is the CPU oracle's or join_keys.join_model's; MC_INGEST_DEBUG's
`[join]` line proves which configuration ran.

Not covered (no size that runs in seconds reaches them): k_dup_find<15, 1024> and its passes (more than 1.2 G keys), more than
65 536 listed keys, more than two slices of level 2.  The key equal to the free-slot mark (-1) is not designed here.

Two statements of the plan this module was written to turned out not to hold, by the code's own arithmetic, and are tested as they are:
one key in 73 regions is noted 72 times, 40 of them beyond the note, so it is listed 41 times, the fix-up plans for 8 * 41 + 64 slots
and the table stays in its bins (`many-slots`); three keys in 33 regions each are listed once each, 99 slots against 88 planned, and
the table leaves its bins (`retreat`) -- with mc_stats.left_bins = 5, the value include/mcgpu.h gives this reason.  Needs a real MI355X."""
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import join_keys as jk
from tests import long_harness as lh
from tests import long_loci as ll

pytestmark = pytest.mark.gpu
JOIN_LINE = re.compile(r"\[join\] (\d+) keys, level 1 by (merge streams|sweep), (\d+) slices, f2_lg (\d+), cap2 (\d+), k_dup_find<(13, 256|15, 1024)>, (\d+) listed")
CASES = [(name,) + p + (src,) for name in jk.FAMILIES for p in jk.PARAMS for src in ("merge streams", "sweep")]
IDS = ["%s-k%d-rule%d-f2lg%d-%s" % (c[:4] + (c[4].split()[0],)) for c in CASES]
WALKS = [(name,) + p for name in ("multi", "phantoms") for p in jk.PARAMS]
_oracles = {}


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


def oracle(F, times):
    key = (F.name, F.k, F.rule, times)
    if key not in _oracles:
        _oracles[key] = lh.oracle_of(F.read_list() * times, F.k)
    return _oracles[key]


def counted(mc, monkeypatch, capfd, F, src):
    """a hinted context with the family counted once and joined; (context, background, the join's debug lines, finalize's answer)"""
    lh.set_switches(monkeypatch, F.rule, **({"MC_DUP_L1_SCALE": "0.05"} if src == "sweep" else {}))
    assert lh.n_leaves(F.k, F.rule) == jk.REGIONS
    B = F.background()
    ctx = mc.Context(F.k, po.KEY_POLY, 0, lh.HINT)
    try:
        ctx.set_coverage_hint(jk.COV_HINT)
        codes, off, _, _ = lh.shuffled(F.read_list(), B.list(), 9700)
        lh.add_reads(ctx, codes, off)
        capfd.readouterr()
        size = ctx.finalize()
        return ctx, B, JOIN_LINE.findall(capfd.readouterr().err), size
    except Exception:
        ctx.close()
        raise


def check_table(ctx, F, B, times, name, extra=None):
    """exports at three thresholds, their counts, and look-ups by key of the designed keys, absent keys and the whole table"""
    t, dk, dc = oracle(F, times)
    if extra is not None:
        dc = np.minimum(dc + np.isin(dk, extra), 32767)
    keys, counts = lh.expected((dk, dc), B, times)
    assert ctx.finalize() == len(keys), name
    got = lh.export(ctx)
    lh.assert_table(got[0], got[1], keys, counts, name)
    for cov in (3, jk.COV_HINT):
        sel = counts >= cov
        gk, gc = ctx.export(cov)
        o = np.argsort(gk, kind="stable")
        lh.assert_table(gk[o], gc[o].astype(np.int64), keys[sel], counts[sel], "%s/cov%d" % (name, cov))
        assert ctx.export_count(cov) == int(sel.sum()), (name, cov)
    assert ctx.export_count(0) == len(keys)
    designed = np.array(sorted(F.designed) + sorted(F.single), dtype=np.int64)
    absent = np.setdiff1d(np.random.default_rng(5).integers(-(1 << 63), 1 << 63, 1000), keys)
    ask = np.concatenate([designed, absent, keys])
    want = lh.answers(keys, counts, ask)
    assert (want[:len(designed)] > 0).all() and (want[len(designed):len(designed) + len(absent)] == -1).all()
    got_counts = ctx.get(ask).astype(np.int64)
    bad = np.nonzero(got_counts != want)[0]
    assert len(bad) == 0, (name, len(bad), ask[bad[:5]], got_counts[bad[:5]], want[bad[:5]])
    return keys, counts


@pytest.mark.parametrize("name,k,rule,f2_lg,src", CASES, ids=IDS)
def test_family_through_the_join(mc, monkeypatch, capfd, name, k, rule, f2_lg, src):
    F = jk.family(name, k, rule, f2_lg)
    m = F.model()
    ctx, B, lines, size = counted(mc, monkeypatch, capfd, F, src)
    try:
        st = ctx.stats()
        with capfd.disabled():
            print("join keys: %s k%d rule %d: %s, dup_keys %d (model %d), left_bins %d" % (name, k, rule, lines, int(st.dup_keys), m["dup_keys"], int(st.left_bins)))
        assert st.long_runs == 1 and st.dup_checks == 1, (st.long_runs, st.dup_checks)
        assert len(lines) == 1, lines
        n_used, level1, slices, f2, _, find, listed = lines[0]
        assert (int(n_used), level1, int(slices), int(f2), find) == (m["slots"], src, 2, f2_lg, "13, 256"), (lines, m["slots"])
        listed, want = int(listed), m["dup_keys"]
        # A sub-bucket's note takes the first DUP_MAX_CAND = 32 occurrences noted (every slot of a key beyond its first) and lists each
        # KEY among them once; every later occurrence is listed as it is, whether or not its key is listed already.  So the list holds
        # at least the keys there are and at most the occurrences beyond 32 of every sub-bucket more.  Where the keys of an overfull
        # sub-bucket have two slots each, every occurrence is another key and the list holds each once; where it has one key, that key
        # once from the note and once for every occurrence beyond it.
        lo = hi = 0
        by_sub = {}
        for key, r in F.designed.items():
            by_sub.setdefault(int(jk.dup_sub(np.array([key]), f2_lg)[0]), []).append(len(r))
        for slots in by_sub.values():
            over = max(0, sum(n - 1 for n in slots) - jk.DUP_MAX_CAND)
            lo += len(slots) + (over if len(slots) == 1 else 0)
            hi += len(slots) + (0 if max(slots) == 2 else over)
        assert (lo - want, hi - want) == {"noted-40": (0, 10), "many-slots": (40, 40), "multi": (77, 77)}.get(name, (0, 0))
        assert lo <= listed <= hi, (listed, lo, hi)
        if name == "retreat":
            assert st.left_bins == 5 and st.dup_keys == 0, (st.left_bins, st.dup_keys)
        else:
            assert st.left_bins == 0 and st.dup_keys == want, (st.left_bins, st.dup_keys, want)
        assert size == m["keys"]
        check_table(ctx, F, B, 1, name)
        if name == "retreat":
            return
        # a second identical batch: the slots get their own counts back, take the batch, and are joined again
        codes, off, _, _ = lh.shuffled(F.read_list(), B.list(), 9701)
        lh.add_reads(ctx, codes, off)
        capfd.readouterr()
        ctx.finalize()
        again = JOIN_LINE.findall(capfd.readouterr().err)
        st2 = ctx.stats()
        assert st2.long_runs == 2 and st2.left_bins == 0 and st2.dup_keys == want and st2.dup_checks == 2, (st2.long_runs, st2.left_bins, st2.dup_keys, st2.dup_checks)
        assert len(again) == 1 and int(again[0][0]) == m["slots"] and again[0][1] == src
        check_table(ctx, F, B, 2, name + "/twice")
        # a stream of bare keys: the table leaves its bins, the counters of a key become one
        extra = np.array((sorted(F.designed) + sorted(F.single))[::2], dtype=np.int64)
        ctx.add_keys_dev(lh.dev(extra), len(extra))
        ctx.finalize()
        st3 = ctx.stats()
        assert st3.left_bins == 1 and st3.dup_keys == 0, (st3.left_bins, st3.dup_keys)
        check_table(ctx, F, B, 2, name + "/keys", extra)
    finally:
        ctx.close()


def touched(F, want, seeds):
    """the keys a walk's check by key must give a second slot: every string the walk looked up (its seeds' windows, the eight
    neighbours of what it reached) whose key the table holds, but not in the region of that string's bases"""
    k = F.k
    keys, regions, _ = jk.occurrences(F.reads, F.copies, k, F.rule)
    held = {}
    for key, r in zip(keys.tolist(), regions.tolist()):
        held.setdefault(key, set()).add(r)
    hi, lo = np.asarray(want["hi"], dtype=np.uint64), np.asarray(want["lo"], dtype=np.uint64)
    c = np.zeros((len(lo), k), dtype=np.uint8)
    for i in range(k):
        sh = 2 * (k - 1 - i)
        c[:, i] = ((hi >> np.uint64(sh - 64)) if sh >= 64 else (lo >> np.uint64(sh))) & np.uint64(3)
    nb = np.zeros((len(lo), 8, k), dtype=np.uint8)
    for b in range(4):
        nb[:, b, :k - 1], nb[:, b, k - 1] = c[:, 1:], b
        nb[:, 4 + b, 1:], nb[:, 4 + b, 0] = c[:, :-1], b
    asked = np.concatenate([nb.reshape(-1, k)] + [np.lib.stride_tricks.sliding_window_view(s, k) for s in seeds])
    ak = ll.window_keys(asked, k).reshape(-1)
    ar = ll.region_of(ll.bin_words(asked, k, F.rule), jk.REGIONS).reshape(-1)
    return {key for key, r in zip(ak.tolist(), ar.tolist()) if key in held and r not in held[key]}


@pytest.mark.parametrize("name,k,rule,f2_lg", WALKS, ids=["%s-k%d-rule%d-f2lg%d" % c for c in WALKS])
def test_walks_ask_the_join_by_key(mc, monkeypatch, capfd, name, k, rule, f2_lg):
    F = jk.family(name, k, rule, f2_lg)
    m = F.model()
    t = oracle(F, 1)[0]
    results = []
    for trimmed in (False, True):  # the check by key from the join's streams, and (mc_trim) from a sweep of the table
        ctx, B, lines, _ = counted(mc, monkeypatch, capfd, F, "merge streams")
        try:
            if trimmed:
                ctx.trim()
            got = []
            if name == "multi":
                # from the key's first k-mer with a threshold only the sum of its counters reaches
                for kmer, key, copies in F.seeds:
                    total = min(sum(copies), 32767)
                    cov = max(max(copies) + 1, total - 1) if total < 32767 else 32767
                    assert max(copies) < cov <= total
                    for d in (0, 1, -1):
                        w = lh.assert_walk(ctx, t, k, [kmer], B, d, cov, 2000)
                        assert w is not None and int(w["cov"][0]) == total
                        got.append(w)
                assert ctx.stats().left_bins == 0
            else:
                st0 = ctx.stats()
                assert st0.dup_keys == 0 and st0.dup_checks == 1
                for n, d in enumerate((0, 1, -1)):
                    w = lh.assert_walk(ctx, t, k, F.seeds, B, d, 4, 20000)
                    got.append(w)
                    reached = set(ll.window_keys(np.stack([np.array([(int(h) << 64 | int(l)) >> 2 * (k - 1 - i) & 3 for i in range(k)], dtype=np.uint8)
                                                           for h, l in zip(w["hi"], w["lo"])]), k).reshape(-1).tolist())
                    st = ctx.stats()
                    if d == 0:
                        # every w is reached, nothing else asks for a key held elsewhere, and one repetition of the walk finds that out
                        assert set(F.extra["w_keys"]) <= reached
                        assert touched(F, w, F.seeds) == set(F.extra["w_keys"])
                    elif d == 1:
                        assert set(F.extra["w_keys"]) <= reached
                    # the first walk gives 70 keys their second slots and joins once more; the later ones find them there
                    assert st.dup_keys == 70 and st.dup_checks == 2 and st.left_bins == 0, (d, st.dup_keys, st.dup_checks, st.left_bins)
            results.append(got)
        finally:
            ctx.close()
    for a, b in zip(*results):
        assert all(np.array_equal(a[f], b[f]) for f in ("hi", "lo", "dist", "cov", "last"))
