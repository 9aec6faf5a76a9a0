"""Read pointers in every granule tier of the read store (csrc/read_ptr.h), on the GPU.  mc_read_store_seek puts one small read set
astride each tier boundary, at the end of the range and inside every granule tier -- the store below is reserved, never touched --
and every way a pointer gets into a slot is a case: the direct kernel, the partitioned pipeline's record forms (super-k-mer
records, one key a window, long records) and the two exchange forms with a sender that keeps no store.  A walk's result never
depends on a pointer, so the pointers themselves are checked, against tests/read_pointers.py (pinned to the header by
tests/test_read_pointers_model.py): (a) every exported hint's range holds a store position whose window has that very key, (b) every
solid key has a hint, none past the end of the range, (c) the walk equals the oracle's and needs fewer rounds than without
pointers, within a measured factor of the rounds at store position 0.

The reads: 4001 of 150 bases over one contig of 16 kb with 0.5 % errors (tests.helpers.synth_case: 37-fold -- at 15-fold one 63-mer
in twenty has fewer than 3 error-free copies and the k = 63 walk ends after 62 levels; here it is one in 60 000), put in the order of
their place in the contig, so that the keys of the contig's left half lie wholly below a boundary the batch straddles and the right half's
wholly above it; 4001 and not 4000 so that the boundaries (multiples of 32) fall inside a read, 96 bases from its start, not
between two reads."""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import read_pointers as rp
from tests import seq_cov_model as sm
from tests.helpers import assert_bfs_equal, oracle_table, seed_windows, synth_case

gpu = pytest.mark.gpu

N_READS, L, COV, CONTIG = 4001, 150, 3, 16000
BASES = N_READS * L
STORE_BASES = (BASES + 31) // 32 * 32  # what a batch takes of the store: whole words
HALF = BASES // 2


def _down32(x):
    return x // 32 * 32


# name -> (store position of the batch, wholly inside the range?, a granule tier it lies wholly inside or None)
POSITIONS = {
    "control": (0, True, None),
    "exact|4": (_down32(rp.EXACT_END - HALF), True, None),
    "4|16": (_down32(rp.T2_POS - HALF), True, None),
    "16|64": (_down32(rp.T3_POS - HALF), True, None),
    "64|end": (_down32(rp.END - HALF), False, None),
    "in4": (rp.T1_POS + (1 << 20), True, 1),
    "in16": (rp.T2_POS + (1 << 20), True, 2),
    "in64": (rp.T3_POS + (1 << 20), True, 3),
}
# rounds(position) / rounds(control) of the two walks, the greatest over the cases and over four runs (0.71 the smallest), measured
# on an MI355X and asserted + 0.25; a reads file's batch in the 16-base tier against the same file at position 0
MEASURED_RATIO = {"in4": 1.45, "in16": 1.49, "in64": 1.42}
MEASURED_FILE_RATIO = 1.81

# name -> (k, key mode, how the pointers get into the slots, environment read at mc_create)
CASES = {
    "direct-k31": (31, po.KEY_PACKED, "count", {"MC_COUNT_PATH": "direct"}),
    "records-k31": (31, po.KEY_PACKED, "count", {"MC_COUNT_PATH": "partition"}),
    "windows-k21": (21, po.KEY_PACKED, "count", {"MC_COUNT_PATH": "partition"}),
    "long-k41": (41, po.KEY_POLY, "long", {"MC_COUNT_PATH": "partition"}),
    "long-k63": (63, po.KEY_POLY, "long", {"MC_COUNT_PATH": "partition"}),
    "windows-k41": (41, po.KEY_POLY, "count", {"MC_COUNT_PATH": "partition", "MC_LONG_RECORDS": "0"}),
    "windows-k32": (32, po.KEY_POLY, "count", {"MC_COUNT_PATH": "partition"}),
    "exchange-records-k31": (31, po.KEY_PACKED, "superkmers", {}),
    "exchange-keys-k41": (41, po.KEY_POLY, "keys", {}),
}
SWITCHES = ("MC_COUNT_PATH", "MC_LONG_RECORDS", "MC_LONG_BINS")


@contextlib.contextmanager
def switches(env):
    """the library's switches as a case wants them while its contexts are created, and back"""
    old = {n: os.environ.get(n) for n in SWITCHES}
    for n in SWITCHES:
        os.environ.pop(n, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


@functools.lru_cache(maxsize=None)
def read_set():
    """(genome, codes, offsets, packed words): the reads in the order of their place in the contig (found by a 21-mer of theirs)"""
    genome, reads, off = synth_case(1, CONTIG, N_READS, L, 50)
    place = {int(key): i for i, key in enumerate(sm.window_keys(genome, 21, po.KEY_PACKED))}
    at = []
    for r in reads.reshape(N_READS, L):
        keys = sm.window_keys(r, 21, po.KEY_PACKED)
        at.append(next((place[int(x)] for x in keys[::16] if int(x) in place), 0))
    codes = np.ascontiguousarray(reads.reshape(N_READS, L)[np.argsort(at, kind="stable")].reshape(-1))
    return genome, codes, off, po.pack(codes)


@functools.lru_cache(maxsize=None)
def host_side(k, mode):
    """what the host knows of the batch at one (k, mode), whatever its store position: the key of the window at every batch
    position (store position = position of the batch + batch position), which positions hold a window of one read, every distinct
    key's first and last such position, the oracle's table and walks"""
    genome, codes, off, _ = read_set()
    wk = sm.window_keys(codes, k, mode)
    valid = (np.arange(len(wk)) % L) <= L - k
    pos = np.nonzero(valid)[0]
    order = np.argsort(wk[pos], kind="stable")
    keys, first, count = np.unique(wk[pos][order], return_index=True, return_counts=True)
    t, n = oracle_table(codes, off, k, mode)
    ok, oc = t.dump()
    assert n == len(pos) and np.array_equal(ok, keys) and np.array_equal(oc, np.minimum(count, 32767))
    seed = genome[CONTIG // 2:CONTIG // 2 + 200]
    want = [po.bfs(t, k, mode, [seed], d, COV, 20000, -1) for d in (-1, 1)]
    assert all(w is not None and w["levels"] >= 7000 for w in want)  # (to the contig's ends: 7800 k-mers either side of the seed)
    return dict(wk=wk, valid=valid, keys=keys, count=count, first=pos[order][first], last=pos[order][first + count - 1], table=t,
                seed=seed_windows(seed, k), want=want)


def not_found(keys, hints, at, H):
    """(a): tests/read_pointers.py not_found over this batch"""
    return rp.not_found(keys, hints, at, H["wk"], H["valid"], BASES)


def _copy_walk(r):
    return None if r is None else {f: (np.array(v) if isinstance(v, np.ndarray) else v) for f, v in r.items()}


def _walks(ctx, H):
    hi, lo = H["seed"]
    return [_copy_walk(ctx.bfs(hi, lo, d, COV, 20000, -1)) for d in (-1, 1)]


def _export(ctx, n):
    import torch
    dev = torch.device("cuda:0")
    pk = torch.zeros(n, dtype=torch.int64, device=dev)
    pc = torch.zeros(n, dtype=torch.int16, device=dev)
    ph = torch.zeros(n, dtype=torch.int32, device=dev)
    assert ctx.export_dev(0, pk, pc, n, ph) == n
    keys, counts, hints = pk.cpu().numpy(), pc.cpu().numpy(), ph.cpu().numpy().view(np.uint32).astype(np.int64)
    o = np.argsort(keys, kind="stable")
    return keys[o], counts[o], hints[o]


def _device_reads():
    import torch
    dev = torch.device("cuda:0")
    _, _, off, words = read_set()
    return torch.from_numpy(words.view(np.int64)).to(dev), torch.from_numpy(off.view(np.int64)).to(dev), len(words)


@functools.lru_cache(maxsize=None)
def counted(case, position):
    """count_once, once a case and position; "rounds": the rounds of its two walks -- at store position 0, what the other positions'
    rounds are divided by, the median of three countings (which occurrence leaves its pointer is decided by the order of atomics:
    the direct kernel's control alone came out between 688 and 875 rounds in five runs)"""
    out = count_once(case, position)
    rounds = [sum(w["rounds"] for w in out["walks"])]
    if position == "control":
        rounds += [sum(w["rounds"] for w in count_once(case, position)["walks"]) for _ in range(2)]
    out["rounds"] = sorted(rounds)[len(rounds) // 2]
    return out


def count_once(case, position):
    """the batch counted at a store position the way the case says: the table's (key, count, hint) in key order, the two walks,
    and for the key exchange the (key, hint) pairs as they were extracted"""
    import metacherchant_amd as mc
    import torch
    k, mode, how, env = CASES[case]
    at = POSITIONS[position][0]
    H = host_side(k, mode)
    d_words, d_off, n_words = _device_reads()
    n_keys, n_windows = len(H["keys"]), int(H["valid"].sum())
    out = {}
    with switches(env):
        ctx = mc.Context(k, mode, 0, int(n_keys * 1.3) if how == "long" else 0)
        sender = mc.Context(k, mode, 0, 0) if how in ("superkmers", "keys") else None
    try:
        ctx.set_coverage_hint(COV)
        if sender is not None:  # (distributed.py's modes: every record the walking rank is handed carries a pointer)
            ctx.set_read_pointers(ctx.PTRS_OWN_STORE | ctx.PTRS_ON_EVERY_RECORD)
            sender.set_read_pointers(ctx.PTRS_STORE_ELSEWHERE | ctx.PTRS_ON_EVERY_RECORD)
            sender.read_store_seek(at)
            assert sender.read_store_tell() == at
        ctx.read_store_seek(at, at + BASES + 64)
        assert ctx.read_store_tell() == at
        if how in ("count", "long"):
            ctx.add_reads_packed_dev(d_words, d_off, N_READS, BASES)
            assert ctx.read_store_tell() == at + STORE_BASES
        else:
            ctx.read_store_import_dev(d_words, n_words, at)
            dev = torch.device("cuda:0")
            if how == "superkmers":
                cap = sender.superkmer_capacity(n_windows, N_READS)
                assert cap > 0
                d_recs = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
                d_ptrs = torch.zeros(cap, dtype=torch.int32, device=dev)
                n_rec = int(sender.extract_superkmers_dev(d_words, d_off, N_READS, BASES, 1, d_recs, d_ptrs, cap)[1])
                assert 0 < n_rec * 4 < n_windows
                ctx.add_superkmers_dev(d_recs, d_ptrs, n_rec)
            else:
                d_keys = torch.zeros(n_windows, dtype=torch.int64, device=dev)
                d_hints = torch.zeros(n_windows, dtype=torch.int32, device=dev)
                assert int(sender.extract_keys_dev(d_words, d_off, N_READS, BASES, 1, d_keys, n_windows, d_hints)[1]) == n_windows
                out["pairs"] = (d_keys.cpu().numpy(), d_hints.cpu().numpy().view(np.uint32).astype(np.int64))
                ctx.add_keys_dev(d_keys, n_windows, d_hints)
            assert sender.read_store_tell() == at + STORE_BASES and ctx.read_store_tell() == at
        assert ctx.finalize() == n_keys
        if how == "long":
            assert ctx.stats().long_runs >= 1
        out["keys"], out["counts"], out["hints"] = _export(ctx, n_keys)
        out["walks"] = _walks(ctx, H)
    finally:
        ctx.close()
        if sender is not None:
            sender.close()
        if at:  # (the pool gives the reserved block back)
            with mc.Context(k, mode, 0, 0) as c:
                c.trim()
    return out


@functools.lru_cache(maxsize=None)
def rounds_without_pointers(k, mode, env_items):
    """the rounds of the two walks over the same reads counted by a context that keeps no read pointers"""
    import metacherchant_amd as mc
    d_words, d_off, _ = _device_reads()
    H = host_side(k, mode)
    with switches(dict(env_items)):
        ctx = mc.Context(k, mode, 0, 0)
    with ctx:
        ctx.set_coverage_hint(COV)
        ctx.set_read_pointers(0)
        ctx.add_reads_packed_dev(d_words, d_off, N_READS, BASES)
        assert ctx.finalize() == len(H["keys"])
        walks = _walks(ctx, H)
    for got, want in zip(walks, H["want"]):
        assert_bfs_equal(got, want)
    return sum(w["rounds"] for w in walks)


def need_memory(position):
    """a position's reservation is the store up to it, a quarter of a byte a base: twice that must be free"""
    import torch
    need = (POSITIONS[position][0] + BASES + 64) // 4
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * need:
        pytest.skip("%s needs a reservation of %.1f GiB and twice that free: %.1f GiB are" % (position, need / 2 ** 30, free / 2 ** 30))


def test_the_batch_lies_where_the_cases_need_it():
    """No GPU, from the model and the oracle alone: at every boundary there are windows of a read on both sides and within
    16 bases below it, so that ptr_advance's boundary arm runs at the end of the exact tier, and the end of the range leaves at
    least 1000 keys of each kind that check (b) looks at"""
    for name, boundary in (("exact|4", rp.EXACT_END), ("4|16", rp.T2_POS), ("16|64", rp.T3_POS), ("64|end", rp.END)):
        at = POSITIONS[name][0]
        assert at % 32 == 0 and at < boundary - 100000 and boundary + 100000 < at + BASES
        for k, mode in {(c[0], c[1]) for c in CASES.values()}:
            H = host_side(k, mode)
            b = boundary - at
            assert b % L == 96 and H["valid"][b - 16:b].any() and H["valid"][b:b + 64].any(), (name, k)  # (k = 63: windows start at 0 .. 87 of a read)
            codes = rp.ptr_encode(at + np.arange(b - 16, b))
            if name == "exact|4":  # the arm: the code of an exact position whose record's later windows lie in the first granules
                assert ((codes - 1 < rp.EXACT_END) & (codes - 1 + 16 >= rp.EXACT_END)).all()
                assert (rp.ptr_range(rp.ptr_advance(codes, 15))[1] > 1).any()
    for name, (at, inside, tier) in POSITIONS.items():
        assert inside == (at + BASES <= rp.END)
        if tier is not None:
            assert (rp.ptr_range(rp.ptr_encode([at, at + BASES - 1]))[1] == rp.TIERS[tier][3]).all() and rp.TIERS[tier][0] <= at and at + BASES + 96 < rp.TIERS[tier][1]
    at = POSITIONS["64|end"][0]
    for k, mode in {(c[0], c[1]) for c in CASES.values()}:
        H = host_side(k, mode)
        assert ((H["first"] + at >= rp.END)).sum() >= 1000 and ((H["count"] >= COV) & (H["last"] + at < rp.END)).sum() >= 1000, k


every_case_and_position = [pytest.mark.gpu, pytest.mark.parametrize("position", list(POSITIONS)), pytest.mark.parametrize("case", list(CASES))]


def _both(case, position):
    need_memory(position)
    k, mode, _, _ = CASES[case]
    H = host_side(k, mode)
    R, R0 = counted(case, position), counted(case, "control")
    assert np.array_equal(R["keys"], H["keys"]) and np.array_equal(R["counts"], np.minimum(H["count"], 32767))
    return H, R, R0


def _mark(f):
    for m in every_case_and_position:
        f = m(f)
    return f


@_mark
def test_every_hint_leads_to_its_key(mc, case, position):
    """(a) the range of every exported hint holds a store position where a window with that key starts -- an exact hint names
    that position itself --, no range begins at or past the end of the codes' range; the (key, hint) pairs of the key exchange
    likewise, before they are added"""
    at, inside, _ = POSITIONS[position]
    H, R, _ = _both(case, position)
    bad = not_found(R["keys"], R["hints"], at, H)
    assert len(bad) == 0, "%d of %d hints lead nowhere, the first: %s" % (len(bad), int((R["hints"] != 0).sum()), [
        (int(R["keys"][i]), int(R["hints"][i]), [int(x[0]) for x in rp.ptr_range(R["hints"][i])], int(H["first"][i]) + at) for i in bad[:5]])
    if "pairs" in R:
        pk, ph = R["pairs"]
        assert inside == bool((ph != 0).all()) and len(not_found(pk, ph, at, H)) == 0


@_mark
def test_every_solid_key_has_a_hint(mc, case, position):
    """(b) inside the range every key with count >= the coverage hint has a hint, and every key that has one at store position 0
    has one; astride the end of the range the keys that lie past it have none and the solid keys below it have one.

    (exchange-records-k31 is the case that found count_pipeline.h k_sk1_records dealing whole tiles of a bucket-ordered record stream
    to its workgroups: 4 752 of the 70 411 records went through the spill list, whose records carry no pointers, and 225 to 255 of
    the 16 023 solid keys had no hint at any position, store position 0 included.)"""
    at, inside, _ = POSITIONS[position]
    H, R, R0 = _both(case, position)
    solid = H["count"] >= COV
    if inside:
        assert (R["hints"][solid] != 0).all(), "%d of %d solid keys without a hint" % (int((R["hints"][solid] == 0).sum()), int(solid.sum()))
        assert (R["hints"][R0["hints"] != 0] != 0).all()
    else:
        # A key has no hint when no occurrence of it can be named: the last granule's range ends 32 bases past the end of the
        # codes' range (a record that begins below the end may carry its later windows' pointers that far), so "past the end" is
        # from there on; the occurrences in those 32 bases may have a hint, and (a) checks it.
        past, below = H["first"] + at >= rp.END + rp.SLACK_LONG, solid & (H["last"] + at < rp.END)
        assert past.sum() >= 1000 and below.sum() >= 1000
        assert not R["hints"][past].any(), int((R["hints"][past] != 0).sum())
        assert (R["hints"][below] != 0).all(), "%d of %d solid keys below the end without a hint" % (int((R["hints"][below] == 0).sum()), int(below.sum()))


@_mark
def test_the_walk_and_its_rounds(mc, case, position):
    """(c) 20 000 k-mers leftwards and rightwards from a 200-base seed at coverage 3: the oracle's result and the control's; inside
    the range fewer rounds than over the same reads counted without read pointers; inside a granule tier at most the measured
    ratio + 0.25 times the control's rounds (which occurrence leaves its pointer depends on the order of atomics: rounds vary by a tenth
    or so from run to run)"""
    k, mode, _, env = CASES[case]
    _, inside, tier = POSITIONS[position]
    H, R, R0 = _both(case, position)
    for got, want, ctl in zip(R["walks"], H["want"], R0["walks"]):
        assert_bfs_equal(got, want)
        assert_bfs_equal(got, ctl)
    rounds, rounds0 = R["rounds"], R0["rounds"]
    without = rounds_without_pointers(k, mode, tuple(sorted(env.items())))
    print("read pointers %s at %s: %d rounds, %d at position 0 (ratio %.2f), %d without pointers, %d levels" % (
        case, position, rounds, rounds0, rounds / rounds0, without, sum(w["levels"] for w in R["walks"])))
    if inside:
        assert rounds < without, (rounds, without)
    if tier is not None:
        assert rounds / rounds0 <= MEASURED_RATIO[position] + 0.25, (rounds, rounds0)


@gpu
def test_reads_file_into_the_16_base_tier(mc, tmp_path):
    """(d) mc_add_reads_file lays the store out itself (reads_file.hip), so the host does not know the positions: the walk alone, after a seek into the 16-base tier, as check (c) has it"""
    k, mode = 31, po.KEY_PACKED
    need_memory("in16")
    H = host_side(k, mode)
    _, codes, _, _ = read_set()
    path = tmp_path / "reads.fastq"
    with open(path, "w") as f:
        for i, r in enumerate(codes.reshape(N_READS, L)):
            f.write("@r%d\n%s\n+\n%s\n" % (i, po.decode(r), "I" * L))
    rounds = {}
    for name, at in (("control", 0), ("in16", POSITIONS["in16"][0])):
        with switches({}):
            ctx = mc.Context(k, mode, 0, 0)
        with ctx:
            ctx.set_coverage_hint(COV)
            ctx.read_store_seek(at, at + 2 * BASES)
            assert ctx.add_reads_file(str(path)) == N_READS
            assert ctx.read_store_tell() >= at + BASES
            assert ctx.finalize() == len(H["keys"])
            walks = _walks(ctx, H)
            if at:
                ctx.trim()
        for got, want in zip(walks, H["want"]):
            assert_bfs_equal(got, want)
        rounds[name] = sum(w["rounds"] for w in walks)
    without = rounds_without_pointers(k, mode, ())
    print("read pointers of a reads file in the 16-base tier: %d rounds, %d at position 0, %d without pointers" % (rounds["in16"], rounds["control"], without))
    assert rounds["control"] < without and rounds["in16"] < without
    assert rounds["in16"] / rounds["control"] <= MEASURED_FILE_RATIO + 0.25


@gpu
@pytest.mark.parametrize("form", ["keys", "superkmers"])
def test_a_sender_past_the_range_sends_no_pointers(mc, form):
    """A context that keeps no store (mode 2) deemed to write at 150 G bases, the ninth of ten ranks' place when 10^9 reads of 150
    bases lie one rank behind the other: every pointer it extracts is 0 (and at position 0 none is), whatever the record form.
    Needs no memory: nothing is reserved."""
    import torch
    dev = torch.device("cuda:0")
    k, mode = (41, po.KEY_POLY) if form == "keys" else (31, po.KEY_PACKED)
    H = host_side(k, mode)
    d_words, d_off, _ = _device_reads()
    n_windows = int(H["valid"].sum())
    for at, some in ((0, True), (150 * 10 ** 9, False)):
        with mc.Context(k, mode, 0, 0) as sender:
            sender.set_read_pointers(sender.PTRS_STORE_ELSEWHERE | sender.PTRS_ON_EVERY_RECORD)
            sender.read_store_seek(at)
            assert at % 32 == 0 and sender.read_store_tell() == at
            if form == "keys":
                d_keys = torch.zeros(n_windows, dtype=torch.int64, device=dev)
                d_ptrs = torch.full((n_windows,), -1, dtype=torch.int32, device=dev)
                n = int(sender.extract_keys_dev(d_words, d_off, N_READS, BASES, 1, d_keys, n_windows, d_ptrs)[1])
                assert n == n_windows
            else:
                cap = sender.superkmer_capacity(n_windows, N_READS)
                d_recs = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
                d_ptrs = torch.full((cap,), -1, dtype=torch.int32, device=dev)
                n = int(sender.extract_superkmers_dev(d_words, d_off, N_READS, BASES, 1, d_recs, d_ptrs, cap)[1])
                assert 0 < n <= cap
            assert sender.read_store_tell() == at + STORE_BASES
            ptrs = d_ptrs[:n].cpu().numpy()
            assert (ptrs != 0).all() if some else not ptrs.any(), (at, int((ptrs != 0).sum()), n)
