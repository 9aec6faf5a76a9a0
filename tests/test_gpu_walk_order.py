"""GPU: mc_walk_order through the C ABI against tests/walk_order_model.py on the designed components of tests/walk_order_shapes.py.
Every shape runs with flags 0 (levels of up to 256 entries in one workgroup's LDS, wider ones across the grid), WIDE_ONLY (every
level across the grid) and NARROW_8 (the two paths change at 8 entries, so small shapes cross many times): order, reached and twice
must be the bounded model's, and the same bytes under all three.  Where the exact replay ends, it is asked too.  The unit
(csrc/walk_order.hip) changes its code path at WO_WIDE_K = 33 (one word a k-mer below, two from it on)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import walk_order_model as wm
from tests import walk_order_shapes as ws

pytestmark = pytest.mark.gpu

EINVAL = -1  # MC_EINVAL
FLAGS = (0, 1, 2)  # 0, MC_WALK_ORDER_WIDE_ONLY, MC_WALK_ORDER_NARROW_8


@functools.lru_cache(maxsize=None)
def _ctx(k):
    import metacherchant_amd as m
    return m.Context(k, m.KEY_PACKED if k <= 31 else m.KEY_POLY, 0, 0)


def _want(comps):
    """the bounded model's answer for a list of components, as the library lays it out"""
    n = sum(len(c) for c in comps)
    order, twice, reached, a = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8), [], 0
    stats = []
    for members in comps:
        o, t, st = wm.bounded_walk(members)
        order[a:a + len(o)] = o
        twice[a:a + len(members)] = t
        reached.append(len(o))
        stats.append(st)
        a += len(members)
    return order, np.array(reached, dtype=np.uint64), twice, stats


def _check(k, comps, flags=FLAGS, garbage=None, hi_none=False, want=None):
    """the device's answer is the model's under every flag setting; returns the result of the first setting"""
    order, reached, twice, stats = want or _want(comps)
    flat = [m for c in comps for m in c]
    hi, lo = ws.pack(flat, k, garbage)
    off = np.cumsum([0] + [len(c) for c in comps]).astype(np.uint64)
    first = None
    for f in flags:
        got = _ctx(k).walk_order(None if hi_none else hi, lo, off, f)
        assert got["n_components"] == len(comps) and got["n_kmers"] == len(flat)
        assert np.array_equal(got["reached"], reached), (k, f, got["reached"][:8], reached[:8])
        assert got["order"].dtype == np.uint32 and np.array_equal(got["order"], order), (k, f, np.nonzero(got["order"] != order)[0][:8])
        assert got["twice"].dtype == np.uint8 and np.array_equal(got["twice"], twice), (k, f, np.nonzero(got["twice"] != twice)[0][:8])
        assert got["queue_entries"] == sum(s["queue"] for s in stats) and got["levels"] == sum(s["levels"] for s in stats)
        if f == 1:
            assert got["wide_levels"] == got["levels"]
        if f == 0 and all(s["widest"] <= 256 for s in stats):
            assert got["wide_levels"] == 0
        if f == 2:
            assert (got["wide_levels"] > 0) == any(s["widest"] > 8 for s in stats)
        first = first or got
    return first


def _exact(members, cap=3_000_000):
    o, t, _ = wm.exact_replay(members, cap)
    return o, t


def test_single_kmers():
    got = _check(21, [[("ACGGT" * 5)[:21]]])
    assert got["order"].tolist() == [0] and got["twice"].tolist() == [0] and got["levels"] == 1
    got = _check(21, [["A" * 21]])  # its own neighbour
    assert got["twice"].tolist() == [1]
    _check(33, [["T" * 33]])
    _check(32, [["T" * 32]], hi_none=True)  # all ones in lo
    _check(6, [["ACGCGT"]])  # a palindrome at even k
    _check(22, [["ACGTTGCATGCATGCAACGT"[:11] + wm.rc("ACGTTGCATGCATGCAACGT"[:11])]])
    fw = ws.members_of(["TTGACCGTAGGTCA"], 7)
    bw = ws.members_of([wm.rc("TTGACCGTAGGTCA")], 7)  # the same k-mers, the seed from the other strand: the slot order changes
    a, b = _check(7, [fw]), _check(7, [bw])
    assert a["reached"].tolist() == b["reached"].tolist() == [len(fw)]


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1025, 5000])
def test_chains(n):
    k = 21 if n != 1025 else 41
    rng = np.random.default_rng(n)
    for seed_at in (0, n // 2):
        members = ws.chain(rng, k, n, seed_at)
        got = _check(k, [members])
        assert got["reached"].tolist() == [n] and not got["twice"].any()
        assert (got["order"].tolist(), [bool(x) for x in got["twice"]]) == _exact(members)


@pytest.mark.parametrize("n", [40, 41, 300, 301])
def test_cycles(n):
    members = ws.cycle(np.random.default_rng(n), 21, n)
    got = _check(21, [members])
    assert got["twice"].sum() == 1
    assert (got["order"].tolist(), [bool(x) for x in got["twice"]]) == _exact(members)


@pytest.mark.parametrize("k", [21, 41])
def test_bubbles(k):
    rng = np.random.default_rng(k)
    for members in (ws.bubbles(rng, k, 1), ws.bubbles(rng, k, 1, seed_end=False), ws.unequal_bubble_and_tip(rng, k), ws.bubbles(rng, k, 10)):
        got = _check(k, [members])
        assert (got["order"].tolist(), [bool(x) for x in got["twice"]]) == _exact(members)


def test_forty_bubbles_in_series():
    """the exact replay cannot end here (2^40 copies of the last stretch); the bounded walk is linear"""
    members = ws.bubbles(np.random.default_rng(40), 21, 40)
    got = _check(21, [members])
    assert got["reached"].tolist() == [len(members)] and got["queue_entries"] <= 2 * len(members)
    assert got["twice"].sum() > len(members) // 2


@pytest.mark.parametrize("k", [3, 4, 5])
def test_complete_graphs(k):
    members = ws.complete(k)
    got = _check(k, [members], hi_none=True)
    assert got["reached"].tolist() == [len(members)]
    if k == 3:
        assert (got["order"].tolist(), [bool(x) for x in got["twice"]]) == _exact(members)


@functools.lru_cache(maxsize=None)
def _random_component(k):
    rng = np.random.default_rng(1000 + k)
    return ws.members_of(ws.random_reads(rng, k), k)


@pytest.mark.parametrize("k", [5, 21, 31, 32, 33, 63])
def test_random_read_components(k):
    members = _random_component(k)
    garbage = np.random.default_rng(k) if k in (31, 32, 33, 63) else None
    got = _check(k, [members], garbage=garbage)
    assert got["reached"].tolist() == [len(members)]


def test_many_small_components_beside_a_large_one():
    rng = np.random.default_rng(77)
    big = ws.members_of(ws.random_reads(rng, 21, genome=18000, n_reads=3600), 21)
    assert 35000 <= len(big) <= 45000
    comps = [ws.chain(rng, 21, 1 + i % 5, (i // 5) % (1 + i % 5)) for i in range(1500)] + [big] + [ws.chain(rng, 21, 1 + i % 5) for i in range(1500)]
    got = _check(21, comps)
    assert got["n_components"] == 3001


def test_disconnected_slice_and_other_components():
    rng = np.random.default_rng(9)
    a, b = ws.chain(rng, 21, 30, 4), ws.chain(rng, 21, 10)
    got = _check(21, [a + b])  # a slice that does not hang together: the seed's part only
    assert got["reached"].tolist() == [30] and sorted(got["order"][:30].tolist()) == list(range(30)) and not got["order"][30:].any()
    # one chain cut into three slices: the neighbours in the other slices are ignored
    whole = ws.chain(rng, 33, 90)
    got = _check(33, [whole[:30], whole[30:70], whole[70:]])
    assert got["reached"].tolist() == [30, 40, 20]
    # a bubble whose one arm lies in another slice: nothing is popped twice any more
    members = ws.bubbles(rng, 21, 1)
    n_main = len(members) - 21
    got = _check(21, [members[:n_main], members[n_main:]])
    assert not got["twice"].any()


def test_bad_arguments():
    import metacherchant_amd as m
    from metacherchant_amd import native
    L = native.load()
    for k in (21, 41):
        ctx = _ctx(k)
        members = ws.chain(np.random.default_rng(3), k, 12)
        hi, lo = ws.pack(members, k)
        off = np.array([0, 5, 12], dtype=np.uint64)
        u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        out = native._WalkOrder()

        def call(hi_=hi, lo_=lo, off_=off, n_comp=2, flags=0, want=EINVAL, out_=out):
            C.memset(C.byref(out), 0x55, C.sizeof(out))
            rc = L.mc_walk_order(ctx._h, u64(hi_) if hi_ is not None else None, u64(lo_) if lo_ is not None else None,
                                 u64(off_) if off_ is not None else None, n_comp, flags, C.byref(out_) if out_ is not None else None)
            assert rc == want, (rc, want)
            if want != 0 and out_ is not None:
                assert bytes(out) == bytes(C.sizeof(out))  # *out is zeroed
        call(lo_=None)
        call(off_=None)
        call(out_=None)
        if k > 32:
            call(hi_=None)
        call(flags=4)
        call(flags=1 << 31)
        call(off_=np.array([1, 5, 12], dtype=np.uint64))  # does not start at 0
        call(off_=np.array([0, 5, 5], dtype=np.uint64))  # an empty component
        call(off_=np.array([0, 7, 5], dtype=np.uint64))  # descends
        call(off_=np.array([0, 1 << 30], dtype=np.uint64), n_comp=1)  # too many k-mers: decided before hi and lo are read
        call(n_comp=1 << 30)
        dup_lo, dup_hi = lo.copy(), hi.copy()
        dup_lo[9], dup_hi[9] = lo[2], hi[2]  # the same k-mer in two components
        call(hi_=dup_hi, lo_=dup_lo)
        rhi, rlo = ws.pack([wm.rc(members[2])], k)
        dup_lo[9], dup_hi[9] = rlo[0], rhi[0]  # its reverse complement
        call(hi_=dup_hi, lo_=dup_lo)
        assert L.mc_walk_order_dev(ctx._h, None, None, None, 2, 0, C.byref(out)) == EINVAL
        with pytest.raises(ValueError):
            ctx.walk_order(hi, lo[:11], off)  # comp_offsets does not end at the number of k-mers
        # nothing to do
        call(n_comp=0, want=0)
        assert out.n_components == 0 and out.n_kmers == 0 and not out.reached and not out.order and not out.twice
        L.mc_walk_order_free(C.byref(out))
        L.mc_walk_order_free(None)
        got = ctx.walk_order(hi[:0], lo[:0], np.zeros(1, dtype=np.uint64))
        assert got["n_components"] == 0 and len(got["order"]) == 0
        good = ctx.walk_order(hi, lo, off)  # and the context still works
        assert good["reached"].tolist() == [5, 7]
    assert m.WALK_ORDER_WIDE_ONLY == 1 and m.WALK_ORDER_NARROW_8 == 2


@pytest.mark.parametrize("k", [31, 63])
def test_the_device_form_and_two_calls(k):
    import torch
    rng = np.random.default_rng(k)
    comps = [ws.chain(rng, k, 700, 100), ws.bubbles(rng, k, 3), ws.chain(rng, k, 3)]
    flat = [m for c in comps for m in c]
    hi, lo = ws.pack(flat, k)
    off = np.cumsum([0] + [len(c) for c in comps]).astype(np.uint64)
    as_dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    d_hi, d_lo, d_off = as_dev(hi), as_dev(lo), as_dev(off)
    ctx = _ctx(k)
    a = _check(k, comps)
    for f in FLAGS:
        b = ctx.walk_order(hi, lo, off, f)
        d = ctx.walk_order_dev(d_hi if k > 32 else None, d_lo, d_off, len(comps), f)
        for name in ("reached", "order", "twice"):
            assert a[name].tobytes() == b[name].tobytes() == d[name].tobytes(), (f, name)
        assert d["device_ms"] > 0 and (d["levels"], d["queue_entries"]) == (a["levels"], a["queue_entries"])
    assert np.array_equal(d_lo.cpu().numpy().view(np.uint64), lo)  # (inputs are only read)


@pytest.mark.parametrize("k,mode", [(21, 0), (41, 1)])
def test_after_mc_components(k, mode):
    """end to end: the components of random reads as mc_components lists them, then their walk orders against the exact replay"""
    import metacherchant_amd as m
    rng = np.random.default_rng(k)
    reads = ws.random_reads(rng, k, genome=1500, n_reads=40, length=80)
    reads += [ws.rand_seq(rng, k + int(rng.integers(0, 6))) for _ in range(12)]  # and small components of their own
    codes = np.concatenate([po.encode(r) for r in reads]).astype(np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    with m.Context(k, mode, 0, 0) as c:
        c.add_reads_packed(po.pack(codes), off)
        c.finalize()
        comp = m.components(c, codes, off)
        assert comp["n_components"] > 5
        results = [m.walk_order(c, comp["hi"] if k > 32 else None, comp["lo"], comp["comp_offsets"], f) for f in FLAGS]
    co = comp["comp_offsets"]
    for ci in range(comp["n_components"]):
        a, b = int(co[ci]), int(co[ci + 1])
        members = [po.kmer_string(int(comp["hi"][i]), int(comp["lo"][i]), k) for i in range(a, b)]
        exact = wm.exact_replay(members, cap=64 * len(members) + 4096)
        order, twice, _ = wm.bounded_walk(members)
        if exact is not None:
            assert (order, twice) == exact[:2]
        for got in results:
            assert int(got["reached"][ci]) == b - a
            assert got["order"][a:b].tolist() == order and got["twice"][a:b].tolist() == [int(t) for t in twice], ci
