"""mc_render_fastq_dev / mc_render_fastq (csrc/render_fastq.hip) through the Python binding against tests/render_model.py, bytes equal:
designed reads at every base residue of a word and records at every byte residue of a 16-byte line, numbers that grow a digit inside a
call and pass 2^32, every stream count, empty streams, both sides into one stream, a ranking over several blocks, slices
(offsets[0] != 0), the unnumbered form, the data errors, the capacity check and the argument checks.  Nothing asserted is random.
Needs a real MI355X."""
import numpy as np
import pytest

from tests import render_model as rm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, GUARD_BYTES = 0xA5, 64
LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
FIRST_NUMBERS = [1, 8, 98, 998, 999999998, 4294967294, 10**18 - 2]


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(mc):
    with mc.Context(31, mc.KEY_PACKED, 0, 0) as c:
        yield c


def _read(n, salt=0):
    """n bases and phreds, both a function of (n, salt); the phreds run over 0 .. 62, the codes over all four (0 is what an N holds)"""
    i = np.arange(n)
    return ((i * 5 + salt) // 3 % 4).astype(np.uint8), ((i * 11 + salt * 7) % 63).astype(np.uint8)


def _arrays(sides, lead):
    """per side the four numpy arrays of the call; phred and stream get one more entry, so none is empty"""
    out = []
    for s, (reads, stream) in enumerate(sides):
        words, phred, offsets = rm.pack_side(reads, lead[s] if lead else 0)
        out.append((words, np.append(phred, np.uint8(63)), offsets, np.append(np.asarray(stream, dtype=np.uint8), np.uint8(99))))
    return out


def _upload(torch, arrays):
    return [tuple(torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(DEV) for a in side) for side in arrays]


def _bound(mc, sides):
    return mc.render_fastq_bound(sum(len(c) for reads, _ in sides for c, _ in reads), sum(len(reads) for reads, _ in sides))


def _call(mc, torch, ctx, sides, n_streams, first, capacity=None, lead=None):
    """(result, the whole buffer with its guard bytes, capacity): one call into a buffer filled with GUARD"""
    dev = _upload(torch, _arrays(sides, lead))
    capacity = _bound(mc, sides) if capacity is None else capacity
    buf = torch.full((capacity + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
    res = mc.render_fastq_dev(ctx, dev, len(sides[0][0]), n_streams, first, buf, capacity)
    return res, buf.cpu().numpy(), capacity


def _streams(res, raw, capacity, n_streams):
    """the streams' bytes; every byte outside them, the guard bytes included, must still hold GUARD"""
    untouched = np.ones(len(raw), dtype=bool)
    out, end = [], 0
    for t in range(n_streams):
        a, n = res["start"][t], res["bytes"][t]
        assert a % 16 == 0 and a >= end and a + n <= capacity, (t, res)
        out.append(raw[a:a + n].tobytes())
        untouched[a:a + n] = False
        end = a + n
    assert (raw[untouched] == GUARD).all(), "bytes outside the streams were written"
    return out


def _check(mc, torch, ctx, sides, n_streams, first, lead=None):
    want, err = rm.render(sides, n_streams, first)
    assert err is None
    res, raw, capacity = _call(mc, torch, ctx, sides, n_streams, first, lead=lead)
    assert res["error"] == 0, res
    got = _streams(res, raw, capacity, n_streams)
    for t in range(n_streams):
        assert got[t] == want[t], "stream %d differs" % t
    n_sides = len(sides)
    want_records = [sum(1 for s in range(n_sides) for x in sides[s][1] if x == t) for t in range(n_streams)]
    assert res["records"] == want_records
    return res, want


def _record_starts(texts_lengths):
    """byte residues mod 16 at which the records of a stream start, from the reads' record lengths"""
    at, seen = 0, set()
    for n in texts_lengths:
        seen.add(at % 16)
        at += n
    return seen


def _every_residue_reads():
    """every length of LENGTHS starting at every base residue mod 32: in front of each such read a filler read brings the position there
    (selected when it has bases, skipped when it is empty -- a skipped read is not looked at)"""
    reads, stream, cur = [], [], 0
    for n in LENGTHS:
        for r in range(32):
            pad = (r - cur) % 32
            reads.append(_read(pad, r))
            stream.append(1 if pad else rm.SKIP)
            cur += pad
            assert cur % 32 == r
            reads.append(_read(n, n + r))
            stream.append(0)
            cur += n
    return reads, stream


def test_every_length_at_every_base_residue(mc, torch, ctx):
    reads, stream = _every_residue_reads()
    res, want = _check(mc, torch, ctx, [(reads, stream)], 2, [1, 1])
    lens = [len(rm.record(c, q, i + 1)) for i, (c, q) in enumerate(r for r, s in zip(reads, stream) if s == 0)]
    assert _record_starts(lens) == set(range(16))
    assert want[0].count(b"\n+\n") == 32 * len(LENGTHS)


def test_every_length_from_both_sides_into_one_stream(mc, torch, ctx):
    reads, stream = _every_residue_reads()
    other = [_read(len(c) + 1, 9) for c, _ in reads]
    # side 1 feeds stream 0 as well (item order: side 0's read, then side 1's), and a stream of its own
    _check(mc, torch, ctx, [(reads, stream), (other, [0 if i % 3 else 2 for i in range(len(other))])], 3, [1, 1, 7])


@pytest.mark.parametrize("numbered", [True, False])
def test_short_reads_share_dwords_and_lines(mc, torch, ctx, numbered):
    lens = [1, 2, 1, 1, 2, 2, 1, 2, 1, 1, 1, 2] * 20
    reads = [_read(n, i) for i, n in enumerate(lens)]
    first = [1 if numbered else rm.UNNUMBERED]
    _check(mc, torch, ctx, [(reads, [0] * len(reads))], 1, first)
    rec = [len(rm.record(c, q, i + 1 if numbered else None)) for i, (c, q) in enumerate(reads)]
    assert min(rec) < 16 and _record_starts(rec) == set(range(16))  # several records in a 16-byte line, at every residue


@pytest.mark.parametrize("first", FIRST_NUMBERS)
def test_numbers_grow_a_digit_inside_a_call(mc, torch, ctx, first):
    reads = [_read(n, n) for n in (3, 150, 1, 17, 64, 2, 5, 33, 4, 31, 16, 1)]
    res, want = _check(mc, torch, ctx, [(reads, [0] * 12)], 1, [first])
    assert len({len(str(first + i)) for i in range(12)}) == 2 or first == 4294967294  # (that one passes 2^32 instead)
    assert (b"@%d\n" % (first + 11)) in want[0]


def test_all_first_numbers_in_one_call(mc, torch, ctx):
    reads = [_read(10 + i % 5, i) for i in range(6 * len(FIRST_NUMBERS))]
    stream = [i % len(FIRST_NUMBERS) for i in range(len(reads))]
    _check(mc, torch, ctx, [(reads, stream)], len(FIRST_NUMBERS), FIRST_NUMBERS)


@pytest.mark.parametrize("n_streams", [1, 2, 9, 16])
def test_stream_counts(mc, torch, ctx, n_streams):
    n = 300
    a = [_read(1 + i % 40, i) for i in range(n)]
    b = [_read(1 + i % 23, i + 1) for i in range(n)]
    pick = lambda x: x if x < n_streams else rm.SKIP  # noqa: E731
    sides = [(a, [pick((i * 7) % (n_streams + 1)) for i in range(n)]), (b, [pick((i * 5 + 3) % (n_streams + 1)) for i in range(n)])]
    res, _ = _check(mc, torch, ctx, sides, n_streams, [1 + 10 * t for t in range(n_streams)])
    assert all(res["records"])


def test_a_stream_with_no_item_all_skipped_and_no_reads(mc, torch, ctx):
    reads = [_read(5 + i, i) for i in range(10)]
    res, _ = _check(mc, torch, ctx, [(reads, [0, 2] * 5)], 3, [1, 1, 1])
    assert res["records"] == [5, 0, 5] and res["bytes"][1] == 0
    res, _ = _check(mc, torch, ctx, [(reads, [rm.SKIP] * 10)], 3, [1, 1, 1])
    assert res["records"] == [0, 0, 0] and res["bytes"] == [0, 0, 0]
    res, _ = _check(mc, torch, ctx, [([], []), ([], [])], 2, [1, 1])
    assert res["records"] == [0, 0] and res["bytes"] == [0, 0]


def test_five_thousand_items_rank_over_several_blocks(mc, torch, ctx):
    n = 2500
    a = [_read(1 + i % 7, i) for i in range(n)]
    b = [_read(1 + i % 5, i + 2) for i in range(n)]
    sides = [(a, [(i * 3) % 9 for i in range(n)]), (b, [(i // 300) % 9 for i in range(n)])]  # (side 1: whole blocks of one stream)
    res, _ = _check(mc, torch, ctx, sides, 9, [1, 8, 98, 998, rm.UNNUMBERED, 1, 1, 4294967000, 1])
    assert sum(res["records"]) == 5000


def test_a_slice_whose_offsets_do_not_start_at_zero(mc, torch, ctx):
    # (the bases in front are other reads'; their phreds are 63, which a selected read may not have)
    a = [_read(n, n) for n in (31, 1, 150, 64, 2)]
    b = [_read(n, n + 1) for n in (7, 33, 1, 100, 65)]
    _check(mc, torch, ctx, [(a, [0, 0, 1, 0, 1]), (b, [1, 0, 0, rm.SKIP, 0])], 2, [1, 98], lead=[37, 64 + 5])


def test_unnumbered_beside_numbered(mc, torch, ctx):
    reads = [_read(1 + i % 33, i) for i in range(200)]
    res, want = _check(mc, torch, ctx, [(reads, [i % 2 for i in range(200)])], 2, [rm.UNNUMBERED, 999])
    lengths = [len(c) for i, (c, _) in enumerate(reads) if i % 2 == 0]
    numbered, _ = rm.render([(reads, [0 if i % 2 == 0 else rm.SKIP for i in range(200)])], 1, [5])
    assert rm.number_bodies(rm.split_bodies(want[0], lengths), 5) == numbered[0]


def _with_phred(read, at, value):
    q = read[1].copy()
    q[at] = value
    return read[0], q


@pytest.mark.parametrize("where", ["empty", "first", "middle", "last"])
def test_data_errors_name_the_item(mc, torch, ctx, where):
    a = [_read(150, i) for i in range(700)]
    b = [_read(150, i + 1) for i in range(700)]
    if where == "empty":
        b[412] = _read(0)
        want = (rm.EMPTY, 1, 412, 0)
    else:
        b[412] = _with_phred(b[412], {"first": 0, "middle": 77, "last": 149}[where], 63)
        want = (rm.QUALITY, 1, 412, 63)
    sides = [(a, [0] * 700), (b, [1] * 700)]
    assert rm.render(sides, 2, [1, 1])[1] == want
    res, _, _ = _call(mc, torch, ctx, sides, 2, [1, 1])
    assert (res["error"], res["error_side"], res["error_read"], res["error_value"]) == want
    sides[1][1][412] = rm.SKIP  # a skipped read is not looked at
    _check(mc, torch, ctx, sides, 2, [1, 1])


@pytest.mark.parametrize("lower", ["quality", "empty"])
def test_of_two_offenders_the_lower_item_is_reported(mc, torch, ctx, lower):
    a = [_read(20, i) for i in range(600)]
    b = [_read(20, i + 1) for i in range(600)]
    if lower == "quality":  # item 2 * 100 + 1 before item 2 * 500
        b[100] = _with_phred(_with_phred(b[100], 3, 70), 11, 63)
        a[500] = _read(0)
        want = (rm.QUALITY, 1, 100, 70)
    else:
        a[100] = _read(0)
        b[100] = _with_phred(b[100], 0, 63)
        want = (rm.EMPTY, 0, 100, 0)
    sides = [(a, [0] * 600), (b, [0] * 600)]
    assert rm.render(sides, 1, [1])[1] == want
    res, _, _ = _call(mc, torch, ctx, sides, 1, [1])
    assert (res["error"], res["error_side"], res["error_read"], res["error_value"]) == want


def _some_sides():
    a = [_read(1 + i % 50, i) for i in range(400)]
    b = [_read(1 + i % 31, i + 3) for i in range(400)]
    return [(a, [i % 3 for i in range(400)]), (b, [(i + 1) % 4 if (i + 1) % 4 < 3 else rm.SKIP for i in range(400)])]


def test_capacity(mc, torch, ctx):
    sides = _some_sides()
    res, raw, capacity = _call(mc, torch, ctx, sides, 3, [1, 1, 1])
    need = res["start"][2] + res["bytes"][2]
    assert need <= capacity == _bound(mc, sides)
    want, _ = rm.render(sides, 3, [1, 1, 1])
    # exactly enough: the same streams, the guard bytes behind them untouched
    res2, raw2, _ = _call(mc, torch, ctx, sides, 3, [1, 1, 1], capacity=need)
    assert _streams(res2, raw2, need, 3) == want
    # one byte short: refused before anything is written
    with pytest.raises(mc.McError) as e:
        _call(mc, torch, ctx, sides, 3, [1, 1, 1], capacity=need - 1)
    assert e.value.code == -5
    dev = _upload(torch, _arrays(sides, None))
    buf = torch.full((need - 1 + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
    with pytest.raises(mc.McError):
        mc.render_fastq_dev(ctx, dev, 400, 3, [1, 1, 1], buf, need - 1)
    assert (buf.cpu().numpy() == GUARD).all()


def test_two_calls_give_the_same_bytes(mc, torch, ctx):
    sides = _some_sides()
    res1, raw1, _ = _call(mc, torch, ctx, sides, 3, [1, 98, 1])
    res2, raw2, _ = _call(mc, torch, ctx, sides, 3, [1, 98, 1])
    assert {k: v for k, v in res1.items() if k != "device_ms"} == {k: v for k, v in res2.items() if k != "device_ms"}
    assert np.array_equal(raw1, raw2)


def test_bad_arguments(mc, torch, ctx):
    sides = _some_sides()
    dev = _upload(torch, _arrays(sides, None))
    buf = torch.full((_bound(mc, sides) + 16,), GUARD, dtype=torch.uint8, device=DEV)
    cap = _bound(mc, sides)

    def refused(*args):
        with pytest.raises(mc.McError) as e:
            mc.render_fastq_dev(ctx, *args)
        assert e.value.code == -1
        return e.value

    for hole in range(4):  # a null pointer in a side
        broken = [dev[0], tuple(None if i == hole else x for i, x in enumerate(dev[1]))]
        refused(broken, 400, 3, [1, 1, 1], buf, cap)
    refused(dev, 400, 3, [1, 1, 1], None, cap)
    refused([], 400, 3, [1, 1, 1], buf, cap)
    refused(dev + dev[:1], 400, 3, [1, 1, 1], buf, cap)
    refused(dev, 400, 0, [1, 1, 1], buf, cap)
    refused(dev, 400, 17, [1] * 17, buf, cap)
    refused(dev, 400, 3, [1, 1, 1], buf[1:], cap)
    e = refused(dev, 400, 2, [1, 1], buf, cap)  # side 1 of read 1 names stream 2, before side 0 of read 2 does
    assert rm.render(sides, 2, [1, 1])[1] == (rm.STREAM, 1, 1, 2)
    assert (e.result["error"], e.result["error_side"], e.result["error_read"], e.result["error_value"]) == (rm.STREAM, 1, 1, 2)
    assert (buf.cpu().numpy() == GUARD).all()
    # sixteen streams take the bytes 0 .. 15: 16 is refused
    reads = [_read(9, i) for i in range(40)]
    ok = [(reads, [i % 16 for i in range(40)])]
    _check(mc, torch, ctx, ok, 16, [1] * 16)
    bad = [(reads, [16 if i == 33 else i % 16 for i in range(40)])]
    assert rm.render(bad, 16, [1] * 16)[1] == (rm.STREAM, 0, 33, 16)
    with pytest.raises(mc.McError) as e:
        _call(mc, torch, ctx, bad, 16, [1] * 16)
    assert e.value.code == -1
    assert (e.value.result["error"], e.value.result["error_read"], e.value.result["error_value"]) == (rm.STREAM, 33, 16)


def test_the_host_form_equals_the_device_form(mc, torch, ctx):
    sides = _some_sides()
    lead = [37, 5]
    res, raw, capacity = _call(mc, torch, ctx, sides, 3, [1, rm.UNNUMBERED, 4294967290], lead=lead)
    dev_streams = _streams(res, raw, capacity, 3)
    text, hres = mc.render_fastq(ctx, _arrays(sides, lead), 400, 3, [1, rm.UNNUMBERED, 4294967290], fill=GUARD)
    assert [hres[k] for k in ("start", "bytes", "records", "error")] == [res[k] for k in ("start", "bytes", "records", "error")]
    assert _streams(hres, text, len(text), 3) == dev_streams
    want, _ = rm.render(sides, 3, [1, rm.UNNUMBERED, 4294967290])
    assert dev_streams == want
    # ... and its errors
    sides[0][0][7] = _with_phred(sides[0][0][7], 0, 63)
    _, hres = mc.render_fastq(ctx, _arrays(sides, lead), 400, 3, [1, 1, 1])
    assert (hres["error"], hres["error_side"], hres["error_read"], hres["error_value"]) == rm.render(sides, 3, [1, 1, 1])[1]
