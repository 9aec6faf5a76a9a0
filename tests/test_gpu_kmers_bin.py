"""mc_kmers_encode_dev / mc_kmers_decode_dev (csrc/kmers_bin.hip) against tests/kmers_bin_model.py: designed tables whose tiles are
mostly empty (empty slices, slices of one record that leave the next one starting in the middle of a dword), dense tables, a
table with a shadow slot of the key join, the argument checks, the decoder at every tile boundary, and the round trip.  The key -1
(the table's free-slot mark, counted out of band) is not exercised here.  Needs a real MI355X."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import kmers_bin_model as kb
from tests import kmers_bin_tables as tables
from tests.helpers import oracle_table, synth_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
THRESHOLDS = [-1, 0, 1, 255, 32766, 32767]
GUARD = 0xA5


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _encode(torch, ctx, threshold, slack=64):
    """(n_total, n_written, the records' bytes, histogram): a count-only call sizes a buffer with `slack` guard bytes behind"""
    hist = torch.full((kb.HIST_BINS,), -1, dtype=torch.int64, device=DEV)
    n_total, n_written = ctx.kmers_encode_dev(threshold, None, 0, hist)
    counted = hist.cpu().numpy().astype(np.uint64)
    buf = torch.full((10 * n_written + slack,), GUARD, dtype=torch.uint8, device=DEV)
    hist.fill_(-1)
    assert ctx.kmers_encode_dev(threshold, buf, 10 * n_written, hist) == (n_total, n_written)
    raw = buf.cpu().numpy()
    assert (raw[10 * n_written:] == GUARD).all(), "bytes behind the records were touched"
    h = hist.cpu().numpy().astype(np.uint64)
    assert np.array_equal(h, counted)
    return n_total, n_written, raw[:10 * n_written].copy(), h


def _check_against(torch, ctx, keys, values, thresholds):
    """keys sorted with their values: what the table holds"""
    for thr in thresholds:
        n_total, n_written, raw, hist = _encode(torch, ctx, thr)
        sel = values.astype(np.int64) > thr
        assert n_total == len(keys) and n_written == int(sel.sum()), (thr, n_total, n_written)
        assert np.array_equal(hist, np.bincount(values.astype(np.int64), minlength=kb.HIST_BINS).astype(np.uint64)), thr
        fk, fc = kb.decode(raw, -32769)  # file order
        assert np.array_equal(kb.encode(fk, fc, -32769)[0], raw), thr
        sk, sc = kb.sorted_records(raw)
        assert np.array_equal(sk, keys[sel]) and np.array_equal(sc, values[sel]), thr


@pytest.mark.parametrize("k,mode", tables.DENSE)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 4097])
def test_encode_designed_tables(mc, torch, n, k, mode):
    ctx, keys, values = tables.designed_context(mc, n, k, mode)
    if n >= 2:
        assert 0 in keys and 0x0102030405060708 in keys
    if n == 4097:
        assert set(tables.DESIGNED_COUNTS) <= set(values.tolist())
        assert mode == po.KEY_PACKED or (keys < 0).any()
    _check_against(torch, ctx, keys, values, THRESHOLDS)
    ctx.close()


@pytest.mark.parametrize("k,mode", tables.DENSE)
def test_encode_a_dense_table_and_the_round_trip(mc, torch, k, mode):
    _, _, _, t, ok, oc = tables.dense_case(k, mode)
    ctx = tables.dense_context(mc, k, mode)
    gk, gc = ctx.export(0)
    assert np.array_equal(gk, ok) and np.array_equal(gc, oc)
    _check_against(torch, ctx, gk, gc, [0, 3])
    a = _encode(torch, ctx, 0)
    b = _encode(torch, ctx, 0)
    assert np.array_equal(a[2], b[2]), "two calls on one table gave different bytes"
    # decode what was encoded, add it to a fresh context: the same table
    n = a[1]
    d_bytes = torch.from_numpy(a[2]).to(DEV)
    d_keys = torch.zeros(n, dtype=torch.int64, device=DEV)
    d_counts = torch.zeros(n, dtype=torch.int16, device=DEV)
    assert ctx.kmers_decode_dev(d_bytes, n, 0, d_keys, d_counts) == n
    ctx2 = mc.Context(k, mode, 0, 0)
    ctx2.add_pairs_dev(d_keys, d_counts, n)
    assert ctx2.finalize() == t.size()
    gk2, gc2 = ctx2.export(0)
    assert np.array_equal(gk2, ok) and np.array_equal(gc2, oc)
    ctx2.close()
    ctx.close()


def _rc(c):
    return (3 - c[::-1]).astype(np.uint8)


def _planted(k, v):
    """tests/test_gpu_collisions.py::_planted for one vector: x inside one contig, y inside another, both tiled with error-free
    reads of 150 bases every 10 on both strands, and 50 000 reads over 2 x 200 kb"""
    rng = np.random.default_rng(7 * k + 1)
    _, reads, off = synth_case(2, 200000, 50000, 150, 50)
    pieces, lens = [reads], np.diff(off).tolist()
    for s in (po.encode(v["x"]), po.encode(v["y"])):
        c = rng.integers(0, 4, 4000).astype(np.uint8)
        c[2000:2000 + k] = s
        for j, st in enumerate(range(0, 4000 - 150 + 1, 10)):
            r = c[st:st + 150]
            pieces.append(_rc(r) if j & 1 else r)
            lens.append(150)
    return np.concatenate(pieces), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def test_encode_counts_a_shadow_slot_once(mc, torch, monkeypatch):
    """two k-mers with one polynomial key sit in two minimizer bins: the key is one record with the sum of the counters"""
    monkeypatch.setenv("MC_COUNT_PATH", "partition")
    monkeypatch.delenv("MC_LONG_RECORDS", raising=False)
    monkeypatch.delenv("MC_LONG_BINS", raising=False)
    v = json.load(open(os.path.join(HERE, "golden", "poly_collisions.json")))["vectors"][0]
    k = v["k"]
    codes, offs = _planted(k, v)
    t, _ = oracle_table(codes, offs, k, po.KEY_POLY)
    ok, oc = t.dump()
    ctx = mc.Context(k, mc.KEY_POLY, 0, int(t.size() * 1.3))
    ctx.add_reads_packed(po.pack(codes), offs)
    assert ctx.finalize() == t.size()
    assert ctx.stats().dup_keys >= 1, "the planted key was meant to sit in two regions"
    n_total, n_written, raw, hist = _encode(torch, ctx, 0)
    assert n_total == n_written == t.size()
    fk, fc = kb.decode(raw, -32769)
    hit = np.nonzero(fk == v["key"])[0]
    assert len(hit) == 1 and int(fc[hit[0]]) == int(t.get(v["key"]))
    sk, sc = kb.sorted_records(raw)
    assert np.array_equal(sk, ok) and np.array_equal(sc, oc)
    assert np.array_equal(hist, np.bincount(oc.astype(np.int64), minlength=kb.HIST_BINS).astype(np.uint64))
    ctx.close()


def test_encode_argument_checks(mc, torch):
    ctx, keys, values = tables.designed_context(mc, 5, 25, po.KEY_PACKED)
    need = 10 * len(keys)
    buf = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=DEV)
    with pytest.raises(mc.native.McError) as e:
        ctx.kmers_encode_dev(-1, buf, need - 10, None)
    assert e.value.code == -1 and str(need) in str(e.value) and str(need - 10) in str(e.value)
    assert (buf.cpu().numpy()[need - 10:] == GUARD).all()
    assert ctx.kmers_encode_dev(-1, None, 0, None) == (5, 5)
    assert ctx.kmers_encode_dev(32767, None, 0, None) == (5, 0)
    with pytest.raises(mc.native.McError, match="16-byte aligned"):
        ctx.kmers_encode_dev(-1, buf[2:], need, None)
    assert (buf.cpu().numpy() == GUARD).all()
    assert ctx.kmers_encode_dev(-1, buf, need, None) == (5, 5)
    ctx.close()
    fresh = mc.Context(25, po.KEY_PACKED, 0, 0)
    with pytest.raises(mc.native.McError) as e:
        fresh.kmers_encode_dev(0, None, 0, None)
    assert e.value.code == -4  # MC_ESTATE
    fresh.close()


@pytest.fixture(scope="module")
def any_ctx(mc):
    ctx = mc.Context(25, po.KEY_PACKED, 0, 0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 409, 2047, 2048, 2049, 4097, 100003])
def test_decode(any_ctx, torch, n):
    rng = np.random.default_rng(77 + n)
    raw = rng.integers(0, 256, 10 * n, dtype=np.uint8)  # keys over all of int64, counts over all of int16
    if n >= 2:
        raw[8:10] = (0x80, 0x00)  # -32768
        raw[18:20] = (0x7F, 0xFF)
    d_bytes = torch.from_numpy(raw).to(DEV) if n else torch.zeros(16, dtype=torch.uint8, device=DEV)
    for thr in (-32768, -1, 0, 3, 32767):
        wk, wc = kb.decode(raw, thr)
        d_keys = torch.full((n + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        d_counts = torch.full((n + 8,), 0x5A5A, dtype=torch.int16, device=DEV)
        kept = any_ctx.kmers_decode_dev(d_bytes, n, thr, d_keys, d_counts)
        assert kept == len(wk), (n, thr)
        gk, gc = d_keys.cpu().numpy(), d_counts.cpu().numpy()
        assert (gk[kept:] == 0x5A5A5A5A5A5A5A5A).all() and (gc[kept:] == 0x5A5A).all(), "entries behind the kept ones were touched"
        o, w = np.lexsort((gc[:kept], gk[:kept])), np.lexsort((wc, wk))
        assert np.array_equal(gk[:kept][o], wk[w]) and np.array_equal(gc[:kept][o], wc[w]), (n, thr)
    if n >= 2:
        assert len(kb.decode(raw, 0)[0]) == len(kb.decode(raw[10:], 0)[0])  # (count bytes 80 00 are dropped at threshold 0)


def test_decode_refuses_a_misaligned_pointer(mc, any_ctx, torch):
    d_bytes = torch.zeros(64, dtype=torch.uint8, device=DEV)
    d_keys = torch.zeros(4, dtype=torch.int64, device=DEV)
    d_counts = torch.zeros(4, dtype=torch.int16, device=DEV)
    with pytest.raises(mc.native.McError, match="16-byte aligned") as e:
        any_ctx.kmers_decode_dev(d_bytes[2:], 4, 0, d_keys, d_counts)
    assert e.value.code == -1
