"""mc_save_kmers_gpu / mc_load_kmers_gpu (csrc/kmers_bin.hip) against the host loops mc_save_kmers / mc_load_kmers on the dense tables
of tests/kmers_bin_tables.py, with MC_KMERS_CHUNK_RECORDS at 64 and 1000 (several chunk boundaries inside a small file) and unset.
Needs a real MI355X."""
import numpy as np
import pytest

from oracle import host_oracle as ho
from oracle import pyoracle as po
from tests import kmers_bin_model as kb
from tests import kmers_bin_tables as tables
from tests.helpers import assert_bfs_equal, seed_windows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNKS = ["64", "1000", None]


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


def _set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("MC_KMERS_CHUNK_RECORDS", raising=False)
    else:
        monkeypatch.setenv("MC_KMERS_CHUNK_RECORDS", chunk)


@pytest.fixture(scope="module")
def reference_files(mc, tmp_path_factory):
    """per dense table: what the host loop writes"""
    out = {}
    d = tmp_path_factory.mktemp("kmers_ref")
    for k, mode in tables.DENSE:
        ctx = tables.dense_context(mc, k, mode)
        b, s = str(d / ("h%d.kmers.bin" % k)), str(d / ("h%d.stat.txt" % k))
        out[k] = dict(bin=b, stat=s, pair=ctx.save_kmers(b, s, 0))
        ctx.close()
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("k,mode", tables.DENSE)
def test_save(mc, monkeypatch, tmp_path, reference_files, k, mode, chunk):
    _set_chunk(monkeypatch, chunk)
    ref = reference_files[k]
    _, _, _, t, ok, oc = tables.dense_case(k, mode)
    ctx = tables.dense_context(mc, k, mode)
    for thr in (0, 3):
        b, s = str(tmp_path / ("g%d.kmers.bin" % thr)), str(tmp_path / ("g%d.stat.txt" % thr))
        hb, hs = str(tmp_path / ("h%d.kmers.bin" % thr)), str(tmp_path / ("h%d.stat.txt" % thr))
        assert ctx.save_kmers_gpu(b, s, thr) == ctx.save_kmers(hb, hs, thr)
        assert open(s, "rb").read() == open(hs, "rb").read() == ho.kmer_counter_files(t, thr)[1].encode()
        assert ho.read_kmers_bin(b) == ho.read_kmers_bin(hb) == ho.kmer_counter_files(t, thr)[0]
    # Where a key sits in its region depends on the order in which the counting kernels' atomics arrived, so two contexts that counted
    # the same reads hold the same table in different slots: the file is compared with mc_kmers_encode_dev's records of THIS context.
    # That call knows no chunks, so files equal to it are equal to each other whatever MC_KMERS_CHUNK_RECORDS is.
    import torch
    n_total, n_written = ref["pair"]
    buf = torch.zeros(10 * n_written, dtype=torch.uint8, device=DEV)
    assert ctx.kmers_encode_dev(0, buf, 10 * n_written, None) == ref["pair"]
    data = open(str(tmp_path / "g0.kmers.bin"), "rb").read()
    assert data == buf.cpu().numpy().tobytes(), "the file is not what mc_kmers_encode_dev gives (chunk %s)" % chunk
    again = str(tmp_path / "again.kmers.bin")
    assert ctx.save_kmers_gpu(again, None, 0) == ref["pair"]
    assert open(again, "rb").read() == data
    with pytest.raises(mc.native.McError, match="cannot write"):
        ctx.save_kmers_gpu(str(tmp_path / "no_such_dir" / "x.kmers.bin"), None, 0)
    ctx.close()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("k,mode", tables.DENSE)
def test_load(mc, monkeypatch, reference_files, k, mode, chunk):
    _set_chunk(monkeypatch, chunk)
    ref = reference_files[k]
    genome, _, _, t, ok, oc = tables.dense_case(k, mode)
    for thr in (0, 3):
        g, h = mc.Context(k, mode, 0, 0), mc.Context(k, mode, 0, 0)
        got, want = g.load_kmers_gpu(ref["bin"], thr), h.load_kmers(ref["bin"], thr)
        assert got == want == (len(ok), int((oc > thr).sum()))
        assert g.finalize() == h.finalize() == want[1]
        gk, gc = g.export(0)
        hk, hc = h.export(0)
        assert np.array_equal(gk, hk) and np.array_equal(gc, hc)
        assert np.array_equal(gk, ok[oc > thr]) and np.array_equal(gc, oc[oc > thr])
        if thr == 0:  # the walk of tests/test_gpu_cli.py::test_cli_kmer_counter_and_reload
            seed = genome[8000:8200]
            hi, lo = seed_windows(seed, k)
            assert_bfs_equal(g.bfs(hi, lo, 0, 4, 3000, -1), po.bfs(t, k, mode, [seed], 0, 4, 3000, -1))
        g.close()
        h.close()


def test_load_refuses_what_the_host_loop_refuses(mc, monkeypatch, tmp_path):
    monkeypatch.setenv("MC_KMERS_CHUNK_RECORDS", "64")
    ctx = mc.Context(25, po.KEY_PACKED, 0, 0)
    bad = tmp_path / "bad.kmers.bin"
    bad.write_bytes(b"123456789012345")
    with pytest.raises(mc.native.McError, match="multiple of the 10-byte record"):
        ctx.load_kmers_gpu(str(bad))
    # ... before anything is added, whatever the file's length: 100 whole records and a half
    recs, _ = kb.encode(np.arange(1, 101, dtype=np.int64), np.full(100, 7, dtype=np.int16), 0)
    bad.write_bytes(recs.tobytes() + b"12345")
    with pytest.raises(mc.native.McError, match="multiple of the 10-byte record"):
        ctx.load_kmers_gpu(str(bad))
    missing = str(tmp_path / "none.kmers.bin")
    with pytest.raises(mc.native.McError) as e:
        ctx.load_kmers_gpu(missing)
    with pytest.raises(mc.native.McError) as e_host:
        ctx.load_kmers(missing)
    assert str(e.value) == str(e_host.value) and "Failed to read from file " + missing in str(e.value)
    empty = tmp_path / "empty.kmers.bin"
    empty.write_bytes(b"")
    assert ctx.load_kmers_gpu(str(empty)) == (0, 0)
    assert ctx.finalize() == 0
    ctx.close()
