"""Two outcomes of the partitioned counting pipeline's driver (csrc/mcgpu.hip, enum RunOutcome) that no other test reaches, each
sized from pipe_prepare's and mc_create's own formulas and compared with the oracle on every (key, count):

* RUN_BATCH_AGAIN -- the merge into an EMPTY table finds regions overflowing, the table is replaced by one sized by what the
  merged leaves held, and add_reads_partitioned runs the batch again;
* RUN_LOST_RECORDS for a flat key stream (mc_add_keys_dev) -- one level-1 bucket overflows its segments and the spill list, nothing
  is merged, and add_keys_partitioned counts the keys with the direct kernel.

Needs a real MI355X."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests.helpers import oracle_table, synth_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import metacherchant_amd as m
    m.native.load()
    return m


def _assert_table(ctx, t):
    ok, oc = t.dump()
    assert ctx.finalize() == t.size()
    gk, gc = ctx.export(0)
    assert np.array_equal(gk, ok) and np.array_equal(gc, oc)


def test_an_empty_table_far_too_small_is_replaced_and_the_batch_runs_again(mc, monkeypatch, capfd):
    """A capacity hint of 1 vouches for the table, so nothing samples the batch: the table keeps mc_create's minimum of 2^22 slots,
    and the list the merge kernel hands occurrences on through takes 2^22 more (mc_ctx::OVF_CAP).  100 000 random reads hold
    12 M distinct 31-mers, 1.4 times the two together: leaves stay unmerged, and since the table held nothing the driver sizes a
    new one from the leaves that were merged and counts the batch again -- once, with the windows booked once."""
    monkeypatch.setenv("MC_COUNT_PATH", "partition")
    monkeypatch.setenv("MC_INGEST_DEBUG", "1")
    n_reads, L, k = 100_000, 150, 31
    reads = np.random.default_rng(20).integers(0, 4, n_reads * L).astype(np.uint8)
    off = np.arange(n_reads + 1, dtype=np.uint64) * L
    t, n = oracle_table(reads, off, k, po.KEY_PACKED)
    assert t.size() > 5 << 21  # (2.5 x 2^22)
    ctx = mc.Context(k, mc.KEY_PACKED, 0, 1)
    ctx.add_reads_packed(po.pack(reads), off)
    err = capfd.readouterr().err
    assert "[count] table too small:" in err, err
    st = ctx.stats()
    assert st.grows >= 1 and st.count_launches == 1 and st.windows == n
    _assert_table(ctx, t)
    ctx.close()


def test_a_key_stream_of_one_heavy_key_loses_records_and_goes_through_the_direct_kernel(mc, monkeypatch):
    """1.5 M copies of one key and 5 000 other keys.  pipe_prepare gives a flat key stream a spill list of max(n / 64, 2^20) keys and
    every level-1 bucket 256 segments of n / np1 / 256 * 1.25 + 256 keys -- under 70 000 in all with the 512 buckets of the smallest
    table: the heavy key's bucket and the spill list hold 1.12 M, the stream loses records, the merge kernel merges nothing, and the
    keys are counted by the direct kernel (which books no launch of the pipeline).  The heavy key's count saturates at 32767 as the
    oracle's does."""
    import torch
    monkeypatch.setenv("MC_COUNT_PATH", "partition")
    k, heavy_n = 31, 1_500_000
    _, reads, off = synth_case(1, 20000, 300, 150, 0)
    small, _ = oracle_table(reads, off, k, po.KEY_PACKED)
    others = small.dump()[0][:5000]
    assert len(others) == 5000
    keys = np.concatenate([np.full(heavy_n, others[0], dtype=np.int64), others])
    t = po.Table()
    t.add(int(others[0]), heavy_n)
    for key_ in others:
        t.add(int(key_), 1)
    ctx = mc.Context(k, mc.KEY_PACKED, 0, 0)
    ctx.add_keys_dev(torch.from_numpy(keys).to("cuda:0"), len(keys))
    st = ctx.stats()
    assert st.count_launches == 0 and st.p3_ms == 0, "the pipeline was meant to lose records and merge nothing"
    _assert_table(ctx, t)
    assert t.get(int(others[0])) == 32767
    ctx.close()
