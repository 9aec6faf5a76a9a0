"""tests/kmers_bin_model.py against the oracle's kmer-counter files and on hand-written records (no GPU)."""
import struct

import numpy as np
import pytest

from oracle import host_oracle as ho
from oracle import pyoracle as po
from tests import kmers_bin_model as kb
from tests.helpers import oracle_table, synth_case


@pytest.fixture(scope="module")
def reads():
    _, codes, off = synth_case(1, 30000, 4000, 150, 80)
    return codes, off


@pytest.mark.parametrize("k,mode", [(25, po.KEY_PACKED), (40, po.KEY_POLY)])
@pytest.mark.parametrize("threshold", [0, 3])
def test_model_equals_the_oracles_files(reads, tmp_path, k, mode, threshold):
    t, _ = oracle_table(reads[0], reads[1], k, mode)
    keys, counts = t.dump()
    want_recs, want_stat = ho.kmer_counter_files(t, threshold)
    data, hist = kb.encode(keys, counts, threshold)
    assert len(data) == 10 * len(want_recs) and int(hist.sum()) == t.size()
    assert kb.stat_text(hist) == want_stat
    path = tmp_path / "m.kmers.bin"
    path.write_bytes(data.tobytes())
    assert ho.read_kmers_bin(str(path)) == want_recs
    dk, dc = kb.decode(data, -1)
    assert sorted(zip(dk.tolist(), dc.tolist())) == want_recs
    dk, dc = kb.decode(data, 5)
    assert sorted(zip(dk.tolist(), dc.tolist())) == [r for r in want_recs if r[1] > 5]
    sk, sc = kb.sorted_records(data)
    assert list(zip(sk.tolist(), sc.tolist())) == want_recs


def test_hand_written_records():
    data, hist = kb.encode([0x0102030405060708], [0x090A], 0)
    assert data.tobytes() == bytes(range(1, 11))
    assert hist[0x090A] == 1 and hist.sum() == 1
    # a negative key, and the order of the input is the order of the records
    data, _ = kb.encode([-2, 5], [7, 1], 0)
    assert data.tobytes() == b"\xff" * 7 + b"\xfe\x00\x07" + b"\x00" * 7 + b"\x05\x00\x01"
    assert data.tobytes() == struct.pack(">qhqh", -2, 7, 5, 1)
    k, c = kb.decode(data, 0)
    assert k.tolist() == [-2, 5] and c.tolist() == [7, 1] and k.dtype == np.int64 and c.dtype == np.int16
    # the threshold: strictly above, and everything counts in the histogram
    data, hist = kb.encode([1, 2, 3], [1, 2, 32767], 1)
    assert kb.decode(data, -1)[0].tolist() == [2, 3] and hist[1] == hist[2] == hist[32767] == 1
    assert len(kb.encode([1, 2, 3], [1, 2, 32767], 32767)[0]) == 0
    # count bytes 80 00 are -32768: the compare is signed
    raw = bytes(range(1, 9)) + b"\x80\x00" + bytes(8) + b"\x00\x01"
    assert kb.decode(raw, 0)[1].tolist() == [1]
    k, c = kb.decode(raw, -32769)
    assert c.tolist() == [-32768, 1] and k.tolist() == [0x0102030405060708, 0]
    assert kb.decode(raw, -32768)[1].tolist() == [1]
    assert kb.decode(b"", 0)[0].size == 0
    with pytest.raises(AssertionError):
        kb.decode(b"123456789012345", 0)
