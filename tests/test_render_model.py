"""CPU: tests/render_model.py against the reads-classifier's model (tests/classifier_model.py outputs / fastq_bytes) on designed pair
lists, and the unnumbered form: numbered by the host afterwards it is the numbered form."""
import numpy as np
import pytest

from tests import classifier_model as cm
from tests import render_model as rm


def _read(n, salt=0, phred=None):
    codes = ((np.arange(n) * 5 + salt) // 3 % 4).astype(np.uint8)
    q = ((np.arange(n) * 11 + salt) % 63).astype(np.uint8) if phred is None else np.full(n, phred, np.uint8)
    return codes, q


# a read is "found" when its first phred is even: designed, so that every list gets pairs
def _found(r):
    return len(r[0]) > 0 and int(r[1][0]) % 2 == 0


def _pairs():
    lens = [1, 2, 3, 9, 10, 11, 99, 100, 101, 150, 5, 7]
    out = []
    for i, n in enumerate(lens * 3):
        a, b = _read(n, i, phred=(i % 4) + 2), _read(n + i % 3, i + 50, phred=(i // 2 % 4) + 2)
        out.append((a, b))
    out.append((_read(4, 1, phred=2), cm.EMPTY))  # first only, with an empty mate: nothing goes to not_found_s
    out.append((_read(4, 1, phred=3), cm.EMPTY))  # second only by the rule for an empty mate
    return out


@pytest.mark.parametrize("name", ["paired", "single_end", "twelve_of_a_kind"])
def test_the_model_gives_the_classifiers_files(name):
    if name == "paired":
        pairs = _pairs()
    elif name == "single_end":
        pairs = cm.single_end([_read(n, i, phred=i % 2 + 4) for i, n in enumerate([1, 5, 150, 33, 2, 64, 65, 9, 10, 11, 12, 13, 14])])
    else:  # more than nine records in a file: the numbers grow a digit
        pairs = [(_read(20, i, phred=2), _read(21, i, phred=5)) for i in range(12)] + [(_read(20, i, phred=3), _read(21, i, phred=4)) for i in range(12)]
    lists = cm.split(pairs, 0, None, verdicts=_found)
    want = cm.outputs(lists)
    got = rm.classifier_files(pairs, _found)
    assert got == want
    assert sum(len(v) for v in want.values()) > 0
    if name == "single_end":  # every not-found read goes through the unnumbered tail
        assert want["not_found_s.fastq"] and not want["not_found_1.fastq"]
        sides = rm.classifier_sides(pairs, _found)
        assert rm.NOT_FOUND_S_TAIL in sides[0][1] and rm.NOT_FOUND_S not in sides[0][1] + sides[1][1]


def test_a_record_is_what_fastq_bytes_writes():
    reads = [_read(n, n) for n in (1, 2, 31, 32, 33, 150)]
    assert b"".join(rm.record(c, q, i + 1) for i, (c, q) in enumerate(reads)) == cm.fastq_bytes(reads)
    for c, q in reads:
        assert len(rm.record(c, q, 12345)) == 2 * len(c) + 5 + 6 and len(rm.record(c, q, None)) == 2 * len(c) + 5


@pytest.mark.parametrize("first", [1, 8, 98, 998, 999999998, 4294967294, 10**18 - 2])
def test_unnumbered_then_numbered_by_the_host_is_the_numbered_form(first):
    reads = [_read(n, n) for n in (1, 2, 3, 17, 150, 4)]
    side = [(reads, [0] * len(reads))]
    numbered, err = rm.render(side, 1, [first])
    assert err is None
    bare, err = rm.render(side, 1, [rm.UNNUMBERED])
    assert err is None
    assert len(bare[0]) == sum(2 * len(c) + 5 for c, _ in reads)
    assert rm.number_bodies(rm.split_bodies(bare[0], [len(c) for c, _ in reads]), first) == numbered[0]


def test_errors_name_the_lowest_item():
    good, empty = _read(5, 1), cm.EMPTY
    bad = (good[0], np.array([1, 63, 2, 70, 3], np.uint8))
    # item order: read 0 side 0, read 0 side 1, read 1 side 0, ...
    sides = [([good, bad, good], [0, 0, 0]), ([good, good, empty], [1, rm.SKIP, 1])]
    assert rm.render(sides, 2, [1, 1]) == (None, (rm.QUALITY, 0, 1, 63))
    sides = [([good, good, bad], [0, 0, 0]), ([good, empty, good], [1, 1, 1])]
    assert rm.render(sides, 2, [1, 1]) == (None, (rm.EMPTY, 1, 1, 0))
    sides = [([good, empty, bad], [0, rm.SKIP, rm.SKIP]), ([good, good, good], [1, 1, 2])]
    assert rm.render(sides, 2, [1, 1]) == (None, (rm.STREAM, 1, 2, 2))  # (skipped reads are not looked at; the stream byte is)
    with pytest.raises(RuntimeError):
        cm.fastq_bytes([bad])
