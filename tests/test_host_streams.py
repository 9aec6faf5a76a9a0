"""CPU: which output stream the classifiers give each read of a pair (csrc/host/classifier_streams.h, the one rule behind --render
host and --render gpu) through `mc_hosttest streams`, for every input the rules have, against tests/render_model.py; again in
mc_hosttest_asan, the same program built with the address and undefined-behaviour sanitizers (a stand-alone binary)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import render_model as rm

ASAN_ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
LENGTHS = (0, 3)
BOTH, FIRST_ONLY, SECOND_ONLY, NEITHER = range(4)  # the PAIR_* counters


@pytest.fixture(scope="module")
def hosttests():
    from metacherchant_amd import build
    build.build_host()
    return {"plain": build.HOSTTEST, "asan": build.build_host_sanitized("asan")}


def _read(n):
    return np.zeros(n, np.uint8), np.full(n, 40, np.uint8)


def _counter(found1, found2, len2):
    """the list PairFinder.run (src/algo/PairFinder.java:32-57) adds the pair to"""
    if len2 == 0:
        found2 = not found1
    return BOTH if found1 and found2 else FIRST_ONLY if found1 else SECOND_ONLY if found2 else NEITHER


def _classifier_rows():
    rows = []
    for f1, f2, l1, l2 in itertools.product((0, 1), (0, 1), LENGTHS, LENGTHS):
        a, b = _read(l1), _read(l2)
        flags = {id(a): bool(f1), id(b): bool(f2)}
        (_, s1), (_, s2) = rm.classifier_sides([(a, b)], lambda r: flags[id(r)])
        rows.append("P %d %d %d %d %d %d %d" % (f1, f2, l1, l2, s1[0], s2[0], _counter(bool(f1), bool(f2), l2)))
    for f1, l1 in itertools.product((0, 1), LENGTHS):  # (a single-end read is paired with an empty one)
        a, b = _read(l1), _read(0)
        flags = {id(a): bool(f1), id(b): False}
        (_, s1), (_, s2) = rm.classifier_sides([(a, b)], lambda r: flags[id(r)])
        rows.append("S %d %d %d %d %d" % (f1, l1, s1[0], s2[0], _counter(bool(f1), False, 0)))
    return rows


def _triple_rows():
    rows = []
    for c1, c2, l1, l2 in itertools.product(range(3), range(3), LENGTHS, LENGTHS):
        (_, s1), (_, s2) = rm.triple_sides([(_read(l1), _read(l2))], [(c1, c2)])
        rows.append("T %d %d %d %d %d %d" % (c1, c2, l1, l2, s1[0], s2[0]))
    return rows


@pytest.mark.parametrize("which", ["plain", "asan"])
def test_every_case_of_both_rules(hosttests, which):
    env = dict(os.environ, **(ASAN_ENV if which == "asan" else {}))
    p = subprocess.run([hosttests[which], "streams"], capture_output=True, text=True, env=env)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    assert lines.pop() == ""
    classifier, triple = _classifier_rows(), _triple_rows()
    assert (len(classifier), len(triple)) == (16 + 4, 36)
    assert lines[:20] == classifier
    assert lines[20:] == triple
