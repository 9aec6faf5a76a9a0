"""CPU: what --render adds to the host's writers (csrc/host/fastq_out.h) -- FastqOut::put_rendered, the body form of SideList and
render_ranges -- through `mc_hosttest render-host <dir>`, against tests/render_model.py; again in mc_hosttest_asan, the same program
built with the address and undefined-behaviour sanitizers (a stand-alone binary)."""
import os
import subprocess

import numpy as np
import pytest

from tests import render_model as rm

ASAN_ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def hosttests():
    from metacherchant_amd import build
    build.build_host()
    return {"plain": build.HOSTTEST, "asan": build.build_host_sanitized("asan")}


def _read(i):
    n = i % 7 + 1
    j = np.arange(n)
    return ((i + j) % 4).astype(np.uint8), ((3 * i + 5 * j) % 63).astype(np.uint8)


def _ranges(covers, n):
    """the cuts at the union of the sides' segment boundaries, with every side's segment: written from the definition"""
    cuts = sorted({0, n} | {min(x, n) for cover in covers for first, m in cover for x in (first, first + m)})
    out = []
    for a, b in zip(cuts, cuts[1:]):
        out.append((a, b) + tuple(next(i for i, (first, m) in enumerate(cover) if first <= a and b <= first + m) for cover in covers))
    return out


@pytest.mark.parametrize("which", ["plain", "asan"])
def test_put_rendered_bodies_and_ranges(hosttests, tmp_path, which):
    env = dict(os.environ, **(ASAN_ENV if which == "asan" else {}))
    p = subprocess.run([hosttests[which], "render-host", str(tmp_path)], capture_output=True, text=True, env=env)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    assert lines.pop() == ""
    assert lines[0] == "a 12 b 10"
    one = lambda reads: rm.render([(reads, [0] * len(reads))], 1, [1])[0][0]  # noqa: E731
    assert (tmp_path / "a.fastq").read_bytes() == one([_read(i) for i in range(12)])
    assert (tmp_path / "b.fastq").read_bytes() == one([_read(i) for i in (8, 9, 0, 1, 2, 3, 4, 5, 6, 7)])
    two = [[(0, 5), (5, 0), (5, 7), (12, 30)], [(0, 3), (3, 3), (6, 20), (26, 10)]]
    single = [[(0, 4), (4, 4), (8, 1)]]
    want = ["R %d %d %d %d" % r for r in _ranges(two, 30)] + ["R %d %d %d 0" % r for r in _ranges(single, 9)] + ["R none 0"]
    assert len(_ranges(two, 30)) == 6
    assert lines[1:1 + len(want)] == want
    assert lines[1 + len(want):] == ["E internal: a batch's device view does not cover it", "E internal: the rendered bodies do not have their reads' lengths"]
