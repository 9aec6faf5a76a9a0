"""CPU: tests/whole_reads_model.py held to the C++ reader it restates.  `mc_hosttest dnaq <file>` prints what DnaQReader delivers for the
inputs the GPU test gives mc_tokenize_whole; `mc_hosttest dnaq-range <file> <chunk>` reads the same file cut at record starts, each
piece through DnaQReader's record functions over a range of memory (what a chunk the device declined goes through).  Both again in
mc_hosttest_asan, the same program built with the address and undefined-behaviour sanitizers (a stand-alone binary)."""
import subprocess

import numpy as np
import pytest

from tests import whole_reads_model as wm

CASES = wm.cases()
ASAN_ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def hosttests():
    from metacherchant_amd import build
    build.build_host()
    return {"plain": build.HOSTTEST, "asan": build.build_host_sanitized("asan")}


@pytest.fixture(scope="module")
def models():
    return {name: wm.read_whole(text, fastq) for name, (text, fastq, _) in CASES.items()}


def parse(stdout):
    """mc_hosttest dnaq's lines -> (fastq, offset, codes, phred, offsets)"""
    lines = stdout.split("\n")
    assert lines.pop() == ""
    head = lines[0].split()
    assert head[0] == "fastq" and head[2] == "offset"
    codes, phred, lens = [], [], []
    for line in lines[1:]:
        tag, bases, quals = line.split("\t")
        n = int(tag.split()[1])
        assert tag.startswith("R ") and len(bases) == n and len(quals) == n
        codes.append(np.array(["AGCT".index(c) for c in bases], dtype=np.uint8))
        phred.append(np.frombuffer(quals.encode(), dtype=np.uint8) - 33)
        lens.append(n)
    z = np.zeros(0, dtype=np.uint8)
    return int(head[1]), int(head[3]), np.concatenate(codes + [z]), np.concatenate(phred + [z]), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def check(exe, env, args, path, m, fastq):
    import os
    p = subprocess.run([exe] + args[:1] + [path] + args[1:], capture_output=True, text=True, env=dict(os.environ, **env))
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    if m.error is not None:
        assert p.returncode == 1 and p.stderr == "error: %s\n" % m.error, (p.returncode, p.stderr[-2000:])
        if not p.stdout:  # (the constructor threw: the model has no reads either)
            assert m.n_reads == 0
            return
    else:
        assert p.returncode == 0, p.stderr[-2000:]
    got_fastq, offset, codes, phred, offsets = parse(p.stdout)
    assert got_fastq == (1 if fastq else 0) and offset == m.offset
    assert np.array_equal(offsets, m.offsets)
    assert np.array_equal(codes, m.codes)
    assert np.array_equal(phred, m.phred)


@pytest.mark.parametrize("which", ["plain", "asan"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_is_the_cpp_reader(hosttests, models, tmp_path, name, which):
    text, fastq, _ = CASES[name]
    path = str(tmp_path / ("reads.fastq" if fastq else "reads.fasta"))
    with open(path, "wb") as f:
        f.write(text)
    env = ASAN_ENV if which == "asan" else {}
    m = models[name]
    check(hosttests[which], env, ["dnaq"], path, m, fastq)
    # the same reads from the pieces of the file (a FASTQ whose first records the counting path's reader cannot take is not mapped)
    if m.error is None and not name.startswith("declined_"):
        for chunk in (64, 700, 5000):
            check(hosttests[which], env, ["dnaq-range", str(chunk)], path, m, fastq)


def test_the_cases_decline_where_they_say(models):
    """a case marked declined is one whose outcome the host reader defines: an error, or a laxer reading of a shape the device refuses"""
    for name, (text, fastq, declined) in CASES.items():
        m = models[name]
        if not declined:
            assert m.error is None, (name, m.error)
    assert models["declined_R"].error.startswith("read contains the character 'R'")
    assert models["declined_fasta_R"].error.startswith("read contains the character 'R'")
    assert models["declined_quality"].error == 'Invalid quality code char: " " char code = 32'
    assert models["declined_lengths"].error == "Bad DnaQ record: length of chars and quality is not the same."
    assert models["declined_three_lines"].error == "Unexpected end of file. File is corrupted/Format mismatch."
    for lax in ("declined_blank_line", "declined_plus_first"):
        assert models[lax].error is None and models[lax].n_reads == 6


def test_the_model_on_reads_written_out_by_hand():
    m = wm.read_whole(b"@a\nACGTN\n+\nIIII!\n@b\n\n+\n\n@c\nacgt.\n+a\n5+*~5\n", True)
    assert m.offset == 33 and m.error is None
    assert m.codes.tolist() == [0, 2, 1, 3, 0] + [0, 2, 1, 3, 0] and m.offsets.tolist() == [0, 5, 5, 10]
    assert m.phred.tolist() == [40, 40, 40, 40, 0] + [20, 10, 9, 93 & 63, 0]
    assert m.bad_pos.tolist() == [4, -1, -2]
    assert m.words()[0] == int("".join(format(c, "02b") for c in m.codes).ljust(64, "0"), 2)
    m = wm.read_whole(b"ACG\n>h\nAC\n\nGN\n>e\n;f\nnn\r\n", False)
    assert m.offset == 0 and m.codes.tolist() == [0, 2, 1, 0, 2, 1, 0, 0, 0] and m.offsets.tolist() == [0, 3, 7, 9]
    assert m.phred.tolist() == [20, 20, 20, 20, 20, 20, 0, 0, 0] and m.bad_pos.tolist() == [-1, 3, -2]
    assert wm.read_whole(b"@a\nAC\n+\nhh\n", True).offset == 64
    assert wm.read_whole(b"@a\nNC\n+\n!h\n", True).offset == 64  # (an unknown base's quality char is not looked at)
