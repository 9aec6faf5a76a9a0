"""`mc_hosttest unitigs`: the host's link analysis (csrc/host/picture.cpp unitigs_by_links) and make_picture with it leave, node
for node, what the loop on labels leaves, and both say what tests/unitigs_model.py says (no GPU)."""
import subprocess

import pytest

import unitigs_model as um

HAND = um.hand_cases()
RANDOM = {"random_k5": (5,) + um.random_set(21, 5, 200), "random_k4": (4,) + um.random_set(22, 4, 50), "random_k21": (21,) + um.random_set(23, 21, 500),
          "mixed_k21": (21,) + um.mixed_set(24, 21), "mixed_k32": (32,) + um.mixed_set(25, 32), "mixed_k33": (33,) + um.mixed_set(26, 33),
          "mixed_k63": (63,) + um.mixed_set(27, 63), "mixed_k4": (4,) + um.mixed_set(28, 4, (1, 2, 3))}


@pytest.fixture(scope="module")
def hosttest():
    from metacherchant_amd import build
    build.build_host()
    return build.HOSTTEST


def run(hosttest, tmp_path, k, kmers, cls):
    path = tmp_path / "kmers.txt"
    path.write_text(um.hosttest_input(k, kmers, cls))
    out = subprocess.run([hosttest, "unitigs", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    rows = {c: [l.split()[1:] for l in out if l.startswith(c + " ")] for c in "UION"}
    assert sum(len(v) for v in rows.values()) == len(out)
    return rows


def model_rows(nodes):
    return [[str(i), "1" if d else "0", "-" if d else str(r), "-" if d else s, "[%s]" % ",".join(map(str, nb))]
            for i, (d, r, s, nb) in enumerate(um.state(nodes))]


def check(hosttest, tmp_path, k, kmers, cls):
    rows = run(hosttest, tmp_path, k, kmers, cls)
    assert rows["O"] == rows["N"]
    assert rows["O"] == model_rows(um.reference_loop(kmers, cls, k))
    res = um.link_analysis(kmers, cls, k)
    assert [int(r[0]) for r in rows["I"]] == res["irregular"]
    assert [(int(a), int(b)) for a, b, _ in rows["U"]] == list(zip(res["first"], res["last_rc"]))
    for (_, _, bases), s in zip(rows["U"], res["seqs"]):
        assert len(bases) == (len(s) + 31) // 32 * 32 and bases == s + "A" * (len(bases) - len(s))


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_shapes(hosttest, tmp_path, name):
    check(hosttest, tmp_path, *HAND[name])


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_and_mixed_sets(hosttest, tmp_path, name):
    check(hosttest, tmp_path, *RANDOM[name])


def test_two_entries_of_one_kmer_are_refused(hosttest, tmp_path):
    path = tmp_path / "kmers.txt"
    path.write_text(um.hosttest_input(5, ["ACGTA", "TACGT"], [0, 0]))
    p = subprocess.run([hosttest, "unitigs", str(path)], capture_output=True, text=True)
    assert p.returncode == 1 and "same k-mer" in p.stderr
