"""GPU: `metacherchant --tool fmt-visualizer --replay host|gpu|auto`.  The walk's order comes from the host's replay of the reference's
queue or from mc_walk_order; the files are the same bytes, and tests/components_model.py's.  A donor graph with 40 equal-arm bubbles
in a row is what the host's queue cannot finish (2^40 copies of the last stretch): `gpu` and `auto` write the files that the model
writes when its walk is tests/walk_order_model.py's bounded one, and `auto` says in the log that it gave the component up."""
import os
import subprocess

import numpy as np
import pytest

from oracle.host_oracle import normalize_dna
from tests import components_model as cm
from tests import walk_order_model as wm
from tests import walk_order_shapes as ws
from tests.recipient_model import all_neighbors
from tests.test_gpu_cli_fmt_visualizer import _phase_inputs
from tests.test_gpu_cli_recipient import _write_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from metacherchant_amd import build
    build.build_all()
    return build.CLI


class BoundedKmerEnv(cm.KmerEnv):
    """KmerEnvCalculator with the bounded walk in place of its queue: the same puts wherever the queue ends"""

    def run_bfs(self):
        seen, members, stack = {normalize_dna(self.sequence)}, [self.sequence], [self.sequence]
        while stack:
            for nb in all_neighbors(stack.pop()):
                if normalize_dna(nb) not in seen and self.graph.get(self._key(nb), -1) > 0:
                    seen.add(normalize_dna(nb))
                    members.append(nb)
                    stack.append(nb)
        order, twice, stats = wm.bounded_walk(members)
        assert len(order) == len(members)
        for m in order:
            key = self._key(members[m])
            self.subgraph.put(normalize_dna(members[m]), 0 if twice[m] else self.graph[key])
            self.members[normalize_dna(members[m])] = self.graph[key]
        for m in members:
            self.graph[self._key(m)] = 0
        self.pops = stats["queue"]
        return True


def _run(cli, tmp_path, tag, k, inputs, ext, replay):
    """writes the inputs (once a tag), runs the tool, returns ({file under the output directory: bytes}, the log)"""
    base = tmp_path / tag
    in_dir, out, wd = str(base / "in"), str(base / ("out_" + replay)), str(base / ("wd_" + replay))
    paths = {name: [str(base / ("%s_a.fasta" % name)), str(base / ("%s_b.fastq" % name))] for name, _ in cm.PHASES}
    if not os.path.exists(in_dir):
        os.makedirs(in_dir)
        for name, classes in cm.PHASES:
            reads, class_reads = inputs[name]
            _write_reads(paths[name][0], reads[:(len(reads) + 1) // 2])
            _write_reads(paths[name][1], reads[(len(reads) + 1) // 2:])
            for c in classes:
                for i, m in enumerate("12s"):
                    _write_reads(os.path.join(in_dir, "%s_%s.%s" % (c, m, ext)), class_reads[c][i::3])
    cmd = [cli, "--tool", "fmt-visualizer", "-k", str(k), "-donor"] + paths["donor"] + ["-before"] + paths["before"] + ["-after"] + paths["after"] + [
        "-i", in_dir, "-ext", ext, "-o", out, "-w", wd, "--force", "-p", "4", "--replay", replay]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    got = {}
    for root, _, names in os.walk(out):
        for n in names:
            got[os.path.relpath(os.path.join(root, n), out)] = open(os.path.join(root, n), "rb").read()
    return got, open(os.path.join(wd, "log")).read()


def _same(got, want):
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        if got[name] != want[name]:
            g, w = got[name].decode().split("\n"), want[name].decode().split("\n")
            bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
            raise AssertionError((name, len(g), len(w), bad[:3], g[bad[0]][:300] if bad else None, w[bad[0]][:300] if bad else None))


@pytest.mark.parametrize("k,mode,ext", [(21, 0, "fasta"), (41, 1, "fastq")])
def test_replay_gpu_and_host_write_the_models_files(cli, tmp_path, k, mode, ext):
    rng = np.random.default_rng(100 + k)
    inputs = {name: _phase_inputs(rng, k, classes) for name, classes in cm.PHASES}
    want, comps = cm.fmt_visualizer(k, mode, inputs)
    assert any("\tKC:i:0\t" in text.decode() for text in want.values())  # a k-mer popped twice is among them
    n_comp = {name: len(comps[name]) for name in comps}
    host, host_log = _run(cli, tmp_path, "t", k, inputs, ext, "host")
    gpu, gpu_log = _run(cli, tmp_path, "t", k, inputs, ext, "gpu")
    _same(host, want)
    _same(gpu, want)
    for name, _ in cm.PHASES:
        assert "Replayed the walks of %d components on the host, 0 on the GPU" % n_comp[name] in host_log
        assert "Replayed the walks of 0 components on the host, %d on the GPU (mc_walk_order)" % n_comp[name] in gpu_log


def test_forty_bubbles_in_the_donor_graph(cli, tmp_path, monkeypatch):
    k, mode = 21, 0
    rng = np.random.default_rng(4040)
    genome_reads = ws.bubble_reads(rng, k, 40)  # the genome and its copy with the 40 substitutions
    members = ws.members_of(genome_reads, k)
    assert 1000 < len(members) < 5000
    inputs = {name: _phase_inputs(rng, k, classes) for name, classes in cm.PHASES}
    donor_reads, donor_classes = inputs["donor"]
    inputs["donor"] = (genome_reads + donor_reads, {"settle": donor_classes["settle"] + [genome_reads[0]], "not_settle": donor_classes["not_settle"] + [genome_reads[1]]})
    assert wm.exact_replay(members, cap=64 * len(members) + 4096) is None
    monkeypatch.setattr(cm, "KmerEnv", BoundedKmerEnv)
    want, comps = cm.fmt_visualizer(k, mode, inputs)
    assert len(comps["donor"][0][2]) == len(members)
    gpu, gpu_log = _run(cli, tmp_path, "b", k, inputs, "fasta", "gpu")
    _same(gpu, want)
    auto, auto_log = _run(cli, tmp_path, "b", k, inputs, "fasta", "auto")
    _same(auto, want)
    n_donor = len(comps["donor"])
    assert "Replayed the walks of %d components on the host, 1 on the GPU (mc_walk_order); the host's queue passed its cap on comp0" % (n_donor - 1) in auto_log
    assert "Replayed the walks of %d components on the host, 0 on the GPU" % len(comps["before"]) in auto_log


def test_replay_refusals(cli, tmp_path):
    def run(args):
        p = subprocess.run([cli, "-w", str(tmp_path / "wd"), "--force"] + args, capture_output=True, text=True, timeout=300)
        return p.returncode, p.stderr + p.stdout
    rc, text = run(["--tool", "fmt-visualizer", "-k", "21", "--replay", "device"])
    assert rc == 1 and "--replay takes host, gpu or auto, not 'device'" in text
    for tool in ("environment-finder", "kmer-counter", "recipient-visualiser", "reads-classifier", "seq-cov"):
        rc, text = run(["--tool", tool, "-k", "21", "--replay", "gpu"])
        assert rc == 1 and "Unrecognized option: --replay" in text, (tool, text)
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=120)
    assert "--replay host|gpu|auto" in p.stdout
