"""The whole-read tokeniser's kernels (csrc/whole_reads.hip), read from the code objects inside libmcgpu.so (no GPU needed): every one in
one code object only, no scratch memory, no spills of vector or scalar registers; the two packing kernels hold a WavePacker a wave in LDS
(65 words for each of a workgroup's four waves) and the others none.  The kernels shared with the counting tokeniser -- the newline
passes and the scans -- stay in reads_file.hip's code object alone.  (The register counts are in DESIGN.md 3.14; no number is pinned.)"""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
PACKING = ("k_wq_emit", "k_wa_pack")
OTHERS = ("k_wq_records", "k_wa_lines", "k_wa_records", "k_wa_rec_keep", "k_wa_lowpos", "k_wa_reads", "k_wr_append_words", "k_wr_append_offsets")
SHARED = ("k_nl_count", "k_nl_write", "k_scan_sums", "k_scan_one", "k_scan_apply")


def test_the_whole_read_kernels_use_no_scratch_and_no_spills(tmp_path):
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm's llvm tools are not here")
    from metacherchant_amd import build
    lib = build.build_lib()
    kernels = {}
    for co in build.code_objects(lib, str(tmp_path)):
        text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
        for block in text.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            assert name not in kernels, "%s is in two code objects" % name
            kernels[name] = {k: int(v) for k, v in re.findall(
                r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block)}
    ours = {n: r for n, r in kernels.items() if re.search(r"k_w[qar]_", n)}
    for w in PACKING + OTHERS:
        hit = [n for n in ours if re.search(r"\d%sE" % w, n)]
        assert len(hit) == 1, (w, sorted(ours))
        r = ours[hit[0]]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hit[0], r)
        assert r["group_segment_fixed_size"] == (4 * 65 * 8 if w in PACKING else 0), (hit[0], r)
        print(hit[0], r)
    assert len(ours) == len(PACKING + OTHERS), sorted(ours)
    for w in SHARED:
        assert len([n for n in kernels if re.search(r"\d%sE" % w, n)]) == 1, w
