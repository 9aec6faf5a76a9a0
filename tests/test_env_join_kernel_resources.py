"""The environment join's kernels, read from the code objects inside libmcgpu.so (no GPU needed): every one in one code object only,
no scratch memory, no spills of vector or scalar registers, for both widths of the k-mers; the pairs kernel's counters fit the 64 KB of
LDS a workgroup may have.  (The register counts are in DESIGN.md 3.13; no number is pinned here.)"""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"


def test_the_env_join_kernels_use_no_scratch_and_no_spills(tmp_path):
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
    ours = {n: r for n, r in kernels.items() if "k_ej_" in n}
    want = ["k_ej_%sILb%dEE" % (name, wide) for name in ("build", "records", "gene", "pairs") for wide in (0, 1)]  # (pairs: large / small G)
    for w in want:
        hit = [n for n in ours if w in n]
        assert len(hit) == 1, (w, sorted(ours))
        r = ours[hit[0]]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hit[0], r)
        if "k_ej_pairs" in w:
            assert 0 < r["group_segment_fixed_size"] <= 64 * 1024, (hit[0], r)
        else:
            assert r["group_segment_fixed_size"] == 0, (hit[0], r)
        print(hit[0], r)
    assert len(ours) == len(want), sorted(ours)
    assert not any("k_ut_" in n for n in ours)  # (tests/test_unitigs_kernel_resources.py counts those)
