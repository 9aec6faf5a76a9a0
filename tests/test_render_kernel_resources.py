"""The FASTQ rendering kernels (csrc/render_fastq.hip), read from the code objects inside libmcgpu.so (no GPU needed): every one in
one code object only, no scratch memory, no spills of vector or scalar registers, and LDS within the 160 KB of a CU (the measuring
pass keeps a count and a 64-bit sum per wave and stream, under 1 KB; the emitter none)."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LDS_BYTES = 160 * 1024


def test_the_render_kernels_use_no_scratch_and_no_spills(tmp_path):
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
    ours = {n: r for n, r in kernels.items() if "k_rf_" in n}
    want = ["k_rf_%sE" % name for name in ("count", "measure", "scan64", "bounds", "emit")]
    for w in want:
        hit = [n for n in ours if w in n]
        assert len(hit) == 1, (w, sorted(ours))
        r = ours[hit[0]]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hit[0], r)
        assert r["group_segment_fixed_size"] <= LDS_BYTES, (hit[0], r)
        print(hit[0], r)
    assert len(ours) == len(want), sorted(ours)
