"""The presence kernels, read from the code objects inside libmcgpu.so (no GPU needed): one for every key mode and number of tables,
each in one code object only, no scratch memory, no spills of vector or scalar registers, no LDS.

Occupancy: the kernel is bound by the latency of random 16-byte slot reads (a lane has as many in flight as there are tables), so
it is meant to keep all eight waves of a SIMD: 64 vector registers at most (512 / 8)."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"


def test_the_presence_kernels_use_no_scratch_and_no_spills(tmp_path):
    from metacherchant_amd import build
    lib = build.build_lib()
    if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("ROCm's llvm tools are not here")
    kernels = {}
    for co in build.code_objects(lib, str(tmp_path)):
        text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
        for block in text.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            assert name not in kernels, "%s is in two code objects" % name
            kernels[name] = {k: int(v) for k, v in re.findall(
                r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block)}
    ours = {n: r for n, r in kernels.items() if "k_presence" in n}
    for mode in range(3):
        for nt in range(1, 5):
            hit = [n for n in ours if "k_presenceILi%dELi%dE" % (mode, nt) in n]
            assert len(hit) == 1, (mode, nt, sorted(ours))
            r = ours[hit[0]]
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hit[0], r)
            assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] == 0, (hit[0], r)
    assert len(ours) == 12, sorted(ours)
