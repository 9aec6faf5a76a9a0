"""The triple-reads-classifier's kernels, read from the code objects inside libmcgpu.so (no GPU needed): no scratch memory, no
spills, and every kernel in one code object only -- hipCUB's sort and selection included, which the last-copy unit instantiates."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"


def test_the_triple_classifier_kernels_use_no_scratch_and_no_spills(tmp_path):
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
            kernels[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block)}
    ours = {n: r for n, r in kernels.items() if "k_lc_fingerprint" in n or "k_lc_resolve" in n or "k_triple_classes" in n}
    assert len(ours) == 3, sorted(ours)
    for name, r in ours.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)  # (8 waves a SIMD: the kernels are bound by memory latency)
    cub = {n: r for n, r in kernels.items() if "rocprim" in n}
    assert cub, "hipCUB's kernels are missing"
    for name, r in cub.items():  # (rocPRIM's onesweep pass keeps an 80-byte private array on gfx950; nothing spills)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] <= 128, (name, r)
