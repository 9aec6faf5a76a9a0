"""The walk-order kernels (csrc/walk_order.hip), read from the code objects inside libmcgpu.so (no GPU needed): every one in one code
object only, no scratch memory, no spills of vector or scalar registers, for both widths of the k-mers; LDS within what DESIGN.md
3.18 states: k_wo_narrow a third of a CU's 160 KB at the most (three workgroups a CU), the grid-wide kernels under 1 KB."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LDS_NARROW = 160 * 1024 // 3
LDS_WIDE = 1024


def test_the_walk_order_kernels_use_no_scratch_and_no_spills(tmp_path):
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
    ours = {n: r for n, r in kernels.items() if "k_wo_" in n}
    want = ["k_wo_%sILb%dEE" % (name, wide) for name in ("build", "adj") for wide in (0, 1)]
    want += ["k_wo_minILi%dEE" % p for p in (1, 2)]
    want += ["k_wo_%sE" % name for name in ("init", "narrow", "keep", "scatter", "twice")]
    for w in want:
        hit = [n for n in ours if w in n]
        assert len(hit) == 1, (w, sorted(ours))
        r = ours[hit[0]]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hit[0], r)
        assert r["group_segment_fixed_size"] <= (LDS_NARROW if "narrow" in w else LDS_WIDE), (hit[0], r)
        print(hit[0], r)
    assert len(ours) == len(want), sorted(ours)
    assert ours[[n for n in ours if "k_wo_narrow" in n][0]]["group_segment_fixed_size"] > 0
