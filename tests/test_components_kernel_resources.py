"""The components kernels, read from the code objects inside libmcgpu.so (no GPU needed): every one in one code object only, no
scratch memory, no spills of vector or scalar registers, in all three key modes and for both widths of the parents.  (The register
counts are in DESIGN.md "components"; no number is pinned here: the passes are bound by random reads of the table and of
parent[], and nobody has measured what occupancy they need.)"""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
INDEX = ("j", "y")  # the mangled unsigned int and unsigned long long


def test_the_components_kernels_use_no_scratch_and_no_spills(tmp_path):
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
    ours = {n: r for n, r in kernels.items() if "k_cc_" in n}
    want = ["k_cc_firstILi%dEE" % mode for mode in range(3)]
    want += ["k_cc_unionILi%dE%sE" % (mode, i) for mode in range(3) for i in INDEX]
    want += ["k_cc_%sI%sE" % (name, i) for name in ("init", "flatten", "members", "rootmin", "roots", "hist", "scatter") for i in INDEX]
    want += ["k_cc_numberE"]
    for w in want:
        hit = [n for n in ours if w in n]
        assert len(hit) == 1, (w, sorted(ours))
        r = ours[hit[0]]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hit[0], r)
        print(hit[0], r)
    assert len(ours) == len(want), sorted(ours)
