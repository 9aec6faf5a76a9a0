"""The reads-in-set kernels, read from the code objects inside libmcgpu.so (no GPU needed): the counting kernel for one- and
two-word k-mers, with and without the bit filter, and the set's build for both widths, each in one code object only, no scratch
memory, no spills of vector or scalar registers.

LDS: the filtered counting kernels hold the whole filter, 2^14 words of 64 bits = 131072 bytes of a CU's 160 KB (one workgroup of
1024 threads a CU); the others hold nothing.  1024 threads a workgroup leave a thread 128 vector registers."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
FILTER_BYTES = (1 << 14) * 8


def test_the_reads_in_set_kernels_use_no_scratch_and_no_spills(tmp_path):
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
    ours = {n: r for n, r in kernels.items() if "k_rs_" in n}
    want_lds = {}
    for wide in (0, 1):
        for filt in (0, 1):
            want_lds["k_rs_countILb%dELb%dEE" % (wide, filt)] = FILTER_BYTES if filt else 0
        want_lds["k_rs_buildILb%dEE" % wide] = 0
    want_lds["k_rs_keepE"] = 0
    for tag, lds in want_lds.items():
        hit = [n for n in ours if tag in n]
        assert len(hit) == 1, (tag, sorted(ours))
        r = ours[hit[0]]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (hit[0], r)
        assert r["group_segment_fixed_size"] == lds, (hit[0], r)
        assert r["vgpr_count"] <= 128, (hit[0], r)
    assert len(ours) == len(want_lds), sorted(ours)
