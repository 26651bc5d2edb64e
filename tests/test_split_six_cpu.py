"""The six-way split kernels (llk_eval_split6_kernel<KSEL>, eval_body SPLIT == kMaxGroups) against the budget
tests/test_kernel_resources_cpu.py holds the other evaluation kernels to, from the code-object notes of the built libvb2.so (no
GPU): at most 128 VGPRs and no scratch memory.  With exactly one point group per workgroup the coefficient reads' address no
longer depends on the item -- hoisted out of the item loop, the sixteen doubles would spill; and the per-virtual-block tile
counts as an indexed array of six went to scratch memory before they became two scalars."""
import os
import re

import pytest

import test_kernel_resources_cpu as res


def test_six_way_split_kernels_fit_128_vgprs_without_scratch():
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = res.all_kernel_notes(res.LIB)
    six = {k: v for k, v in notes.items() if re.search(r"\bvb2::llk_eval_split6_kernel<", k[1])}
    for k, v in sorted(six.items()):
        print("%4d VGPRs %5d B scratch  %s  [%s]" % (v["vgpr_count"], v["private_segment_fixed_size"], k[1].split("(")[0], k[0]))
    assert len({k[1] for k in six}) == 3, six                       # KSEL 4, 2, 0
    over = {k[1].split("(")[0]: v for k, v in six.items() if v["vgpr_count"] > res.VGPR_LIMIT or v["private_segment_fixed_size"] != 0}
    assert not over, over
