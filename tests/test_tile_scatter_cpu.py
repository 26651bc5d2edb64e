"""The split kernels with the tile butterfly as a reduce-scatter (eval_body, EPI_SCATTER), from the built libvb2.so, no GPU: the
nine of them -- three llk_eval_split6_kernel<KSEL>, six llk_eval_split_kernel<KSEL, S> -- stay within the budget
tests/test_kernel_resources_cpu.py holds the evaluation kernels to (at most 128 VGPRs, no scratch memory; from the code-object
notes, as tests/test_split_six_cpu.py reads them), and each one's code contains v_permlane16_swap, the move that puts point 0's
dword and point 1's side by side across the two 16-lane rows."""
import os
import re
import tempfile

import pytest

import test_kernel_resources_cpu as res

SPLIT = re.compile(r"\bvb2::llk_eval_split6?_kernel<")


def need_tools():
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    return isa_diff


def test_nine_split_kernels_fit_128_vgprs_without_scratch():
    need_tools()
    notes = res.all_kernel_notes(res.LIB)
    mine = {k: v for k, v in notes.items() if SPLIT.search(k[1])}
    for k, v in sorted(mine.items()):
        print("%4d VGPRs %5d B scratch  %s  [%s]" % (v["vgpr_count"], v["private_segment_fixed_size"], k[1].split("(")[0], k[0]))
    assert len({k[1] for k in mine}) == 9, sorted(k[1].split("(")[0] for k in mine)
    over = {k[1].split("(")[0]: v for k, v in mine.items() if v["vgpr_count"] > res.VGPR_LIMIT or v["private_segment_fixed_size"] != 0}
    assert not over, over


def test_nine_split_kernels_contain_the_row_swap():
    isa_diff = need_tools()
    with tempfile.TemporaryDirectory() as tmp:
        code = isa_diff.kernels(isa_diff.code_object(res.LIB, tmp), every=True)
    mine = {k: v for k, v in code.items() if SPLIT.search(k)}
    assert len(mine) == 9, sorted(k.split("(")[0] for k in mine)
    for k, v in sorted(mine.items()):
        n = sum(1 for ins in v if ins.startswith("v_permlane16_swap"))
        print("%3d v_permlane16_swap in %6d instructions  %s" % (n, len(v), k.split("(")[0]))
        assert n >= 1, k
