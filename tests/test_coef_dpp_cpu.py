"""The six-way split kernels with the projection's coefficients resident in the lanes of the DPP rows (eval_body, COEF_DPP), from
the gfx950 code of the built libvb2.so (no GPU):
  * all nine split kernels (llk_eval_split6_kernel<KSEL>, llk_eval_split_kernel<KSEL, 2 | 3>) within what tests/test_addr_scalar_cpu.py
    holds them to -- at most 128 VGPRs, no scratch memory, no scalar register spilled to a vector lane --, read from the code object's
    notes;
  * the item loops of llk_eval_split6_kernel<4> and <2> through tools/item_census.py: no projection coefficient is read from LDS --
    164 -> 156 and 160 -> 156 ds_read_b128 (the walk's twelve reads a row, in every copy of the row body, are what is left) -- and
    the projection is 2 x 16 and 2 x 8 v_fmac_f64_dpp: every FMA twice, under complementary bank masks;
  * llk_eval_split6_kernel<0> and the three-way kernel of --NumPC 4 keep the old text: no v_fmac_f64_dpp, the parent's reads."""
import os

import pytest

import test_addr_scalar_cpu as notes_of
import test_kernel_resources_cpu as res


def need_tools():
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")


def test_nine_split_kernels_fit_128_vgprs_without_scratch_or_scalar_spills():
    need_tools()
    notes = notes_of.split_kernel_notes(res.LIB)
    for k, v in sorted(notes.items()):
        print("%4d VGPRs %5d B scratch %3d SGPRs spilled %3d VGPRs spilled  %s"
              % (v["vgpr_count"], v["private_segment_fixed_size"], v["sgpr_spill_count"], v["vgpr_spill_count"], k))
    assert len(notes) == 9, sorted(notes)                    # KSEL 4, 2, 0 x sets of six, two and three workgroups
    over = {k: v for k, v in notes.items()
            if v["vgpr_count"] > res.VGPR_LIMIT or v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0 or v["sgpr_spill_count"] != 0}
    assert not over, over


# kernel -> (ds_read_b128, v_fmac_f64_dpp) in its item loop
CENSUS = {
    "llk_eval_split6_kernel<4>": (156, 32),
    "llk_eval_split6_kernel<2>": (156, 16),
    "llk_eval_split6_kernel<0>": (166, 0),
    "llk_eval_split_kernel<4, 3>": (164, 0),
}


@pytest.mark.parametrize("kernel", sorted(CENSUS))
def test_item_loop_reads_and_dpp_fmas(kernel):
    need_tools()
    import item_census
    name, code, (lo, hi), counts = item_census.census(res.LIB, kernel)
    print("%s: item loop %d..%d, ds_read_b128 %d, v_fmac_f64_dpp %d, other FP64 %d, v_mul_f64 in the walk %d"
          % (name.split("(")[0], lo, hi, counts["ds_read_b128"], counts["v_fmac_f64_dpp"], counts["other FP64"], counts["v_mul_f64 in the walk"]))
    assert (counts["ds_read_b128"], counts["v_fmac_f64_dpp"]) == CENSUS[kernel]
    assert counts["v_mul_f64 in the walk"] == 276            # (the walk: untouched)
