"""The nine split kernels (llk_eval_split6_kernel<KSEL>, llk_eval_split_kernel<KSEL, 2 | 3>) with the item loop's uniform address
arithmetic on the scalar unit (eval_body, ADDR_SCALAR: the per-marker constants and the list words through buffer descriptors, the
tile record decoded and the queue drawn by scalar instructions) against their budget, from the code-object notes of the built
libvb2.so (no GPU): at most 128 VGPRs, no scratch memory and no spilled scalar register.  Nine descriptors kept across the item loop
would be 36 scalar registers: the base of a column goes through an opaque scalar pair per load, so ONE descriptor's registers serve
all nine.

The six kernels of --NumPC 4 and 2 spilled none before the change and spill none.  The three KSEL 0 kernels (--NumPC other than 2
and 4, or known allele frequencies: the number of components and the known-AF pointer are run-time values in scalar registers)
spilled 14 / 28 / 31 scalar registers to vector lanes BEFORE the change and 28 / 30 / 28 with ADDR_SCALAR alone.  They spill none
since (eval_body, kItemScalars) what an item derives from those run-time values is computed where it is used, not kept across the
item loop as masks and bases (0 / 7 / 10), and the kernel arguments that only the hand-off behind the item loop needs are read
again from the kernel-argument segment there (0 / 0 / 0)."""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_resources_cpu as res

FIELDS = ("vgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


def split_kernel_notes(lib):
    """{kernel name: {field: int}} of the split kernels, from the amdhsa.kernels notes of every code object of the library"""
    import isa_diff
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in isa_diff.code_object(lib, tmp):
            txt = subprocess.run([isa_diff.LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            entries, inside = [], False
            for line in txt.splitlines():
                if line.startswith("amdhsa."):
                    inside = line.startswith("amdhsa.kernels:")
                    continue
                m = re.match(r"^  ([- ]) \.(\w+):\s*(.*)$", line) if inside else None
                if not m:
                    continue
                if m.group(1) == "-":
                    entries.append({})
                entries[-1][m.group(2)] = m.group(3).strip().strip("'\"")
            names = [e["name"] for e in entries]
            if not names:
                continue
            dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
            for d, e in zip(dem, entries):
                if re.search(r"\bvb2::llk_eval_split6?_kernel<", d):
                    assert d.split("(")[0] not in out, d                  # (one translation unit compiles them)
                    out[d.split("(")[0]] = {f: int(e[f]) for f in FIELDS}
    return out


def test_split_kernels_fit_128_vgprs_without_scratch_or_scalar_spills():
    import isa_diff
    if not os.path.exists(res.LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = split_kernel_notes(res.LIB)
    for k, v in sorted(notes.items()):
        print("%4d VGPRs %5d B scratch %3d SGPRs spilled %3d VGPRs spilled  %s"
              % (v["vgpr_count"], v["private_segment_fixed_size"], v["sgpr_spill_count"], v["vgpr_spill_count"], k))
    assert len(notes) == 9, sorted(notes)                    # KSEL 4, 2, 0 x sets of six, two and three workgroups
    over = {k: v for k, v in notes.items()
            if v["vgpr_count"] > res.VGPR_LIMIT or v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0 or v["sgpr_spill_count"] != 0}
    assert not over, over
