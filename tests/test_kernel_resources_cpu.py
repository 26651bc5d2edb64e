"""The register and scratch budget of the evaluation kernels, read from the code-object metadata of the built libvb2.so (no
GPU): every llk_eval_split_kernel and llk_eval_kernel instantiation stays within 128 VGPRs -- a 1 024-thread workgroup has
no more per lane -- and uses no scratch memory: a read loop that spills pays a trip to memory per spilled value and step.
The notes only; no instruction is looked at.

Where it stands: the six split kernels take 112-116 VGPRs, the probability-domain llk_eval_kernel<2..4, *, *, true> 96-128, none
with scratch.  Two run-word kernels of the static deal, llk_eval_kernel<3, 0, 0, false> and <4, 0, 0, false>, used to carry 20 B: a
spill slot the register allocator left behind when it chose to reload a quad of kernel arguments instead -- no instruction
touched it, but every launch had scratch memory set up for it (eval_body: kOwnSizes)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "verifybamid_amd", "libvb2.so")
STAMPS_LIB = os.path.join(ROOT, "verifybamid_amd", "libvb2_stamps.so")

VGPR_LIMIT = 128


def kernel_notes(code_obj, readelf):
    """{demangled kernel name: {field: int}} from the amdhsa.kernels note of one code object"""
    txt = subprocess.run([readelf, "--notes", code_obj], capture_output=True, text=True, check=True).stdout
    entries, inside = [], False
    for line in txt.splitlines():
        if line.startswith("amdhsa."):
            inside = line.startswith("amdhsa.kernels:")
            continue
        m = re.match(r"^  ([- ]) \.(\w+):\s*(.*)$", line) if inside else None       # an entry's own fields, not its arguments'
        if not m:
            continue
        if m.group(1) == "-":
            entries.append({})
        entries[-1][m.group(2)] = m.group(3).strip().strip("'\"")
    out = {e["name"]: {f: int(e[f]) for f in ("vgpr_count", "private_segment_fixed_size")} for e in entries}
    if not out:
        return {}
    dem = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: v for d, v in zip(dem, out.values())}


def all_kernel_notes(lib):
    """{(code object, kernel name): notes}: a kernel that two translation units both compile is checked in each"""
    import isa_diff
    readelf = isa_diff.LLVM + "llvm-readelf"
    notes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in isa_diff.code_object(lib, tmp):
            for name, v in kernel_notes(co, readelf).items():
                notes[(os.path.basename(co), name)] = v
    return notes


def test_evaluation_kernels_fit_128_vgprs_without_scratch():
    import isa_diff
    if not os.path.exists(LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    notes = all_kernel_notes(LIB)
    mine = {k: v for k, v in notes.items() if re.search(r"\bvb2::llk_eval_(split_)?kernel<", k[1])}
    split = {k[1] for k in mine if "llk_eval_split_kernel<" in k[1]}
    plain = {k[1] for k in mine if "llk_eval_kernel<" in k[1]}
    for k, v in sorted(mine.items()):
        print("%4d VGPRs %5d B scratch  %s  [%s]" % (v["vgpr_count"], v["private_segment_fixed_size"], k[1].split("(")[0], k[0]))
    assert len(split) == 6, split                       # KSEL 4, 2, 0 x sets of two and of three workgroups
    assert len(plain) >= 12, plain
    over = {(k[0], k[1].split("(")[0]): v for k, v in mine.items() if v["vgpr_count"] > VGPR_LIMIT or v["private_segment_fixed_size"] != 0}
    assert not over, over


def test_each_evaluation_kernel_is_compiled_once_and_the_stamps_build_has_the_same_units():
    """Every vb2::llk_* kernel belongs to one translation unit -- the one with its launcher and its scheduler (csrc/Makefile) --
    so its name shows in one code object of libvb2.so only; and the profiling library libvb2_stamps.so is made of the same
    units: the same kernel names at the same code-object positions.  Names from the notes only."""
    import isa_diff
    if not os.path.exists(LIB):
        pytest.skip("libvb2.so is not built")
    if not all(os.path.exists(isa_diff.LLVM + t) for t in ("llvm-objdump", "llvm-readelf")):
        pytest.skip("the ROCm binutils are not installed")
    ship = set(all_kernel_notes(LIB))
    homes = {}
    for co, name in ship:
        if re.search(r"\bvb2::llk_", name):
            homes.setdefault(name, []).append(co)
    assert len(homes) >= 85, len(homes)                 # 12+ plain, 6 split, 6 pass-per-group, 72 cohort kernels, the resident ones
    twice = {n.split("(")[0]: sorted(c) for n, c in homes.items() if len(c) > 1}
    assert not twice, twice
    if not os.path.exists(STAMPS_LIB):
        return
    stamps = set(all_kernel_notes(STAMPS_LIB))
    assert stamps == ship, sorted((co, n.split("(")[0]) for co, n in stamps ^ ship)
