"""Instruction census of a kernel's item loop from the gfx950 code of a built libvb2.so (no GPU needed).

    python tools/item_census.py LIB.so [kernel name substring, default 'llk_eval_split6_kernel<4>'] [--list]

The item loop is found in the disassembly, not assumed: the innermost span between a backward branch and its target that holds
both `s_setprio 1` (a wave enters its read loop) and `s_setprio 0` (it leaves it); blocks the compiler placed behind the loop --
the branch of the tiny likelihoods, the refills of a long list -- lie outside the span and are not counted.  Counts are STATIC:
an instruction of the walk's unrolled row body counts once however many rows a tile has.  Classes: v_mul_f64 between the two
s_setprio (the walk's multiplies), v_fmac_f64_dpp (the projection's FMAs whose coefficient is a lane of the DPP row: eval_body,
COEF_DPP), every other FP64 arithmetic instruction (v_*_f64 but compares), DPP moves (v_mov_b32_dpp),
v_permlane16_swap, ds_read_b128, other LDS instructions (ds_*), v_cndmask, v_lshl_add_u64 (a 64-bit address made per lane), other
vector ALU (v_*), vector memory by the form of its address -- a scalar base or a buffer descriptor with a 32-bit vector offset
(global_* with an SGPR pair, buffer_*) against a 64-bit vector address (global_* ... off, flat_*) --, s_nop, scalar and the rest
(s_*).  --list prints the span's instructions behind the table.
"""
import re
import subprocess
import sys
import tempfile

import isa_diff

CLASSES = ("v_mul_f64 in the walk", "v_fmac_f64_dpp", "other FP64", "DPP moves", "v_permlane16_swap", "ds_read_b128", "other LDS", "v_cndmask",
           "v_lshl_add_u64", "other VALU", "vector memory, scalar base", "vector memory, vector address", "s_nop", "scalar and the rest")


def disassemble(co):
    """{demangled name: [(address, instruction text)]}"""
    dis = subprocess.run([isa_diff.LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if cur is not None and m:
            cur.append((int(m.group(2), 16), m.group(1)))
    dem = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: out[k] for k, d in zip(out, dem)}


def item_loop(code):
    """(first, last) instruction index of the innermost backward-branch span with both s_setprio"""
    at = {a: i for i, (a, _) in enumerate(code)}
    up = [i for i, (_, t) in enumerate(code) if t.startswith("s_setprio 1")]
    down = [i for i, (_, t) in enumerate(code) if t.startswith("s_setprio 0")]
    best = None
    for i, (a, t) in enumerate(code):
        m = re.match(r"s_c?branch\w*\s+(\d+)", t)
        if not m:
            continue
        off = int(m.group(1))
        off -= 65536 if off >= 32768 else 0
        j = at.get(a + 4 + 4 * off)
        if j is None or j > i:
            continue
        if any(j <= u <= i for u in up) and any(j <= d <= i for d in down) and (best is None or i - j < best[1] - best[0]):
            best = (j, i)
    if best is None:
        raise SystemExit("no loop with both s_setprio found")
    return best


def classify(text, in_walk):
    op = text.split()[0]
    if op.startswith("v_permlane16_swap"):
        return "v_permlane16_swap"
    if op.startswith("v_fmac_f64_dpp"):      # (FP64 arithmetic with a DPP operand: neither a move nor "other FP64")
        return "v_fmac_f64_dpp"
    if "_dpp" in op or " row_" in text or " quad_perm" in text:
        return "DPP moves"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith("ds_read_b128"):
        return "ds_read_b128"
    if op.startswith("ds_"):
        return "other LDS"
    if re.match(r"v_\w+_f64", op) and not op.startswith("v_cmp"):
        return "v_mul_f64 in the walk" if in_walk and op.startswith("v_mul_f64") else "other FP64"
    if op.startswith("v_lshl_add_u64"):
        return "v_lshl_add_u64"
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        # (global_load v, v[a:b], off: the address is a 64-bit vector pair; global_load v, v, s[a:b] and buffer_*: a 32-bit offset)
        vector_address = op.startswith("flat_") or (op.startswith("global_") and re.search(r",\s*off\b", text) is not None)
        return "vector memory, vector address" if vector_address else "vector memory, scalar base"
    if op.startswith("s_nop"):
        return "s_nop"
    return "scalar and the rest"


def census(lib, want):
    """(kernel name, its code, (first, last) of the item loop, {class: count}) of the one kernel of lib whose name holds `want`"""
    with tempfile.TemporaryDirectory() as tmp:
        found = [(k, v) for co in isa_diff.code_object(lib, tmp) for k, v in disassemble(co).items() if want in k]
    if len(found) != 1:
        raise SystemExit("%d kernels match %r" % (len(found), want))
    name, code = found[0]
    lo, hi = item_loop(code)
    counts, walk = dict.fromkeys(CLASSES, 0), False
    for _, t in code[lo:hi + 1]:
        if t.startswith("s_setprio"):
            walk = t.startswith("s_setprio 1")
        counts[classify(t, walk)] += 1
    return name, code, (lo, hi), counts


def main():
    args = [a for a in sys.argv[1:] if a != "--list"]
    lib, want = args[0], (args[1] if len(args) > 1 else "llk_eval_split6_kernel<4>")
    name, code, (lo, hi), counts = census(lib, want)
    span = code[lo:hi + 1]
    print("%s\n  %d instructions in the kernel, item loop: instructions %d..%d (%d)" % (name.split("(")[0], len(code), lo, hi, len(span)))
    for c in CLASSES:
        print("  %-30s %5d" % (c, counts[c]))
    valu = sum(counts[c] for c in ("v_mul_f64 in the walk", "v_fmac_f64_dpp", "other FP64", "DPP moves", "v_permlane16_swap", "v_cndmask", "v_lshl_add_u64",
                                   "other VALU"))
    print("  %-30s %5d\n  %-30s %5d" % ("all vector ALU", valu, "all LDS", counts["ds_read_b128"] + counts["other LDS"]))
    if "--list" in sys.argv[1:]:
        for a, t in span:
            print("    %06x  %s" % (a, t))


if __name__ == "__main__":
    sys.exit(main())
