"""Compare the gfx950 code of two libvb2.so builds kernel by kernel (a refactoring aid; runs where there is no GPU).

    python tools/isa_diff.py OLD.so NEW.so ['old kernel name substring=new kernel name substring' ...]
    python tools/isa_diff.py OLD.so NEW.so --all

Without pairs: lists both builds' kernels with instruction counts, VGPR/SGPR/scratch/LDS figures.  With pairs: the
instruction streams of each pair (addresses, symbol names and branch targets stripped) are diffed -- identical streams
mean identical kernels.  --all: every function of EVERY code object of the two builds (one per translation unit), paired by
name -- prints the ones that differ or exist on one side only, and the count of identical ones.  Uses llvm-objdump / llvm-readelf from /opt/rocm/lib/llvm/bin.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def code_object(so, tmp):
    d = os.path.join(tmp, os.path.basename(so) + ".d")
    os.makedirs(d, exist_ok=True)
    local = os.path.join(d, "lib.so")
    subprocess.check_call(["cp", so, local])
    subprocess.check_call([LLVM + "llvm-objdump", "--offloading", local], cwd=d, stdout=subprocess.DEVNULL)
    co = sorted(f for f in os.listdir(d) if "amdgcn" in f)
    return [os.path.join(d, f) for f in co]


def kernels(cos, every=False):
    out = {}
    for co in (cos if every else cos[:1]):
        for k, v in kernels_of(co).items():
            out[k if k not in out else k + " [" + os.path.basename(co) + "]"] = v
    return out


def kernels_of(co):
    dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    names, cur, out = {}, None, {}
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        ins = line.split("//")[0].strip()
        ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
        if ins:
            out[cur].append(ins)
    dem = subprocess.run(["c++filt"], input="\n".join(out.keys()), capture_output=True, text=True).stdout.splitlines()
    return {d: out[k] for k, d in zip(out.keys(), dem)}


def normalise(ins):
    ins = re.sub(r"<[^>]*>", "<sym>", ins)
    ins = re.sub(r"\b(s_c?branch\w*|s_call\w*)\s+\S+", r"\1 <target>", ins)
    return ins


def normalise_all(stream):
    """normalise() over a stream, and the literals of a pc-relative address -- the s_add_u32 / s_addc_u32 pair behind an
    s_getpc_b64, on its registers: the distance to a constant table moves when any other function changes its size"""
    out, lo, hi = [], None, None
    for ins in stream:
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if m:
            lo, hi = "s" + m.group(1), "s" + m.group(2)
        elif lo and re.match(r"s_add_u32 %s, %s, 0x[0-9a-f]+$" % (lo, lo), ins):
            ins, lo = "s_add_u32 %s, %s, <pcrel>" % (lo, lo), None
        elif hi and re.match(r"s_addc_u32 %s, %s, (0x[0-9a-f]+|-1|0)$" % (hi, hi), ins):
            ins, hi = "s_addc_u32 %s, %s, <pcrel>" % (hi, hi), None
        out.append(normalise(ins))
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    every = "--all" in sys.argv[3:]
    pairs = [p.split("=", 1) for p in sys.argv[3:] if p != "--all"]
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "old")), os.makedirs(os.path.join(tmp, "new"))
        ko, kn = kernels(code_object(old, os.path.join(tmp, "old")), every), kernels(code_object(new, os.path.join(tmp, "new")), every)
    if every:
        same = 0
        for k in sorted(set(ko) | set(kn)):
            if k not in ko or k not in kn:
                print("ONLY IN %s  %s" % ("OLD" if k in ko else "NEW", k[:150]))
            elif normalise_all(ko[k]) == normalise_all(kn[k]):
                same += 1
            else:
                print("DIFFERENT  %d -> %d instructions  %s" % (len(ko[k]), len(kn[k]), k[:150]))
        print("%d functions identical" % same)
        return 0
    if not pairs:
        for tag, ks in (("OLD", ko), ("NEW", kn)):
            print("%s: %d functions, %d instructions" % (tag, len(ks), sum(len(v) for v in ks.values())))
            for k, v in ks.items():
                print("  %6d  %s" % (len(v), k[:150]))
        return 0
    bad = 0
    for a, b in pairs:
        ca = [k for k in ko if a in k]
        cb = [k for k in kn if b in k]
        if len(ca) != 1 or len(cb) != 1:
            print("ambiguous pair %r (%d) = %r (%d)" % (a, len(ca), b, len(cb)))
            bad += 1
            continue
        ia, ib = [normalise(x) for x in ko[ca[0]]], [normalise(x) for x in kn[cb[0]]]
        if ia == ib:
            print("IDENTICAL  %d instructions  %s" % (len(ia), b))
        else:
            d = list(difflib.unified_diff(ia, ib, lineterm="", n=0))
            print("DIFFERENT  %d -> %d instructions, %d diff lines  %s" % (len(ia), len(ib), len(d), b))
            for line in d[:40]:
                print("    " + line)
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
