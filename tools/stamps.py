"""In-kernel timeline of llk_eval_kernel from per-workgroup wall-clock stamps (VB2_STAMPS=1)."""
import os, sys, ctypes as C
os.environ["VB2_STAMPS"] = "1"
_stamps_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "verifybamid_amd", "libvb2_stamps.so")
if os.path.exists(_stamps_lib):
    os.environ.setdefault("VB2_LIB_PATH", _stamps_lib)      # (the stamps are compiled out of libvb2.so)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import verifybamid_amd as vb
from verifybamid_amd import _abi
B = int(os.environ.get("VB2_B", 8)); M = int(os.environ.get("VB2_M", 100000))
d = vb.synth.make_pileup(M, 30, 4, 0.05, 2)
rng = np.random.default_rng(5)
ctx = vb.LikelihoodContext(d)
pc1 = rng.normal(0, 0.03, size=(B, 4)); pc2 = rng.normal(0, 0.03, size=(B, 4)); al = rng.uniform(0, 0.5, size=B)
for _ in range(5): ctx.llk(pc1, pc2, al)
lib = _abi.lib()
buf = (C.c_ulonglong * (8 * 512))()
lib.vb2_debug_read_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
nb = lib.vb2_debug_read_stamps(ctx._h, buf, 512)
s = np.array(buf[:8 * nb], dtype=np.float64).reshape(nb, 8)
s = s[s[:, 0] > 0]
t0 = s[:, 0].min()
us = (s - t0) / 100.0          # 100 MHz -> us
names = ["entry", "points in LDS", "table built", "wave0 tiles done", "last wave tiles done", "block reduced", "finalized (last block)"]
print("blocks with stamps:", len(s), "B =", B)
for i, n in enumerate(names):
    col = us[:, i][s[:, i] > 0]
    if len(col): print("%-24s min %6.2f  median %6.2f  max %6.2f us" % (n, col.min(), np.median(col), col.max()))
if os.environ.get("VB2_STAMPS_DETAIL"):
    t4 = us[:, 4]
    print("last wave done, median by workgroup index mod 8 (XCD): " + " ".join("%.2f" % np.median(t4[x::8]) for x in range(8)))
    print("   by index mod 16: " + " ".join("%.1f" % np.median(t4[x::16]) for x in range(16)))
    print("   by index // 32:  " + " ".join("%.2f" % np.median(t4[32 * x:32 * x + 32]) for x in range(8)))
    # (a split launch's workgroups leave 1 + their XCC id in word 7 -- not the workgroups 0, 20, 21: by the XCD itself, and
    # by the depth of a workgroup's tiles -- its index among the workgroups of its XCD, the tiles being dealt deepest first)
    xcc = s[:, 7].astype(np.int64) - 1
    has = (xcc >= 0) & (xcc < 8)
    has[[i for i in (0, 20, 21) if i < len(has)]] = False
    if has.sum() > 8:
        t5 = us[:, 5]
        print("by XCC id (workgroups, last wave done median / max, block reduced median): " +
              "  ".join("%d: %d %.2f / %.2f %.2f" % (x, (has & (xcc == x)).sum(), np.median(t4[has & (xcc == x)]), t4[has & (xcc == x)].max(),
                                                  np.median(t5[has & (xcc == x)])) for x in range(8) if (has & (xcc == x)).any()))
        idx = np.arange(len(t4))
        print("   workgroups whose XCC id is that of their index mod 8's majority: %d of %d"
              % (sum((xcc[i] == np.bincount(xcc[has & (idx % 8 == i % 8)]).argmax()) for i in idx[has]), has.sum()))
        resid = t4 - np.array([np.median(t4[has & (xcc == xcc[i])]) if has[i] else 0.0 for i in idx])
        q = len(t4) // 4
        print("   last wave done minus its XCD's median, by quarter of the workgroup index (first quarter = deepest tiles): " +
              " ".join("%.2f" % np.median(resid[has & (idx >= a) & (idx < a + q)]) for a in range(0, 4 * q, q)))
        print("   spread (max - min) of last wave done: all %.2f us; within an XCD, median over XCDs %.2f us; between the XCDs' medians %.2f us"
              % (t4[has].max() - t4[has].min(), np.median([t4[has & (xcc == x)].max() - t4[has & (xcc == x)].min() for x in range(8) if (has & (xcc == x)).any()]),
                 np.ptp([np.median(t4[has & (xcc == x)]) for x in range(8) if (has & (xcc == x)).any()])))
    order = np.argsort(-t4)
    print("   slowest: " + ", ".join("%d: %.1f" % (i, t4[i]) for i in order[:16]))
    print("   fastest: " + ", ".join("%d: %.1f" % (i, t4[i]) for i in order[-16:]))
ctx.close()
