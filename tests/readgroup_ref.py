"""readgroup_ref.py -- TEST INFRASTRUCTURE ONLY: the test side of --PerReadGroup.

A restatement of the definition of a read group's pileup, built from bam_ref's site_entries, resolve_overlaps and
site_strings, and helpers that give test records their auxiliary fields.  Expected values of the tests come from here and
from the reference's golden files, never from the code under test.

The definition.  Groups are the header's @RG lines in header order, identified by ID:.  A record belongs to the group its
RG field of type Z names; a record without one, with an RG of another type or with an ID the header lacks belongs to no
group.  A record dict carries the test's own truth as r["rg"] (an ID or None) beside the bytes in r["aux"].  Per site: the
whole sample's entries in file order after the read filters, --max-depth on the whole site, the mate-overlap rule on those
survivors; group g's site is the ordered sub-list of the survivors that belong to g, put through --min-BQ, the characters
and the deletion quirk; it is indexed when g has at least one survivor there, even with depth 0, absent otherwise.
"""
import bisect
import struct

import bam_ref as br

# one auxiliary field of every type of the SAM specification (SAMv1 4.2.4), B with every subtype
AUX_FIELDS = {
    "A": b"XAA" + b"q",
    "c": b"Xcc" + struct.pack("<b", -3),
    "C": b"XCC" + struct.pack("<B", 200),
    "s": b"Xss" + struct.pack("<h", -300),
    "S": b"XSS" + struct.pack("<H", 60000),
    "i": b"Xii" + struct.pack("<i", -70000),
    "I": b"XII" + struct.pack("<I", 4000000000),
    "f": b"Xff" + struct.pack("<f", 1.5),
    "Z": b"XZZ" + b"some text\0",
    "Z_empty": b"YZZ" + b"\0",
    "H": b"XHH" + b"1AE301\0",
    "Bc": b"BcB" + b"c" + struct.pack("<I", 3) + struct.pack("<3b", -1, 0, 1),
    "BC": b"BCB" + b"C" + struct.pack("<I", 2) + struct.pack("<2B", 1, 255),
    "Bs": b"BsB" + b"s" + struct.pack("<I", 2) + struct.pack("<2h", -2, 2),
    "BS": b"BSB" + b"S" + struct.pack("<I", 1) + struct.pack("<H", 7),
    "Bi": b"BiB" + b"i" + struct.pack("<I", 2) + struct.pack("<2i", -9, 9),
    "BI": b"BIB" + b"I" + struct.pack("<I", 3) + struct.pack("<3I", 1, 2, 3),
    "Bf": b"BfB" + b"f" + struct.pack("<I", 2) + struct.pack("<2f", 0.5, -0.5),
    "B_empty": b"BeB" + b"i" + struct.pack("<I", 0),
}


def rg_field(group_id):
    return b"RGZ" + group_id.encode() + b"\0"


def tag(r, group_id, before=b"", after=b"", truth="same"):
    """gives record r the auxiliary bytes before + RG:Z:group_id + after (group_id None: no RG field) and the test's own
    truth r["rg"]: group_id, or what `truth` says where the bytes name no group of the header"""
    r["aux"] = before + (b"" if group_id is None else rg_field(group_id)) + after
    r["rg"] = group_id if truth == "same" else truth
    return r


def rg_header(refs, groups, sample="S1"):
    """header text with one @RG line per (id, extra fields before ID:, extra fields behind it)"""
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    for g in groups:
        gid, pre, post = (g, "", "") if isinstance(g, str) else g
        text += "@RG" + "".join("\t" + f for f in pre.split("\t") if f) + "\tID:" + gid + "\tSM:" + sample + \
                "".join("\t" + f for f in post.split("\t") if f) + "\n"
    return text


def _candidates(records, refs, bed_rows):
    """(chr, pos1) -> the records, in file order, whose reference span reaches the position: what site_entries needs to
    look at (it does the exact test itself)"""
    tid_of = {}
    for t, (name, _) in enumerate(refs):
        tid_of.setdefault(name, t)
    pos_of = {}
    for c, p, _, _ in bed_rows:
        if c in tid_of:
            pos_of.setdefault(tid_of[c], set()).add(p)
    pos_of = {t: sorted(ps) for t, ps in pos_of.items()}
    name_of = {t: c for c, t in tid_of.items()}
    out = {}
    for r in records:
        ps = pos_of.get(r["tid"])
        if not ps or r["pos"] < 0:
            continue
        lo = bisect.bisect_left(ps, r["pos"] + 1)
        hi = bisect.bisect_right(ps, br.record_end(r))
        for p in ps[lo:hi]:
            out.setdefault((name_of[r["tid"]], p), []).append(r)
    return out, tid_of


def group_pileup_ref(records, refs, bed_rows, group_ids, opts=None, num_marker=None):
    """What --PerReadGroup must produce: a list with one dict per group, as bam_ref.pileup_ref returns for a sample
    (sites, rows, num_site, num_bases, avg_depth), and the bases of the survivors that belong to no group."""
    assert len(set(group_ids)) == len(group_ids)
    o = dict(br.DEFAULT_OPTS)
    o.update(opts or {})
    last = dict(o, incl_flags=o["incl_flags"] & ~1024, max_depth=1 << 30)      # the last step: no cap, no overlap rule
    cand, tid_of = _candidates(records, refs, bed_rows)
    ref_of = {}
    for c, p, ref, _ in bed_rows:
        ref_of[(c, p)] = ref
    index = {gid: g for g, gid in enumerate(group_ids)}
    sites = [dict() for _ in group_ids]
    unassigned_bases = 0
    for (c, p), ref in ref_of.items():
        if c not in tid_of:
            continue
        ent = br.site_entries(cand.get((c, p), []), tid_of[c], p, o)
        ent = ent[:max(o["max_depth"], 0)]                  # the cap on the whole site first
        if o["incl_flags"] & 1024:
            br.resolve_overlaps(ent)                        # ... the overlap rule on those survivors
        sub = [[] for _ in group_ids]
        nobody = []
        for e in ent:
            g = index.get(e["rec"].get("rg"))
            (nobody if g is None else sub[g]).append(e)
        for g, es in enumerate(sub):
            if es:
                sites[g][(c, p)] = br.site_strings(es, ref, last)
        unassigned_bases += len(br.site_strings(nobody, ref, last)[0])
    M = len(bed_rows) if num_marker is None else num_marker
    out = []
    for s in sites:
        num_bases = sum(len(b) for b, _ in s.values())
        eff = sum(1 for b, _ in s.values() if b)
        out.append(dict(sites=s, rows=[s.get((c, p), ("", "")) for c, p, _, _ in bed_rows[:M]],
                        num_site=sum(1 for c, p, _, _ in bed_rows[:M] if (c, p) in s), num_bases=num_bases,
                        avg_depth=num_bases / eff if eff else 0.0))
    return out, unassigned_bases
