#!/usr/bin/env python
"""Regenerates tests/golden/baq/kpa_cases.json: what the reference's OWN banded profile HMM gives on seeded cases.

    python tests/golden/make_baq_fixtures.py [--reference /root/reference] [--check]

The reference's samtools/kprobaln.c (kpa_glocal; nothing but libc) is compiled together with tests/golden/baq/kpa_driver.c
into a temporary directory, run on the cases below and thrown away: nothing compiled and no text of the reference is
committed, only the cases and what its program wrote for them (`state`, `q`).  tests/test_baq_cpu.py holds the Python
restatement (tests/baq_ref.py) and the library's host core (csrc/baq_core.h) to the file.

The cases: query lengths 1, 2, 3, 8, 40, 100, 151 and one of 600; l_ref below, at and above l_query +- bw; bw 1, 7, 10 and
|l_ref - l_query| + 3 with a difference of 12; code 4 in reference and query; qualities 0, 2, 41, 93 and 255; a query that
matches nowhere.  A row whose posterior sum (or 1 - max/sum) is not positive makes the reference convert a NaN or an
infinity to int, which is outside the contract: the recipe finds such cases with the restatement, names them and leaves
them out, so the file holds none.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import baq_ref  # noqa: E402

OUT = os.path.join(HERE, "baq", "kpa_cases.json")
QUALS = [0, 2, 41, 93, 255]


def make_cases():
    rng = random.Random(20261021)
    cases = []

    def add(name, l_query, l_ref, bw, kind="mutated"):
        ref = [rng.randrange(4) for _ in range(l_ref)]
        if kind == "nowhere":
            ref = [0] * l_ref
            query = [3] * l_query
        else:
            # the query follows the reference's middle, with substitutions, so that posteriors are not all alike
            off = max(0, (l_ref - l_query) // 2)
            query = [ref[(off + i) % l_ref] if l_ref and rng.random() > 0.08 else rng.randrange(4) for i in range(l_query)]
        if kind == "n":
            for a in (ref, query):
                for _ in range(max(1, len(a) // 10)):
                    a[rng.randrange(len(a))] = 4
        if kind == "extreme":
            qual = [QUALS[rng.randrange(len(QUALS))] for _ in range(l_query)]
        else:
            qual = [rng.randrange(2, 42) for _ in range(l_query)]
        cases.append(dict(name=name, bw=bw, ref=ref, query=query, qual=qual))

    for lq in (1, 2, 3, 8, 40, 100, 151):
        for bw in (1, 7, 10):
            for d in (-bw - 2, -bw, -1, 0, 1, bw, bw + 2):
                if lq + d < 1:
                    continue
                add("lq%d_bw%d_d%+d" % (lq, bw, d), lq, lq + d, bw)
        add("lq%d_extreme" % lq, lq, lq + 5, 7, "extreme")
        add("lq%d_n" % lq, lq, lq + 7, 7, "n")
    add("delta12_more_ref", 100, 112, 15)
    add("delta12_less_ref", 100, 88, 15)
    add("nowhere", 40, 47, 7, "nowhere")
    add("nowhere_extreme", 8, 15, 7, "nowhere")
    add("lq600", 600, 607, 7)
    add("all_n_ref", 16, 23, 7)
    cases[-1]["ref"] = [4] * 23
    add("all_n_query", 16, 23, 7)
    cases[-1]["query"] = [4] * 16
    return cases


def hexs(a):
    return bytes(a).hex() if a else "-"


def run_reference(reference, cases):
    src = os.path.join(reference, "samtools", "kprobaln.c")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "kpa_driver")
        subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-I", os.path.join(reference, "samtools"), "-o", exe,
                               os.path.join(HERE, "baq", "kpa_driver.c"), src, "-lm"])
        text = "".join("%d %d %d %s %s %s\n" % (len(c["ref"]), len(c["query"]), c["bw"], hexs(c["ref"]), hexs(c["query"]),
                                               hexs(c["qual"])) for c in cases)
        out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases), (len(out), len(cases))
    for c, line in zip(cases, out):
        st, q = line.split("|")
        c["state"] = [int(x) for x in st.split()]
        c["q"] = list(bytes.fromhex(q.strip()))
        assert len(c["state"]) == len(c["query"]) == len(c["q"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    cases = make_cases()
    run_reference(a.reference, cases)
    kept = []
    for c in cases:
        _, _, undefined = baq_ref.kpa_glocal(c["ref"], c["query"], c["qual"], c["bw"])
        if undefined:      # (a one-base reference under a longer query: the only state left has posterior exactly 1)
            print("left out, %d row(s) outside the contract: %s" % (undefined, c["name"]))
            continue
        kept.append(c)
    cases = kept
    assert all(any(c["name"].startswith("lq%d_" % lq) for c in cases) for lq in (1, 2, 3, 8, 40, 100, 151))
    doc = dict(recipe="tests/golden/make_baq_fixtures.py",
               cases=[dict(name=c["name"], bw=c["bw"], ref=bytes(c["ref"]).hex(), query=bytes(c["query"]).hex(),
                           qual=bytes(c["qual"]).hex(),
                           state=b"".join((s & 0xffffffff).to_bytes(4, "little") for s in c["state"]).hex(),
                           q=bytes(c["q"]).hex()) for c in cases])
    text = json.dumps(doc, indent=0, sort_keys=True) + "\n"
    if a.check:
        assert open(OUT).read() == text, "kpa_cases.json does not reproduce"
        print("kpa_cases.json reproduces: %d cases" % len(cases))
        return
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), len(text)))


if __name__ == "__main__":
    main()
