"""The built-in BAM reader (DESIGN.md sections 18 and 19) at a size where its code takes the branches a file of 500 reads
never reaches: more than one round of the one-workgroup scan, more than one entry buffer, a site deeper than the default
--max-depth, hundreds of entries per record, and coordinates beyond 2^26.  This module builds the scenario -- tests/
test_bam_scale_gpu.py imports it from here -- and holds the tests that need no device: the scenario really reaches each of
those branches (counted by the restatement alone), bam_ref.pileup_ref is the same function with and without candidate
lists, and the host stage fetches what it must, in the library and in the stand-alone program under the sanitizers.

Expected values come from tests/bam_ref.py and tests/readgroup_ref.py over the list of records, never from the code under
test."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
import readgroup_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 29                                        # the last position a .bai can index
REFS = [("chr1", 3000000), ("chr2", 3000000), ("chr3", 3000000), ("chrBig", BIG)]
IDS = ["lane%d" % g for g in range(8)]
PP = br.FPAIRED | br.FPROPER
SEED = 20
CLUSTERS = 560                                       # per sequence; three markers 30 bases apart per cluster
READS_DEEP, READS_SHALLOW = 190, 31                  # every twelfth cluster lies deeper than 100; about 44 reads on average
DENSE0, DENSE_N, DENSE_READS = 2950001, 200, 30      # chr1: positions DENSE0 .. DENSE0 + 199 (1-based)
DEEP, DEEP_READS = 2950000, 8200                     # chr3: one marker (1-based) under 8 200 reads
BOUNDS = (1 << 20, 1 << 23, 1 << 26, 3 << 26)        # chrBig: a read across b lives in a level 2, 1, 0, 0 bin
BATCH_BYTES = 1 << 20                                # tunable bam_batch_kb = 1024


def _scenario():
    """(records, bed rows, at): at maps a named place to its (chr, pos1) or to a list of them"""
    rng = np.random.default_rng(SEED)
    pool_n = 1 << 16
    pool_b = "".join("ACGT"[x] for x in rng.integers(0, 4, size=pool_n))
    pool_q = [int(x) for x in rng.integers(2, 42, size=pool_n)]          # 2..41: some fall below --min-BQ 13
    R, rows, at = [], [], {}

    def cut(n):
        o = int(rng.integers(0, pool_n - n))
        return pool_b[o:o + n], pool_q[o:o + n]

    def marker(c, p):
        ref = "ACGT"[int(rng.integers(0, 4))]
        rows.append((c, p, ref, "ACGT"[("ACGT".index(ref) + 1 + int(rng.integers(0, 3))) % 4]))
        return (c, p)

    # -- bulk: clusters of three markers, reads of 100 bases around them, a mate for about one read in ten
    for tid in range(3):
        c = REFS[tid][0]
        for k in range(CLUSTERS):
            p = 6000 + 5150 * k + int(rng.integers(0, 3000))
            for d in (0, 30, 60):
                marker(c, p + d)
            n_reads = READS_DEEP if k % 12 == 5 else READS_SHALLOW
            starts = rng.integers(-100, 60, size=n_reads)
            paired = rng.random(n_reads) < 0.1
            ahead = rng.integers(0, 60, size=n_reads)
            for j in range(n_reads):
                s = p - 1 + int(starts[j])
                name, strand = "b%d_%d_%d" % (tid, k, j), br.FREVERSE if j & 1 else 0
                seq, q = cut(100)
                if paired[j]:
                    s2 = s + int(ahead[j])
                    R.append(br.rec(name, tid, s, "100M", seq, q, flag=PP | 64 | strand, mtid=tid, mpos=s2, tlen=s2 - s + 100))
                    seq, q = cut(100)
                    R.append(br.rec(name, tid, s2, "100M", seq, q, flag=PP | 128 | (strand ^ br.FREVERSE), mtid=tid, mpos=s,
                                    tlen=-(s2 - s + 100)))
                else:                                # a few reads that the host keeps and the read filters drop
                    n = len(R)
                    R.append(br.rec(name, tid, s, "100M", seq, q, flag=strand | (br.FDUP if n % 53 == 0 else 0),
                                    mapq=1 if n % 59 == 0 else 60))
    # -- the dense stretch: 200 neighbouring markers under reads of 260 reference bases with a deletion in the middle
    at["dense"] = [marker("chr1", DENSE0 + i) for i in range(DENSE_N)]
    for k in range(DENSE_READS):
        seq, q = cut(250)
        R.append(br.rec("dense%d" % k, 0, DENSE0 - 1 - 90 + 3 * k, "100M10D150M", seq, q, flag=br.FREVERSE if k & 1 else 0))
    # -- the deep site: ascending starts, so file order is i; read i = 1 (mod 5) is the first of a proper pair whose mate
    #    is read i + 4: the pair (7996, 8000) has the default cap between its mates, (8096, 8100) a cap of 8 100
    at["deep"] = marker("chr3", DEEP)
    t = DEEP - 1

    def deep_pos(i):
        return t - 99 + (i * 99) // DEEP_READS

    for i in range(DEEP_READS):
        pos, name, flag, mpos = deep_pos(i), "deep%d" % i, 0, -1
        if i % 5 == 1 and i + 4 < DEEP_READS:
            name, flag, mpos = "deep_p%d" % i, PP | 64, deep_pos(i + 4)
        if i % 5 == 0 and i >= 5:
            name, flag, mpos = "deep_p%d" % (i - 4), PP | 128 | br.FREVERSE, deep_pos(i - 4)
        k = t - pos - 1
        cigar = "%dM4D%dM" % (k, 100 - k) if i % 211 == 7 and k >= 1 else "100M"
        seq, q = cut(100)
        R.append(br.rec(name, 2, pos, cigar, seq, q, flag=flag | (br.FREVERSE if i % 3 == 0 else 0), mtid=2 if flag else -1, mpos=mpos))
    # -- high coordinates: markers on both sides of 0-based b; reads across it, one that ends at it, one that begins at it
    at["big"], at["crossing"] = [], {}
    for b in BOUNDS:
        at["big"] += [marker("chrBig", b - 1), marker("chrBig", b), marker("chrBig", b + 1)]
        at["crossing"][b] = []
        for k in range(6):
            seq, q = cut(100)
            R.append(br.rec("cross%d_%d" % (b, k), 3, b - 50 + 9 * k, "100M", seq, q, flag=br.FREVERSE if k & 1 else 0))
            at["crossing"][b].append(R[-1]["name"])
        for name, pos in (("ends_at%d" % b, b - 100), ("begins_at%d" % b, b), ("one_base_over%d" % b, b - 99)):
            seq, q = cut(100)
            R.append(br.rec(name, 3, pos, "100M", seq, q))
        at["crossing"][b].append("one_base_over%d" % b)
    at["big"] += [marker("chrBig", BIG - 1), marker("chrBig", BIG)]
    for k, n in enumerate((120, 100, 100, 37)):      # they end exactly at the sequence's last base
        seq, q = cut(n)
        R.append(br.rec("tail%d" % k, 3, BIG - n, "%dM" % n, seq, q, flag=br.FREVERSE if k & 1 else 0))
    # -- markers that no read reaches, and a sequence the header lacks
    at["unreached"] = [marker("chr2", 2990000), marker("chrBig", 100000000), marker("chrZ", 7500)]
    R.sort(key=lambda r: (r["tid"], r["pos"]))       # (stable: the deep site's reads keep their order)
    for i, r in enumerate(R):
        rr.tag(r, None if i % 97 == 96 else IDS[i % len(IDS)])
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return R, rows, at


def build_fixture(d):
    """the scenario written once: panel files with their rows in shuffled order, the BAM in blocks of 300 payload bytes and
    its index, the candidate lists, and the restatement's answers per option set (computed on demand, then kept)"""
    recs, rows, at = _scenario()
    pre = os.path.join(d, "panel")
    with open(pre + ".bed", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s\t%d\t%d\t%s\t%s\n" % (c, p - 1, p, r, a))
    with open(pre + ".UD", "w") as fh:
        for i in range(len(rows)):
            fh.write("%g %g\n" % (0.01 * (i % 7 - 3), 0.02 * (i % 5 - 2)))
    with open(pre + ".mu", "w") as fh:
        for c, p, r, a in rows:
            fh.write("%s:%d_%s/%s 0.4\n" % (c, p, r, a))
    bam = os.path.join(d, "s.bam")
    vo, ve, _ = br.write_indexed_bam(bam, REFS, recs, block_payload=300, text=rr.rg_header(REFS, IDS))
    cand, _ = rr._candidates(recs, REFS, rows)
    index_of = {id(r): i for i, r in enumerate(recs)}
    spanning = sorted({index_of[id(r)] for rs in cand.values() for r in rs})
    whole, groups = {}, {}

    def want(**opts):
        key = tuple(sorted(opts.items()))
        if key not in whole:
            whole[key] = br.pileup_ref(recs, REFS, rows, opts, candidates=cand)
        return whole[key]

    def want_groups(**opts):
        key = tuple(sorted(opts.items()))
        if key not in groups:
            groups[key] = rr.group_pileup_ref(recs, REFS, rows, IDS, opts)
        return groups[key]

    return dict(recs=recs, rows=rows, at=at, pre=pre, bam=bam, vo=vo, cand=cand, spanning=spanning, index_of=index_of, want=want,
                want_groups=want_groups, dir=d)


@pytest.fixture(scope="module")
def scale(tmp_path_factory):
    return build_fixture(str(tmp_path_factory.mktemp("bam_scale")))


def _entries(f, c, p):
    return br.site_entries(f["cand"].get((c, p), []), [n for n, _ in REFS].index(c), p, dict(br.DEFAULT_OPTS))


def test_candidate_lists_do_not_change_the_restatement():
    """pileup_ref with and without candidates on the 458-read scenario of tests/test_bam_gpu.py: equal dicts."""
    import test_bam_gpu as small
    recs, rows, _ = small._scenario()
    cand, _ = rr._candidates(recs, small.REFS, rows)
    for opts in ({}, dict(max_depth=5)):
        plain = br.pileup_ref(recs, small.REFS, rows, opts)
        assert plain["entries"] > 400 and len(plain["sites"]) > 40
        assert br.pileup_ref(recs, small.REFS, rows, opts, candidates=cand) == plain


def test_the_scenario_holds_its_cases(scale):
    """Conditions, not measurements: each says that a branch of the reader is reached, from the restatement and the
    records alone."""
    f, at = scale, scale["at"]
    w = f["want"]()
    print("records %d, spanning a marker %d, slots %d, sites %d, entries %d, pairs resolved %d, capped sites %d" % (
        len(f["recs"]), len(f["spanning"]), len({(c, p) for c, p, _, _ in f["rows"]}), len(w["sites"]), w["entries"],
        w["pairs_resolved"], w["capped_sites"]))
    assert w["entries"] > 131072                                   # the entry buffer of 65 536 doubles at least twice
    assert len({(c, p) for c, p, _, _ in f["rows"] if c != "chrZ"}) > 4096 and len(w["sites"]) > 4096      # a scan of > 4 rounds
    deep = _entries(f, *at["deep"])
    assert len(deep) == DEEP_READS > 8000 and w["capped_sites"] == 1
    assert len(w["sites"][at["deep"]][0]) > 126 * 64 * 0.6          # bases of the site kernel's 126th round are stored
    first = {e["rec"]["name"]: i for i, e in enumerate(deep) if e["eligible"] and e["rec"]["flag"] & 64}
    second = {e["rec"]["name"]: i for i, e in enumerate(deep) if e["eligible"] and e["rec"]["flag"] & 128}
    for cap in (8000, 8100):                                        # a pair with the cap between its mates
        assert [n for n in first if n in second and first[n] < cap <= second[n]] == ["deep_p%d" % (cap - 4)]
    assert sum(1 for e in deep if e["deleted"]) >= 10 and sum(1 for e in deep if e["q"] < 13) > 1000
    assert f["want"](max_depth=8100)["capped_sites"] == 1 and f["want"](max_depth=8100)["pairs_resolved"] > w["pairs_resolved"]
    per_record = {}
    for c, p in at["dense"]:
        for e in _entries(f, c, p):
            per_record[e["rec"]["name"]] = per_record.get(e["rec"]["name"], 0) + 1
    assert max(per_record.values()) >= 200 and min(per_record.values()) < 200
    assert sum(1 for c, p in at["dense"] if any(e["deleted"] for e in _entries(f, c, p))) >= 50      # D in the middle of the run
    for c, p in at["big"]:
        assert w["sites"][(c, p)][0], (c, p)                        # non-empty
    for site in at["unreached"]:
        assert site not in w["sites"]
    assert w["pairs_resolved"] > 2000
    assert 300 < f["want"](max_depth=100)["capped_sites"] < 1000
    # reads in the index's higher levels, and a linear index of 32 768 windows
    by_name = {r["name"]: r for r in f["recs"]}
    for b, bin_ in zip(BOUNDS, (9, 1, 0, 0)):        # 9 + (beg >> 23), 1 + (beg >> 26), and the root
        for name in at["crossing"][b]:
            r = by_name[name]
            assert r["pos"] < b < br.record_end(r) and br.reg2bin(r["pos"], br.record_end(r)) == bin_, name
        assert len(at["crossing"][b]) == 7
        assert br.record_end(by_name["ends_at%d" % b]) == b and by_name["begins_at%d" % b]["pos"] == b
    assert all(br.record_end(by_name["tail%d" % k]) == BIG for k in range(4)) and (BIG - 1) >> 14 == 32767
    # groups: round-robin, every 97th record none
    assert sum(1 for r in f["recs"] if r["rg"] is None) == len(f["recs"]) // 97
    assert all(sum(1 for r in f["recs"] if r["rg"] == g) > len(f["recs"]) // 9 for g in IDS)
    # the .bed is not sorted by position
    pos = [(c, p) for c, p, _, _ in f["rows"]]
    assert sum(1 for a, b in zip(pos, pos[1:]) if a > b) > len(pos) // 3


def test_batches_of_one_mib_hold_many_records_and_few_entries(scale):
    """bam_batch_kb = 1024 closes a batch when the next record's variable bytes would pass 1 MiB.  Whatever the cuts: every
    run of consecutive kept records that fits 1 MiB and cannot grow holds fewer than 65 536 entries -- so, with more than
    131 072 in all, the entry buffer grows at least twice, each time with earlier batches' entries to carry over -- and
    more than 1 024 records: every batch's scan has a carry.  The reader's own cuts, from the first record on, make at
    least 8 batches."""
    f = scale
    n_entries = {}
    for (c, p) in f["want"]()["sites"]:
        for e in _entries(f, c, p):
            n_entries[id(e["rec"])] = n_entries.get(id(e["rec"]), 0) + 1
    assert sum(n_entries.values()) == f["want"]()["entries"]
    kept = [f["recs"][i] for i in f["spanning"]]
    size = [len(r["name"]) + 1 + 4 * len(r["cigar"]) + (len(r["seq"]) + 1) // 2 + len(r["seq"]) for r in kept]
    ent = [n_entries.get(id(r), 0) for r in kept]
    assert sum(ent) == f["want"]()["entries"] and max(ent) >= 200
    upto = [0]
    for n in ent:
        upto.append(upto[-1] + n)
    runs, j, nbytes, prev_j = 0, 0, 0, 0
    for i in range(len(kept)):                       # the longest run from i; it cannot grow to the left if it ends behind i - 1's
        while j < len(kept) and nbytes + size[j] <= BATCH_BYTES:
            nbytes += size[j]
            j += 1
        if i == 0 or j > prev_j:
            runs += 1
            assert j - i > 1024, (i, j)
            assert upto[j] - upto[i] < 65536, (i, j, upto[j] - upto[i])
        prev_j = j
        nbytes -= size[i]
    cuts, i = 0, 0
    while i < len(kept):
        nbytes = 0
        while i < len(kept) and nbytes + size[i] <= BATCH_BYTES:
            nbytes += size[i]
            i += 1
        cuts += 1
    print("kept records %d, variable bytes %d, runs looked at %d, the reader's batches %d" % (len(kept), sum(size), runs, cuts))
    assert cuts >= 8 and len(kept) / cuts > 1024 and runs > 1000


def test_host_scan_fetches_the_spanning_records(scale):
    f = scale
    got = vb.api.bam_scan(f["bam"], f["pre"] + ".bed", groups=True)
    fetched = [int(x) for x in got["voffsets"]]
    assert fetched == sorted(fetched) and len(set(fetched)) == len(fetched)
    assert got["stats"]["records_kept"] == len(fetched)
    print("fetched %d, spanning by the restatement %d" % (len(fetched), len(f["spanning"])), got["stats"])
    assert {f["vo"][i] for i in f["spanning"]} <= set(fetched)
    by_name = {r["name"]: f["vo"][i] for i, r in enumerate(f["recs"]) if r["tid"] == 3}
    for b in BOUNDS[:3]:
        for name in f["at"]["crossing"][b]:
            assert by_name[name] in set(fetched), name
    assert all(by_name["tail%d" % k] in set(fetched) for k in range(4))
    # the records' groups are the test's own tags
    assert got["group_ids"] == IDS
    tag_of = {f["vo"][i]: (0xFFFF if r["rg"] is None else IDS.index(r["rg"])) for i, r in enumerate(f["recs"])}
    assert [int(g) for g in got["record_groups"]] == [tag_of[v] for v in fetched]
    assert len(set(int(g) for g in got["record_groups"])) == len(IDS) + 1


def test_host_stage_alone_under_the_sanitizers(scale, tmp_path):
    """tests/bam_io_check_main.cpp + bam_io.cpp with -fsanitize=address,undefined, run directly over this file with the deep
    site, a dense position and the chrBig positions as markers: no report, and as many records as the restatement says
    span those markers."""
    f, at = scale, scale["at"]
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bam_io_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "verifybamid_amd", "csrc"), os.path.join(ROOT, "tests", "bam_io_check_main.cpp"),
           os.path.join(ROOT, "verifybamid_amd", "csrc", "bam_io.cpp"), "-lz", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        if "asan" in b.stderr.lower() or "ubsan" in b.stderr.lower() or "sanitize" in b.stderr.lower():
            pytest.skip("the sanitizer runtime does not link here: " + b.stderr[-300:])
        pytest.fail(b.stderr[-2000:])
    chosen = [at["deep"], at["dense"][DENSE_N // 2]] + at["big"] + at["unreached"]
    markers = str(tmp_path / "markers.txt")
    with open(markers, "w") as fh:
        for c, p in chosen:
            fh.write("%s %d\n" % (c, p))
    want = {f["index_of"][id(r)] for site in chosen for r in f["cand"].get(site, [])}
    assert len(want) > DEEP_READS + DENSE_READS // 2 + 6 * len(BOUNDS)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, markers, "4", "ok", f["bam"]], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    line = r.stdout.split()
    assert line[0] == "ok" and int(line[1]) == len(want), (line, len(want))
