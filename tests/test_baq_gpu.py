"""--ApplyBAQ on the device: the stage's records byte for byte against the host core of the same
header (csrc/baq_core.h), and the loaded pileup byte for byte against bam_ref.pileup_ref over the records baq_ref.py
transformed.  The host core itself is held to the reference's compiled HMM and to the restatement in test_baq_cpu.py.
Expected values never come from the code under test."""
import os
import subprocess
import sys

import numpy as np
import pytest

import verifybamid_amd as vb

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as br  # noqa: E402
import baq_ref  # noqa: E402
import baq_scenario as sc  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
BATCH_KB = 8          # the 5 kb read alone fills a batch: a dozen upload batches


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    return sc.write_all(str(tmp_path_factory.mktemp("baq")))


def _records_equal(dev, host):
    assert np.array_equal(dev["outcome"], host["outcome"])
    assert np.array_equal(dev["qual_off"], host["qual_off"])
    assert dev["qual"].tobytes() == host["qual"].tobytes()
    assert np.array_equal(dev["cap4"], host["cap4"])
    assert np.array_equal(dev["mapq"], host["mapq"])


@gpu
@pytest.mark.parametrize("name", sorted(sc.OPTION_SETS))
def test_device_records_equal_the_host_core_byte_for_byte(scenario, name, tunable):
    """outcome, every adjusted quality, the cap's four integers and the final mapQ of every record, with the LDS budget so low
    that query lengths 16 and 17 straddle the tiers and with batches so small that the file goes up in a dozen of them"""
    tunable("baq_lds_kb", sc.LDS_KB)
    tunable("bam_batch_kb", BATCH_KB)
    bed = scenario["pre"] + ".bed"
    opts = sc.OPTION_SETS[name] or None
    host = vb.api.baq_records(scenario["bam"], bed, scenario["fasta"], mpileup=opts, where=0)
    dev = vb.api.baq_records(scenario["bam"], bed, scenario["fasta"], mpileup=opts, where=1)
    print(name, dev["stats"])
    assert len(dev["mapq"]) == len(scenario["recs"])
    _records_equal(dev, host)
    for k in ("records", "realigned", "left_alone", "tag_applied", "no_reference", "dropped_outside", "dropped_cap", "not_asked",
              "undefined_rows"):
        assert dev["stats"][k] == host["stats"][k], k
    if name != "cap_only":
        # both tiers, split where the formula says: 16 bases fit a quarter of the LDS, 17 do not
        slot = sc.LDS_KB * 1024 // 4
        L = vb._abi.lib()
        assert L.vb2_baq_work_bytes(16 + 7, 16, 7) <= slot < L.vb2_baq_work_bytes(17 + 7, 17, 7)
        assert dev["stats"]["records_lds"] > 0 and dev["stats"]["records_global"] > 0
        assert dev["stats"]["records_lds"] + dev["stats"]["records_global"] == dev["stats"]["realigned"] + \
            sum(1 for a in scenario["adjusted"](name) if a["outcome"] == baq_ref.CAP_DROPPED and a["shape"] is not None)


@gpu
def test_stats_are_the_restatements(scenario, tunable):
    tunable("baq_lds_kb", sc.LDS_KB)
    dev = vb.api.baq_records(scenario["bam"], scenario["pre"] + ".bed", scenario["fasta"], where=1)
    want = scenario["adjusted"]("defaults")
    count = lambda oc: sum(1 for a in want if a["outcome"] == oc)  # noqa: E731
    st = dev["stats"]
    assert st["realigned"] == count(baq_ref.REALIGNED) and st["left_alone"] == count(baq_ref.ALONE)
    assert st["tag_applied"] == count(baq_ref.TAG_APPLIED) and st["no_reference"] == count(baq_ref.NO_REFERENCE)
    assert st["dropped_outside"] == count(baq_ref.OUTSIDE) == 1 and st["dropped_cap"] == count(baq_ref.CAP_DROPPED) >= 1
    assert st["undefined_rows"] == 0 == sum(a["undefined"] for a in want)
    assert st["records_lds"] > 0 and st["records_global"] > 0
    # the default budget holds the short reads in LDS too, the 5 kb read never
    tunable("baq_lds_kb", 64)
    dflt = vb.api.baq_records(scenario["bam"], scenario["pre"] + ".bed", scenario["fasta"], where=1)
    assert dflt["stats"]["records_global"] >= 1 and dflt["stats"]["records_lds"] > st["records_lds"]
    assert dflt["qual"].tobytes() == dev["qual"].tobytes() and np.array_equal(dflt["mapq"], dev["mapq"])


@gpu
def test_three_records_share_a_wave_with_an_empty_slot(tmp_path):
    recs, rows, genome, _ = sc.build()
    keep = [r for r in recs if r["name"] in ("len7", "len8", "len16")]
    assert len(keep) == 3
    bam = str(tmp_path / "three.bam")
    br.write_indexed_bam(bam, sc.REFS, keep, block_payload=300)
    pre = str(tmp_path / "panel")
    sc.write_panel(pre, rows)
    fasta = str(tmp_path / "g.fa")
    baq_ref.write_fasta(fasta, sc.fasta_genome(genome))
    host = vb.api.baq_records(bam, pre + ".bed", fasta, where=0)
    dev = vb.api.baq_records(bam, pre + ".bed", fasta, where=1)
    assert len(dev["mapq"]) == 3 and dev["stats"]["records_lds"] == 3
    _records_equal(dev, host)


@gpu
def test_records_and_load_report_equal_stats(scenario, tunable):
    """vb2_baq_records(where = 1) and a --ApplyBAQ load cut the same batches and finish their records alike"""
    tunable("baq_lds_kb", sc.LDS_KB)
    tunable("bam_batch_kb", BATCH_KB)
    dev = vb.api.baq_records(scenario["bam"], scenario["pre"] + ".bed", scenario["fasta"], where=1)
    got = vb.api.load_bam(scenario["pre"], scenario["bam"], apply_baq=True, reference_path=scenario["fasta"])
    print(dev["stats"], got["baq"])
    for k in ("records", "realigned", "left_alone", "tag_applied", "no_reference", "dropped_outside", "dropped_cap", "not_asked",
              "undefined_rows", "records_lds", "records_global", "fasta_bytes"):
        assert dev["stats"][k] == got["baq"][k], k
    assert got["baq"]["records"] == len(scenario["recs"])


@gpu
def test_batches_of_four_gib_are_refused(scenario, tunable):
    tunable("bam_batch_kb", 0xfff00000 // 1024 + 1)
    with pytest.raises(vb._abi.Vb2Error) as e:
        vb.api.baq_records(scenario["bam"], scenario["pre"] + ".bed", scenario["fasta"], where=1)
    assert e.value.code == vb._abi.VB2_ERR_INVALID
    assert str(e.value).endswith("vb2_baq_records: bam_batch_kb asks for batches of 4 GiB or more")
    with pytest.raises(vb._abi.Vb2Error) as e:
        vb.api.load_bam(scenario["pre"], scenario["bam"], apply_baq=True, reference_path=scenario["fasta"])
    assert e.value.code == vb._abi.VB2_ERR_INVALID
    assert str(e.value).endswith("--BamFile: bam_batch_kb asks for batches of 4 GiB or more")


@gpu
def test_records_that_all_miss_the_panel_leave_nothing(scenario, tmp_path):
    """reads on chr1 only, one marker on chr2: the stage sees no record; the FASTA's index is still opened (an absent
    FASTA is the load's error as with records), and none of its bases are read"""
    recs = [r for r in scenario["recs"] if r["tid"] == 0][:12]
    assert len(recs) == 12
    pre, bam = str(tmp_path / "miss"), str(tmp_path / "miss.bam")
    sc.write_panel(pre, [("chr2", 1000, "A", "C")])
    br.write_indexed_bam(bam, sc.REFS, recs, block_payload=300)
    got = vb.api.load_bam(pre, bam, apply_baq=True, reference_path=scenario["fasta"])
    print(got["stats"], got["baq"])
    st = got["stats"]
    assert (st["records_kept"], st["batches"], st["entries"], st["sites"]) == (0, 0, 0, 0)
    assert (got["num_site"], got["num_bases"], got["avg_depth"]) == (0, 0, 0.0)
    assert got["baq"]["records"] == 0 and got["baq"]["fasta_bytes"] == 0
    assert got["baq"]["records_lds"] == 0 == got["baq"]["records_global"]
    with pytest.raises(vb._abi.Vb2Error) as e:
        vb.api.load_bam(pre, bam, apply_baq=True, reference_path=scenario["dir"] + "/absent.fa")
    assert e.value.code == vb._abi.VB2_ERR_IO
    dev = vb.api.baq_records(bam, pre + ".bed", scenario["fasta"], where=1)
    assert len(dev["mapq"]) == 0 and list(dev["qual_off"]) == [0] and dev["stats"]["records"] == 0


def _same(got, want, rows):
    off = got["read_off"]
    assert len(off) == len(rows) + 1
    for i, (c, p, _, _) in enumerate(rows):
        b, q = got["bases"][off[i]:off[i + 1]].decode("latin-1"), got["quals"][off[i]:off[i + 1]].decode("latin-1")
        assert (b, q) == want["rows"][i], ("%s:%d" % (c, p), b, q, want["rows"][i])
    assert got["num_site"] == want["num_site"]
    assert got["num_bases"] == want["num_bases"]
    assert got["avg_depth"] == want["avg_depth"]


@gpu
@pytest.mark.parametrize("name", sorted(sc.OPTION_SETS))
def test_pileup_is_the_restatements_over_transformed_records(scenario, name, tunable):
    tunable("baq_lds_kb", sc.LDS_KB)
    tunable("bam_batch_kb", BATCH_KB)
    got = vb.api.load_bam(scenario["pre"], scenario["bam"], mpileup=sc.OPTION_SETS[name] or None, apply_baq=True,
                          reference_path=scenario["fasta"])
    print(name, got["stats"], got["baq"])
    _same(got, scenario["want"](name), scenario["rows"])
    assert got["stats"]["batches"] >= 3 and got["baq"]["records"] == len(scenario["recs"])
    if name == "defaults":
        # the switch changes what is piled up: a pair's winner, a base under min-BQ, a read the cap drops
        plain = br.pileup_ref(scenario["recs"], sc.REFS, scenario["rows"], {})
        w = scenario["want"](name)["sites"]
        at = scenario["at"]
        assert w[at["pair_baq"]] != plain["sites"][at["pair_baq"]]
        assert at["cap_drops"] in plain["sites"] and at["cap_drops"] not in w
        assert sum(len(b) for b, _ in w.values()) < sum(len(b) for b, _ in plain["sites"].values())


@gpu
def test_switch_off_is_todays_pileup(scenario):
    got = vb.api.load_bam(scenario["pre"], scenario["bam"])
    _same(got, br.pileup_ref(scenario["recs"], sc.REFS, scenario["rows"], {}), scenario["rows"])
    assert "baq" not in got
    with pytest.raises(vb._abi.Vb2Error):
        vb.api.load_bam(scenario["pre"], scenario["bam"], apply_baq=True)          # no FASTA named


@gpu
def test_neither_step_asked_for_leaves_the_fasta_unopened(scenario):
    o = dict(incl_flags=1024, adjust_mq=0)
    got = vb.api.load_bam(scenario["pre"], scenario["bam"], mpileup=o, apply_baq=True, reference_path=scenario["dir"] + "/absent.fa")
    _same(got, br.pileup_ref(scenario["recs"], sc.REFS, scenario["rows"], o), scenario["rows"])
    assert got["baq"]["fasta_bytes"] == 0 and got["baq"]["not_asked"] == len(scenario["recs"])


@gpu
def test_cohort_line_and_command_line_give_the_single_runs_numbers(scenario, tmp_path):
    """a cohort with the BAM as a .bam line gives the single run's estimate bitwise; #READS of .selfSM is the adjusted pileup's
    bases; the command line says what it applied and keeps quiet about what it did not leave out"""
    kw = dict(disable_sanity=True, apply_baq=True, reference_path=scenario["fasta"])
    one = vb.api.run_files(scenario["pre"], None, bam_path=scenario["bam"], **kw)
    many = vb.api.run_cohort_files(scenario["pre"], [scenario["bam"]], **kw)
    many = many[0] if isinstance(many, tuple) else many
    want = scenario["want"]("defaults")
    assert one["num_bases"] == want["num_bases"] == many[0]["num_bases"]
    for k in ("alpha", "llk1", "llk0"):
        if k in one:
            assert one[k] == many[0][k], k
    out = str(tmp_path / "cli")
    r = subprocess.run([EXE, "--SVDPrefix", scenario["pre"], "--BamFile", scenario["bam"], "--Reference", scenario["fasta"],
                        "--ApplyBAQ", "--DisableSanityCheck", "--Output", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "is not applied" not in r.stderr and r.stderr.count("NOTICE - --ApplyBAQ") == 1 and scenario["fasta"] in r.stderr
    cols = open(out + ".selfSM").read().splitlines()
    head, row = cols[0].split("\t"), cols[1].split("\t")
    assert int(row[head.index("#READS")]) == want["num_bases"]
    plain = subprocess.run([EXE, "--SVDPrefix", scenario["pre"], "--BamFile", scenario["bam"], "--Reference", scenario["fasta"],
                            "--DisableSanityCheck", "--Output", out + "_plain"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and plain.stderr.count("is not applied") == 2 and "--ApplyBAQ" not in plain.stderr


@gpu
def test_read_group_pileups_see_the_adjusted_values(scenario, tmp_path, tunable):
    """--PerReadGroup under --ApplyBAQ: every group's pileup, and the whole sample's, from the transformed records"""
    import readgroup_ref as rg
    tunable("baq_lds_kb", sc.LDS_KB)
    recs = []
    for i, r in enumerate(scenario["recs"]):
        t = dict(r)
        rg.tag(t, None if i % 7 == 6 else "AB"[i % 2], before=r.get("aux", b""))
        recs.append(t)
    bam = str(tmp_path / "rg.bam")
    br.write_indexed_bam(bam, sc.REFS, recs, block_payload=300, text=rg.rg_header(sc.REFS, ["A", "B"]))
    adj = []
    for t, a in zip(recs, scenario["adjusted"]("defaults")):      # (an RG field changes nothing of what BAQ reads)
        if a["mapq"] < 0:
            continue
        u = dict(t)
        u["qual"], u["mapq"] = a["qual"], a["mapq"]
        adj.append(u)
    want, _ = rg.group_pileup_ref(adj, sc.REFS, scenario["rows"], ["A", "B"])
    got = vb.api.load_bam_groups(scenario["pre"], bam, apply_baq=True, reference_path=scenario["fasta"])
    _same(got, scenario["want"]("defaults"), scenario["rows"])
    assert [g["id"] for g in got["groups"]] == ["A", "B"]
    for g, w in zip(got["groups"], want):
        _same(g, w, scenario["rows"])
    plain = vb.api.load_bam_groups(scenario["pre"], bam)
    assert plain["groups"][0]["num_bases"] > got["groups"][0]["num_bases"]
