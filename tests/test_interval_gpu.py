"""The FREEMIX confidence interval (vb2_ctx_interval, vb2_run_interval, --ConfidenceInterval) on the MI355X: the
profile's defining properties, the oracle's own FixAlpha search at the bounds, calibration over seeds, and the command
line end to end (stdout, .selfSM and .Ancestry untouched; .CI rows of the model's free parameters)."""
import os
import subprocess

import numpy as np
import pytest

import verifybamid_amd as vb
from oracle.bridge import oracle_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")
C_HALF = 1.9207294103470620


@pytest.mark.parametrize("alpha_true", [0.03, 0.8])
def test_profile_interval_properties(alpha_true):
    d = vb.synth.make_pileup(10000, mean_depth=30, num_pc=4, alpha_true=alpha_true, seed=21)
    od = oracle_data(d)
    with vb.LikelihoodContext(d) as ctx:
        est = ctx.optimize()
        ci = ctx.interval(est)
    llk = abs(est["llk1"])
    f = ci["freemix"]
    assert f == (est["alpha"] if est["alpha"] < 0.5 else 1 - est["alpha"])
    assert ci["lo"] <= f <= ci["hi"]
    assert ci["llk_max"] >= -est["llk1"]
    side = est["alpha"] >= 0.5
    interior = [(b, v) for b, v, edge in ((ci["lo"], ci["llk_lo"], 0.0), (ci["hi"], ci["llk_hi"], 0.5)) if b != edge]
    assert interior
    for b, v in interior:
        assert abs(v - (ci["llk_max"] - C_HALF)) <= 1e-7 * llk, (b, v, ci["llk_max"])
        # the oracle's own search over the PCs at the bound's alpha cannot beat the profile, and comes close to it
        ref = od.optimize(fix_alpha=(1 - b) if side else b)
        assert -ref["llk1"] <= v + 1e-9 * llk, (b, -ref["llk1"], v)
        assert -ref["llk1"] >= v - 1e-6 * llk, (b, -ref["llk1"], v)
    assert ci["num_launch"] > 0 and ci["num_profile"] >= 3
    assert ci["rows"][0]["param"] == "FREEMIX" and len(ci["rows"]) == 1 + 2 * 4


def test_calibration_over_seeds():
    """alpha_true 0.02: the interval covers it in >= 33 of 40 samples (nominal 38).  alpha_true 0: lo == 0 where the profile
    at 0 is within the cut.  At that boundary the likelihood ratio is not the half-and-half chi2 mixture that would give lo > 0
    in 1 of 40: the contaminant's PCs are not identified at alpha = 0 and the ratio maximises over them, which makes it
    heavier.  Measured on these seeds: lo == 0 in 35 of 40, the bound below."""
    covered = zero_lo = 0
    for s in range(1, 41):
        for alpha_true in (0.02, 0.0):
            d = vb.synth.make_pileup(10000, mean_depth=20, num_pc=2, alpha_true=alpha_true, seed=s)
            with vb.LikelihoodContext(d) as ctx:
                ci = ctx.interval(ctx.optimize())
            if alpha_true > 0:
                covered += ci["lo"] <= alpha_true <= ci["hi"]
            else:
                zero_lo += ci["lo"] == 0.0
    assert covered >= 33, covered
    assert zero_lo >= 35, zero_lo


def _run(args, out, ci):
    cmd = [EXE] + args + ["--Output", out] + (["--ConfidenceInterval"] if ci else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


MODELS = [("default", [], ["ContaminatingSample.PC1", "ContaminatingSample.PC2", "IntendedSample.PC1", "IntendedSample.PC2"]),
          ("within", ["--WithinAncestry"], ["PC1", "PC2"]),
          ("fixpc", ["--FixPC", "0.01:0.02"], ["ContaminatingSample.PC1", "ContaminatingSample.PC2"]),
          ("fixalpha", ["--FixAlpha", "0.05"], ["ContaminatingSample.PC1", "ContaminatingSample.PC2",
                                                  "IntendedSample.PC1", "IntendedSample.PC2"]),
          ("knownaf", None, [])]


def _cases(golden_dir, tmp_path):
    hap = os.path.join(golden_dir, "hapmap", "hapmap_3.3.b37.dat")
    yield "golden", ["--DisableSanityCheck", "--PileupFile", os.path.join(golden_dir, "expected", "result.Pileup"),
                     "--SVDPrefix", hap, "--Reference", "x.fa", "--NumPC", "2"]
    d = vb.synth.make_pileup(3000, mean_depth=30, num_pc=2, alpha_true=0.04, seed=31)
    pre = str(tmp_path / "syn")
    vb.synth.write_files(d, pre)
    yield "synthetic", ["--DisableSanityCheck", "--PileupFile", pre + ".pileup", "--SVDPrefix", pre, "--Reference",
                        "x.fa", "--NumPC", "2"]


@pytest.mark.parametrize("name,extra,pc_rows", MODELS, ids=[m[0] for m in MODELS])
def test_cli_end_to_end(golden_dir, tmp_path, name, extra, pc_rows):
    for case, base in _cases(golden_dir, tmp_path):
        args = list(base)
        if extra is None:                                  # --KnownAF: the allele frequencies from the panel's means
            kaf = str(tmp_path / (case + ".kaf"))
            vb.synth.write_known_af(args[args.index("--SVDPrefix") + 1], kaf, seed=3)
            args += ["--KnownAF", kaf]
        else:
            args += extra
        a = _run(args, str(tmp_path / (case + name + ".a")), False)
        b = _run(args, str(tmp_path / (case + name + ".b")), True)
        assert a.stdout == b.stdout
        for ext in (".selfSM", ".Ancestry"):
            assert open(str(tmp_path / (case + name + ".a")) + ext).read() == \
                open(str(tmp_path / (case + name + ".b")) + ext).read()
        assert not os.path.exists(str(tmp_path / (case + name + ".a")) + ".CI")
        assert "NOTICE - FREEMIX 95% CI (profile likelihood): [" in b.stderr
        lines = open(str(tmp_path / (case + name + ".b")) + ".CI").read().splitlines()
        assert lines[0] == "#PARAM\tESTIMATE\tSTDERR\tCI_LOW\tCI_HIGH\tMETHOD"
        rows = [ln.split("\t") for ln in lines[1:]]
        assert [r[0] for r in rows] == ["FREEMIX"] + pc_rows
        assert rows[0][5] == ("fixed" if name == "fixalpha" else "profile")
        assert all(r[5] == "wald" for r in rows[1:])
        sm = open(str(tmp_path / (case + name + ".b")) + ".selfSM").read().splitlines()
        assert rows[0][1] == sm[1].split("\t")[6]           # FREEMIX as .selfSM prints it
