"""--ConfidenceInterval without a GPU: the new struct's layout against its ctypes mirror, and the command line's refusals
of what the interval does not serve (cohorts, marker shards) before any file is read or any device call is made."""
import ctypes as C
import os
import subprocess

from verifybamid_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "verifybamid_amd", "bin", "VerifyBamID")


def test_interval_struct_layout_matches_the_binding(tmp_path):
    fields = [f for f, _ in _abi.Interval._fields_]
    src = tmp_path / "ci_check.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vb2_abi.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(vb2_interval));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(vb2_interval, %s));\n' % (f, f) for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "ci_check"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_abi.Interval)
    for f in fields:
        assert int(got[f]) == getattr(_abi.Interval, f).offset, f
    for name in ("vb2_ctx_interval", "vb2_run_interval"):
        assert name in _abi.SYMBOLS and hasattr(_abi.lib(), name)


def _refused(tmp_path, extra):
    # no panel, pileup or list file exists: a refusal that came after reading one would name the missing file
    cmd = [EXE, "--ConfidenceInterval", "--SVDPrefix", str(tmp_path / "nopanel"), "--Reference", "x.fa",
           "--Output", str(tmp_path / "o")] + extra
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode != 0
    assert "FATAL ERROR" in p.stderr
    assert not (tmp_path / "o.CI").exists()
    return p.stderr


def test_cli_refuses_a_pileup_list(tmp_path):
    err = _refused(tmp_path, ["--PileupList", str(tmp_path / "list.txt")])
    assert "--ConfidenceInterval cannot be combined with --PileupList" in err
    assert "cannot open --PileupList" not in err


def test_cli_refuses_several_devices(tmp_path):
    err = _refused(tmp_path, ["--PileupFile", str(tmp_path / "s.pileup"), "--Devices", "0,1"])
    assert "--ConfidenceInterval cannot be combined with more than one --Devices" in err
    assert "NOTICE - Starting phase" not in err
