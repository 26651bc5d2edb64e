#!/usr/bin/env python
"""Records tests/golden/run_notices.json: what the single-sample entry points print and write on the bundled golden input
(tests/test_run_pipeline_gpu.py: record), on a machine with the device.

    python tests/golden/make_run_notices.py [out.json]      # default: tests/golden/run_notices.json
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_run_pipeline_gpu as t  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        out = t.record(tmp)
    with open(sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
