#!/usr/bin/env python3
"""Records tests/golden/pass_heads.npz: what the runs of tests/pass_heads_cases.py return on the GPU with the library
that is loaded, bit for bit, and the launch counts their timing reports.  Run it at the commit whose results are to be
kept (the parent of a change that must not alter a bit) and pass that commit's hash:

    python3 scripts/record_pass_heads_golden.py <commit hash> [out.npz]

Every case runs twice on fresh plans; the two runs must agree before anything is written."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pass_heads_cases as pc   # noqa: E402
from gpmp2_amd import engine   # noqa: E402


def main():
    commit = sys.argv[1]
    assert len(commit) == 40, "pass the full commit hash"
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "pass_heads.npz")
    eng = engine.Engine()
    arrays, meta = {}, {"commit": commit, "launches": {}}
    for name, run in pc.cases().items():
        a, b = run(eng), run(eng)
        for k in pc.RESULT_KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
            arrays[f"{name}/{k}"] = a[k]
        assert a["launches"] == b["launches"], (name, a["launches"], b["launches"])
        meta["launches"][name] = a["launches"]
        print(name, "iters", list(a["iters"][:8]), "status", list(a["status"][:8]), "launches", a["launches"], flush=True)
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
