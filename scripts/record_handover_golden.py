#!/usr/bin/env python3
"""Records tests/golden/handover_stores.npz: what the plans of tests/handover_cases.py return on the GPU with the
library that is loaded, bit for bit.  Run it at the commit whose results are to be kept (the parent of a change that
must not alter a bit) and pass that commit's hash:

    python3 scripts/record_handover_golden.py <commit hash> [out.npz]

Every case runs twice on fresh plans; the two runs must agree before anything is written."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import handover_cases as hc   # noqa: E402
from gpmp2_amd import engine   # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "handover_stores.npz")
    eng = engine.Engine()
    arrays, meta = {}, {"commit": commit, "raw": {}}
    for name, make in hc.cases().items():
        a, b = hc.run_case(eng, make), hc.run_case(eng, make)
        for k in hc.RESULT_KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
            arrays[f"{name}/{k}"] = a[k]
        assert a["raw"] == b["raw"], (name, a["raw"], b["raw"])
        meta["raw"][name] = a["raw"]
        print(name, "iters", list(a["iters"]), "status", list(a["status"]), "final_error", list(a["final_error"]))
        if name.startswith("planar2"):
            assert a["iters"][hc.ALREADY_OPTIMAL_ROW] == 0 and a["final_error"][hc.ALREADY_OPTIMAL_ROW] == 0.0, name
            assert (a["iters"][: hc.ALREADY_OPTIMAL_ROW] >= 1).all(), name
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
