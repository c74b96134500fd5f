#!/usr/bin/env python3
"""Records tests/golden/linearize_tail.npz: what the plans of tests/linearize_tail_cases.py return on the GPU with the
library that is loaded, bit for bit -- one linearization at the initial trajectories (g and err as values, Hdiag and
Hoff as SHA-256), a whole optimize (tests/handover_cases.run_case) and, for the cases named there, a fixed-iteration
plan.  Run it at the commit whose results are to be kept (the parent of a change that must not alter a bit) and pass
that commit's hash:

    python3 scripts/record_linearize_tail_golden.py <commit hash> [out.npz]

Every case runs twice on fresh plans; the two runs must agree before anything is written."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import handover_cases as hc   # noqa: E402
import linearize_tail_cases as lc   # noqa: E402
from gpmp2_amd import engine   # noqa: E402


def twice(run, eng, make, name):
    a, b = run(eng, make), run(eng, make)
    for k in a:
        same = a[k] == b[k] if isinstance(a[k], dict) else a[k].tobytes() == b[k].tobytes()
        assert same, (name, k)
    return a


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "linearize_tail.npz")
    eng = engine.Engine()
    arrays, meta = {}, {"commit": commit, "raw": {}, "lin_digest": {}, "update_raw": {}}
    for name, make in lc.cases().items():
        lin = twice(lc.run_linearize, eng, make, name)
        for k in lc.LIN_VALUE_KEYS:
            arrays[f"{name}/{k}"] = lin[k]
        meta["lin_digest"][name] = lin["lin_digest"]
        assert lin["lin_err"][lc.ALREADY_OPTIMAL_ROW] == 0.0 and (lin["lin_err"][: lc.ALREADY_OPTIMAL_ROW] > 0.0).all(), name
        a = twice(hc.run_case, eng, make, name)
        for k in lc.RESULT_KEYS:
            arrays[f"{name}/{k}"] = a[k]
        meta["raw"][name] = a["raw"]
        print(name, "iters", list(a["iters"]), "status", list(a["status"]), "final_error", list(a["final_error"]))
        assert a["iters"][lc.ALREADY_OPTIMAL_ROW] == 0 and a["final_error"][lc.ALREADY_OPTIMAL_ROW] == 0.0, name
        assert (a["iters"][: lc.ALREADY_OPTIMAL_ROW] >= 1).all(), name
        if name in lc.UPDATE_CASES:
            u = twice(lc.run_update, eng, make, name)
            for k in lc.RESULT_KEYS:
                arrays[f"{name}/update/{k}"] = u[k]
            meta["update_raw"][name] = u["raw"]
            print(name, "update: iters", list(u["iters"]), "final_error", list(u["final_error"]))
    arrays["meta"] = np.array(json.dumps(meta, sort_keys=True))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
