#!/usr/bin/env python3
"""Kernel boundaries of the Gauss-Newton fast path from a rocprofv3 --kernel-trace CSV of bench.py: for every pass of a
step (linearize -> assemble -> gn_step_cr, then the next pass's linearize) the predecessor's duration and the gap from
its end to the successor's start, as medians over the steps of the run.  Early passes have every trajectory live, late
ones a few: a write-back of the predecessor's dirty lines at the boundary would show as early - late.

usage: python3 scripts/probes/handover_boundary.py kernel_trace.csv [steps to skip, default 5]"""
import csv
import statistics as st
import sys

KIND = (("k_linearize", "L"), ("k_assemble", "A"), ("k_gn_step_cr", "S"))


def kind(name):
    for key, k in KIND:
        if key in name:
            return k
    return None


def main():
    rows = []
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    seq = [(s, e, kind(n)) for s, e, n in rows]
    # a step: passes L A S ... closed by a linearize that no assemble follows
    steps, cur, i = [], [], 0
    while i + 2 < len(seq):
        a, b, c = seq[i], seq[i + 1], seq[i + 2]
        if (a[2], b[2], c[2]) == ("L", "A", "S"):
            nxt = seq[i + 3] if i + 3 < len(seq) else None
            cur.append((a, b, c, nxt if nxt and nxt[2] == "L" else None))
            i += 3
        else:
            if cur:
                steps.append(cur)
                cur = []
            i += 1
    if cur:
        steps.append(cur)
    steps = [s for s in steps if len(s) >= 2][skip:]
    npass = max(len(s) for s in steps)
    print(f"{len(steps)} steps, up to {npass} passes; microseconds, median over steps [min .. max]")
    print("pass  n | dur L   gap L->A       | dur A   gap A->S       | dur S   gap S->L")
    med = lambda v: st.median(v) if v else float("nan")
    table = []
    for p in range(npass):
        col = {k: [] for k in ("dL", "gLA", "dA", "gAS", "dS", "gSL")}
        for s in steps:
            if p >= len(s):
                continue
            L, A, S, N = s[p]
            col["dL"].append((L[1] - L[0]) / 1e3); col["gLA"].append((A[0] - L[1]) / 1e3)
            col["dA"].append((A[1] - A[0]) / 1e3); col["gAS"].append((S[0] - A[1]) / 1e3)
            col["dS"].append((S[1] - S[0]) / 1e3)
            if N:
                col["gSL"].append((N[0] - S[1]) / 1e3)
        g = lambda k: f"{med(col[k]):5.2f} [{min(col[k]):4.2f}..{max(col[k]):5.2f}]" if col[k] else "  -"
        print(f"{p + 1:4d} {len(col['dL']):2d} | {med(col['dL']):5.1f}  {g('gLA')} | {med(col['dA']):5.1f}  {g('gAS')} | "
              f"{med(col['dS']):5.1f}  {g('gSL')}")
        table.append({k: med(v) for k, v in col.items()})
    wall = [(s[-1][3] or s[-1][2])[1] - s[0][0][0] for s in steps]
    print(f"first linearize start -> last kernel end of a step: median {med(wall) / 1e3:.1f} us")
    for k in ("gLA", "gAS", "gSL", "dL", "dA", "dS"):
        early = st.mean(t[k] for t in table[:3])
        late = st.mean(t[k] for t in table[-3:] if t[k] == t[k])
        print(f"{k}: passes 1-3 {early:.2f} us, last three {late:.2f} us, early - late {early - late:+.2f} us")


if __name__ == "__main__":
    main()
