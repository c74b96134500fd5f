"""Time of the posterior on the executed timeline on the headline problem (WAM restarts, N = 100, I = 5, Synth200,
Gauss-Newton, after optimize): Plan.risk_dev plus a wait, Plan.risk and Plan.marginals_dense against the only way to the
same answers through the entry points that existed before them: Plan.marginals to the host, the interpolation formula
in numpy, then Engine.interpolate_traj -> sphere_centers -> sdf_query and a numpy reduction.

Same process, variants alternated, every shape warmed; a window is >= --window seconds of repeated calls ended by a
device synchronise; per variant the median and min / max of the per-call time over --windows windows.  The baseline's
numpy part is timed over the first --base-rows trajectories and scaled to B, its device calls over all B; one call per
window.  Also: risk_dev minus marginals_dev (the posterior sweep is shared cost), and for k_gp_interp_cov the rate of
marginals_dense_dev minus marginals_dev over its algorithmic bytes B N (3 + J + 1) n^2 8.  One JSON line.

usage: python scripts/risk_throughput.py [--B 1 64 1024] [--J 5 9] [--kappa 3] [--window 0.5] [--windows 5] [--base-rows 8]
       python scripts/risk_throughput.py --trace     (a short run for rocprofv3 --kernel-trace --stats: no timing)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch                      # torch's HIP runtime first, as bench.py does; it owns the device outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from gpmp2_amd import engine, problems  # noqa: E402
import risk_reference as ref  # noqa: E402


def windows(variants, window, count):
    """alternates the variants; per variant the per-call seconds of `count` windows"""
    out = {name: [] for name in variants}
    for fn in variants.values():    # warm every shape
        fn()
    torch.cuda.synchronize()
    for _ in range(count):
        for name, fn in variants.items():
            calls, t0 = 0, time.perf_counter()
            while True:
                fn()
                calls += 1
                if time.perf_counter() - t0 >= window:
                    break
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / calls)
    return out


def stats(ts):
    return dict(median=round(1e3 * statistics.median(ts), 4), min=round(1e3 * min(ts), 4), max=round(1e3 * max(ts), 4),
                windows=len(ts))


def numpy_cov(Sd, So, Qc, dt, J, xx_only):
    """the interpolation formula over rows [R][N+1][n][n] in float64 -> [R][Md][n][n], or its top-left D x D blocks"""
    R, N, n = Sd.shape[0], So.shape[1], Sd.shape[2]
    D = n // 2
    I = np.eye(D)
    m = D if xx_only else n
    out = np.zeros((R, N * (J + 1) + 1, m, m))
    out[:, ::J + 1] = Sd[:, :, :m, :m]
    for j in range(1, J + 1):
        tau = j * (dt / (J + 1))
        L2, P2 = ref.gp_scalars(dt, tau, np.float64)
        L, P = np.kron(L2, I)[:m], np.kron(P2, I)[:m]
        X = P @ So @ L.T
        Q = np.kron(ref.qc_closed(dt, tau, np.float64), Qc)[:m, :m]
        out[:, j:N * (J + 1):J + 1] = L @ Sd[:, :-1] @ L.T + P @ Sd[:, 1:] @ P.T + X + np.swapaxes(X, -1, -2) + Q
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--J", type=int, nargs="+", default=[5, 9])
    ap.add_argument("--kappa", type=float, default=3.0)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--base-rows", type=int, default=8)
    ap.add_argument("--base-windows", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    eng = engine.Engine()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    cases = []
    for B in ([64] if a.trace else a.B):
        p = problems.wam_restarts(B=B, opt="GN")
        r, s = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
        N, D = p.setting.total_step, p.setting.dof
        nb, n, S = N + 1, 2 * D, r.S
        dt = p.setting.total_time / N
        Qc = np.eye(D) if p.setting.Qc is None else np.asarray(p.setting.Qc, dtype=np.float64)
        radius = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
        pl = eng.plan(r, s, p.setting, B)
        pl.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
        pl.optimize()
        traj = pl.result()["traj"]
        Sd = torch.zeros((B, nb, n, n), dtype=torch.float64, device=dev)
        So = torch.zeros((B, nb - 1, n, n), dtype=torch.float64, device=dev)
        ok = torch.zeros((B,), dtype=torch.int32, device=dev)
        rc = torch.zeros((B,), dtype=torch.float64, device=dev)
        wo = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        for J in ([5] if a.trace else a.J):
            Md = N * (J + 1) + 1
            cov = torch.zeros((B, Md, n, n), dtype=torch.float64, device=dev)

            def risk_dev():
                pl.risk_dev(J, a.kappa, rc, wo, stream=st.cuda_stream)
                st.synchronize()

            def risk_host():
                pl.risk(J, a.kappa, want_sigma=False)

            def dense_host():
                pl.marginals_dense(J)

            def dense_dev():
                pl.marginals_dense_dev(J, cov, ok, stream=st.cuda_stream)
                st.synchronize()

            def marginals_dev():
                pl.marginals_dev(Sd, So, ok, stream=st.cuda_stream)
                st.synchronize()

            if a.trace:
                for _ in range(20):
                    risk_dev()
                    dense_dev()
                continue
            rows = min(B, a.base_rows)
            base = dict(marginals=[], cov_xx=[], cov_full=[], geometry=[], reduce=[])
            c_base = None
            for _ in range(a.base_windows):
                t0 = time.perf_counter()
                m = pl.marginals()
                t1 = time.perf_counter()
                xx = numpy_cov(m["Sdiag"][:rows], m["Soff"][:rows], Qc, dt, J, True)
                t2 = time.perf_counter()
                numpy_cov(m["Sdiag"][:rows], m["Soff"][:rows], Qc, dt, J, False)
                t3 = time.perf_counter()
                up = eng.interpolate_traj(D, False, None, dt, J, traj)
                cen, Jc = eng.sphere_centers(r, np.ascontiguousarray(up[:, :, :D]).reshape(-1, D))
                dist, grad, inr = eng.sdf_query(s, cen.reshape(-1, 3))
                t4 = time.perf_counter()
                h = np.einsum("msk,mskd->msd", grad.reshape(B * Md, S, 3)[:rows * Md], Jc[:rows * Md])
                s2 = np.einsum("msa,mab,msb->ms", h, xx.reshape(rows * Md, D, D), h)
                ck = (dist.reshape(B * Md, S)[:rows * Md] - radius) - a.kappa * np.sqrt(np.maximum(s2, 0))
                ck[inr.reshape(B * Md, S)[:rows * Md] == 0] = np.inf
                c_base = ck.reshape(rows, Md * S).min(axis=1)
                t5 = time.perf_counter()
                base["marginals"].append(t1 - t0)
                base["cov_xx"].append((t2 - t1) * B / rows)
                base["cov_full"].append((t3 - t2) * B / rows)
                base["geometry"].append(t4 - t3)
                base["reduce"].append((t5 - t4) * B / rows)
            risk_dev()
            agree = float(np.abs(rc.cpu().numpy()[:rows] - c_base).max())
            assert agree < 1e-8, agree
            t = windows({"risk_dev": risk_dev, "risk": risk_host, "marginals_dense": dense_host,
                         "marginals_dense_dev": dense_dev, "marginals_dev": marginals_dev}, a.window, a.windows)
            b_risk = [w + x + y + z for w, x, y, z in zip(base["marginals"], base["cov_xx"], base["geometry"], base["reduce"])]
            b_dense = [w + x for w, x in zip(base["marginals"], base["cov_full"])]
            row = dict(B=B, N=N, J=J, dof=D, checked_states=Md, spheres=S, agreement=float(f"{agree:.3g}"),
                       baseline_rows_timed=rows, **{k + "_ms": stats(v) for k, v in t.items()},
                       baseline_risk_ms=stats(b_risk), baseline_dense_ms=stats(b_dense),
                       baseline_parts_ms={k: stats(v) for k, v in base.items()})
            med = lambda k: row[k + "_ms"]["median"]
            for k, bk in (("risk_dev", "baseline_risk"), ("risk", "baseline_risk"), ("marginals_dense", "baseline_dense")):
                row[k + "_accepted"] = bool(med(k) < row[bk + "_ms"]["min"])
                row[k + "_speedup"] = round(row[bk + "_ms"]["median"] / med(k), 1)
            row["risk_dev_minus_marginals_dev_ms"] = round(med("risk_dev") - med("marginals_dev"), 4)
            interp_ms = med("marginals_dense_dev") - med("marginals_dev")
            row["interp_cov_ms_by_difference"] = round(interp_ms, 4)
            row["interp_cov_algorithmic_bytes"] = B * N * (3 + J + 1) * n * n * 8
            row["interp_cov_GBps_by_difference"] = (round(row["interp_cov_algorithmic_bytes"] / (interp_ms * 1e-3) / 1e9, 1)
                                                    if interp_ms > 0 else None)
            cases.append(row)
            del cov
        pl.close()
    if not a.trace:
        print(json.dumps(dict(script="risk_throughput", problem="wam_restarts N=100 I=5 Synth200 GN", kappa=a.kappa,
                              window_s=a.window, cases=cases)))


if __name__ == "__main__":
    main()
