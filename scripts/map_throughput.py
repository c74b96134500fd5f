"""Time of a live-map update (include/gpmp2mi.h "live map") against the route that gives the same answer without it.

Setup: the 200^3 synthetic map of problems.synth200_sdf() as the base (its obstacle set, field < 0), a cloud of 307 200
points (one 640 x 480 frame: the static scene seen again, a new box, the robot's own arm, a few stray and non-finite
points) and the WAM self filter.  Timed by device events on a non-default stream, every shape warmed first:
  - sdf_update_from_points_dev: the whole call, and its stages from the library's stage timer (seed + mark, the three
    axis passes, finish, pack);
  - sdf_update_from_occupancy_dev: the same.
Baseline, by a host clock around calls that end in a device synchronise: numpy voxelisation and filtering on the host,
gpmp2mi_sdf_create_from_occupancy, and a new gpmp2mi_plan_create of the headline plan (WAM restarts, B = 64, N = 100).
The two routes must leave the same field, bit for bit; the script fails otherwise.

The bytes per stage are the ones the algorithm needs, computed from the shapes (an estimate of the traffic, not a
counter): the rates are those bytes over the measured time.

usage: python scripts/map_throughput.py [--reps 30] [--baseline-reps 3] [--out profiles/map_throughput.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAME = 640 * 480
MARGIN = 0.02
STAGES = ("seed_mark", "passes", "finish", "pack")


def frame_cloud(occ, origin, cell, centers, radii, seed=1):
    """FRAME points [M][3]: 70 % on obstacle cells of the map, 12 % on a new 20^3-cell box, 15 % in the robot's body
    spheres, the rest beyond the grid or non-finite"""
    rng = np.random.default_rng(seed)
    o = np.asarray(origin, dtype=np.float64)
    n_scene, n_box, n_self = int(0.70 * FRAME), int(0.12 * FRAME), int(0.15 * FRAME)
    zyx = np.argwhere(occ > 0.5)
    pick = zyx[rng.integers(0, len(zyx), n_scene)][:, ::-1].astype(np.float64)
    scene = o + (pick + rng.uniform(-0.45, 0.45, size=pick.shape)) * cell
    box = o + (np.array([150.0, 40.0, 120.0]) + rng.uniform(0.0, 20.0, size=(n_box, 3))) * cell
    k = rng.integers(0, len(radii), n_self)
    d = rng.normal(size=(n_self, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    body = centers[k] + d * (radii[k] * rng.uniform(0.5, 1.0, n_self))[:, None]
    rest = rng.uniform(-3.0, 3.0, size=(FRAME - n_scene - n_box - n_self, 3))
    rest[::7, 2] = np.nan
    rest[3::11, 0] = np.inf
    pts = np.concatenate([scene, box, body, rest])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def host_route(eng, occ_base, pts, origin, cell, centers, radii, r, p):
    """what a caller does today for the same map: voxelise and filter in numpy, a new field handle, a new plan"""
    n = np.asarray(occ_base.shape[::-1], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(pts).all(axis=1)
        d = pts[:, None, :] - centers[None, :, :]
        own = (np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) <= (radii + MARGIN)[None]).any(axis=1)
        u = (pts - np.asarray(origin)[None]) / cell + 0.5
        inside = ((u >= 0.0) & (u < n[None])).all(axis=1)
    keep = finite & ~own & inside
    idx = np.floor(u[keep]).astype(np.int64)
    occ = occ_base.copy()
    occ[idx[:, 2], idx[:, 1], idx[:, 0]] = 1.0
    s = eng.sdf_from_occupancy(origin, cell, occ)
    pl = eng.plan(r, s, p.setting, p.B)
    stats = dict(kept=int(keep.sum()), non_finite=int((~finite).sum()), self=int((finite & own).sum()),
                 outside=int((finite & ~own & ~inside).sum()))
    return s, pl, stats


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_throughput.json"))
    a = ap.parse_args()
    import torch                      # torch's HIP runtime first, as bench.py does
    torch.cuda.init()
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    p = problems.wam_restarts(B=64, total_step=100, obs_check_inter=5)
    origin, cell, field = p.sdf_origin, p.sdf_cell, np.asarray(p.sdf_data)
    occ = (field < 0.0).astype(np.float64)
    r = eng.robot(p.model)
    conf = problems.WAM_START.copy()
    centers = eng.sphere_centers(r, conf)[0][0]
    radii = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
    pts = frame_cloud(occ, origin, cell, centers, radii)
    s = eng.sdf(origin, cell, field)
    dev = torch.device("cuda:0")
    t_occ, t_pts, t_conf = (torch.from_numpy(x).to(dev) for x in (occ, pts, conf))
    t_stats = torch.zeros(4, dtype=torch.int32, device=dev)
    eng.sdf_reserve_update(s)
    eng.sdf_update_timing(s, True)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)

    def from_points():
        eng.sdf_update_from_points_dev(s, FRAME, t_pts, True, r, t_conf, MARGIN, t_stats, stream=st.cuda_stream)

    def from_occupancy():
        eng.sdf_update_from_occupancy_dev(s, t_occ, stream=st.cuda_stream)

    def timed(fn, reps):
        whole, stages = [], {k: [] for k in STAGES}
        for _ in range(5):            # warm-up: code objects, the workspace, the caches
            fn()
        st.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            whole.append(e0.elapsed_time(e1))
            for k, v in eng.sdf_update_timing(s, True, read=True).items():
                stages[k].append(v)
        return whole, stages

    from_occupancy()                  # the base
    st.synchronize()
    occ_whole, occ_stages = timed(from_occupancy, a.reps)
    pts_whole, pts_stages = timed(from_points, a.reps)
    stats = dict(zip(("kept", "non_finite", "self", "outside"), (int(x) for x in t_stats.cpu().numpy())))
    live_field = eng.sdf_field(s)["data"]

    base_ms, agree = [], True
    for k in range(a.baseline_reps + 1):           # the first one warms
        t0 = time.perf_counter()
        s2, pl2, stats2 = host_route(eng, occ, pts, origin, cell, centers, radii, r, p)
        dt = 1e3 * (time.perf_counter() - t0)
        if k:
            base_ms.append(dt)
        else:
            agree = bool(np.array_equal(eng.sdf_field(s2)["data"], live_field) and stats2 == stats)
        pl2.close()
        s2.close()

    n = field.size
    bytes_ = dict(seed_mark=9 * n + 24 * FRAME, passes=48 * n, finish=16 * n, pack=72 * n)
    row = dict(case="synth200 + one 640x480 frame, WAM self filter", cells=n, points=FRAME, stats=stats, margin=MARGIN,
               reps=a.reps, agrees_with_host_route=agree,
               update_from_points_dev_ms=summary(pts_whole), update_from_occupancy_dev_ms=summary(occ_whole),
               from_points_stage_ms={k: summary(v) for k, v in pts_stages.items()},
               from_occupancy_stage_ms={k: summary(v) for k, v in occ_stages.items()},
               algorithmic_bytes=bytes_,
               from_points_stage_GBps={k: round(bytes_[k] / (1e6 * statistics.median(v)), 1) for k, v in pts_stages.items()},
               host_route_ms=summary(base_ms), host_route_reps=a.baseline_reps,
               host_route="numpy voxelise + filter, sdf_create_from_occupancy, plan_create (B = 64, N = 100)")
    line = json.dumps(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
