"""Time of one depth frame integrated into a field handle's evidence (include/gpmp2mi.h "sensor map") against the two
routes that existed before it.

Setup, the live-map configuration of DESIGN.md: the 200^3 synthetic map of problems.synth200_sdf() as the base (its
obstacle set, field < 0), one 640 x 480 depth frame of that scene from a camera inside the map (rendered here by marching
the base along every pixel's ray; pixels that see nothing within depth_max carve up to it, one pixel in a hundred is a
drop-out), and the WAM self filter.  Timed by device events on a non-default stream, 5 warm-up calls, medians of --reps:
  - sdf_integrate_depth_dev: the whole call, and its stages from the library's stage timer (deproject and classify, walk,
    apply + seed, the three axis passes, finish, pack);
  (a) sdf_update_from_points_dev on the frame's end points: what carving costs over marking alone;
  (b) the route a user has today, by a host clock around calls that end in a device synchronise: the numpy walk of
      tests/sensor_reference.py on the host into an occupancy volume, then sdf_update_from_occupancy (64 MB uploaded).
The map of (b) must equal the map of the first integrate call bit for bit; the script fails otherwise.

Steps per ray and bytes of marks are computed from the shapes (the walk lengths the rule gives, an upper bound on what
the kernel does: it leaves a ray that cannot come back to the grid), not read from a counter.

usage: python scripts/sensor_throughput.py [--reps 30] [--baseline-reps 1] [--out profiles/sensor_throughput.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H = 640, 480
MARGIN = 0.02
STAGES = ("deproject", "walk", "apply_seed", "passes", "finish", "pack")
MAP_STAGES = ("seed_mark", "passes", "finish", "pack")


def look_at(position, target):
    """camera -> world [3][4]: the optical axis (camera z) from position to target, camera x level"""
    z = np.asarray(target, dtype=np.float64) - np.asarray(position, dtype=np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], axis=1), np.asarray(position, dtype=np.float64)[:, None]], axis=1)


def render_depth(occ, origin, cell, cam, seed=1):
    """[H][W] float32: the depth at which each pixel's ray first meets an obstacle cell of occ, marched a cell at a time;
    10 m (beyond depth_max) where it meets none; NaN for one pixel in a hundred"""
    P = np.asarray(cam["pose"])
    v, u = np.divmod(np.arange(W * H), W)
    d = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones(W * H)], axis=1) @ P[:, :3].T
    depth = np.full(W * H, 10.0)
    live = np.arange(W * H)
    n = np.asarray(occ.shape[::-1])
    z = cam["depth_min"]
    while z < cam["depth_max"] and len(live):
        idx = np.floor((P[:, 3][None] + z * d[live] - np.asarray(origin)[None]) / cell + 0.5).astype(np.int64)
        inside = ((idx >= 0) & (idx < n[None])).all(axis=1)
        met = np.zeros(len(live), dtype=bool)
        met[inside] = occ[idx[inside, 2], idx[inside, 1], idx[inside, 0]] > 0.5
        depth[live[met]] = z
        live = live[~met]
        z += cell
    depth[np.random.default_rng(seed).integers(0, W * H, W * H // 100)] = np.nan
    return depth.reshape(H, W).astype(np.float32)


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--baseline-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_throughput.json"))
    a = ap.parse_args()
    import torch                      # torch's HIP runtime first, as bench.py does
    torch.cuda.init()
    import sensor_reference as sr
    from gpmp2_amd import engine, problems
    eng = engine.Engine()
    p = problems.wam_restarts(B=1, total_step=10, obs_check_inter=1)
    origin, cell, field = p.sdf_origin, float(p.sdf_cell), np.asarray(p.sdf_data)
    n = field.shape[::-1]
    occ = (field < 0.0).astype(np.float64)
    r = eng.robot(p.model)
    conf = problems.WAM_START.copy()
    centers = eng.sphere_centers(r, conf)[0][0]
    radii = np.asarray(p.model.flat()["sphere_radius"], dtype=np.float64)
    cam = dict(width=W, height=H, fx=525.0, fy=525.0, cx=319.5, cy=239.5, depth_min=0.05, depth_max=2.5,
               pose=look_at([-0.85, -0.8, 0.7], [0.1, 0.1, -0.1]))
    depth = render_depth(occ, origin, cell, cam)
    opts = dict(use_base=True)
    ro = sr.options(**opts)
    E0 = np.zeros(field.shape, dtype=np.int16)

    # the frame as the rules see it: classes, walk lengths, end points
    z64 = depth.astype(np.float64).reshape(-1)
    cls, ca, cb, ends = sr.classify(n, origin, cell, sr.camera_origin(cam), sr.deproject(cam, z64), z64, cam, centers, radii,
                                    MARGIN)
    carve = cls != sr.INVALID
    steps = np.abs(np.floor(cb[carve]) - np.floor(ca)[None]).sum(axis=1)
    end_points = np.where((cls == sr.INVALID)[:, None], np.nan, ends)

    s = eng.sdf(origin, cell, field)
    dev = torch.device("cuda:0")
    t_occ, t_depth, t_conf, t_pts = (torch.from_numpy(x).to(dev) for x in (occ, depth, conf, np.ascontiguousarray(end_points)))
    t_stats, t_stats4 = torch.zeros(6, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    eng.sdf_reserve_update(s)
    eng.sdf_reserve_evidence(s)
    eng.sdf_integrate_timing(s, True)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)

    def integrate():
        eng.sdf_integrate_depth_dev(s, cam, t_depth, r, t_conf, MARGIN, t_stats, stream=st.cuda_stream, **opts)

    def from_points():
        eng.sdf_update_from_points_dev(s, W * H, t_pts, True, r, t_conf, MARGIN, t_stats4, stream=st.cuda_stream)

    def timed(fn, reps, read, names):
        whole, stages = [], {k: [] for k in names}
        for _ in range(5):            # warm-up: code objects, the workspaces, the caches
            fn()
        st.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            whole.append(e0.elapsed_time(e1))
            for k, v in read(s, True, read=True).items():
                stages[k].append(v)
        return whole, stages

    eng.sdf_update_from_occupancy_dev(s, t_occ, stream=st.cuda_stream)       # the base
    integrate()                                                             # the first frame on zero evidence
    st.synchronize()
    stats = dict(zip(eng.EVIDENCE_STATS, (int(x) for x in t_stats.cpu().numpy())))
    first_field, first_E = eng.sdf_field(s)["data"], eng.sdf_evidence(s)

    # (b) the host route, once per rep: numpy walk -> occupancy -> update_from_occupancy on a second handle
    s2 = eng.sdf(origin, cell, field)
    host_ms, walk_ms, agree = [], [], True
    for _ in range(a.baseline_reps):
        t0 = time.perf_counter()
        E1, ref_stats = sr.integrate_depth(E0, n, origin, cell, cam, depth, ro, centers, radii, MARGIN, batch=True)
        t1 = time.perf_counter()
        eng.sdf_update_from_occupancy(s2, sr.occupied_set(E1, ro["occupied_at"], occ))
        t2 = time.perf_counter()
        host_ms.append(1e3 * (t2 - t0))
        walk_ms.append(1e3 * (t1 - t0))
        agree = agree and bool(np.array_equal(E1, first_E) and ref_stats == stats and
                               np.array_equal(eng.sdf_field(s2)["data"].view(np.int64), first_field.view(np.int64)))
    s2.close()

    int_whole, int_stages = timed(integrate, a.reps, eng.sdf_integrate_timing, STAGES)
    pts_whole, pts_stages = timed(from_points, a.reps, eng.sdf_update_timing, MAP_STAGES)
    passes = statistics.median(int_stages["passes"])
    walk = statistics.median(int_stages["walk"])
    cells = field.size
    row = dict(case="synth200 as base + one 640x480 depth frame from inside the map, WAM self filter", cells=cells,
               rays=W * H, stats=stats, margin=MARGIN, reps=a.reps, agrees_with_host_route=agree,
               integrate_depth_dev_ms=summary(int_whole), integrate_stage_ms={k: summary(v) for k, v in int_stages.items()},
               update_from_points_dev_ms=summary(pts_whole),
               update_from_points_stage_ms={k: summary(v) for k, v in pts_stages.items()},
               host_route_ms=summary(host_ms), host_route_walk_ms=summary(walk_ms), host_route_reps=a.baseline_reps,
               host_route="numpy walk of tests/sensor_reference.py (batched) -> occupancy -> sdf_update_from_occupancy",
               walk_over_three_passes=round(walk / passes, 3),
               estimated_from_shapes=dict(steps_per_ray_mean=round(float(steps.mean()), 1), steps_per_ray_max=int(steps.max()),
                                          mark_bytes_stored=int(steps.sum() + (cls == sr.HIT).sum()),
                                          apply_seed_bytes=int(cells * (2 + 2 + 1 + 8)), ray_record_bytes=28 * W * H))
    line = json.dumps(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    med = lambda d, k: statistics.median(d[k])
    print("| measured, ms | whole call | deproject | walk | apply + seed | three passes | finish | pack |")
    print("|---|---|---|---|---|---|---|---|")
    print("| `gpmp2mi_sdf_integrate_depth_dev` | %.3f | %s |" % (statistics.median(int_whole),
                                                                " | ".join("%.3f" % med(int_stages, k) for k in STAGES)))
    print("| (a) `gpmp2mi_sdf_update_from_points_dev` | %.3f | - | - | %.3f (seed + mark) | %.3f | %.3f | %.3f |" % (
        statistics.median(pts_whole), med(pts_stages, "seed_mark"), med(pts_stages, "passes"), med(pts_stages, "finish"),
        med(pts_stages, "pack")))
    print("| (b) host walk + `gpmp2mi_sdf_update_from_occupancy` | %.1f (walk %.1f) | | | | | | |" % (
        statistics.median(host_ms), statistics.median(walk_ms)))
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
