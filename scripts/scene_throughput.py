"""Time of one update of the 200^3 map from a scene (include/gpmp2mi.h "scene") against the only way there is without it.

Scene: a table (box), four more primitives (a rotated box, a sphere, two cylinders) and one generated closed mesh of
20 480 triangles (an icosphere, rotated), on the grid of the headline map: 200^3 cells of 0.01 m from (-1, -1, -1).
  - gpmp2mi_sdf_update_from_scene: the host form by a host clock (it ends in a device synchronise), and its stages in
    device time from the library's two stage timers: seed, primitives, meshes (quantize + cross + fill), the three axis
    passes, finish, pack.  The whole update in device time is the sum of the stages (the events are contiguous).
  - the host path: the same mask painted into a float64 occupancy array on the host and given to
    gpmp2mi_sdf_update_from_occupancy, upload of 8 B a cell included, by the same host clock.  The primitives are painted
    with numpy over their bounding boxes.  The mesh has no host voxeliser to be timed: its cells are taken from
    gpmp2mi_scene_rasterize beforehand and only copied in, so the host path's time is a LOWER bound.
The two routes must leave the same field, bit for bit; the script fails otherwise.  Warm-up calls first, then `reps` timed
calls; median, min and max are reported.

usage: python scripts/scene_throughput.py [--reps 20] [--out profiles/scene_throughput.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, ORIGIN, CELL = 200, (-1.0, -1.0, -1.0), 0.01


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_objects(S):
    v, t = S.icosphere_mesh(0.3, 5)
    return [S.Box([0.7, 0.5, 0.03], S.pose_of(t=(0.0, 0.0, -0.4))),                       # the table
            S.Box([0.2, 0.1, 0.15], S.pose_of(rot((0.2, 0.1, 1.0), 0.6), (0.4, -0.3, -0.2))),
            S.Sphere(0.12, (-0.5, 0.4, 0.1)),
            S.Cylinder(0.04, 0.45, S.pose_of(t=(0.55, 0.4, 0.05))),                       # a post
            S.Cylinder(0.08, 0.3, S.pose_of(rot((1.0, 0.0, 0.0), 1.2), (-0.4, -0.5, 0.3))),
            S.Mesh(v, t, S.pose_of(rot((0.3, -0.5, 0.8), 0.7), (0.0, 0.1, 0.25)))]


def paint_primitives(occ, objs):
    """what a user writes today: each primitive tested with numpy over its bounding box of cells"""
    o = np.asarray(ORIGIN)
    for b in objs:
        if b.vertices is not None:
            continue
        s = b.size + b.inflate
        R, t = b.pose[:, :3], b.pose[:, 3]
        r = s[0] if b.kind == 1 else np.linalg.norm(s)
        lo = np.clip(np.floor((t - r - o) / CELL).astype(int) - 1, 0, N)
        hi = np.clip(np.ceil((t + r - o) / CELL).astype(int) + 2, 0, N)
        ax = [o[a] + np.arange(lo[a], hi[a]) * CELL - t[a] for a in range(3)]
        d = [ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]]
        if b.kind == 1:
            hit = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= s[0]
        else:
            l = [(R[0, m] * d[0] + R[1, m] * d[1]) + R[2, m] * d[2] for m in range(3)]
            hit = ((np.abs(l[0]) <= s[0]) & (np.abs(l[1]) <= s[1]) & (np.abs(l[2]) <= s[2])) if b.kind == 0 else \
                  ((np.sqrt(l[0] * l[0] + l[1] * l[1]) <= s[0]) & (np.abs(l[2]) <= s[1]))
        occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]][hit] = 1.0


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_throughput.txt"))
    a = ap.parse_args()
    from gpmp2_amd import engine, scene as S
    eng = engine.Engine()
    objs = make_objects(S)
    sc = eng.scene(objs)
    shape = (N, N, N)
    s = eng.sdf(ORIGIN, CELL, np.zeros(shape))
    eng.sdf_reserve_update(s)
    sc.reserve(shape)
    eng.sdf_update_timing(s, True)
    eng.scene_timing(sc, True)
    mesh_only = eng.scene([objs[-1]])
    mesh_mask, mesh_cells = mesh_only.rasterize(ORIGIN, CELL, shape)
    mesh_idx = np.nonzero(mesh_mask)

    wall, stages = [], {k: [] for k in ("seed", "primitives", "meshes", "passes", "finish", "pack")}
    cells = None
    for k in range(3 + a.reps):                   # the first three warm: code objects, the workspaces, the caches
        t0 = time.perf_counter()
        cells = eng.sdf_update_from_scene(s, sc)
        dt = 1e3 * (time.perf_counter() - t0)
        if k < 3:
            continue
        wall.append(dt)
        u, r = eng.sdf_update_timing(s, True, read=True), eng.scene_timing(sc, True, read=True)
        stages["seed"].append(u["seed_mark"] - r["primitives"] - r["meshes"])
        for name in ("primitives", "meshes"):
            stages[name].append(r[name])
        for name in ("passes", "finish", "pack"):
            stages[name].append(u[name])
    device = [sum(stages[k][i] for k in stages) for i in range(a.reps)]
    scene_field = eng.sdf_field(s)["data"]

    host_wall, host_paint, host_update, occ_stages = [], [], [], []
    agree = True
    for k in range(2 + a.reps):
        t0 = time.perf_counter()
        occ = np.zeros(shape)
        paint_primitives(occ, objs)
        occ[mesh_idx] = 1.0
        t1 = time.perf_counter()
        eng.sdf_update_from_occupancy(s, occ)     # upload included
        t2 = time.perf_counter()
        if k == 0:
            agree = bool(np.array_equal(eng.sdf_field(s)["data"].view(np.int64), scene_field.view(np.int64)))
        if k < 2:
            continue
        host_wall.append(1e3 * (t2 - t0))
        host_paint.append(1e3 * (t1 - t0))
        host_update.append(1e3 * (t2 - t1))
        occ_stages.append(sum(eng.sdf_update_timing(s, True, read=True).values()))

    med = {k: statistics.median(v) for k, v in stages.items()}
    transform = med["passes"] + med["finish"] + med["pack"]
    row = dict(case="200^3 map; table + 4 primitives + icosphere of 20480 triangles", cells=N ** 3,
               object_cells=[int(x) for x in cells], occupied=int(sum(max(int(x), 0) for x in cells)), reps=a.reps,
               agrees_with_host_path=agree,
               update_from_scene_host_form_wall_ms=summary(wall), update_from_scene_device_ms=summary(device),
               stage_ms={k: summary(v) for k, v in stages.items()},
               distance_transform_share=round(transform / statistics.median(device), 4),
               host_path_wall_ms=summary(host_wall), host_path_paint_ms=summary(host_paint),
               host_path_upload_and_update_ms=summary(host_update), host_path_update_device_ms=summary(occ_stages),
               host_path="numpy paint of the primitives, mesh cells copied in (no host voxeliser timed: a lower bound), "
                         "gpmp2mi_sdf_update_from_occupancy with the 64 MB upload")
    lines = [
        "scene throughput (scripts/scene_throughput.py): one update of the 200^3 map, median [min .. max] ms over "
        f"{a.reps} calls after warm-up",
        f"  objects: table, box, sphere, 2 cylinders, icosphere mesh (20480 triangles); cells {row['object_cells']}",
        f"  gpmp2mi_sdf_update_from_scene, host form, host clock     {fmt(row['update_from_scene_host_form_wall_ms'])}",
        f"  gpmp2mi_sdf_update_from_scene, device time (all stages)  {fmt(row['update_from_scene_device_ms'])}",
    ] + [f"    stage {k:<11s} {fmt(row['stage_ms'][k])}" for k in stages] + [
        f"  share of the unchanged distance transform (passes + finish + pack) in the device time: "
        f"{100 * row['distance_transform_share']:.1f} %",
        f"  host path (paint + upload + update_from_occupancy), host clock   {fmt(row['host_path_wall_ms'])}",
        f"    numpy paint (mesh cells copied, not voxelised)          {fmt(row['host_path_paint_ms'])}",
        f"    upload + gpmp2mi_sdf_update_from_occupancy              {fmt(row['host_path_upload_and_update_ms'])}",
        f"    of which device time of the update                      {fmt(row['host_path_update_device_ms'])}",
        f"  the two routes leave the same field bit for bit: {agree}",
        json.dumps(row),
    ]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return 0 if agree else 1


def fmt(s):
    return f"{s['median']:9.3f} [{s['min']:.3f} .. {s['max']:.3f}]"


if __name__ == "__main__":
    sys.exit(main())
