#!/usr/bin/env python3
"""Known geometry as a planning scene (include/gpmp2mi.h "scene"): the 7-DOF WAM arm plans over a table (a box), past a
post (a cylinder) and around a closed triangle mesh.  The objects are rasterised on the device into the obstacle set of
the field -- no occupancy array is painted on the host and nothing of 8 B a cell is uploaded.  Then the mesh moves: one
set_poses, one update_from_scene, and the same plan, bound to the same field handle, is solved again.  Runs on an
MI355X; there is no CPU path."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpmp2_amd as g
from gpmp2_amd import engine
from gpmp2_amd.scene import Box, Cylinder, Mesh, Scene, icosphere_mesh, pose_of

# ---- the map: 150^3 cells of 1 cm around the arm, empty to begin with
n, cell, origin = 150, 0.01, [-0.75, -0.75, -0.55]
sdf = g.SignedDistanceField(origin, cell, n, n, n)
for z in range(n):
    sdf.initFieldData(z, np.full((n, n), 1000.0))

# ---- robot, settings and restarts (examples/wam_planner.py)
arm = g.generateArm("WAMArm")
start_conf = np.array([-0.8, -1.70, 1.64, 1.29, 1.1, -0.106, 2.2])
end_conf = np.array([-0.0, 0.94, 0, 1.6, 0, -0.919, 1.55])
zero = np.zeros(7)
total_time_sec, total_time_step, B = 2.0, 10, 16
opt_setting = g.TrajOptimizerSetting(7)
opt_setting.set_total_step(total_time_step)
opt_setting.set_total_time(total_time_sec)
opt_setting.set_epsilon(0.2)
opt_setting.set_cost_sigma(0.02)
opt_setting.set_obs_check_inter(9)
opt_setting.set_conf_prior_model(0.0001)
opt_setting.set_vel_prior_model(0.0001)
opt_setting.set_Qc_model(np.eye(7))
opt_setting.setDogleg()
straight = g.initArmTrajStraightLine(start_conf, end_conf, total_time_step)
inits = np.repeat(straight[None], B, axis=0)
bump = np.sin(np.pi * np.arange(total_time_step + 1) / total_time_step)
for b in range(1, B):
    inits[b, :, :7] += bump[:, None] * np.random.default_rng(1234 + b).normal(0.0, 0.5, size=7)[None, :]

eng = engine.Engine()
robot = eng.robot(arm)
plan = eng.plan(robot, sdf.handle(), opt_setting, B)        # bound to the field handle for life


def solve(label):
    plan.set_problem(*[np.repeat(v[None], B, axis=0) for v in (start_conf, zero, end_conf, zero)], inits)
    plan.optimize()
    pick = plan.select(9, required_clearance=0.0, require_in_range=False)
    scores = plan.score(9)
    if pick["best"] >= 0:
        print(f"{label}: {pick['n_eligible']} of {B} restarts clear of the scene when up-sampled; best = restart "
              f"{pick['best']}, clearance {scores['min_clearance'][pick['best']]:.3f} m")
    else:
        print(f"{label}: no restart is clear of the scene; best clearance {scores['min_clearance'].max():.3f} m")
    return pick


# ---- the scene: the table the arm stands on, a post beside it, and a boulder (a closed mesh) where the hand passes
hand = eng.sphere_centers(robot, 0.5 * (start_conf + end_conf))[0][0][-1]
half_diagonal = cell * np.sqrt(3.0) / 2.0                   # with this inflate every cell an object touches is marked
vertices, triangles = icosphere_mesh(0.08, 3)               # 1 280 triangles
vertices = vertices * np.array([1.0, 0.7, 1.3])             # squashed: any closed mesh will do
scene = Scene([Box([0.6, 0.6, 0.02], pose_of(t=(0.0, 0.0, -0.35)), inflate=half_diagonal),
               Cylinder(0.03, 0.4, pose_of(t=(0.45, -0.45, 0.05)), inflate=half_diagonal),
               Mesh(vertices, triangles, pose_of(t=hand))], eng)
t0 = time.perf_counter()
cells = sdf.update_from_scene(scene)
print(f"scene -> field in {1e3 * (time.perf_counter() - t0):.1f} ms (read-back of the field included): table {cells[0]} cells, "
      f"post {cells[1]}, mesh {cells[2]}")
solve("mesh in the hand's way")

# ---- the tracked object moves 25 cm along x: its new pose, the field again, the same plan again
moved = pose_of(t=hand + np.array([0.25, 0.0, 0.0]))
scene.set_pose(2, moved)
cells = sdf.update_from_scene(scene)
print(f"mesh moved: {cells[2]} cells at its new place")
solve("mesh moved aside")
plan.close()
