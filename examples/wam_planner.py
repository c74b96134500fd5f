#!/usr/bin/env python3
"""The reference's matlab/WAMPlannerExample.m with gpmp2_amd: 7-DOF WAM arm in the desk scene, signed distance
field built on the GPU, batch trajectory optimisation, dense up-sampling, collision cost, dense collision and self-collision check and
best-of-restarts selection on the device, then one replanning step (matlab/WAMReplannerExample.m:102-126).  Runs on an MI355X; there is no CPU path."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpmp2_amd as g
from gpmp2_amd import engine

# ---- scene: occupancy grid -> signed distance field (both on the device)
dataset = g.generate3Ddataset("WAMDeskDataset")
t0 = time.perf_counter()
field = g.signedDistanceField3D(dataset.map, dataset.cell_size)          # [x][y][z] like the MATLAB utility
print(f"signed distance field {field.shape}: {1e3 * (time.perf_counter() - t0):.0f} ms")
layers = g.sdf3_zyx(field)                                               # field(:,:,z)' of the MATLAB script
sdf = g.SignedDistanceField([dataset.origin_x, dataset.origin_y, dataset.origin_z], dataset.cell_size,
                            layers.shape[1], layers.shape[2], layers.shape[0])
for z in range(layers.shape[0]):
    sdf.initFieldData(z, layers[z])

# ---- robot and settings (WAMPlannerExample.m:34-75)
arm = g.generateArm("WAMArm")
start_conf = np.array([-0.8, -1.70, 1.64, 1.29, 1.1, -0.106, 2.2])
end_conf = np.array([-0.0, 0.94, 0, 1.6, 0, -0.919, 1.55])
zero = np.zeros(7)
total_time_sec, total_time_step, total_check_step = 2.0, 10, 100
opt_setting = g.TrajOptimizerSetting(7)
opt_setting.set_total_step(total_time_step)
opt_setting.set_total_time(total_time_sec)
opt_setting.set_epsilon(0.2)
opt_setting.set_cost_sigma(0.02)
opt_setting.set_obs_check_inter(total_check_step // total_time_step - 1)
opt_setting.set_conf_prior_model(0.0001)
opt_setting.set_vel_prior_model(0.0001)
opt_setting.set_Qc_model(np.eye(7))
opt_setting.setDogleg()

# ---- batch plan
init_values = g.values_from_traj(g.initArmTrajStraightLine(start_conf, end_conf, total_time_step))
t0 = time.perf_counter()
result = g.BatchTrajOptimize3DArm(arm, sdf, start_conf, zero, end_conf, zero, init_values, opt_setting)
print(f"BatchTrajOptimize3DArm: {1e3 * (time.perf_counter() - t0):.1f} ms, "
      f"collision cost {g.CollisionCost3DArm(arm, sdf, result, opt_setting):.4f}")
dense = g.interpolateArmTraj(result, opt_setting.Qc, total_time_sec / total_time_step, 9)
print(f"up-sampled to {len(dense) // 2} states; x_50 = {np.round(dense[('x', 50)], 3)}")

# ---- what gets executed: the up-sampled states, checked on the device (the support states alone can look clean)
print(f"dense collision cost {g.DenseCollisionCost3DArm(arm, sdf, result, opt_setting, 9):.4f}, minimum clearance "
      "%.4f m at checked state %d, sphere %d" % g.MinClearance3DArm(arm, sdf, result, opt_setting, 9))

# ---- restarts: 16 perturbed initial trajectories in one plan, then pick the one to execute on the device
eng, B = engine.Engine(), 16
straight = g.initArmTrajStraightLine(start_conf, end_conf, total_time_step)
inits = np.repeat(straight[None], B, axis=0)
bump = np.sin(np.pi * np.arange(total_time_step + 1) / total_time_step)
for b in range(1, B):
    inits[b, :, :7] += bump[:, None] * np.random.default_rng(1234 + b).normal(0.0, 0.5, size=7)[None, :]
robot = eng.robot(arm)
plan = eng.plan(robot, sdf.handle(), opt_setting, B)
plan.set_problem(*[np.repeat(v[None], B, axis=0) for v in (start_conf, zero, end_conf, zero)], inits)
plan.optimize()
# the robot must clear itself too: every sphere pair two joints apart or more that does not touch at the zero configuration
pairs = eng.generate_self_pairs(robot, min_joint_gap=2, ref_conf=np.zeros(7))
scores, self_scores = plan.score(9), plan.self_score(pairs, 9)
pick = plan.select_checked(9, pairs, required_clearance=0.0, require_in_range=True, required_self_clearance=0.0)
hidden = int(((scores["support_cost"] == 0) & (scores["dense_cost"] > 0)).sum())
touching = int((self_scores["min_self_clearance"] < 0).sum())
print(f"{B} restarts: {pick['n_eligible']} clear of the obstacles and of themselves when up-sampled, {hidden} clean at the "
      f"support states only, {touching} in self-collision ({pairs.P} pairs); best = restart {pick['best']}")
if pick["best"] >= 0:
    b = pick["best"]
    print(f"  support cost {scores['support_cost'][b]:.4f}, dense cost {scores['dense_cost'][b]:.4f}, clearance "
          f"{scores['min_clearance'][b]:.4f} m, self clearance {self_scores['min_self_clearance'][b]:.4f} m; "
          f"{pick['dense_best'].shape[0]} states ready to execute")

# ---- replanning: execute to state 5, the goal moves (WAMReplannerExample.m:102-126)
isam = g.ISAM2TrajOptimizer3DArm(arm, sdf, opt_setting)
isam.initFactorGraph(start_conf, zero, end_conf, zero)
isam.initValues(result)
isam.update()
values = isam.values()
isam.fixConfigAndVel(5, values[("x", 5)], values[("v", 5)])
isam.changeGoalConfigAndVel(np.array([-0.6, 0.94, 0, 1.6, 0, -0.919, 1.55]), zero)
isam.update()
isam.update()
replanned = isam.values()
print(f"replanned: goal reached {np.round(replanned[('x', total_time_step)], 3)}, "
      f"state 5 moved by {np.abs(replanned[('x', 5)] - values[('x', 5)]).max():.1e}")

# ---- can the arm execute it?  The Barrett WAM's joint ranges, 2 rad/s, 20 rad/s^2 and 1.5 m/s for any point of the body: the
# best row that stays inside its joint ranges, and the factor by which its duration must be stretched to meet the rates
limits = engine.MotionLimits(7, pos_down=[-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0],
                             pos_up=[2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0], vel=2.0, acc=20.0, point_speed=1.5)
motion = plan.motion_score(limits, 9)
feasible = plan.select_feasible(9, limits, required_pos_margin=0.0, max_time_scale=np.inf, require_in_range=True, pairs=pairs)
print(f"{int((motion['pos_margin'] < 0).sum())} restarts leave the joint ranges, {int((motion['time_scale'] > 1).sum())} are "
      f"too fast as planned; executable: {feasible['n_eligible']}, best = restart {feasible['best']}")
if feasible["best"] >= 0:
    s = feasible["time_scale_best"]
    print(f"  time_scale {s:.3f}: run it over {max(s, 1.0) * total_time_sec:.2f} s instead of {total_time_sec:.2f} s "
          f"(velocities divided by {max(s, 1.0):.3f})")

# ---- the static map changes.  The field is rewritten in place (include/gpmp2mi.h "live map"): `plan` and the replanner
# above keep their memory and read the new map in their next call.  The desk scene becomes the base; this cycle's cloud, a
# box where the hand passes half-way, is united with it, and the points on the robot's own arm are dropped.
sdf.updateFromOccupancy(g.sdf3_zyx(np.asarray(dataset.map, dtype=np.float64)))
hand = eng.sphere_centers(robot, 0.5 * (start_conf + end_conf))[0][0][-1]
side = np.arange(-3, 4) * dataset.cell_size
cloud = np.array([[hand[0] + dx, hand[1] + dy, hand[2] + dz] for dx in side for dy in side for dz in side])
on_arm = eng.sphere_centers(robot, start_conf)[0][0]
counts = sdf.updateFromPoints(np.concatenate([cloud, on_arm]), use_base=True, robot=arm, conf=start_conf, margin=0.02)
plan.set_problem(*[np.repeat(v[None], B, axis=0) for v in (start_conf, zero, end_conf, zero)], inits)
plan.optimize()
again = plan.select_checked(9, pairs, required_clearance=0.0, require_in_range=True, required_self_clearance=0.0)
print(f"map changed in place ({counts['kept']} points kept, {counts['self']} on the robot itself dropped): "
      f"{again['n_eligible']} restarts clear of the new map, best = restart {again['best']}")
plan.close()
