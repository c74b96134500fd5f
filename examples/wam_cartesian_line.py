#!/usr/bin/env python3
"""Move the tool along a straight line: the 7-DOF WAM arm in the desk scene is given two poses of its tool frame.
Batched inverse kinematics turns them into a start and a goal configuration (include/gpmp2mi.h "goal configurations"),
the straight line between the poses becomes the plan's workspace path ("workspace path": one POSE target per support
state), 64 seeded restarts are solved with the path as a factor, and the best restart that stays on the line is picked
on the device.  The same problem planned without the path shows what the factor buys.  Runs on an MI355X; there is no
CPU path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpmp2_amd as g
from gpmp2_amd import engine, problems, scoring

eng, B, N, LINK, J = engine.Engine(), 64, 20, 6, 4
p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=4, opt="LM", sdf="40")
robot, sdf = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)

# ---- the task: two poses of the tool that the arm can reach (here: where two configurations put it)
reach = np.stack([problems.WAM_START, problems.WAM_START + np.array([0.8, 0.5, -0.4, 0.5, 0.3, 0.0, 0.0])])
pose_a, pose_b = eng.forward_kinematics(robot, reach)[0][:, LINK]
print("tool from", np.round(pose_a[:3, 3], 3), "to", np.round(pose_b[:3, 3], 3))

# ---- pose -> configuration: the answers nearest to the start configuration
limits = ([-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0], [2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0])
opts = eng.ik_opts(robot, limits=limits)
goals = eng.ik_goals(robot, opts, np.stack([pose_a, pose_b]), M=256, seed=7, radius=0.5, max_goals=4,
                     near=problems.WAM_START)
print(f"{goals['n_converged'][0]} and {goals['n_converged'][1]} of 256 seeds converged, {goals['n_goals'][0]} and "
      f"{goals['n_goals'][1]} distinct configurations")
if int(goals["n_goals"].min()) == 0:
    sys.exit("a pose has no configuration inside the joint ranges")
start, end = goals["goal_conf"][0, 0], goals["goal_conf"][1, 0]
print("start configuration", np.round(start, 2), "\ngoal configuration ", np.round(end, 2))

# ---- the path: positions on the line, orientations on the geodesic, 1 mm / 1 mrad noise on every support state
des = scoring.line_path(pose_a, pose_b, N)
setting = p.setting
setting.set_workspace_path(2, LINK)
plan = eng.plan(robot, sdf, setting, B)

# ---- seeded restarts around the straight line in joint space, solved with and without the path
zero = np.zeros((B, 7))
starts, ends = np.repeat(start[None], B, axis=0), np.repeat(end[None], B, axis=0)
inits = np.repeat(g.initArmTrajStraightLine(start, end, N)[None], B, axis=0)
bump = np.sin(np.pi * np.arange(N + 1) / N)
for b in range(1, B):
    inits[b, :, :7] += bump[:, None] * np.random.default_rng(1234 + b).normal(0.0, 0.3, size=7)[None, :]
dt, SIGMA = setting.total_time / N, 0.001
for label, path in (("without the path", None), ("with the path", des)):
    plan.set_workspace_path(path, None if path is None else SIGMA)
    plan.set_problem(starts, zero, ends, zero, inits)
    plan.optimize()
    res = plan.result()
    dev = eng.path_score_traj(robot, 2, LINK, des, SIGMA, dt, J, res["traj"])
    pick = plan.select_path(J, max_pos_dev_allowed=0.02, max_rot_dev_allowed=0.1) if path is not None else plan.select(J)
    b = pick["best"]
    print(f"{label}: {pick['n_eligible']} of {B} restarts eligible; over the restarts the tool leaves the line by "
          f"{1e3 * dev['max_pos_dev'].min():.1f} .. {1e3 * dev['max_pos_dev'].max():.1f} mm and "
          f"{1e3 * dev['max_rot_dev'].min():.1f} .. {1e3 * dev['max_rot_dev'].max():.1f} mrad")
    if b < 0:
        print("  none chosen")
        continue
    print(f"  restart {b} chosen, error {res['final_error'][b]:.2f}: at most {1e3 * dev['max_pos_dev'][b]:.1f} mm and "
          f"{1e3 * dev['max_rot_dev'][b]:.1f} mrad off the line (checked states {dev['worst'][b, 0]} and "
          f"{dev['worst'][b, 1]} of {scoring.checked_states(N, J)})")
plan.close()
