#!/usr/bin/env python3
"""From a pose of the hand to a plan: the 7-DOF WAM arm in the desk scene is given the pose its tool frame should reach,
not joint angles.  Batched inverse kinematics on the device turns the pose into the distinct collision-free goal
configurations (include/gpmp2mi.h "goal configurations"), 64 restarts are spread over them, and the distinct solutions
among what they lead to are picked on the device ("distinct alternatives").  Runs on an MI355X; there is no CPU path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpmp2_amd as g
from gpmp2_amd import engine, problems

eng, B, N = engine.Engine(), 64, 20
p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=4, opt="GN", sdf="40")
robot, sdf = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
start = problems.WAM_START

# ---- the task: the pose of the last link (here: where the example's usual goal configuration puts it)
pose = eng.forward_kinematics(robot, problems.WAM_END)[0][0, 6]
print("desired position of the hand:", np.round(pose[:3, 3], 3))

# ---- pose -> goal configurations: 256 seeds inside the Barrett WAM's joint ranges, answers 0.5 rad apart are different
# goals, a goal must clear the obstacles by 2 cm; the goals come ordered by their distance to the start configuration
limits = ([-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0], [2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0])
opts = eng.ik_opts(robot, limits=limits)
goals = eng.ik_goals(robot, opts, pose, sdf=sdf, M=256, seed=2024, radius=0.5, max_goals=8, required_clearance=0.02,
                     require_in_range=True, near=start)
n = min(int(goals["n_goals"][0]), 8)
print(f"{goals['n_converged'][0]} of 256 seeds converged, {goals['n_eligible'][0]} clear of the obstacles, "
      f"{goals['n_goals'][0]} distinct goal configurations")
for k in range(n):
    print(f"  goal {k}: seed {goals['goal_seed'][0, k]:3d}, {goals['goal_score'][0, k]:.2f} rad from the start, clearance "
          f"{goals['goal_clearance'][0, k]:.3f} m, q = {np.round(goals['goal_conf'][0, k], 2)}")
if n == 0:
    sys.exit("the pose has no collision-free configuration inside the joint ranges")

# ---- 64 restarts over the goals: row b plans towards goal b % n from a perturbed straight line
ends = eng.goal_rows(goals, B)
inits = np.zeros((B, N + 1, 14))
bump = np.sin(np.pi * np.arange(N + 1) / N)
for b in range(B):
    inits[b] = g.initArmTrajStraightLine(start, ends[b], N)
    if b >= n:
        inits[b, :, :7] += bump[:, None] * np.random.default_rng(1234 + b).normal(0.0, 0.5, size=7)[None, :]
zero = np.zeros((B, 7))
plan = eng.plan(robot, sdf, p.setting, B)
plan.set_problem(np.repeat(start[None], B, axis=0), zero, ends, zero, inits)
plan.optimize()

# ---- the distinct executions among them, best first
pick = plan.select_distinct(4, radius=0.5, max_alt=8, required_clearance=0.0, require_in_range=True)
print(f"{pick['n_eligible']} of {B} restarts are clear when up-sampled; {pick['n_modes']} distinct trajectories")
for k in range(min(pick["n_modes"], 8)):
    b = int(pick["alt"][k])
    print(f"  alternative {k}: restart {b} (towards goal {b % n}), {pick['alt_size'][k]} restarts like it, "
          f"error {pick['alt_error'][k]:.3f}")
plan.close()
