#!/usr/bin/env python3
"""How fast can the drives run the plan?  The 7-DOF WAM arm plans through the desk scene from 64 restarts, and the result
is chosen by how long it takes once it is re-timed under its joint torque limits: a speed profile along the unchanged
path, per executed state, as fast as the torques, the joint speeds, the joint accelerations and the Cartesian speed of the
body allow, with gravity taken off each torque limit state by state (include/gpmp2mi.h "re-timing under torque limits").
Beside it the uniform stretch of "torque limits" and "motion limits", where one demanding stage slows the whole
trajectory, and the feed-forward torques of the re-timed result.

THE INERTIAL TABLE IS ILLUSTRATIVE (gpmp2_amd/dynamics.py): made-up numbers of the right order of magnitude, not the
manufacturer's data.  Bring the table of your robot.  Runs on an MI355X; there is no CPU path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import dynamics, engine, problems

np.set_printoptions(suppress=True, linewidth=120)
eng, B, N, J = engine.Engine(), 64, 20, 4
p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=4, opt="GN", sdf="40")
robot, sdf = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
plan = eng.plan(robot, sdf, p.setting, B)
plan.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
plan.optimize()

limits = engine.MotionLimits(7, pos_down=[-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0], pos_up=[2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0],
                             vel=2.0, acc=20.0, point_speed=1.5)
table = dynamics.illustrative_wam()          # ILLUSTRATIVE, see above
dyn = eng.dynamics(robot, table["mass"], table["com"], table["inertia"], torque=table["torque"])
rates = dict(max_rate=2.0)                   # the robot may run up to twice as fast as planned
total = p.setting.total_time

# ---- every restart: the uniform stretch against the two re-timed durations
stretch = np.maximum(plan.motion_score(limits, J)["time_scale"], plan.torque_score(dyn, J, tau=False)["torque_time_scale"])
uniform = np.maximum(stretch, 1.0 / rates["max_rate"]) * total
plain = plan.retime(limits, J, **rates)
rt = plan.retime_dynamic(dyn, limits, J, **rates)
ok = rt["status"] == 0
print(f"{int(ok.sum())} of {B} restarts re-time under the torque limits {table['torque']} N m (illustrative); "
      f"{int((rt['status'] == 4).sum())} cannot be held against gravity; planned duration {total:.2f} s")
if not ok.any():
    sys.exit("no restart re-times")
print(f"  uniform stretch (rates and torques):    {uniform[ok].min():.2f} - {uniform[ok].max():.2f} s")
print(f"  re-timed, rate limits alone:            {plain['duration'][ok].min():.2f} - {plain['duration'][ok].max():.2f} s")
print(f"  re-timed, rate and torque limits:       {rt['duration'][ok].min():.2f} - {rt['duration'][ok].max():.2f} s")
print(f"  largest torque ratio of a re-timed row: {rt['achieved'][ok, 4].max():.6f} (gravity alone: up to {rt['achieved'][ok, 5].max():.2f})")

# ---- the cheapest restart that is clear of the obstacles, inside its joint ranges and executable within the bound
bound = float(np.median(rt["duration"][ok]))
pick = plan.select_retimed_dynamic(J, limits, dyn, required_pos_margin=0.0, max_duration=bound, required_clearance=0.0,
                                   require_in_range=True, **rates)
if pick["best"] < 0:
    sys.exit(f"no restart is clear, in range and executable within {bound:.2f} s")
b = pick["best"]
print(f"chosen: restart {b} of {pick['n_eligible']} eligible, {pick['duration_best']:.2f} s re-timed against "
      f"{uniform[b]:.2f} s uniformly stretched")
print("  rate of planned against executed time along it:", np.round(rt["sdot"][b][::J + 1], 2))
print("  the executable trajectory: states dense_best with the time stamps", np.round(pick["stamps_best"][::J + 1], 2))
print("  feed-forward torques of the re-timed result, every support state, joints 0..3 [N m]:")
print(np.round(pick["tau_best"][::J + 1, :4], 2))
print("  share of each limit at its peak:", np.round(np.abs(pick["tau_best"]).max(axis=0) / table["torque"], 3))
plan.close()
