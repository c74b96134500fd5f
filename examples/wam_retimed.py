#!/usr/bin/env python3
"""How fast can the plan be run?  The 7-DOF WAM arm plans through the desk scene from 64 restarts, and the result is
chosen by how long it takes once it is re-timed: a speed profile along the unchanged path, per executed state, as fast as
joint speeds, joint accelerations and the Cartesian speed of the body allow (include/gpmp2mi.h "re-timing").  Beside it
the uniform stretch of "motion limits", where one sharp corner slows the whole trajectory.  Runs on an MI355X; there is
no CPU path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import engine, problems

eng, B, N, J = engine.Engine(), 64, 20, 4
p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=4, opt="GN", sdf="40")
robot, sdf = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
plan = eng.plan(robot, sdf, p.setting, B)
plan.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
plan.optimize()

# the Barrett WAM's ranges and round rate limits; the robot may run up to twice as fast as planned, and starts and ends
# at rest
limits = engine.MotionLimits(7, pos_down=[-2.6, -2.0, -2.8, -0.9, -4.76, -1.6, -3.0], pos_up=[2.6, 2.0, 2.8, 3.1, 1.24, 1.6, 3.0],
                             vel=2.0, acc=20.0, point_speed=1.5)
rates = dict(max_rate=2.0, rate_start=0.0, rate_end=0.0)
total = p.setting.total_time

# ---- every restart: the uniform stretch against the re-timed duration
scale = plan.motion_score(limits, J)["time_scale"]
rt = plan.retime(limits, J, **rates)
ok = rt["status"] == 0
print(f"{int(ok.sum())} of {B} restarts re-time; planned duration {total:.2f} s")
print(f"  uniform stretch: {np.min(scale * total):.2f} - {np.max(scale * total):.2f} s (starts and ends moving)")
print(f"  re-timed:        {rt['duration'][ok].min():.2f} - {rt['duration'][ok].max():.2f} s (from rest to rest)")

# ---- the cheapest restart that is clear of the obstacles, inside its joint ranges and executable within the bound
bound = float(np.median(rt["duration"][ok]))
pick = plan.select_retimed(J, limits, required_pos_margin=0.0, max_duration=bound, required_clearance=0.0,
                           require_in_range=True, **rates)
if pick["best"] < 0:
    sys.exit(f"no restart is clear, in range and executable within {bound:.2f} s")
b = pick["best"]
print(f"chosen: restart {b} of {pick['n_eligible']} eligible, {pick['duration_best']:.2f} s re-timed against "
      f"{scale[b] * total:.2f} s uniformly stretched")
sdot = rt["sdot"][b]
print("  rate of planned against executed time along it:", np.round(sdot[::J + 1], 2))
print("  largest ratios after re-timing (velocity, acceleration at the states, between them, point speed):",
      np.round(rt["achieved"][b], 3))
print("  the executable trajectory: states dense_best with the time stamps", np.round(pick["stamps_best"][::J + 1], 2))
plan.close()
