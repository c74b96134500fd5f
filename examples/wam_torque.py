#!/usr/bin/env python3
"""Can the drives produce the plan?  The 7-DOF WAM arm plans through the desk scene from 64 restarts; every restart's
joint torques come from inverse dynamics at every executed state (include/gpmp2mi.h "torque limits"), and the result is
the cheapest restart that is clear, inside its joint ranges and executable once the duration is stretched by no more
than a bound: the larger of the stretch its rate limits ask for and the stretch its torque limits ask for.

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
total = p.setting.total_time

# ---- every restart: what the rate limits ask for against what the torque limits ask for
rate = plan.motion_score(limits, J)["time_scale"]
tq = plan.torque_score(dyn, J)
print(f"{B} restarts, planned duration {total:.2f} s, torque limits {table['torque']} N m (illustrative)")
print(f"  gravity alone takes up to {tq['static_ratio'].max():.2f} of a limit; the motion brings it to {tq['torque_ratio'].max():.2f}")
print(f"  stretch for the rate limits:   {rate.min():.2f} - {rate.max():.2f}")
print(f"  stretch for the torque limits: {tq['torque_time_scale'].min():.2f} - {tq['torque_time_scale'].max():.2f}")

# ---- the cheapest restart that is clear, in range and executable within the bound
bound = float(np.median(np.maximum(rate, tq["torque_time_scale"])))
pick = plan.select_dynamic(J, limits, dyn, required_pos_margin=0.0, max_time_scale=bound, required_clearance=0.0,
                           require_in_range=True)
if pick["best"] < 0:
    sys.exit(f"no restart is clear, in range and executable within a stretch of {bound:.2f}")
b = pick["best"]
state, joint = tq["worst"][b, 0]
print(f"chosen: restart {b} of {pick['n_eligible']} eligible")
print(f"  its torque peaks at checked state {state} (t = {state * total / (N * (J + 1)):.2f} s), joint {joint}: "
      f"{tq['torque_ratio'][b]:.2f} of the limit, {tq['static_ratio'][b]:.2f} of some limit spent on gravity")
print(f"  the stretch that fixes it: {tq['torque_time_scale'][b]:.2f} for the torques, {rate[b]:.2f} for the rates -> run it over "
      f"{pick['time_scale_best'] * total:.2f} s")
print("  feed-forward torques at planned timing, every support state, joints 0..3 [N m]:")
print(np.round(pick["tau_best"][::J + 1, :4], 2))
plan.close()
