#!/usr/bin/env python3
"""Carry a rod through the desk scene: 16 restarts of the 7-DOF WAM are solved twice by the same plan, once as if the hand
were empty and once with the rod -- 12 spheres along the z axis of the last link, half a metre long -- as a factor on
every support state (include/gpmp2mi.h "carried object").  Both results go through the carried check, which looks between the support
states as well, and the script prints the check of the chosen row for the plain plan and for the plan with the factor.
The set is given and cleared between the solves; the plan, its field and its robot handle are made once.  Runs on an
MI355X; there is no CPU path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import engine, problems, scoring

eng, B, N, J = engine.Engine(), 16, 12, 4
EPSILON, SIGMA = 0.05, 0.05
p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=3, sdf="40")
robot, sdf = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)
link = robot.L - 1

# ---- the rod: spheres of 3 cm every 4 cm, from 8 cm to 52 cm in front of the hand
centers = np.ascontiguousarray(np.stack([np.zeros(12), np.zeros(12), np.linspace(0.08, 0.52, 12)], axis=1))
radius = np.full(len(centers), 0.03)
print(f"{len(radius)} spheres on link {link}")

p.setting.set_carried_spheres(len(radius), EPSILON, SIGMA)          # room for the rod on all support states
plan = eng.plan(robot, sdf, p.setting, B)
for label, held in (("plain", False), ("with the factor", True)):
    plan.set_carried(link, radius if held else None, centers if held else None)      # grasp / release: two copies
    plan.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    plan.optimize()
    res = plan.result()
    plan.set_carried(link, radius, centers)                          # the check is about the rod in both cases
    obstacle, box = plan.score(J), plan.carried_score(J)
    passing = scoring.eligible(res["final_error"], res["status"], obstacle["min_clearance"], obstacle["out_of_range"])
    touching = passing & (box["min_carried_clearance"] < 0.0)
    print(f"{label}: {res['iters'].sum()} iterations; {int(passing.sum())} of {B} restarts pass the obstacle rule, the rod of "
          f"{int(touching.sum())} of them touches an obstacle (smallest rod clearance among them "
          f"{100 * np.min(box['min_carried_clearance'][passing], initial=np.inf):+.1f} cm, their dense rod cost "
          f"{box['carried_dense_cost'][passing].sum():.3f})")
    pick = plan.select(J)                        # the rule that does not know about the rod
    b = pick["best"]
    if b >= 0:
        print(f"  select: restart {b}, error {res['final_error'][b]:.2f}; its rod: clearance "
              f"{100 * box['min_carried_clearance'][b]:+.1f} cm at (state, sphere) {tuple(int(x) for x in box['worst'][b])}, "
              f"dense cost {box['carried_dense_cost'][b]:.3f}, {box['out_of_range'][b]} centres out of the field")
    safe = plan.select_carried(J, required_carried_clearance=0.0)
    print(f"  select_carried, rod clear of the obstacles: {safe['n_eligible']} eligible, restart {safe['best']} chosen")
plan.close()
