#!/usr/bin/env python3
"""Keep the arm off itself while it plans: 16 restarts of the 7-DOF WAM in the desk scene are solved twice, once plainly
and once with the arm's full self-collision table -- the 78 generated sphere pairs, epsilon 5 cm, sigma 5 mm -- as a
factor on every support state (include/gpmp2mi.h "self-collision table in a plan").  Both batches then go through the
checked selection ("self-collision check"), which looks between the support states as well, and the script prints how
many of the restarts that pass the obstacle rule touch themselves.  Runs on an MI355X; there is no CPU path."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpmp2_amd import engine, problems, scoring

eng, B, N, J = engine.Engine(), 16, 12, 4
EPSILON, SIGMA = 0.05, 0.005
p = problems.wam_restarts(B=B, total_step=N, obs_check_inter=3, sdf="40")
robot, sdf = eng.robot(p.model), eng.sdf(p.sdf_origin, p.sdf_cell, p.sdf_data)

# ---- the tables: pairs at least two joints apart that do not touch at the zero configuration.  The check asks for
# contact (epsilon 0); the factor starts pushing 5 cm before it
check = eng.generate_self_pairs(robot, 2, np.zeros((1, 7)))
factor = eng.generate_self_pairs(robot, 2, np.zeros((1, 7)), EPSILON, SIGMA)
print(f"{check.P} sphere pairs")

p.setting.set_self_pairs(factor.P)          # room for the table on all support states
plan = eng.plan(robot, sdf, p.setting, B)
for label, table in (("plain", None), ("with the table", factor)):
    plan.set_self_pairs(table)
    plan.set_problem(p.start_conf, p.start_vel, p.end_conf, p.end_vel, p.init)
    plan.optimize()
    res = plan.result()
    obstacle, own = plan.score(J), plan.self_score(check, J)
    passing = scoring.eligible(res["final_error"], res["status"], obstacle["min_clearance"], obstacle["out_of_range"])
    touching = passing & (own["min_self_clearance"] < 0.0)
    pick = plan.select_checked(J, check)
    print(f"{label}: {int(passing.sum())} of {B} restarts pass the obstacle rule, {int(touching.sum())} of them touch "
          f"themselves (smallest clearance to itself among them {100 * own['min_self_clearance'][passing].min():+.1f} cm); "
          f"{res['iters'].sum()} iterations")
    if pick["best"] < 0:
        print("  none chosen")
    else:
        print(f"  restart {pick['best']} chosen out of {pick['n_eligible']} eligible, error {res['final_error'][pick['best']]:.2f}")
plan.close()
