"""Inertial tables for the torque limits (include/gpmp2mi.h "torque limits").

ILLUSTRATIVE ONLY.  The numbers below are made up to have the orders of magnitude of a 7-joint arm of the WAM's size
(link masses between 0.3 and 6 kg, centres of mass a few centimetres off the link frames, shoulder limits of tens of
newton metres).  They are NOT the manufacturer's data and must not be used to run a real arm; bring the table of your
robot.  They exist so that the example, the measurement scripts and the tests have a physically valid table (positive
masses, positive-definite inertias) to work with."""
from __future__ import annotations

import numpy as np


def box_inertia(mass, sx, sy, sz, ixy=0.0, ixz=0.0, iyz=0.0):
    """ixx iyy izz ixy ixz iyz of a solid box of the given mass and edge lengths, with optional products of inertia"""
    return [mass * (sy * sy + sz * sz) / 12.0, mass * (sx * sx + sz * sz) / 12.0, mass * (sx * sx + sy * sy) / 12.0,
            ixy, ixz, iyz]


def illustrative_wam():
    """dict(mass [7], com [7][3], inertia [7][6], torque [7]) for robots.generateArm("WAMArm"): illustrative, see above"""
    mass = np.array([5.8, 3.9, 2.4, 1.1, 0.45, 0.4, 0.3])
    com = np.array([[0.002, 0.11, 0.004], [-0.003, -0.017, 0.26], [-0.038, 0.09, 0.001], [0.011, -0.002, 0.13],
                    [0.0006, 0.024, 0.002], [-0.0003, -0.012, 0.025], [0.001, -0.0007, 0.02]])
    edges = [(0.2, 0.3, 0.2), (0.12, 0.12, 0.5), (0.12, 0.3, 0.1), (0.08, 0.08, 0.3), (0.08, 0.1, 0.08),
             (0.07, 0.07, 0.1), (0.09, 0.09, 0.04)]
    prod = [(2e-3, -1e-3, 5e-4), (-4e-4, 8e-4, 1.5e-3), (6e-4, 2e-4, -3e-4), (1e-4, -2e-4, 1e-4),
            (2e-5, 1e-5, -1e-5), (-1e-5, 2e-5, 1e-5), (5e-6, -5e-6, 1e-5)]
    inertia = np.array([box_inertia(m, *e, *p) for m, e, p in zip(mass, edges, prod)])
    torque = np.array([75.0, 110.0, 45.0, 40.0, 9.0, 8.0, 4.0])
    return dict(mass=mass, com=com, inertia=inertia, torque=torque)
