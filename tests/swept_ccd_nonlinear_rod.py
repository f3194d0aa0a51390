"""The rod of the SweepMode::NonLinear tests and its independent float64 geometry (shared by test_swept_ccd_nonlinear_cpu.py and
test_gpu_swept_ccd_nonlinear.py).

A cuboid he = (L, w, w) spins at omega about z beside a wall whose face is the plane y = D, hypot(L, w) > D > w.  The corner (L, w) touches at
t* = (asin(D / rho) - atan2(w, L)) / omega, rho = hypot(L, w).  The exact gap at any time is D minus the largest y of the eight corners,
computed with float64 rotation matrices about the centre of mass; it shares no code with swept_ccd_nonlinear_reference.  `band` is the
forward-error bound of spatial_cast_exact_geometry (32 eps * scale)."""
import math

import numpy as np

import spatial_cast_exact_geometry as XC
from spatial_exact_geometry import CUBOID, Collider

TOL = 0.005   # avn_config::contact_tolerance's default
ROD_L, ROD_W, WALL_D, WALL_TH, ROD_OMEGA = 0.5, 0.02, 0.3, 0.05, 40.0
WALL_HE = (2.0, WALL_TH, 2.0)
WALL_POS = (0.0, WALL_D + WALL_TH, 0.0)


def t_star(L=ROD_L, w=ROD_W, D=WALL_D, omega=ROD_OMEGA):
    return (math.asin(D / math.hypot(L, w)) - math.atan2(w, L)) / omega


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def exact_rod_gap(t, he, pos, com, v, omega_z, D=WALL_D):
    """D - the largest corner y of a rod that starts unrotated at `pos` and turns about its centre of mass (float64 matrices)."""
    he, pos, com, v = (np.asarray(x, np.float64) for x in (he, pos, com, v))
    c0 = pos + com
    corners = np.array([[sx * he[0], sy * he[1], sz * he[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    world = (c0 + v * t)[None, :] + (corners - com[None, :]) @ rot_z(omega_z * t).T
    return D - float(world[:, 1].max())


def band_of(bits, he1, pos1, he2, pos2):
    ident = (0.0, 0.0, 0.0, 1.0)
    return XC.scale_of(bits, Collider(CUBOID, he1, pos1, ident), Collider(CUBOID, he2, pos2, ident))[1]
