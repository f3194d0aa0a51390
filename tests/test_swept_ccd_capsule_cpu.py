"""CPU: swept CCD with Capsule colliders (include/avian_mi355x_ccd.h, "capsule colliders"): the export, and tests/swept_ccd_capsule_reference.py
against independent geometry.

THE GAP (N2's capsule arms) is held to a distance computed another way for a fixed seeded set per arm: capsule - ball and capsule - capsule by
closed forms written here in extended precision (numpy longdouble: point - segment; segment - segment as the smallest of the interior solution
of the two lines, where it exists, and the four end - segment distances), capsule - cuboid by sampling the core.  The tolerance is derived:
  * rounding: the reference's distance is the length of a difference of two points, each computed from coordinates no larger than
    scale = |p1| + |p2| + the shapes' sizes (max-norms) in a dozen roundings, so |dist - exact| <= band = 32 eps scale (the forward-error
    bound of spatial_cast_exact_geometry, unchanged);
  * sampling (capsule - cuboid): point - box distance is 1-Lipschitz, so the minimum over K uniform samples of a core of length |u| exceeds the
    true minimum by at most |u| / (2 K).
  * the axis: n is the unit vector of a difference v of points of two convex sets with |v| <= D + band, D the distance.  The midpoint of v and
    the minimal vector v* is a difference of points of the sets too, so |v + v*| >= 2 D and |v - v*|^2 = 2 |v|^2 + 2 |v*|^2 - |v + v*|^2
    <= 4 D band + 2 band^2: the sine of the angle between n and v* is at most sqrt(4 band / D + 2 (band / D)^2).
THE SPINNING CAPSULE.  r = 0.05, h = 0.5 turning at 40 rad / s about z with its centre fixed, its axis (y) parallel to the wall face x = D = 0.3.
The lower end of the core is at x = h sin(w t), so the cap touches at t* = asin((D - r) / h) / w and the exact gap at t is D - r - h |sin(w t)|.
THE ROUND SET is at the end of the file."""
import ctypes
import math
import os

import numpy as np
import pytest

import spatial_cast_exact_geometry as XC
import swept_ccd_capsule_reference as CAPR
import swept_ccd_nonlinear_reference as NL
import swept_ccd_reference as CR
from spatial_exact_geometry import CUBOID as X_CUBOID, Collider
from swept_ccd_capsule_rounds import (ROUNDS_EXHAUSTED_UNDER_CAP, ROUNDS_NEWTON_CAPPED, ROUNDS_PAIRS, batch_advance, batch_newton_rounds, rounds_set, run_pair)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [32, 64]
DT = {32: np.float32, 64: np.float64}
DT_NS = 16666667
TOL = 0.005
BALL, CUBOID, CAPSULE = CAPR.SHAPE_BALL, CAPR.SHAPE_CUBOID, CAPR.SHAPE_CAPSULE
LD = np.longdouble
IDENT = (0.0, 0.0, 0.0, 1.0)


# ---- 1. the export and the binding ----------------------------------------------------------------------------------------------------------
def test_1_the_library_exports_the_switch_and_the_binding_reaches_it():
    path = os.path.join(REPO, "avian_amd", "csrc", "libavian_mi355x.so")
    dll = ctypes.CDLL(path)
    assert hasattr(dll, "avn_swept_ccd_capsules_set")
    header = open(os.path.join(REPO, "include", "avian_mi355x_ccd.h")).read()
    assert "AVN_API avn_status avn_swept_ccd_capsules_set(avn_world* w, uint32_t enabled);" in header
    from avian_amd import _ffi as F
    from avian_amd.swept_ccd import SweptCcd
    assert callable(getattr(SweptCcd, "set_capsules"))
    assert "avn_swept_ccd_capsules_set" in F.SWEPT_CCD_CAPSULES_SYMBOLS
    F.declare_swept_ccd(dll)
    assert dll.avn_swept_ccd_capsules_set.argtypes == [ctypes.c_void_p, ctypes.c_uint32]
    import inspect
    assert list(inspect.signature(SweptCcd.__init__).parameters)[1:] == ["world", "non_linear", "capsules"]


# ---- 2. the gap against independent geometry --------------------------------------------------------------------------------------------------
def rot_ld(q):
    x, y, z, w = (LD(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], LD)


def core_ld(pos, q, h):
    m = rot_ld(q)
    a = np.asarray(pos, LD) - m[:, 1] * LD(h)
    return a, m[:, 1] * LD(2) * LD(h)


def point_segment_ld(p, a, u):
    uu = u @ u
    s = LD(0) if uu == 0 else min(max(((p - a) @ u) / uu, LD(0)), LD(1))
    return a + u * s


def segment_segment_ld(a1, u1, a2, u2):
    """The closest points of two segments: the smallest of the lines' interior solution (where both parameters lie in [0, 1]) and the four ends
    against the other segment."""
    cands = []
    c = np.cross(u1, u2)
    cc = c @ c
    if cc > 0:
        w = a2 - a1
        s = (np.cross(w, u2) @ c) / cc
        t = (np.cross(w, u1) @ c) / cc
        if 0 <= s <= 1 and 0 <= t <= 1:
            cands.append((a1 + u1 * s, a2 + u2 * t))
    for e in (a1, a1 + u1):
        cands.append((e, point_segment_ld(e, a2, u2)))
    for e in (a2, a2 + u2):
        cands.append((point_segment_ld(e, a1, u1), e))
    return min(cands, key=lambda pq: (pq[1] - pq[0]) @ (pq[1] - pq[0]))


SAMPLES = 4096


def capsule_box_ld(a, u, box_pos, box_q, he):
    """(the minimum over SAMPLES uniform samples of the core of the exact point - box distance, the minimal vector box -> core in the world frame).
    The vector is found apart from the samples: the squared distance along the core is convex, so its derivative e(s) . u changes sign once and a
    bisection on that sign finds the minimiser."""
    m = rot_ld(box_q)
    al = np.asarray(m.T @ (a - np.asarray(box_pos, LD)), np.float64)
    ul = np.asarray(m.T @ u, np.float64)
    hev = np.asarray(he, np.float64)
    s = np.linspace(0.0, 1.0, SAMPLES)
    pts = al[None, :] + s[:, None] * ul[None, :]
    e = pts - np.clip(pts, -hev, hev)
    sampled = float(np.sqrt((e * e).sum(1)).min())
    al_, ul_, he_ = [float(x) for x in al], [float(x) for x in ul], [float(x) for x in hev]

    def vec(x):
        p = [al_[i] + ul_[i] * x for i in range(3)]
        return [p[i] - min(max(p[i], -he_[i]), he_[i]) for i in range(3)]

    slope = lambda x: sum(c * w for c, w in zip(vec(x), ul_))
    lo, hi = 0.0, 1.0
    if slope(0.0) >= 0:
        hi = 0.0
    elif slope(1.0) <= 0:
        lo = 1.0
    else:
        for _ in range(80):
            mid = (lo + hi) / 2
            if slope(mid) < 0:
                lo = mid
            else:
                hi = mid
    return LD(sampled), m @ np.asarray(vec((lo + hi) / 2), LD)


def unit_quat(rng):
    q = rng.normal(size=4)
    return tuple(q / np.linalg.norm(q))


def gap_poses(arm, n=2100, seed=77):
    """n poses of one arm: sizes 0.02 .. 2 (log-uniform), random rotations; a third far to near, a third moved along the independent minimal
    vector until the shapes touch, a third overlapping (core points inside the other shape included)."""
    rng = np.random.default_rng(seed + {"ball": 0, "capsule": 1, "cuboid": 2}[arm])
    size = lambda k=1: np.exp(rng.uniform(np.log(0.02), np.log(2.0), k))
    out = []
    for i in range(n):
        r, h = size(2)
        he_c = (float(r), float(h), 0.0)
        if arm == "ball":
            he_o = (float(size()[0]), 0.0, 0.0)
        elif arm == "capsule":
            ro, ho = size(2)
            he_o = (float(ro), float(ho), 0.0)
        else:
            he_o = tuple(float(x) for x in size(3))
        reach = (r + h) + (he_o[0] if arm == "ball" else (he_o[0] + he_o[1] if arm == "capsule" else float(np.linalg.norm(he_o))))
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        frac = rng.uniform(0.0, 0.6) if i % 3 == 2 else rng.uniform(0.3, 2.5)
        pc = rng.uniform(-1, 1, 3)
        po = pc + u * reach * frac
        out.append(dict(he_c=he_c, he_o=he_o, pc=pc, qc=unit_quat(rng), po=po, qo=unit_quat(rng), touch=i % 3 == 1, cap_first=bool(rng.integers(0, 2))))
    return out


def independent(arm, p):
    """(exact distance of the core from the other shape's core, the minimal vector from the capsule's core towards the other's, sampling error)."""
    a, u = core_ld(p["pc"], p["qc"], p["he_c"][1])
    if arm == "ball":
        c = np.asarray(p["po"], LD)
        v = c - point_segment_ld(c, a, u)
        return np.sqrt(v @ v), v, LD(0)
    if arm == "capsule":
        a2, u2 = core_ld(p["po"], p["qo"], p["he_o"][1])
        x, y = segment_segment_ld(a, u, a2, u2)
        v = y - x
        return np.sqrt(v @ v), v, LD(0)
    d, v = capsule_box_ld(a, u, p["po"], p["qo"], p["he_o"])
    return d, -v, np.sqrt(u @ u) / (2 * (SAMPLES - 1))


@pytest.mark.parametrize("arm", ["ball", "capsule", "cuboid"])
def test_2_the_gap_is_the_distance_of_the_cores_minus_the_radii(arm):
    dt = np.float64
    eps = float(np.finfo(dt).eps)
    poses = gap_poses(arm)
    assert len(poses) >= 2000
    other = {"ball": BALL, "capsule": CAPSULE, "cuboid": CUBOID}[arm]
    radii = lambda p: p["he_c"][0] + (p["he_o"][0] if arm != "cuboid" else 0.0)
    checked_n = touching = penetrating = 0
    f = lambda a: tuple(dt(x) for x in a)
    for p in poses:
        if p["touch"]:
            _, v, _ = independent(arm, p)
            nv = np.sqrt(v @ v)
            if nv > 0:      # along the minimal vector until the shapes touch
                p["po"] = np.asarray(p["po"] - np.asarray(v / nv * (nv - LD(radii(p))), np.float64), np.float64)
        dist, v, samp = independent(arm, p)
        scale = float(np.abs(p["pc"]).max() + np.abs(p["po"]).max() + sum(p["he_c"][:2]) + (max(p["he_o"]) if arm == "cuboid" else sum(p["he_o"][:2])))
        band = 32 * eps * scale
        cap = (CAPSULE, f(p["he_c"]), f(p["pc"]), f(p["qc"]))
        oth = (other, f(p["he_o"]), f(p["po"]), f(p["qo"]))
        first, second = (cap, oth) if p["cap_first"] else (oth, cap)
        with np.errstate(all="ignore"):
            g, n = CAPR.gap(*first, *second, dt)
        want = float(dist) - radii(p)
        assert want - float(samp) - band <= float(g) <= want + band, (arm, p, float(g), want, band)
        exact = float(np.sqrt(v @ v)) - radii(p)
        touching += abs(exact) <= 1e-9
        penetrating += exact < -1e-9
        if float(dist) > band:
            nn = np.array(n, np.float64)
            assert abs(np.linalg.norm(nn) - 1) <= 8 * eps
            m = np.asarray(v, np.float64) * (1.0 if p["cap_first"] else -1.0)      # from collider 1 towards 2
            m /= np.linalg.norm(m)
            assert nn @ m > 0
            b = (band + float(samp)) / float(dist)
            assert np.linalg.norm(np.cross(nn, m)) <= math.sqrt(4 * b + 2 * b * b) + 8 * eps, (arm, p, nn, m)
            checked_n += 1
    assert touching >= len(poses) // 4 and penetrating >= len(poses) // 8 and checked_n >= len(poses) // 2, (touching, penetrating, checked_n)


def test_2_a_core_point_on_the_other_core_answers_minus_the_radii_and_the_named_axis():
    dt = np.float64
    f = lambda a: tuple(dt(x) for x in a)
    cap = (CAPSULE, f((0.1, 0.5, 0)), f((0, 0, 0)), f(IDENT))
    up = (0.0, 1.0, 0.0)
    for other, want in (((BALL, f((0.2, 0, 0)), f((0, 0.25, 0)), f(IDENT)), -(0.1 + 0.2)),                       # the ball's centre on the core
                        ((CAPSULE, f((0.3, 0.4, 0)), f((0, 0.125, 0)), f(IDENT)), -(0.1 + 0.3)),                    # collinear cores that overlap
                        ((CUBOID, f((0.2, 0.2, 0.2)), f((0.05, 0.3, 0)), f(IDENT)), -0.1)):                         # the core crosses the box
        for first, second in ((cap, other), (other, cap)):
            g, n = CAPR.gap(*first, *second, dt)
            assert float(g) == want and tuple(float(x) for x in n) == up


def test_2_rho_of_a_capsule_is_its_half_length_plus_its_radius():
    for bits in BITS:
        dt = DT[bits]
        assert CAPR.rho(CAPSULE, (dt(0.1), dt(0.3), dt(0)), dt) == dt(0.3) + dt(0.1)
        assert CAPR.rho(BALL, (dt(0.1), dt(0), dt(0)), dt) == NL.rho(BALL, (dt(0.1), dt(0), dt(0)), dt)


# ---- 3. a capsule that only spins ---------------------------------------------------------------------------------------------------------------
SPIN_R, SPIN_H, SPIN_OMEGA, SPIN_D, SPIN_WALL_TH = 0.05, 0.5, 40.0, 0.3, 0.05
SPIN_WALL_HE = (SPIN_WALL_TH, 2.0, 2.0)
SPIN_WALL_POS = (SPIN_D + SPIN_WALL_TH, 0.0, 0.0)


def spin_t_star():
    return math.asin((SPIN_D - SPIN_R) / SPIN_H) / SPIN_OMEGA


def spin_exact_gap(t, omega=SPIN_OMEGA):
    return SPIN_D - SPIN_R - SPIN_H * abs(math.sin(omega * t))


def spin_band(bits):
    """The forward-error bound of spatial_cast_exact_geometry with the capsule's bounding box (r, h + r, r) standing for it."""
    return XC.scale_of(bits, Collider(X_CUBOID, (SPIN_R, SPIN_H + SPIN_R, SPIN_R), (0, 0, 0), IDENT), Collider(X_CUBOID, SPIN_WALL_HE, SPIN_WALL_POS, IDENT))[1]


def spin_advance(bits, capsule_first, cap=CAPR.CCD_NL_ROUNDS):
    dt = DT[bits]
    hc, hw = tuple(dt(x) for x in (SPIN_R, SPIN_H, 0)), tuple(dt(x) for x in SPIN_WALL_HE)
    zero = (0.0, 0.0, 0.0)
    mc = NL.motion(zero, IDENT, zero, zero, (0.0, 0.0, SPIN_OMEGA), CAPR.rho(CAPSULE, hc, dt), dt)
    mw = NL.motion(SPIN_WALL_POS, IDENT, zero, zero, zero, CAPR.rho(CUBOID, hw, dt), dt)
    d = (dt(0), dt(0), dt(0))
    a, b = ((CAPSULE, hc, mc), (CUBOID, hw, mw)) if capsule_first else ((CUBOID, hw, mw), (CAPSULE, hc, mc))
    return CAPR.advance(*a, *b, d, CR.dt_adjusted(DT_NS, dt), dt(TOL), dt, cap)


@pytest.mark.parametrize("capsule_first", [True, False])
@pytest.mark.parametrize("bits", BITS)
def test_3_a_capsule_that_only_spins_is_stopped_before_its_cap_reaches_the_wall(bits, capsule_first):
    dt = DT[bits]
    res, toi, rounds = spin_advance(bits, capsule_first)
    ts = spin_t_star()
    assert res == CAPR.HIT and 1 < rounds <= CAPR.CCD_NL_ROUNDS and 0 < ts < 1 / 60
    assert 0 < float(toi) <= ts
    band = spin_band(bits)
    g = spin_exact_gap(float(toi))
    assert -band < g <= TOL + band, (g, band)
    assert abs(spin_exact_gap(ts)) < 1e-15
    # Linear answers nothing: d = 0
    hc = tuple(dt(x) for x in (SPIN_R, SPIN_H, 0))
    d = (dt(0), dt(0), dt(0))
    if capsule_first:
        hit, _, _ = CAPR.pair_cast(CUBOID, SPIN_WALL_HE, SPIN_WALL_POS, IDENT, d, CR.dt_adjusted(DT_NS, dt), CAPSULE, hc, (0, 0, 0), IDENT, dt)
    else:
        hit, _, _ = CAPR.pair_cast(CAPSULE, hc, (0, 0, 0), IDENT, d, CR.dt_adjusted(DT_NS, dt), CUBOID, SPIN_WALL_HE, SPIN_WALL_POS, IDENT, dt)
    assert not hit


# ---- 4. without spin NonLinear never answers later than the Linear cast ---------------------------------------------------------------------------
Q_TURN = tuple(np.array([0.2, -0.3, 0.1, 0.9]) / np.linalg.norm([0.2, -0.3, 0.1, 0.9]))
COMBOS = {   # (collider 1, cast shape 2): kind, half extents
    "cuboid<-capsule": ((CUBOID, (0.05, 1.0, 2.0)), (CAPSULE, (0.1, 0.3, 0.0))),
    "ball<-capsule": ((BALL, (0.4, 0.0, 0.0)), (CAPSULE, (0.1, 0.3, 0.0))),
    "capsule<-ball": ((CAPSULE, (0.05, 1.0, 0.0)), (BALL, (0.07, 0.0, 0.0))),
    "capsule<-cuboid": ((CAPSULE, (0.05, 1.0, 0.0)), (CUBOID, (0.05, 0.08, 0.06))),
    "capsule<-capsule": ((CAPSULE, (0.05, 1.0, 0.0)), (CAPSULE, (0.1, 0.3, 0.0))),
}


@pytest.mark.parametrize("speed", [30.0, 77.7, 240.0])
@pytest.mark.parametrize("combo", sorted(COMBOS))
@pytest.mark.parametrize("bits", BITS)
def test_4_without_spin_the_mode_does_not_push_a_hit_later(bits, combo, speed):
    dt = DT[bits]
    (s1, he1), (s2, he2) = COMBOS[combo]
    he1, he2 = tuple(dt(x) for x in he1), tuple(dt(x) for x in he2)
    pos1, rot1 = (0.0, 0.0, 0.0), IDENT
    pos2, rot2 = (-1.0, 0.07, 0.03), Q_TURN
    zero = (0.0, 0.0, 0.0)
    v2 = (speed, 0.0, 0.0)
    dt_step = dt(1.0) if speed < 100 else CR.dt_adjusted(DT_NS, dt)
    m1 = NL.motion(pos1, rot1, zero, zero, zero, CAPR.rho(s1, he1, dt), dt)
    m2 = NL.motion(pos2, rot2, zero, v2, zero, CAPR.rho(s2, he2, dt), dt)
    d = tuple(dt(x) for x in v2)
    res, toi, rounds = CAPR.advance(s1, he1, m1, s2, he2, m2, d, dt_step, dt(TOL), dt)
    hit, lin, _ = CAPR.pair_cast(s2, he2, pos2, rot2, d, dt_step, s1, he1, pos1, rot1, dt)
    assert hit and res == CAPR.HIT and 0 < float(toi) <= float(lin), (toi, lin, rounds)
    assert float(lin) - float(toi) < 0.5 / speed        # and not by much: the two answers are the same approach


# ---- 5. a capsule without length is the ball ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_5_a_capsule_of_length_zero_answers_as_the_ball(bits):
    """Both modes, the capsule as collider and as cast shape, against balls and cuboids.  Unit speed, so that the cast's time is a length and the
    bound is test_spatial_capsule_cpu.py's for the same identity: BAND_EPS eps scale, scale = |pos2| + 1 + |pos1| + max half-extent + toi."""
    dt = DT[bits]
    eps = float(np.finfo(dt).eps)
    rng = np.random.default_rng(23)
    f = lambda a: tuple(dt(x) for x in a)
    seen = {"lin": 0, "nl": 0}
    zero = (0.0, 0.0, 0.0)
    for i in range(60):
        r = float(dt(rng.uniform(0.1, 0.8)))
        other = BALL if i % 2 else CUBOID
        he_o = f((rng.uniform(0.1, 0.8), 0, 0)) if other == BALL else f(rng.uniform(0.1, 0.8, 3))
        pos_o, rot_o = f(rng.uniform(-1, 1, 3)), f(unit_quat(rng))
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        pos_c, rot_c = f(np.array(pos_o, np.float64) + u * rng.uniform(2.5, 4.0)), f(unit_quat(rng))
        aim = -u + 0.15 * rng.normal(size=3)
        d_c = aim / np.linalg.norm(aim)                                      # the capsule's velocity, unit speed
        for cap_is_cast in (True, False):
            answers = {}
            for kind, he in ((CAPSULE, f((r, 0.0, 7.0))), (BALL, f((r, 0.0, 0.0)))):
                if cap_is_cast:
                    a1, a2, d = (other, he_o, pos_o, rot_o), (kind, he, pos_c, rot_c), f(d_c)
                else:
                    a1, a2, d = (kind, he, pos_c, rot_c), (other, he_o, pos_o, rot_o), f(-d_c)
                hit, t, _ = CAPR.pair_cast(a2[0], a2[1], a2[2], a2[3], d, dt(10.0), *a1, dt)
                v1, v2 = (zero, d_c) if cap_is_cast else (d_c, zero)
                m1 = NL.motion(a1[2], a1[3], zero, v1, zero, CAPR.rho(a1[0], a1[1], dt), dt)
                m2 = NL.motion(a2[2], a2[3], zero, v2, zero, CAPR.rho(a2[0], a2[1], dt), dt)
                res, tn, _ = CAPR.advance(a1[0], a1[1], m1, a2[0], a2[1], m2, d, dt(10.0), dt(TOL), dt)
                answers[kind] = (hit, float(t), res, float(tn))
            (ch, ct, cres, ctn), (bh, bt, bres, btn) = answers[CAPSULE], answers[BALL]
            scale = max(abs(float(x)) for x in pos_c) + 1.0 + max(abs(float(x)) for x in pos_o) + max(float(x) for x in he_o) + max(ct, bt, ctn, btn)
            tol = XC.BAND_EPS * eps * scale
            assert ch == bh and cres == bres
            if ch:
                assert abs(ct - bt) <= tol, (ct, bt, tol)
                seen["lin"] += 1
            if cres == CAPR.HIT:
                assert abs(ctn - btn) <= tol, (ctn, btn, tol)
                seen["nl"] += 1
    assert seen["lin"] >= 40 and seen["nl"] >= 40, seen


# ---- 6. the round set ---------------------------------------------------------------------------------------------------------------------------
def test_6_the_batched_advancement_is_the_reference_bit_for_bit():
    """swept_ccd_capsule_rounds.batch_advance runs the whole set at once; on a slice that holds every combination and kind it must return what
    the scalar reference returns pair by pair: outcome, time and rounds."""
    pairs = rounds_set()[:400]
    res, t, rounds = batch_advance(pairs, CAPR.CCD_NL_ROUNDS)
    newton = batch_newton_rounds(pairs)
    for i, p in enumerate(pairs):
        want, want_newton = run_pair(p, CAPR.CCD_NL_ROUNDS)
        assert (int(res[i]), float(t[i]), int(rounds[i])) == (want[0], float(want[1]), want[2]), (i, p["combo"], p["kind"])
        assert int(newton[i]) == want_newton, (i, p["combo"], p["kind"])


def test_6_the_round_set_leaves_the_recorded_counts():
    pairs = rounds_set()
    assert len(pairs) == ROUNDS_PAIRS == 20000
    assert [sum(1 for p in pairs if p["kind"] == k) for k in range(4)] == [ROUNDS_PAIRS // 4] * 4
    assert [sum(1 for p in pairs if p["combo"] == c) for c in range(5)] == [ROUNDS_PAIRS // 5] * 5
    assert all(CAPSULE in p["shape"] for p in pairs)
    res, _, rounds = batch_advance(pairs, CAPR.CCD_NL_ROUNDS)
    exhausted = int((res == CAPR.EXHAUSTED).sum())
    capped = int((batch_newton_rounds(pairs) == CAPR.SP_CAPSULE_ROUNDS).sum())
    print("exhausted under the cap of", CAPR.CCD_NL_ROUNDS, ":", exhausted, "; Linear Newton casts that end on SP_CAPSULE_ROUNDS:", capped)
    assert exhausted == ROUNDS_EXHAUSTED_UNDER_CAP
    assert capped == ROUNDS_NEWTON_CAPPED
    assert int((res == CAPR.HIT).sum()) > ROUNDS_PAIRS // 10 and int((res == CAPR.MISSED).sum()) > ROUNDS_PAIRS // 10
