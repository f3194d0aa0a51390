"""CPU: tests/swept_ccd_nonlinear_reference.py (SweepMode::NonLinear as include/avian_mi355x_ccd.h defines it, N0 - N4) against independent
float64 geometry, and the measured round cap.

THE ROD (tests/swept_ccd_nonlinear_rod.py).  A cuboid he = (L, w, w) spins at omega about z beside a wall whose face is the plane y = D, hypot(L, w) > D > w.  The corner (L, w)
touches at t* = (asin(D / rho) - atan2(w, L)) / omega, rho = hypot(L, w).  The exact gap at any time is D minus the largest y of the eight
corners, computed with float64 rotation matrices about the centre of mass: a second derivation of the pose that shares no code with the
reference.  `band` is the forward-error bound of spatial_cast_exact_geometry (32 eps * scale).

THE ROUNDS SET.  rounds_set() is the fixed random set the cap CCD_NL_ROUNDS was measured on (tools/swept_ccd_nonlinear_rounds.py runs the
reference over it with a cap of 4096 and writes profiles/swept_ccd_nonlinear_rounds.txt); the test below asserts that under the chosen cap the
set stays within the share of exhausted pairs recorded there and in DESIGN 4.10."""
import math

import numpy as np
import pytest

import spatial_shape_reference as S
import swept_ccd_nonlinear_reference as NL
import swept_ccd_reference as CR
from swept_ccd_nonlinear_rod import ROD_L, ROD_OMEGA, ROD_W, TOL, WALL_HE, WALL_POS, band_of, exact_rod_gap, rot_z, t_star

BITS = [32, 64]
DT = {32: np.float32, 64: np.float64}
DT_NS = 16666667
BALL, CUBOID = NL.SHAPE_BALL, NL.SHAPE_CUBOID

def rod_advance(bits, omega=(0.0, 0.0, ROD_OMEGA), v=(0.0, 0.0, 0.0), com=(0.0, 0.0, 0.0), pos=(0.0, 0.0, 0.0), tol=TOL, cap=NL.CCD_NL_ROUNDS, trace=None):
    dt = DT[bits]
    he1 = tuple(dt(x) for x in (ROD_L, ROD_W, ROD_W))
    he2 = tuple(dt(x) for x in WALL_HE)
    ident, zero = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
    m1 = NL.motion(pos, ident, com, v, omega, NL.rho(CUBOID, he1, dt), dt)
    m2 = NL.motion(WALL_POS, ident, zero, zero, zero, NL.rho(CUBOID, he2, dt), dt)
    d = tuple(-dt(x) for x in v)
    return NL.advance(CUBOID, he1, m1, CUBOID, he2, m2, d, CR.dt_adjusted(DT_NS, dt), dt(tol), dt, cap, trace)


@pytest.mark.parametrize("bits", BITS)
def test_a_the_spinning_rod_stops_before_its_corner_reaches_the_wall(bits):
    res, toi, rounds = rod_advance(bits)
    assert res == NL.HIT and 1 < rounds <= NL.CCD_NL_ROUNDS
    ts = t_star()
    assert 0 < ts < 1 / 60
    assert 0 < float(toi) <= ts
    band = band_of(bits, (ROD_L, ROD_W, ROD_W), (0, 0, 0), WALL_HE, WALL_POS)
    g = exact_rod_gap(float(toi), (ROD_L, ROD_W, ROD_W), (0, 0, 0), (0, 0, 0), (0, 0, 0), ROD_OMEGA)
    assert -band < g <= TOL + band, (g, band)
    # the closed form and the corner search agree: the scene is what the docstring says it is
    assert abs(exact_rod_gap(ts, (ROD_L, ROD_W, ROD_W), (0, 0, 0), (0, 0, 0), (0, 0, 0), ROD_OMEGA)) < 1e-12
    # and the linear cast sees nothing: d = 0
    dt = DT[bits]
    hit, _ = CR.pair_cast(CUBOID, WALL_HE, WALL_POS, (0, 0, 0, 1), (dt(0), dt(0), dt(0)), CR.dt_adjusted(DT_NS, dt), CUBOID, (ROD_L, ROD_W, ROD_W), (0, 0, 0), (0, 0, 0, 1), dt)
    assert not hit


@pytest.mark.parametrize("speed", [30.0, 77.7, 240.0])
@pytest.mark.parametrize("bits", BITS)
def test_b_without_spin_the_mode_does_not_push_a_hit_later(bits, speed):
    dt = DT[bits]
    pos, v = (0.013, -0.1, 0.02), (0.0, speed, 0.0)
    res, toi, rounds = rod_advance(bits, omega=(0, 0, 0), v=v, pos=pos)
    assert res == NL.HIT and rounds == 2     # one jump along the face normal lands within the tolerance
    d = tuple(-dt(x) for x in v)
    hit, lin = CR.pair_cast(CUBOID, WALL_HE, WALL_POS, (0, 0, 0, 1), d, CR.dt_adjusted(DT_NS, dt), CUBOID, (ROD_L, ROD_W, ROD_W), pos, (0, 0, 0, 1), dt)
    assert hit and float(toi) <= float(lin), (toi, lin)
    band = band_of(bits, (ROD_L, ROD_W, ROD_W), pos, WALL_HE, WALL_POS)
    assert exact_rod_gap(float(toi), (ROD_L, ROD_W, ROD_W), pos, (0, 0, 0), v, 0.0) <= TOL + band


@pytest.mark.parametrize("bits", BITS)
def test_c_a_rod_that_turns_about_an_offset_centre_of_mass(bits):
    dt = DT[bits]
    com, pos, v = (-0.2, -0.05, 0.03), (0.05, -0.02, 0.0), (1.5, 2.0, -0.5)
    he = (ROD_L, ROD_W, ROD_W)
    m = NL.motion(pos, (0, 0, 0, 1), com, v, (0, 0, ROD_OMEGA), NL.rho(CUBOID, tuple(dt(x) for x in he), dt), dt)
    eps = float(np.finfo(dt).eps)
    for t in (0.0, 0.004, 1 / 60):
        p, q = NL.pose(m, dt(t), dt)
        # the second derivation: the centre of mass moves on a line, the origin turns about it
        c = np.asarray(pos) + np.asarray(com) + np.asarray(v) * t
        want = c - rot_z(ROD_OMEGA * t) @ np.asarray(com)
        assert np.abs(np.array(p, np.float64) - want).max() <= 64 * eps
        assert abs(float(q[2]) - math.sin(ROD_OMEGA * t / 2)) <= 16 * eps and abs(float(q[3]) - math.cos(ROD_OMEGA * t / 2)) <= 16 * eps
    res, toi, _ = rod_advance(bits, v=v, com=com, pos=pos)
    assert res == NL.HIT and float(toi) > 0
    band = band_of(bits, he, pos, WALL_HE, WALL_POS)
    g = exact_rod_gap(float(toi), he, pos, com, v, ROD_OMEGA)
    assert -band < g <= TOL + band, (g, band)
    # at no earlier time does the rod reach the wall: the answer is not a later touch
    ts = np.linspace(0.0, float(toi), 400, endpoint=False)
    assert min(exact_rod_gap(float(t), he, pos, com, v, ROD_OMEGA) for t in ts) > g - band > -band


@pytest.mark.parametrize("bits", BITS)
def test_d_spin_about_the_axis_and_a_receding_pair_miss_in_one_round(bits):
    res, _, rounds = rod_advance(bits, omega=(0.0, ROD_OMEGA, 0.0))         # omega parallel to n: the rod sweeps a plane parallel to the wall
    assert (res, rounds) == (NL.MISSED, 1)
    res, _, rounds = rod_advance(bits, omega=(0, 0, 0), v=(0.0, -50.0, 3.0))
    assert (res, rounds) == (NL.MISSED, 1)
    dt = DT[bits]
    ball = lambda pos, v, r: NL.motion(pos, (0, 0, 0, 1), (0, 0, 0), v, (0, 0, 0), r, dt)
    he = lambda r: (dt(r), dt(0), dt(0))
    res, _, rounds = NL.advance(BALL, he(0.1), ball((0, 0, 0), (0, 0, 0), 0.1), BALL, he(0.2), ball((1, 0, 0), (5, 0, 0), 0.2), (dt(5), dt(0), dt(0)), CR.dt_adjusted(DT_NS, dt), dt(TOL), dt)
    assert (res, rounds) == (NL.MISSED, 1)


@pytest.mark.parametrize("bits", BITS)
def test_the_sat_sweeps_are_those_of_the_shape_reference(bits):
    """The scalar sweeps of swept_ccd_nonlinear_reference return the separations of spatial_shape_reference's broadcasting ones, bit for bit."""
    dt = DT[bits]
    rng = np.random.default_rng(5)
    for _ in range(50):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        r = tuple(dt(x) for x in q)
        t = tuple(dt(x) for x in rng.uniform(-2, 2, 3))
        he1, he2 = (tuple(dt(x) for x in rng.uniform(0.05, 1, 3)) for _ in range(2))
        col = lambda a: tuple(np.array([x], dt) for x in a)
        with np.errstate(all="ignore"):
            assert NL.sat_normal_oneway(he1, he2, r, t, dt)[0] == S.sat_normal_oneway(col(he1), col(he2), col(r), col(t), dt)[0]
            sep, axis = NL.sat_edge_twoway(he1, he2, r, t, dt)
            assert sep == S.sat_edge_twoway(col(he1), col(he2), col(r), col(t), dt)[0]
            assert abs(float(np.sqrt(S.na_dot(axis, axis))) - 1) < 8 * float(np.finfo(dt).eps)


def test_an_interior_gap_is_minus_the_radius_and_grows_monotonically_outside():
    dt = np.float64
    he = (dt(0.5), dt(0.2), dt(0.3))
    ident = (dt(0), dt(0), dt(0), dt(1))
    z = (dt(0), dt(0), dt(0))
    g, n = NL.gap(CUBOID, he, z, ident, BALL, (dt(0.1), dt(0), dt(0)), (dt(0.1), dt(0.15), dt(0)), ident, dt)
    assert g == -0.1 and n == (0.0, 1.0, 0.0)                     # the nearest face is +y
    g, n = NL.gap(BALL, (dt(0.1), dt(0), dt(0)), (dt(0.1), dt(0.15), dt(0)), ident, CUBOID, he, z, ident, dt)
    assert g == -0.1 and n == (0.0, -1.0, 0.0)                    # from the ball (collider 1) towards the cuboid
    g, n = NL.gap(CUBOID, he, z, ident, BALL, (dt(0.1), dt(0), dt(0)), (dt(0.9), dt(0.5), dt(0)), ident, dt)
    assert abs(float(g) - (0.5 - 0.1)) < 1e-15 and abs(n[0] - 0.8) < 1e-15 and abs(n[1] - 0.6) < 1e-15


# ---- (e) the rounds set ------------------------------------------------------------------------------------------------------------------------
ROUNDS_SEED, ROUNDS_PAIRS, ROUNDS_MEASURE_CAP = 20261020, 20000, 4096
# what tools/swept_ccd_nonlinear_rounds.py measured on this set with a cap of 4096 (profiles/swept_ccd_nonlinear_rounds.txt)
ROUNDS_P999, ROUNDS_MAX, ROUNDS_EXHAUSTED_UNDER_CAP = 42, 119, 10


def rounds_set(n=ROUNDS_PAIRS, seed=ROUNDS_SEED):
    """n Ball / Cuboid pairs: sizes 0.02 .. 2, |v| up to 300, |omega| up to 100, dt = 1 / 60; kind 0: general, 1: aimed to graze, 2: pure spin,
    3: pure translation (a quarter each, interleaved)."""
    rng = np.random.default_rng(seed)
    unit = lambda: (lambda x: x / np.linalg.norm(x))(rng.normal(size=3))
    out = []
    for i in range(n):
        kind = i % 4
        shapes = [int(rng.integers(0, 2)) for _ in range(2)]
        hes, radii = [], []
        for s in shapes:
            size = np.exp(rng.uniform(np.log(0.02), np.log(2.0), 3))
            hes.append((size[0], 0.0, 0.0) if s == BALL else tuple(size))
            radii.append(size[0] if s == BALL else float(np.linalg.norm(size)))
        rots = [unit4(rng) for _ in range(2)]
        speed = [rng.uniform(0, 300) for _ in range(2)]
        spin = [rng.uniform(0, 100) for _ in range(2)]
        if kind == 2:
            speed = [0.0, 0.0]
        if kind == 3:
            spin = [0.0, 0.0]
        reach = (speed[0] + speed[1]) / 60 + radii[0] + radii[1]
        u = unit()
        dist = rng.uniform(0.2, 1.0) * reach + (radii[0] + radii[1]) * rng.uniform(0.0, 0.3)
        p2 = u * dist
        if kind == 1:      # body 1 flies past body 2 so that the bounding spheres about graze
            side = np.cross(u, unit()); side /= np.linalg.norm(side)
            aim = p2 + side * (radii[0] + radii[1]) * rng.uniform(0.5, 1.05)
            v1, v2 = aim / np.linalg.norm(aim) * speed[0], np.zeros(3)
        else:
            v1, v2 = (u + 0.3 * unit()) * speed[0], (-u + 0.3 * unit()) * speed[1]
        out.append(dict(kind=kind, shape=shapes, he=hes, pos=[np.zeros(3), p2], rot=rots, v=[v1, v2], om=[unit() * spin[0], unit() * spin[1]],
                        com=[np.zeros(3), np.zeros(3)] if i % 8 < 4 else [unit() * 0.3 * radii[0], unit() * 0.3 * radii[1]]))
    return out


def unit4(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def run_rounds_pair(p, cap, bits=64):
    dt = DT[bits]
    he = [tuple(dt(x) for x in h) for h in p["he"]]
    m = [NL.motion(p["pos"][k], p["rot"][k], p["com"][k], p["v"][k], p["om"][k], NL.rho(p["shape"][k], he[k], dt), dt) for k in range(2)]
    d = tuple(b - a for a, b in zip(m[0]["v"], m[1]["v"]))
    return NL.advance(p["shape"][0], he[0], m[0], p["shape"][1], he[1], m[1], d, CR.dt_adjusted(DT_NS, dt), dt(TOL), dt, cap)


def test_e_the_rounds_set_stays_within_the_caps_recorded_share():
    assert ROUNDS_P999 is not None, "the cap has not been measured"
    cap = NL.CCD_NL_ROUNDS
    assert cap & (cap - 1) == 0 and cap >= ROUNDS_P999 and cap // 2 < ROUNDS_P999     # the smallest power of two >= the 99.9th percentile
    pairs = rounds_set()
    assert len(pairs) == ROUNDS_PAIRS and [sum(1 for p in pairs if p["kind"] == k) for k in range(4)] == [ROUNDS_PAIRS // 4] * 4
    results = [run_rounds_pair(p, cap) for p in pairs]
    exhausted = sum(1 for r in results if r[0] == NL.EXHAUSTED)
    assert exhausted <= ROUNDS_EXHAUSTED_UNDER_CAP <= ROUNDS_PAIRS // 1000        # at most the share beyond the 99.9th percentile
    assert sum(1 for r in results if r[0] == NL.HIT) > ROUNDS_PAIRS // 10 and sum(1 for r in results if r[0] == NL.MISSED) > ROUNDS_PAIRS // 10
    assert max(r[2] for r in results) == (cap if exhausted else min(cap, ROUNDS_MAX))


# ---- (f) N0 -------------------------------------------------------------------------------------------------------------------------------------
def test_f_the_pairs_mode_goes_by_body():
    L, N = NL.SWEEP_LINEAR, NL.SWEEP_NON_LINEAR
    # (the entry's mode, b2 listed?, b2's mode) -> NonLinear?
    for entry_mode, listed2, mode2, want in ((L, False, None, False), (N, False, None, True), (L, True, L, False), (L, True, N, True), (N, True, L, True), (N, True, N, True)):
        listed = {0: entry_mode}
        if listed2:
            listed[1] = mode2
        assert NL.pair_is_nonlinear(entry_mode, 1, listed) is want, (entry_mode, listed2, mode2)


@pytest.mark.parametrize("modes,want", [((0, None), 0), ((1, None), 1), ((0, 0), 0), ((0, 1), 2), ((1, 0), 2), ((1, 1), 2)])
def test_f_a_whole_pass_counts_its_nonlinear_pair_tests(modes, want):
    """Two dynamic balls closing in on each other, one pair row; body 1 listed or not.  The pair is tested once per listed body."""
    bits, dt = 64, np.float64
    cols = dict(entity=np.array([100, 101]), body=np.array([0, 1]), shape=np.array([BALL, BALL]), half_extents=np.array([[0.1, 0, 0], [0.1, 0, 0]]), child=np.array([0, 0]))
    scene = dict(colliders=cols, pairs=[(0, 1)], rb_type=np.array([0, 0]), body_flags=np.array([0, 0]))
    ident = np.tile([0.0, 0, 0, 1], (2, 1))
    state = dict(position=np.array([[0.0, 0, 0], [1.0, 0, 0]]), rotation=ident, linear_velocity=np.array([[60.0, 0, 0], [-30.0, 0, 0]]), angular_velocity=np.zeros((2, 3)),
                 delta_position=np.zeros((2, 3)), delta_rotation=ident.copy())
    entries = [dict(body=b, mode=m, include_dynamic=1, linear_threshold=0.0, angular_threshold=0.0) for b, m in enumerate(modes) if m is not None]
    rec, dp, dq, stats = NL.swept_ccd(bits, entries, scene, state, DT_NS, float(np.finfo(np.float64).max))
    assert stats["nonlinear_tested"] == want and stats["exhausted"] == 0
    assert (rec["tested"] == 1).all() and (rec["hit_body"] >= 0).all()
    lin, *_ = CR.swept_ccd(bits, entries, scene, state, DT_NS, float(np.finfo(np.float64).max))
    assert (rec["toi"] <= lin["toi"]).all() and (lin["toi"] - rec["toi"] < (TOL + 1e-9) / 90).all()    # touching within the tolerance, closing at 90
