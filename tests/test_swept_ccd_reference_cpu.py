"""CPU: the numpy restatement of swept CCD (tests/swept_ccd_reference.py) against analytic geometry and against the serial loop it transcribes.

The time of impact is a cast along an UNNORMALISED direction d = v2 - v1, so the cast's distance is time.  The forward-error bound of
tests/spatial_cast_exact_geometry.py is a bound on positions (band = 32 eps * scale, plus the square root's grazing term on round features):
a position error of `bound` along a motion of speed |d| is a time error of bound / |d|, and the quotient that turns the entry into a time adds
its own rounding, 4 eps * toi.  That sum is the tolerance below; nothing in it comes from the values under test."""
import numpy as np
import pytest

from helpers import F
import spatial_cast_exact_geometry as XC
from spatial_exact_geometry import EPS
from spatial_shape_exact_geometry import Shape
import swept_ccd_reference as CR
import swept_ccd_scenes as SC

DTYPES = {32: np.float32, 64: np.float64}


def time_bound(bits, shape2, he2, pos2, d, shape1, he1, pos1, toi):
    ident = (0, 0, 0, 1)
    q, c = Shape(shape2, he2, pos2, ident), XC.Collider(shape1, he1, pos1, ident)
    exact = XC.cast(q, tuple(float(x) for x in d), c)
    speed = float(np.sqrt(sum(float(x) ** 2 for x in d)))
    _, band = XC.scale_of(bits, q, c, distance=float(toi) * speed)
    return exact, XC.distance_bound(band, exact, q, c) / speed + 4 * EPS[bits] * float(toi)


@pytest.mark.parametrize("bits", [32, 64])
def test_ball_against_wall_is_gap_over_speed(bits):
    dt = DTYPES[bits]
    # the tunnelling scene: a ball r = 0.05 at x = -1 moving at 240 towards a wall whose face is at x = -0.05: gap 0.9
    hit, t = CR.pair_cast(F.SHAPE_CUBOID, (0.05, 1, 2), (0, 0, 0), (0, 0, 0, 1), (-240.0, 0, 0), CR.dt_adjusted(SC.DT_NS, dt), F.SHAPE_BALL, (0.05, 0, 0), (-1, 0, 0), (0, 0, 0, 1), dt)
    exact, tol = time_bound(bits, F.SHAPE_CUBOID, (0.05, 1, 2), (0, 0, 0), (-240.0, 0, 0), F.SHAPE_BALL, (0.05, 0, 0), (-1, 0, 0), t)
    assert hit and exact.hit
    assert abs(float(t) - 0.9 / 240) <= tol and abs(float(t) - float(exact.toi)) <= tol, (t, float(exact.toi), tol)
    # slower than gap / dt: no impact inside the step
    hit, _ = CR.pair_cast(F.SHAPE_CUBOID, (0.05, 1, 2), (0, 0, 0), (0, 0, 0, 1), (-50.0, 0, 0), CR.dt_adjusted(SC.DT_NS, dt), F.SHAPE_BALL, (0.05, 0, 0), (-1, 0, 0), (0, 0, 0, 1), dt)
    assert not hit


@pytest.mark.parametrize("bits", [32, 64])
def test_ball_against_moving_ball_is_gap_over_closing_speed(bits):
    dt = DTYPES[bits]
    # ball 1 (r 0.2) at the origin moving at (90, 0, 0); ball 2 (r 0.3) at (1.5, 0, 0) moving at (-30, 0, 0): gap 1.0, closing speed 120
    d = (-30.0 - 90.0, 0.0, 0.0)
    hit, t = CR.pair_cast(F.SHAPE_BALL, (0.3, 0, 0), (1.5, 0, 0), (0, 0, 0, 1), d, CR.dt_adjusted(SC.DT_NS, dt), F.SHAPE_BALL, (0.2, 0, 0), (0, 0, 0), (0, 0, 0, 1), dt)
    exact, tol = time_bound(bits, F.SHAPE_BALL, (0.3, 0, 0), (1.5, 0, 0), d, F.SHAPE_BALL, (0.2, 0, 0), (0, 0, 0), t)
    assert hit and exact.hit
    assert abs(float(t) - 1.0 / 120) <= tol and abs(float(t) - float(exact.toi)) <= tol, (t, float(exact.toi), tol)


@pytest.mark.parametrize("bits", [32, 64])
def test_two_wall_halves_sharing_a_seam_answer_the_same_time(bits):
    dt = DTYPES[bits]
    args = lambda y: (F.SHAPE_CUBOID, (0.05, 0.5, 2), (0, y, 0), (0, 0, 0, 1), (-240.0, 0, 0), CR.dt_adjusted(SC.DT_NS, dt), F.SHAPE_BALL, (0.05, 0, 0), (-1, 0, 0), (0, 0, 0, 1), dt)
    (h1, t1), (h2, t2) = CR.pair_cast(*args(0.5)), CR.pair_cast(*args(-0.5))
    assert h1 and h2 and t1.tobytes() == t2.tobytes()


def _serial(bits, hits, has_sb, state):
    """The reference's loop written out once more, body by body (ccd/mod.rs:644-683), on python lists."""
    dt = DTYPES[bits]
    dp = [list(map(dt, r)) for r in state["delta_position"]]
    dq = [tuple(map(dt, r)) for r in state["delta_rotation"]]
    for b1, b2, toi in hits:
        if toi is None:
            continue
        min_toi = dt(toi) * dt(1.0001)
        for b in (b1, b2):
            if b is None or not has_sb[b]:
                continue
            v = [dt(x) for x in state["linear_velocity"][b]]; w = [dt(x) for x in state["angular_velocity"][b]]
            dp[b] = [min_toi * v[0], min_toi * v[1], min_toi * v[2]]
            dq[b] = CR.qmul(CR.from_scaled_axis((w[0] * min_toi, w[1] * min_toi, w[2] * min_toi), dt), dq[b], dt)
    return np.array(dp, dt), np.array(dq, dt)


@pytest.mark.parametrize("bits", [32, 64])
def test_apply_equals_the_serial_loop_for_colliding_write_sets(bits):
    dt = DTYPES[bits]
    rng = np.random.default_rng(7)
    n = 6
    rb = np.array([0, 0, 0, 1, 2, 0]); flags = np.array([0, 0, 0, 0, 0, 1])   # 3: static, 4: kinematic, 5: asleep
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1)[:, None]
    state = dict(linear_velocity=rng.normal(scale=20, size=(n, 3)).astype(dt), angular_velocity=rng.normal(scale=3, size=(n, 3)).astype(dt),
                 delta_position=rng.normal(size=(n, 3)).astype(dt), delta_rotation=q.astype(dt))
    scene = dict(rb_type=rb, body_flags=flags)
    # bodies 0 and 1 hit body 2 at different times; 2 itself hits 0; then static, kinematic and sleeping targets; one entry without a hit
    hits = [(0, 2, dt(0.004)), (1, 2, dt(0.009)), (2, 0, dt(0.0021)), (1, 3, dt(0.001)), (0, 4, dt(0.0123)), (2, 5, dt(0.0007)), (1, None, None)]
    has_sb = CR.has_solver_body(rb, flags)
    for order in (hits, hits[::-1], [hits[i] for i in (2, 0, 5, 1, 4, 3, 6)]):
        dp, dq = CR.apply_serial(bits, order, scene, state)
        rp, rq = _serial(bits, order, has_sb, state)
        assert dp.tobytes() == rp.tobytes() and dq.tobytes() == rq.tobytes()
        for b in (3, 5):   # no SolverBody: untouched
            assert np.array_equal(dp[b], state["delta_position"][b]) and np.array_equal(dq[b], state["delta_rotation"][b])
    a, b = CR.apply_serial(bits, hits, scene, state), CR.apply_serial(bits, hits[::-1], scene, state)
    assert not np.array_equal(a[1][2], b[1][2]) and not np.array_equal(a[0][2], b[0][2])   # the order shows on the body written twice


def test_from_scaled_axis_is_a_unit_rotation_about_the_axis():
    for dt in (np.float32, np.float64):
        q = CR.from_scaled_axis((dt(0.3), dt(-0.4), dt(1.2)), dt)
        assert abs(sum(float(x) ** 2 for x in q) - 1) < 8 * np.finfo(dt).eps
        assert abs(float(q[3]) - np.cos(0.65)) < 4 * np.finfo(dt).eps
        assert CR.from_scaled_axis((dt(0), dt(0), dt(0)), dt) == (0, 0, 0, 1)
