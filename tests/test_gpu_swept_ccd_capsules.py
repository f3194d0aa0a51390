"""GPU: swept CCD with Capsule colliders (include/avian_mi355x_ccd.h, "capsule colliders"; k_ccd_toi_cap / k_ccd_toi_nl_cap / k_ccd_origin_cap /
k_ccd_origin_nl_cap behind avn_swept_ccd_capsules_set) against tests/swept_ccd_capsule_reference.py at tolerance 0, in f32 and f64.

The two-worlds method of test_gpu_swept_ccd_nonlinear.py: world B steps without a list and supplies the step-start poses and the pre-CCD solver
bodies, world A has the list; A's records, its delta_position / delta_rotation bytes, its unchanged velocities and its avn_swept_ccd_stats must be
the reference's.  Every scene but the one that exists to cross a wave boundary has ten bodies or fewer."""
import math

import numpy as np
import pytest

from avian_amd.swept_ccd import MISS, SWEEP_LINEAR, SWEEP_NON_LINEAR, SweptCcd
from helpers import F, hip_lib
import swept_ccd_capsule_reference as CAPR
import swept_ccd_scenes as SC
import swept_ccd_nonlinear_rod as ROD
import test_gpu_swept_ccd_nonlinear as TN
import test_swept_ccd_capsule_cpu as CPU

pytestmark = pytest.mark.gpu
BITS = [32, 64]
L, N = SWEEP_LINEAR, SWEEP_NON_LINEAR
MODES = [L, N]
CAPSULE = F.SHAPE_CAPSULE
Q_TURN = CPU.Q_TURN
Q_ABOUT_X = (math.sin(0.3), 0.0, 0.0, math.cos(0.3))                      # 0.6 rad about x, the line of flight: the axis leans in the wall's plane
Q_Y_TO_Z = (math.sin(math.pi / 4), 0.0, 0.0, math.cos(math.pi / 4))      # a quarter turn about x: the capsule's axis along z
Q_Y_TO_X = (0.0, 0.0, -math.sin(math.pi / 4), math.cos(math.pi / 4))     # a quarter turn about z: the capsule's axis along x
BULLET = (0.1, 0.3)                                                      # (r, h) of the capsule bullet
ZERO_STATS = dict(nonlinear_tested=0, rounds_max=0, exhausted=0)
entries_of, upload = TN.entries_of, TN.upload


class Scene(TN.Scene):
    """test_gpu_swept_ccd_nonlinear.Scene with capsule colliders: half_extents = (r, h, 0)."""

    def collider(self, body, shape, he, flags=0, child=None):
        slot = super().collider(body, F.SHAPE_CUBOID if shape == CAPSULE else shape, he, flags, child)
        self.c_shape[slot] = shape
        return slot

    def capsule(self, pos, r, h, rb=F.RB_STATIC, ccd=False, cflags=0, **kw):
        b = self.body(pos, rb=rb, **kw)
        self.collider(b, CAPSULE, (r, h, 0.0), cflags | (F.COLLIDER_SWEPT_CCD if ccd else 0))
        return b

    def bullet(self, pos, lv, rh=BULLET, **kw):
        return self.capsule(pos, rh[0], rh[1], rb=F.RB_DYNAMIC, ccd=True, lv=lv, **kw)


def adopt(scene):
    s = Scene(gravity=scene.gravity, margin=scene.margin)
    for k, v in vars(scene).items():
        setattr(s, k, v)
    s.tol, s.com = None, {}
    return s


def check(scene, bits, entries, capsules=True, info=None, exhausted=0, worlds=None):
    """Steps A (list; the switch as given) and B (no list) once; A must equal the reference.  worlds: (A, its SweptCcd, B) of an earlier call whose
    step left A's bodies as B's.  Returns (records, stats, A's solver bodies, B's, A, B, A's SweptCcd)."""
    if worlds is None:
        a, b = scene.world(hip_lib(), bits), scene.world(hip_lib(), bits)
        ccd = SweptCcd(a, non_linear=True, capsules=capsules)
        upload(ccd, entries)
    else:
        a, ccd, b = worlds
        ccd.set_capsules(capsules)
    start = b.bodies_download()
    assert all(a.bodies_download()[k].tobytes() == start[k].tobytes() for k in ("position", "rotation"))
    b.step(); b.synchronize()
    sb = b.solver_bodies_download()
    state = dict(position=start["position"], rotation=start["rotation"], linear_velocity=sb["linear_velocity"], angular_velocity=sb["angular_velocity"],
                 delta_position=sb["delta_position"], delta_rotation=sb["delta_rotation"], center_of_mass=scene.body_kwargs()["center_of_mass"])
    rec, dp, dq, stats = CAPR.swept_ccd(bits, entries, scene.reference_scene(list(b.pairs_get())), state, SC.DT_NS, scene.margin_cfg(),
                                        tol_cfg=0.005 if scene.tol is None else scene.tol, info=info, capsules=capsules)
    a.step(); a.synchronize()
    got, sb_a, got_stats = ccd.results(), a.solver_bodies_download(), ccd.stats()
    assert got.tobytes() == rec.tobytes(), (got, rec)
    assert sb_a["delta_position"].tobytes() == dp.tobytes(), (sb_a["delta_position"], dp)
    assert sb_a["delta_rotation"].tobytes() == dq.tobytes(), (sb_a["delta_rotation"], dq)
    for k in ("linear_velocity", "angular_velocity"):
        assert sb_a[k].tobytes() == sb[k].tobytes(), k   # velocities are never changed
    assert got_stats == {k: stats[k] for k in ("nonlinear_tested", "rounds_max", "exhausted")}, (got_stats, stats)
    assert got_stats["exhausted"] == exhausted
    return got, got_stats, sb_a, sb, a, b, ccd


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
def capsule_at_a_wall(av=(0, 0, 0), walls=((0.0, 0.0, 0.0),), rot=Q_TURN):
    """The capsule bullet, turned so that it is not axis-aligned, at 240 units / s towards 0.1-thick static walls.  Q_TURN: it meets the wall
    with one cap; Q_ABOUT_X: broadside, along its whole side."""
    s = Scene()
    b = s.bullet((-1, 0, 0), (240.0, 0, 0), rot=rot, av=av)
    for p in walls:
        s.cuboid(p, (0.05, 1, 2))
    return s, b


def capsule_at_a_ball():
    s = Scene()
    b = s.bullet((-1, 0.05, 0.02), (240.0, 0, 0), rot=Q_TURN)
    target = s.body((0, 0, 0), rb=F.RB_STATIC)
    s.collider(target, F.SHAPE_BALL, 0.4)
    return s, b


def at_a_bar(kind):
    """A ball or a turned cuboid bullet against a thin static capsule bar along y."""
    s = Scene()
    if kind == "ball":
        b = s.ball((-1, 0.1, 0.01), 0.05, lv=(240.0, 0, 0))
    else:
        b = s.body((-1, 0.1, 0.01), lv=(240.0, 0, 0), rot=Q_TURN)
        s.collider(b, F.SHAPE_CUBOID, (0.05, 0.08, 0.06), F.COLLIDER_SWEPT_CCD)
    s.capsule((0, 0, 0), 0.05, 1.0)
    return s, b


def capsule_at_a_bar(how):
    """skew: the bullet turned, closest points inside both cores; parallel: both axes along y (the segment - segment routine's degenerate
    branch); tips: the bullet above the bar, its lower cap against the bar's upper one."""
    s = Scene()
    if how == "skew":
        b = s.bullet((-1, 0.1, 0.01), (240.0, 0, 0), rot=Q_TURN)
    elif how == "parallel":
        b = s.bullet((-1, 0.2, 0.03), (240.0, 0, 0))
    else:
        b = s.bullet((-1, 1.36, 0.02), (240.0, 0, 0))
    s.capsule((0, 0, 0), 0.05, 1.0)
    return s, b


def capsule_meets_ball():
    """A dynamic CCD capsule and a dynamic ball that comes to meet it: relative speed 210."""
    s = Scene()
    a = s.bullet((-1, 0, 0), (150.0, 0, 0), rot=Q_TURN)
    c = s.ball((1, 0.05, 0), 0.2, lv=(-60.0, 0, 0), ccd=False)
    return s, a, c


def overlapping(kind, speed, margin):
    """A shape that starts overlapping a sensor by 0.01 (the sensor takes no velocity away before the pass).  capsule: an upright capsule against a
    sensor wall; core: the same with its core inside the wall (dist == 0); ball: a ball against a sensor capsule bar."""
    s = Scene(margin=margin)
    if kind == "ball":
        b = s.ball((-0.09, 0, 0), 0.05, lv=(speed, 0, 0))
        s.capsule((0, 0, 0), 0.05, 1.0, cflags=F.COLLIDER_SENSOR)
    else:
        b = s.bullet((-0.09 if kind == "capsule" else -0.04, 0, 0), (speed, 0, 0), rh=(0.05, 0.3))
        s.cuboid((0, 0, 0), (0.05, 1, 2), cflags=F.COLLIDER_SENSOR)
    return s, b


def spinning_capsule(com=None):
    """The capsule of test_swept_ccd_capsule_cpu.py's test 3 beside its wall."""
    s = Scene()
    c = s.bullet((0, 0, 0), (0, 0, 0), rh=(CPU.SPIN_R, CPU.SPIN_H), av=(0, 0, CPU.SPIN_OMEGA))
    if com is not None:
        s.com[c] = com
    s.cuboid(CPU.SPIN_WALL_POS, CPU.SPIN_WALL_HE)
    return s, c


def rod_at_a_bar():
    """The rod of swept_ccd_nonlinear_rod.py spinning beside a static capsule bar along x whose surface reaches down to y = D, where the wall's
    face was: the middle of the rod's far edge touches it at t*."""
    s = Scene()
    rod = s.body((0, 0, 0), av=(0, 0, ROD.ROD_OMEGA))
    s.collider(rod, F.SHAPE_CUBOID, TN.ROD_HE, F.COLLIDER_SWEPT_CCD)
    s.capsule((0, ROD.WALL_D + 0.05, 0), 0.05, 1.0, rot=Q_Y_TO_X)
    return s, rod


def capsule_tie(incoming):
    """SC.tie with an upright capsule centred on the seam of the two wall halves."""
    s = Scene()
    b = s.bullet((1, 0, 0), (-57.0, 0, 0), rh=(0.05, 0.3)) if incoming else s.bullet((-1, 0, 0), (240.0, 0, 0), rh=(0.05, 0.3))
    s.cuboid((0, 0.5, 0), (0.05, 0.5, 2))
    s.cuboid((0, -0.5, 0), (0.05, 0.5, 2))
    return s, b


def write_order():
    """A ball and a capsule bullet at different distances hit one awake dynamic cuboid that moves and spins."""
    s = Scene()
    a = s.ball((-1, 0, 0), 0.05, lv=(200.0, 0, 0))
    b = s.bullet((0, 0, -2), (0, 0, 150.0), rot=Q_TURN)
    c = s.cuboid((0, 0, 0), (0.3, 0.3, 0.3), rb=F.RB_DYNAMIC, lv=(0, 3.0, 0), av=(0, 0, 2.0))
    return s, (a, b, c)


def mixed_traffic(n=72):
    """n bullets on one wall, Ball / Cuboid / Capsule in turn, and a static capsule bar along z in front of the first third of them."""
    s = Scene()
    bullets = []
    for k in range(n):
        pos = (-1, 0, (k - (n - 1) / 2) * 0.2)
        if k % 3 == 0:
            bullets.append(s.ball(pos, 0.05, lv=(240.0, 0, 0)))
        elif k % 3 == 1:
            b = s.body(pos, lv=(240.0, 0, 0), av=(0, 0, 20.0))
            s.collider(b, F.SHAPE_CUBOID, (0.05, 0.08, 0.06), F.COLLIDER_SWEPT_CCD)
            bullets.append(b)
        else:
            bullets.append(s.bullet(pos, (240.0, 0, 0), rh=(0.04, 0.05), av=(0, 0, 20.0)))
    wall = s.cuboid((0, 0, 0), (0.05, 1, 8))
    third = n // 3
    bar = s.capsule((-0.5, 0, (third / 2 - n / 2) * 0.2), 0.05, third * 0.1 - 0.05, rot=Q_Y_TO_Z)   # its core ends between bullets third - 1 and third
    return s, bullets, wall, bar


# ---- 1. the switch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_1_the_switch_gates_the_capsule_pairs(bits):
    scene, bullet = capsule_at_a_wall()
    rec, stats, _, _, a, b, _ = check(scene, bits, entries_of([bullet], L), capsules=False)
    assert rec["tested"][0] == 0 and rec["hit_body"][0] == -1 and rec["hit_collider"][0] == MISS and stats == ZERO_STATS
    assert a.bodies_download()["position"][bullet][0] > 0.1                  # through the wall, as ever
    for k, v in a.bodies_download().items():
        assert v.tobytes() == b.bodies_download()[k].tobytes(), k            # and nothing else differs from a world without a list
    rec, _, _, _, a, b, _ = check(scene, bits, entries_of([bullet], L), capsules=True)
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == 1 and rec["hit_collider"][0] == SC.ENTITY0 + 1
    assert b.bodies_download()["position"][bullet][0] > 0.1 and a.bodies_download()["position"][bullet][0] < -0.05


@pytest.mark.parametrize("bits", BITS)
def test_1_toggling_between_steps_takes_effect_on_the_next_step(bits):
    """Two walls four units apart: the bullet crosses the first in step 1 (switch off: untested), would cross the second in step 2 (switch on:
    stopped)."""
    scene, bullet = capsule_at_a_wall(walls=((0.0, 0.0, 0.0), (4.5, 0.0, 0.0)))
    entries = entries_of([bullet], L)
    rec, _, _, _, a, b, ccd = check(scene, bits, entries, capsules=False)
    assert rec["tested"][0] == 0 and rec["hit_body"][0] == -1
    rec, *_ = check(scene, bits, entries, capsules=True, worlds=(a, ccd, b))
    assert rec["tested"][0] >= 1 and rec["hit_body"][0] == 2
    assert 2.9 < a.bodies_download()["position"][bullet][0] < 4.4 < b.bodies_download()["position"][bullet][0]
    ccd.set_capsules(False)
    a.step(); a.synchronize()
    assert (ccd.results()["tested"] == 0).all()


@pytest.mark.parametrize("name", ["tunnelling", "write_order"])
@pytest.mark.parametrize("bits", BITS)
def test_1_and_8_a_world_without_a_capsule_is_byte_equal_with_the_switch_on_or_off(bits, name):
    """The Ball / Cuboid scenes of swept_ccd_scenes.py over 5 steps: records, solver bodies, bodies, statistics and the number of kernel launches."""
    scene, bodies = getattr(SC, name)()
    entries = SC.entries_of(list(bodies))
    out = []
    for on in (False, True):
        w = scene.world(hip_lib(), bits)
        ccd = SweptCcd(w, capsules=on)
        SC.upload(ccd, entries)
        steps = []
        for _ in range(5):
            w.step(); w.synchronize()
            steps.append((ccd.results().tobytes(), {k: v.tobytes() for k, v in w.solver_bodies_download().items()}, {k: v.tobytes() for k, v in w.bodies_download().items()},
                          w.timers().kernel_launches, ccd.stats()))
        out.append(steps)
    assert out[0] == out[1]
    assert any(np.frombuffer(s[0], ccd.result_dtype)["hit_body"].max() >= 0 for s in out[0])


@pytest.mark.parametrize("bits", BITS)
def test_8_the_capsule_kernels_launch_only_with_the_switch_on_and_a_capsule_in_the_table(bits):
    scene, bullet = capsule_at_a_wall()
    launches = []
    for on in (False, True):
        w = scene.world(hip_lib(), bits)
        ccd = SweptCcd(w, capsules=on)
        upload(ccd, entries_of([bullet], L))
        w.step(); w.synchronize()
        launches.append(w.timers().kernel_launches)
    assert launches[1] == launches[0] + 1            # k_ccd_toi_cap (a Linear list, an unbounded margin)


# ---- 2. Linear: the five role / kind combinations ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_2_a_capsule_bullet_stops_at_a_thin_wall_and_stays_in_front_of_it(bits):
    """The 30 steps that follow belong to the contact solver: each starts touching (t == 0; with the default unbounded margin the origin rule
    answers nothing).  The bullet meets the wall broadside here.  One that meets it with a cap (Q_TURN: test_1, test_2_cap_first) is stopped by the
    pass just the same, but the solver then lets it turn about that cap and through the wall in the next step, at 130 rad / s, as it lets a
    Ball / Cuboid-only world's cuboid rod of the same size ("capsule colliders": measured, an open item of the solver's)."""
    scene, bullet = capsule_at_a_wall(rot=Q_ABOUT_X)
    rec, _, _, _, a, b, _ = check(scene, bits, entries_of([bullet], L))
    assert rec["hit_body"][0] == 1 and 0 < float(rec["toi"][0]) < 0.9 / 240
    assert b.bodies_download()["position"][bullet][0] > 0.1 and a.bodies_download()["position"][bullet][0] < -0.05
    for _ in range(30):
        a.step()
        assert a.bodies_download()["position"][bullet][0] < 0.05


LINEAR_SCENES = {
    "capsule-at-wall-cap-first": capsule_at_a_wall,
    "capsule-at-ball": capsule_at_a_ball,
    "ball-at-bar": lambda: at_a_bar("ball"),
    "cuboid-at-bar": lambda: at_a_bar("cuboid"),
    "capsule-at-bar-skew": lambda: capsule_at_a_bar("skew"),
    "capsule-at-bar-parallel": lambda: capsule_at_a_bar("parallel"),
    "capsule-at-bar-tips": lambda: capsule_at_a_bar("tips"),
}


@pytest.mark.parametrize("name", sorted(LINEAR_SCENES))
@pytest.mark.parametrize("bits", BITS)
def test_2_every_combination_stops_the_bullet(bits, name):
    scene, bullet = LINEAR_SCENES[name]()
    rec, stats, _, _, a, b, _ = check(scene, bits, entries_of([bullet], L))
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == 1 and stats == ZERO_STATS
    assert 0 < float(rec["toi"][0]) < 1.0 / 240
    assert b.bodies_download()["position"][bullet][0] > 0.2 and a.bodies_download()["position"][bullet][0] < 0.0


# ---- 3. both bodies moving -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", BITS)
def test_3_include_dynamic_and_the_thresholds(bits, mode):
    scene, a, c = capsule_meets_ball()
    rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of([a], mode, include_dynamic=1))
    assert rec["hit_body"][0] == c and stats["nonlinear_tested"] == (1 if mode == N else 0)
    for body in (a, c):                                          # both are written
        assert not np.array_equal(sb_a["delta_position"][body], sb_b["delta_position"][body])
    rec, *_ = check(scene, bits, entries_of([a], mode, include_dynamic=0))
    assert rec["tested"][0] == 0 and rec["hit_body"][0] == -1
    v = sb_b["linear_velocity"].astype(np.float64)
    speed = float(np.linalg.norm(v[a] - v[c]))                   # what the pass sees: about 210
    assert 200 < speed < 220
    rec, *_ = check(scene, bits, entries_of([a], mode, linear_threshold=speed * 1.001, angular_threshold=1.0))     # just above the relative speed
    assert rec["tested"][0] == 0 and rec["hit_body"][0] == -1
    rec, *_ = check(scene, bits, entries_of([a], mode, linear_threshold=speed * 0.999, angular_threshold=1.0))     # just below
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == c


# ---- 4. the origin rule with a bounded margin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["capsule", "ball"])
@pytest.mark.parametrize("bits", BITS)
def test_4_the_origin_rule_with_a_bounded_margin(bits, kind, mode):
    info = {}
    scene, body = overlapping(kind, 30.0, 0.02)
    rec, stats, *_ = check(scene, bits, entries_of([body], mode), info=info)
    assert info["origin"] == [1] and rec["hit_body"][0] == 1 and abs(float(rec["toi"][0]) - 0.02 / 30) < 0.0051 / 30      # moving in: the small ball hits
    for args in ((-30.0, 0.02), (30.0, None)):                     # moving out; an unbounded margin
        info = {}
        scene, body = overlapping(kind, *args)
        rec, stats, *_ = check(scene, bits, entries_of([body], mode), info=info)
        assert info["origin"] == [1] and rec["tested"][0] == 1 and rec["hit_body"][0] == -1, args


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("speed", [30.0, -30.0])
@pytest.mark.parametrize("bits", BITS)
def test_4_a_core_that_crosses_the_box_at_the_start(bits, speed, mode):
    info = {}
    scene, body = overlapping("core", speed, 0.02)
    rec, stats, *_ = check(scene, bits, entries_of([body], mode), info=info)
    assert info["origin"] == [1] and rec["tested"][0] == 1
    if mode == N:
        assert stats["nonlinear_tested"] == 1


# ---- 5. NonLinear ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_5_a_capsule_that_only_spins_is_stopped_at_the_wall(bits):
    scene, cap = spinning_capsule()
    rec, stats, *_ = check(scene, bits, entries_of([cap], L))
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == -1 and stats == ZERO_STATS                # d = 0: the linear sweep sees nothing
    rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of([cap], N))
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == 1 and rec["hit_collider"][0] == SC.ENTITY0 + 1
    assert stats["nonlinear_tested"] == 1 and 1 < stats["rounds_max"] <= CAPR.CCD_NL_ROUNDS
    toi = float(rec["toi"][0])
    assert 0 < toi <= CPU.spin_t_star()
    band = CPU.spin_band(bits)
    g = CPU.spin_exact_gap(toi, float(sb_b["angular_velocity"][cap][2]))
    assert -band < g <= CPU.TOL + band, (g, band)
    assert not np.array_equal(sb_a["delta_rotation"][cap], sb_b["delta_rotation"][cap])              # the capsule was turned back


@pytest.mark.parametrize("bits", BITS)
def test_5_a_spinning_capsule_bullet_stops_in_front_of_the_wall_and_stays_there(bits):
    scene, bullet = capsule_at_a_wall(av=(20.0, 0, 0), rot=Q_ABOUT_X)     # whirling about the line of flight: broadside all the way (see test_2)
    rec, stats, _, _, a, b, _ = check(scene, bits, entries_of([bullet], N))
    assert rec["hit_body"][0] == 1 and stats["nonlinear_tested"] == 1
    assert b.bodies_download()["position"][bullet][0] > 0.1 and a.bodies_download()["position"][bullet][0] < -0.05
    for _ in range(30):
        a.step()
        assert a.bodies_download()["position"][bullet][0] < 0.05


@pytest.mark.parametrize("bits", BITS)
def test_5_a_spinning_rod_is_stopped_at_a_capsule_bar(bits):
    scene, rod = rod_at_a_bar()
    rec, stats, *_ = check(scene, bits, entries_of([rod], L))
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == -1
    rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of([rod], N))
    assert rec["hit_body"][0] == 1 and stats["nonlinear_tested"] == 1 and 0 < float(rec["toi"][0]) <= ROD.t_star()
    assert not np.array_equal(sb_a["delta_rotation"][rod], sb_b["delta_rotation"][rod])


@pytest.mark.parametrize("bits", BITS)
def test_5_a_capsule_with_a_centre_of_mass_off_its_origin(bits):
    scene, cap = spinning_capsule(com=(-0.05, 0.2, 0.03))     # the lower end turns towards the wall on a longer arm
    rec, *_ = check(scene, bits, entries_of([cap], N))
    assert rec["hit_body"][0] == 1
    plain, _ = spinning_capsule()
    rec0, *_ = check(plain, bits, entries_of([cap], N))
    assert float(rec0["toi"][0]) != float(rec["toi"][0])          # the ends turn on other arms: the centre of mass is read


@pytest.mark.parametrize("bits", BITS)
def test_5_the_pairs_mode_goes_by_body_with_a_capsule_as_the_listed_b2(bits):
    scene, (ball, cap, cub) = write_order()
    # every body's swept AABB meets the other two: each entry tests two pairs
    rec, stats, *_ = check(scene, bits, entries_of([ball, cap], [L, N]))          # ball - cap runs NonLinear from both sides, and cap - cub
    assert rec["tested"].tolist() == [2, 2] and stats["nonlinear_tested"] == 3
    rec, stats, *_ = check(scene, bits, entries_of([ball, cap], [L, L]))
    assert rec["tested"].tolist() == [2, 2] and stats == ZERO_STATS


# ---- 6. ties and the write order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("incoming", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_6_equal_times_go_to_the_first_edge_in_neighbors_order(bits, incoming, mode):
    scene, bullet = capsule_tie(incoming)
    rec, stats, _, _, a, _, _ = check(scene, bits, entries_of([bullet], mode))
    pairs = a.pairs_get()
    assert len(pairs) == 2 and rec["tested"][0] == 2 and rec["hit_body"][0] >= 0
    assert rec["hit_collider"][0] == pairs[-1]["collider1" if incoming else "collider2"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", BITS)
def test_6_a_ball_a_cuboid_and_a_capsule_writing_one_body(bits, mode):
    scene, (ball, cap, cub) = write_order()
    out = {}
    for order in ((ball, cap), (cap, ball), (ball, cub, cap)):
        rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of(list(order), mode))
        assert (rec["hit_body"] >= 0).all()
        out[order] = (sb_a["delta_position"][cub].copy(), sb_a["delta_rotation"][cub].copy())
    assert not np.array_equal(out[(ball, cap)][0], out[(cap, ball)][0])
    assert not np.array_equal(out[(ball, cap)][1], out[(ball, cub, cap)][1])


# ---- 7. mixed traffic: more than one wave, every kind and both modes in one pass ------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_7_seventy_two_bullets_of_three_kinds_and_two_modes(bits):
    scene, bullets, wall, bar = mixed_traffic()
    modes = [L if k % 2 == 0 else N for k in range(len(bullets))]
    rec, stats, _, _, a, _, _ = check(scene, bits, entries_of(bullets, modes))
    assert len(rec) == 72 and len(a.pairs_get()) > 64 and (rec["tested"] >= 1).all()
    assert (rec["hit_body"][:24] == bar).all() and (rec["hit_body"][24:] == wall).all()
    assert stats["nonlinear_tested"] >= 36
    # with the switch off the capsule bullets fly on and the others no longer see the bar
    rec, *_ = check(scene, bits, entries_of(bullets, modes), capsules=False)
    assert (rec["hit_body"][2::3] == -1).all() and (rec["tested"][2::3] == 0).all()
    assert (rec["hit_body"][0::3] == wall).all() and (rec["hit_body"][1::3] == wall).all()
