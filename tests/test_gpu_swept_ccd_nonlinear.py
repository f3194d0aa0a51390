"""GPU: SweepMode::NonLinear of swept CCD (include/avian_mi355x_ccd.h, N0 - N4; k_ccd_toi_nl / k_ccd_origin_nl) against
tests/swept_ccd_nonlinear_reference.py at tolerance 0, in f32 and f64.

The two-worlds method of test_gpu_swept_ccd.py: world B steps without a list and supplies the pre-CCD state, world A has the list; A's records,
its delta_position / delta_rotation bytes and its avn_swept_ccd_stats must be the reference's.  Every scene but the one that exists to cross a
wave boundary has ten bodies or fewer."""
import math

import numpy as np
import pytest

from avian_amd.swept_ccd import MISS, SWEEP_LINEAR, SWEEP_NON_LINEAR, SweptCcd
from helpers import F, hip_lib
import swept_ccd_nonlinear_reference as NL
import swept_ccd_scenes as SC
import swept_ccd_nonlinear_rod as CPU

pytestmark = pytest.mark.gpu
BITS = [32, 64]
L, N = SWEEP_LINEAR, SWEEP_NON_LINEAR
ROD_HE = (CPU.ROD_L, CPU.ROD_W, CPU.ROD_W)


class Scene(SC.Scene):
    """swept_ccd_scenes.Scene with a local centre of mass per body and a configurable contact_tolerance."""

    def __init__(self, tol=None, **kw):
        super().__init__(**kw)
        self.tol, self.com = tol, {}

    def body_kwargs(self):
        kw = super().body_kwargs()
        com = np.zeros((len(self.pos), 3))
        for b, c in self.com.items():
            com[b] = c
        kw["center_of_mass"] = com
        return kw

    def world(self, lib, bits, closed_loop=True):
        kw = dict(substeps=4, gravity=self.gravity, dt_ns=SC.DT_NS)
        if self.margin is not None:
            kw["default_speculative_margin"] = self.margin
        if self.tol is not None:
            kw["contact_tolerance"] = self.tol
        w = F.World(lib, F.default_config(bits, **kw))
        w.bodies_upload(**self.body_kwargs()); w.colliders_upload(**self.collider_kwargs())
        w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5, restitution=0.0)
        w.pipeline_enable()
        return w


def adopt(scene):
    """A swept_ccd_scenes scene as a Scene of this module (the same tables)."""
    s = Scene(gravity=scene.gravity, margin=scene.margin)
    for k, v in vars(scene).items():
        setattr(s, k, v)
    s.tol, s.com = None, {}
    return s


def entries_of(bodies, modes, **kw):
    out = SC.entries_of(list(bodies), **kw)
    for e, m in zip(out, modes if isinstance(modes, (list, tuple)) else [modes] * len(out)):
        e["mode"] = m
    return out


def upload(ccd, entries):
    ccd.upload([e["body"] for e in entries], mode=[e["mode"] for e in entries], include_dynamic=[e["include_dynamic"] for e in entries],
               linear_threshold=[e["linear_threshold"] for e in entries], angular_threshold=[e["angular_threshold"] for e in entries])


def check(scene, bits, entries, info=None, exhausted=0):
    """Steps A (list, switch on) and B (no list) once; A must equal the reference.  Returns (records, stats, A's solver bodies, B's, A, B)."""
    a, b = scene.world(hip_lib(), bits), scene.world(hip_lib(), bits)
    ccd = SweptCcd(a, non_linear=True)
    upload(ccd, entries)
    start = b.bodies_download()
    b.step(); b.synchronize()
    sb = b.solver_bodies_download()
    state = dict(position=start["position"], rotation=start["rotation"], linear_velocity=sb["linear_velocity"], angular_velocity=sb["angular_velocity"],
                 delta_position=sb["delta_position"], delta_rotation=sb["delta_rotation"], center_of_mass=scene.body_kwargs()["center_of_mass"])
    rec, dp, dq, stats = NL.swept_ccd(bits, entries, scene.reference_scene(list(b.pairs_get())), state, SC.DT_NS, scene.margin_cfg(),
                                      tol_cfg=0.005 if scene.tol is None else scene.tol, info=info)
    a.step(); a.synchronize()
    got, sb_a, got_stats = ccd.results(), a.solver_bodies_download(), ccd.stats()
    assert got.tobytes() == rec.tobytes(), (got, rec)
    assert sb_a["delta_position"].tobytes() == dp.tobytes(), (sb_a["delta_position"], dp)
    assert sb_a["delta_rotation"].tobytes() == dq.tobytes(), (sb_a["delta_rotation"], dq)
    for k in ("linear_velocity", "angular_velocity"):
        assert sb_a[k].tobytes() == sb[k].tobytes(), k   # velocities are never changed
    assert got_stats == {k: stats[k] for k in ("nonlinear_tested", "rounds_max", "exhausted")}, (got_stats, stats)
    assert got_stats["exhausted"] == exhausted
    return got, got_stats, sb_a, sb, a, b


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
def rod_scene(com=None, omega=CPU.ROD_OMEGA, lv=(0, 0, 0), pos=(0, 0, 0)):
    """The rod of swept_ccd_nonlinear_rod.py beside a 0.1-thick static wall whose face is the plane y = D."""
    s = Scene()
    rod = s.body(pos, lv=lv, av=(0, 0, omega))
    s.collider(rod, F.SHAPE_CUBOID, ROD_HE, F.COLLIDER_SWEPT_CCD)
    if com is not None:
        s.com[rod] = com
    s.cuboid(CPU.WALL_POS, CPU.WALL_HE)
    return s, rod


def exhausting_scene(clearance):
    """The rod, started at 75 degrees, sweeps its corner past a wall tilted by 10 degrees about z at a closest gap of `clearance`, with a
    contact_tolerance of 0.0005.  The CPU reference runs out of its 64 rounds for clearances of 0.0007 .. 0.0023 and misses in fewer beyond."""
    s = Scene(tol=0.0005)
    r0, tilt = math.radians(75), math.radians(10)
    rod = s.body((0, 0, 0), av=(0, 0, CPU.ROD_OMEGA), rot=(0, 0, math.sin(r0 / 2), math.cos(r0 / 2)))
    s.collider(rod, F.SHAPE_CUBOID, ROD_HE, F.COLLIDER_SWEPT_CCD)
    off = math.hypot(CPU.ROD_L, CPU.ROD_W) + clearance + CPU.WALL_TH
    s.cuboid((-math.sin(tilt) * off, math.cos(tilt) * off, 0.0), CPU.WALL_HE, rot=(0, 0, math.sin(tilt / 2), math.cos(tilt / 2)))
    return s, rod


def spinning_bullet(spin=20.0):
    s = Scene()
    b = s.body((-1, 0, 0), lv=(240.0, 0, 0), av=(0, 0, spin))
    s.collider(b, F.SHAPE_CUBOID, (0.05, 0.08, 0.06), F.COLLIDER_SWEPT_CCD)
    s.cuboid((0, 0, 0), (0.05, 1, 2))
    return s, b


def both_move_and_spin():
    s = Scene()
    q = np.array([0.1, 0.2, -0.1, 0.95]); q = q / np.linalg.norm(q)
    a = s.body((-1.1, 0.05, 0.02), lv=(180.0, 10.0, 0), av=(5.0, -8.0, 30.0), rot=tuple(q))
    s.collider(a, F.SHAPE_CUBOID, (0.2, 0.03, 0.04), F.COLLIDER_SWEPT_CCD)
    c = s.cuboid((0, 0, 0), (0.3, 0.3, 0.3), rb=F.RB_DYNAMIC, lv=(-20.0, 3.0, 0), av=(0, 6.0, 12.0))
    return s, a, c


def bullets_on_one_wall(n=70):
    s = Scene()
    bullets = [s.ball((-1, 0, (k - (n - 1) / 2) * 0.2), 0.05, lv=(240.0, 0, 0)) for k in range(n)]
    s.cuboid((0, 0, 0), (0.05, 1, 8))
    return s, bullets


# ---- 1. the switch ----------------------------------------------------------------------------------------------------------------------------------
def test_1_the_switch_gates_the_mode_and_refuses_to_strand_a_list():
    scene, bodies = SC.tunnelling()
    a = scene.world(hip_lib(), 32)
    ccd = SweptCcd(a)
    with pytest.raises(F.AvnError) as e:
        ccd.upload(bodies, mode=[N])
    assert e.value.status == 1 and "NonLinear" in str(e.value)
    assert ccd.stats() == dict(nonlinear_tested=0, rounds_max=0, exhausted=0)
    ccd.set_non_linear(True)
    ccd.upload(bodies, mode=[N])
    with pytest.raises(F.AvnError) as e:
        ccd.upload(bodies, mode=[2])
    assert e.value.status == 1
    with pytest.raises(F.AvnError) as e:
        ccd.set_non_linear(False)
    assert e.value.status == 6                                   # AVN_ERR_STATE; the switch and the list stay
    a.step(); a.synchronize()
    rec = ccd.results()
    assert len(rec) == 1 and rec["hit_body"][0] == 1 and ccd.stats()["nonlinear_tested"] == 1
    ccd.upload(bodies, mode=[N])                                 # still accepted
    ccd.upload(bodies, mode=[L])
    ccd.set_non_linear(False)                                    # a Linear list does not hold the switch
    with pytest.raises(F.AvnError):
        ccd.upload(bodies, mode=[N])
    ccd.set_non_linear(True); ccd.upload(bodies, mode=[N]); ccd.clear()
    ccd.set_non_linear(False)                                    # nor does no list


@pytest.mark.parametrize("name", ["tunnelling", "write_order"])
@pytest.mark.parametrize("bits", BITS)
def test_1_a_linear_list_is_byte_equal_with_the_switch_on_or_off(bits, name):
    scene, bodies = getattr(SC, name)()
    entries = SC.entries_of(list(bodies))
    out = []
    for on in (False, True):
        w = scene.world(hip_lib(), bits)
        ccd = SweptCcd(w, non_linear=on)
        SC.upload(ccd, entries)
        w.step(); w.synchronize()
        first = (ccd.results(), w.solver_bodies_download(), w.timers().kernel_launches, ccd.stats())
        w.step(); w.synchronize()                                # the step after the hit
        out.append(first[:2] + (w.bodies_download(),) + first[2:])
    (ra, sa, ba, la, ta), (rb, sb, bb, lb, tb) = out
    assert ra.tobytes() == rb.tobytes() and (ra["hit_body"] >= 0).any()
    for x, y in ((sa, sb), (ba, bb)):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), k
    assert la == lb                                              # the same launches
    assert ta == tb == dict(nonlinear_tested=0, rounds_max=0, exhausted=0)


# ---- 2. pure spin ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_2_a_rod_that_only_spins_is_stopped_at_the_wall(bits):
    scene, rod = rod_scene()
    rec, stats, *_ = check(scene, bits, entries_of([rod], L))
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == -1 and stats["nonlinear_tested"] == 0     # d = 0: the linear sweep sees nothing
    rec, stats, sb_a, sb_b, a, b = check(scene, bits, entries_of([rod], N))
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == 1 and rec["hit_collider"][0] == SC.ENTITY0 + 1
    assert stats["nonlinear_tested"] == 1 and 1 < stats["rounds_max"] <= NL.CCD_NL_ROUNDS
    toi = float(rec["toi"][0])
    assert 0 < toi <= CPU.t_star()
    band = CPU.band_of(bits, ROD_HE, (0, 0, 0), CPU.WALL_HE, CPU.WALL_POS)
    g = CPU.exact_rod_gap(toi, ROD_HE, (0, 0, 0), (0, 0, 0), (0, 0, 0), float(sb_b["angular_velocity"][rod][2]))
    assert -band < g <= CPU.TOL + band, (g, band)
    assert not np.array_equal(sb_a["delta_rotation"][rod], sb_b["delta_rotation"][rod])              # the rod was turned back


# ---- 3. a spinning bullet -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_3_a_spinning_cuboid_bullet_stops_in_front_of_the_wall_and_stays_there(bits):
    scene, bullet = spinning_bullet()
    rec, stats, _, _, a, b = check(scene, bits, entries_of([bullet], N))
    assert rec["hit_body"][0] == 1 and stats["nonlinear_tested"] == 1
    assert b.bodies_download()["position"][bullet][0] > 0.1      # without the list it ends behind the wall
    assert a.bodies_download()["position"][bullet][0] < -0.05    # with it, in front
    for _ in range(30):
        a.step()
        assert a.bodies_download()["position"][bullet][0] < 0.05


# ---- 4. both bodies move and spin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_4_both_bodies_move_and_spin(bits):
    scene, a, c = both_move_and_spin()
    rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of([a], N, include_dynamic=1))
    assert rec["hit_body"][0] == c and stats["nonlinear_tested"] == 1
    for body in (a, c):                                          # both are written
        assert not np.array_equal(sb_a["delta_position"][body], sb_b["delta_position"][body])
        assert not np.array_equal(sb_a["delta_rotation"][body], sb_b["delta_rotation"][body])
    rec, stats, *_ = check(scene, bits, entries_of([a], N, include_dynamic=0))
    assert rec["tested"][0] == 0 and rec["hit_body"][0] == -1 and stats == dict(nonlinear_tested=0, rounds_max=0, exhausted=0)


# ---- 5. a centre of mass off the origin ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_5_a_body_with_a_centre_of_mass_off_its_origin(bits):
    com = (-0.2, -0.05, 0.03)
    scene, rod = rod_scene(com=com)
    rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of([rod], N))
    assert rec["hit_body"][0] == 1
    toi = float(rec["toi"][0])
    band = CPU.band_of(bits, ROD_HE, (0, 0, 0), CPU.WALL_HE, CPU.WALL_POS)
    g = CPU.exact_rod_gap(toi, ROD_HE, (0, 0, 0), com, sb_b["linear_velocity"][rod].astype(np.float64), float(sb_b["angular_velocity"][rod][2]))
    assert -8 * band < g <= CPU.TOL + 8 * band, (g, band)         # (8: the world's velocities carry the solver's own rounding)
    plain, _ = rod_scene()
    rec0, *_ = check(plain, bits, entries_of([rod], N))
    assert float(rec0["toi"][0]) != toi                          # the far end turns on a longer arm: the centre of mass is read


# ---- 6. N0 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_6_the_pairs_mode_goes_by_body(bits):
    scene, (ba, bb, cub) = SC.write_order()
    scene = adopt(scene)
    # every body's swept AABB meets the other two: each entry tests two pairs
    # ba is Linear, its target cub is listed NonLinear: ba's pair with cub runs the NonLinear test (its pair with bb does not), and so do cub's two
    rec, stats, *_ = check(scene, bits, entries_of([ba, cub], [L, N]))
    assert rec["tested"].tolist() == [2, 2] and stats["nonlinear_tested"] == 3
    rec, stats, *_ = check(scene, bits, entries_of([ba, cub, bb], [L, N, L]))            # bb's pair with cub too; ba - bb stays Linear both ways
    assert rec["tested"].tolist() == [2, 2, 2] and stats["nonlinear_tested"] == 4
    rec, stats, *_ = check(scene, bits, entries_of([ba, cub], [L, L]))                   # both listed Linear stays Linear
    assert rec["tested"].tolist() == [2, 2] and stats["nonlinear_tested"] == 0
    rec, stats, *_ = check(scene, bits, entries_of([ba, bb], [N, L]))                    # cub is not listed: ba's two pairs, and bb's pair with ba
    assert stats["nonlinear_tested"] == 3 and (rec["hit_body"] == cub).all()


# ---- 7. ties and the write order --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("incoming", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_7_equal_times_go_to_the_first_edge_in_neighbors_order(bits, incoming):
    scene, bodies = SC.tie(incoming)
    rec, stats, _, _, a, _ = check(adopt(scene), bits, entries_of(bodies, N))
    pairs = a.pairs_get()
    assert len(pairs) == 2 and rec["tested"][0] == 2 and stats["nonlinear_tested"] == 2
    assert rec["hit_collider"][0] == pairs[-1]["collider1" if incoming else "collider2"]


@pytest.mark.parametrize("bits", BITS)
def test_7_several_entries_writing_one_body_leave_what_the_serial_loop_leaves(bits):
    scene, (ba, bb, cub) = SC.write_order()
    scene = adopt(scene)
    out = {}
    for order in ((ba, bb), (bb, ba), (ba, cub, bb)):
        rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of(list(order), N))
        assert (rec["hit_body"] >= 0).all()
        out[order] = (sb_a["delta_position"][cub].copy(), sb_a["delta_rotation"][cub].copy())
    assert not np.array_equal(out[(ba, bb)][0], out[(bb, ba)][0])
    assert not np.array_equal(out[(ba, bb)][1], out[(ba, cub, bb)][1])


# ---- 8. the origin rule -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_8_the_origin_rule_with_a_bounded_margin(bits):
    info = {}
    scene, bodies = SC.overlapping(30.0, 0.02)
    rec, stats, *_ = check(adopt(scene), bits, entries_of(bodies, N), info=info)
    assert info["origin"] == [1] and rec["hit_body"][0] == 1 and abs(float(rec["toi"][0]) - 0.02 / 30) < 0.0051 / 30    # moving in: the small ball hits
    assert stats["nonlinear_tested"] == 1 and stats["rounds_max"] == 2                                                   # (the fallback's two rounds)
    for args in ((-30.0, 0.02), (30.0, None)):                     # moving out; an unbounded margin
        info = {}
        scene, bodies = SC.overlapping(*args)
        rec, stats, *_ = check(adopt(scene), bits, entries_of(bodies, N), info=info)
        assert info["origin"] == [1] and rec["tested"][0] == 1 and rec["hit_body"][0] == -1 and stats["rounds_max"] == 1, args


# ---- 9. exhaustion ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_9_a_pair_that_runs_out_of_rounds_answers_nothing(bits):
    scene, rod = exhausting_scene(0.0015)
    rec, stats, sb_a, sb_b, *_ = check(scene, bits, entries_of([rod], N), exhausted=1)
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == -1 and rec["hit_collider"][0] == MISS and rec["toi"][0] == 0
    assert stats == dict(nonlinear_tested=1, rounds_max=NL.CCD_NL_ROUNDS, exhausted=1)
    assert sb_a["delta_rotation"].tobytes() == sb_b["delta_rotation"].tobytes()          # nobody is frozen in time
    scene, rod = exhausting_scene(0.004)                                                   # a wider pass: a miss inside the cap
    rec, stats, *_ = check(scene, bits, entries_of([rod], N))
    assert rec["hit_body"][0] == -1 and 32 < stats["rounds_max"] < NL.CCD_NL_ROUNDS


# ---- 10. more than one wave, both kernels in one pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_10_seventy_bullets_with_alternating_modes(bits):
    scene, bullets = bullets_on_one_wall()
    rec, stats, *_ = check(scene, bits, entries_of(bullets, [L if k % 2 == 0 else N for k in range(len(bullets))]))
    assert len(rec) == 70 and (rec["tested"] == 1).all() and (rec["hit_body"] == 70).all()
    assert stats["nonlinear_tested"] == 35 and stats["rounds_max"] == 2
    assert (np.abs(rec["toi"] - 0.9 / 240) < 1e-6).all()
