"""GPU: swept CCD in the device closed loop (include/avian_mi355x_ccd.h) against tests/swept_ccd_reference.py at tolerance 0.

Two identical worlds, restitution 0 everywhere (no restitution pass runs after the place the CCD pass takes).  World B steps without a list:
its step-start poses and its avn_solver_bodies_download are the pre-CCD state the reference is fed.  World A has the list: its records and
the delta_position / delta_rotation bytes of its solver bodies must be the reference's.  The edge order is avn_pairs_get's emission order;
every scene creates all edges of its CCD bodies in the step under test."""
import numpy as np
import pytest

from avian_amd.swept_ccd import MISS, SWEEP_NON_LINEAR, SweptCcd
from helpers import F, hip_lib
import swept_ccd_scenes as SC

pytestmark = pytest.mark.gpu
BITS = [32, 64]


def worlds(scene, bits, entries):
    a, b = scene.world(hip_lib(), bits), scene.world(hip_lib(), bits)
    ccd = SweptCcd(a)
    SC.upload(ccd, entries)
    return a, ccd, b


def check(scene, bits, entries, info=None):
    a, ccd, b = worlds(scene, bits, entries)
    rec, sb_a, sb_b = SC.assert_equals_reference(scene, bits, entries, a, ccd, b, info=info)
    return rec, sb_a, sb_b, a, b


@pytest.mark.parametrize("bits", BITS)
def test_a_bullet_stops_at_a_thin_wall_instead_of_tunnelling(bits):
    """The ball (r 0.05 at x = -1, v = 240) crosses the wall (faces at x = +-0.05) in one step of 1 / 60 without the list and stops at its
    front face with it.  The CPU oracle's closed loop, started from the post-CCD pose (x = -1 + 0.00375 * 1.0001 * 240) with v = 240, holds the
    ball: its x never exceeds -0.0865 in 30 steps, in f32 and f64, so the speed of the issue is kept."""
    scene, bodies = SC.tunnelling()
    entries = SC.entries_of(bodies)
    rec, _, _, a, b = check(scene, bits, entries)
    assert rec["hit_collider"][0] == SC.ENTITY0 + 1 and rec["hit_body"][0] == 1 and rec["tested"][0] == 1
    assert abs(float(rec["toi"][0]) - 0.9 / 240) < 1e-6
    assert b.bodies_download()["position"][0][0] > 0.1            # without the list it is beyond the wall: the scene proves something
    x = a.bodies_download()["position"][0][0]
    assert -0.11 < x < -0.09
    for _ in range(30):
        a.step()
        assert a.bodies_download()["position"][0][0] < 0.05      # never past the wall's back face


@pytest.mark.parametrize("bits", BITS)
def test_bodies_that_hit_nothing_are_left_alone(bits):
    scene, bodies = SC.neutrality()
    a, ccd, b = worlds(scene, bits, SC.entries_of(bodies))
    for step in range(5):
        a.step(); b.step(); a.synchronize(); b.synchronize()
        x, y = a.bodies_download(), b.bodies_download()
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), (step, k)
        rec = ccd.results()
        assert len(rec) == 2 and (rec["hit_collider"] == MISS).all() and (rec["hit_body"] == -1).all() and (rec["toi"] == 0).all()
        assert (rec["tested"] >= 1).all(), (step, rec)   # both balls stay inside the slab's AABB: their pairs exist for the five steps
        assert a.diagnostics().swept_ccd_ms > 0.0 and b.diagnostics().swept_ccd_ms == 0.0


@pytest.mark.parametrize("incoming", [False, True])
@pytest.mark.parametrize("bits", BITS)
def test_equal_times_go_to_the_first_edge_in_neighbors_order(bits, incoming):
    scene, bodies = SC.tie(incoming)
    rec, _, _, a, _ = check(scene, bits, SC.entries_of(bodies))
    pairs = a.pairs_get()
    ball = SC.ENTITY0
    assert len(pairs) == 2 and all(p["collider2" if incoming else "collider1"] == ball for p in pairs)
    # outgoing (or incoming) edges newest first: the pair emitted LAST
    assert rec["tested"][0] == 2 and rec["hit_collider"][0] == pairs[-1]["collider1" if incoming else "collider2"]


@pytest.mark.parametrize("bits", BITS)
def test_several_entries_writing_one_body_leave_what_the_serial_loop_leaves(bits):
    scene, (ba, bb, cub) = SC.write_order()
    out = {}
    for order in ((ba, bb), (bb, ba), (ba, cub, bb), (bb, cub, ba)):   # the last two: a CCD body that is itself hit by an earlier and a later entry
        rec, sb_a, sb_b, _, _ = check(scene, bits, SC.entries_of(list(order)))
        assert (rec["hit_body"] >= 0).all()
        out[order] = (sb_a["delta_position"][cub].copy(), sb_a["delta_rotation"][cub].copy())
        assert not np.array_equal(out[order][0], sb_b["delta_position"][cub])
    assert not np.array_equal(out[(ba, bb)][0], out[(bb, ba)][0])                 # the last delta_position stays
    assert not np.array_equal(out[(ba, bb)][1], out[(ba, cub, bb)][1])            # one more factor on delta_rotation


@pytest.mark.parametrize("bits", BITS)
def test_include_dynamic_and_the_thresholds(bits):
    scene, bullets = SC.target_kinds()
    rec, *_ = check(scene, bits, SC.entries_of(bullets, include_dynamic=0))
    assert rec["tested"].tolist() == [0, 1, 1] and rec["hit_body"].tolist() == [-1, 4, 5]       # the dynamic target is skipped; kinematic and static stop the bullet
    rec, *_ = check(scene, bits, SC.entries_of(bullets, include_dynamic=[1, 0, 1]))
    assert rec["hit_body"].tolist() == [3, 4, 5]
    scene, bodies = SC.tunnelling()
    rec, *_ = check(scene, bits, SC.entries_of(bodies, linear_threshold=1000.0, angular_threshold=1.0))
    assert rec["tested"][0] == 0 and rec["hit_body"][0] == -1                                   # both below
    rec, *_ = check(scene, bits, SC.entries_of(bodies, linear_threshold=100.0, angular_threshold=1.0))
    assert rec["tested"][0] == 1 and rec["hit_body"][0] == 1                                    # the linear one exceeded


@pytest.mark.parametrize("bits", BITS)
def test_target_kinds(bits):
    scene, bodies = SC.wall_with(cflags=F.COLLIDER_SENSOR)
    rec, *_ = check(scene, bits, SC.entries_of(bodies))
    assert rec["hit_body"][0] == 1                                     # sensors are not filtered
    scene, bodies = SC.wall_with(child=True)
    rec, _, _, a, _ = check(scene, bits, SC.entries_of(bodies))
    assert len(a.pairs_get()) == 1 and rec["tested"][0] == 0 and rec["hit_body"][0] == -1   # the pair exists, a child collider is not tested
    scene, bodies = SC.sat_bullet()
    rec, *_ = check(scene, bits, SC.entries_of(bodies))
    assert rec["hit_body"][0] == 1 and 0 < rec["toi"][0] < 1 / 60      # cuboid against a turned cuboid
    scene, bodies = SC.moving_balls()
    rec, *_ = check(scene, bits, SC.entries_of(bodies))
    assert rec["hit_body"][0] == 1 and abs(float(rec["toi"][0]) - 0.00835739) < 1e-6   # 1.755 (the centres' way to touching) / 210


@pytest.mark.parametrize("bits", BITS)
def test_the_origin_penetration_rule(bits):
    info = {}
    scene, bodies = SC.overlapping(30.0, 0.02)
    rec, *_ = check(scene, bits, SC.entries_of(bodies), info=info)
    assert info["origin"] == [1] and rec["hit_body"][0] == 1 and abs(float(rec["toi"][0]) - 0.02 / 30) < 1e-6   # moving in: the small ball hits
    for args in ((-30.0, 0.02), (30.0, None), (30.0, 0.02, False)):    # moving out; margin unbounded; a solid wall (the solver stops the ball: d = 0)
        info = {}
        scene, bodies = SC.overlapping(*args)
        rec, *_ = check(scene, bits, SC.entries_of(bodies), info=info)
        assert info["origin"] == [1] and rec["tested"][0] == 1 and rec["hit_body"][0] == -1, args


def test_interface():
    scene, bodies = SC.tunnelling()
    a = scene.world(hip_lib(), 32)
    ccd = SweptCcd(a)
    assert len(ccd.results()) == 0
    ccd.upload(bodies)
    assert len(ccd.results()) == 0                                     # no pass has run
    for bad, word in ((dict(body=[0], mode=[SWEEP_NON_LINEAR]), "NonLinear"), (dict(body=[2]), "range"), (dict(body=[0, 0]), "twice")):
        with pytest.raises(F.AvnError) as e:
            ccd.upload(**bad)
        assert e.value.status == 1 and word in str(e.value)
    a.step(); a.synchronize()
    rec = ccd.results()
    assert len(rec) == 1 and rec["hit_body"][0] == 1                   # the old list is still in force
    # outside the device closed loop
    for kw in (dict(closed_loop=False),):
        w = scene.world(hip_lib(), 32, **kw)
        c2 = SweptCcd(w); c2.upload(bodies)
        for call in (w.step, lambda: w.run_system("SOLVER")):
            with pytest.raises(F.AvnError) as e:
                call()
            assert e.value.status == 6
        c2.clear()
        w.step(); w.synchronize()
    w = scene.world(hip_lib(), 32, closed_loop=False); w.pipeline_enable(True, host_bookkeeping=True)
    c2 = SweptCcd(w); c2.upload(bodies)
    with pytest.raises(F.AvnError) as e:
        w.step()
    assert e.value.status == 6
    # another body count clears the list
    kw = scene.body_kwargs()
    grown = {k: np.concatenate([v, v[-1:]]) for k, v in kw.items()}
    grown["position"][-1] = [0, 50, 0]
    a.bodies_upload(**grown)
    a.step(); a.synchronize()
    assert len(ccd.results()) == 0 and a.diagnostics().swept_ccd_ms == 0.0
    # so does avn_despawn
    ccd.upload(bodies)
    a.step(); a.synchronize()
    assert len(ccd.results()) == 1
    state = a.bodies_download()
    a.despawn(bodies=[2])
    back = scene.body_kwargs()
    for k in ("position", "rotation", "linear_velocity", "angular_velocity"):
        back[k] = state[k][:2].astype(np.float64)
    a.bodies_upload(**back); a.colliders_upload(**scene.collider_kwargs()); a.collider_materials_upload(friction=0.5, restitution=0.0)
    a.step(); a.synchronize()
    assert len(ccd.results()) == 0
