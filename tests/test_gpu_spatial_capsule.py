"""GPU: the capsule query shape (AVN_SHAPE_CAPSULE; include/avian_mi355x_spatial.h, "capsule query shapes") through every entry point that
takes a query shape, against the brute force of tests/spatial_capsule_reference.py, tolerance 0: every byte of every record and every count,
f32 and f64.  Calls mix capsules with balls and cuboids, so the Ball / Cuboid lanes are checked against today's references in the same
comparison and the two kernel instantiations are seen to write disjoint lanes."""
import numpy as np
import pytest

from avian_amd.spatial_query import CASTER_SHAPE, MAX_HITS, MISS, SHAPE_CAPSULE, SpatialQuery
from compound_helpers import compound_world
from helpers import F, hip_lib, random_unit_quats
import spatial_capsule_reference as C
import spatial_contact_reference as CR
import spatial_move_scenes as MS
import spatial_query_reference as R
import spatial_scenes as SC
from test_gpu_spatial_casters import run_and_check
from test_gpu_spatial_contacts import mixed_scene, world_of
from test_gpu_spatial_query import same_ids, same_records, snapshot_of
from test_spatial_casters_cpu import BODY, caster_set, layered_compound_scene

pytestmark = pytest.mark.gpu

I = [0.0, 0.0, 0.0, 1.0]
DT = {32: np.float32, 64: np.float64}
FAR = np.array([1000.0, -2000.0, 1500.0])
DEPEN = dict(skin_width=0.05, max_depenetration_error=1e-4, penetration_rejection_threshold=0.3, iterations=16)


def scene_40():
    """The mixed scene of 40 Ball / Cuboid colliders (layers, sensors), collider 7 a child of its body, body 11 moved to around 1e3."""
    bodies, cols = mixed_scene(seed=4, n=40)
    rng = np.random.default_rng(77)
    tf = dict(is_child=np.zeros(40, np.uint8), translation=np.zeros((40, 3)), rotation=np.tile(I, (40, 1)))
    tf["is_child"][7] = 1; tf["translation"][7] = [0.5, 0.2, -0.3]; tf["rotation"][7] = random_unit_quats(rng, 1)[0]
    bodies["position"][11] = FAR
    sensor = (cols["collider_flags"] & F.COLLIDER_SENSOR) != 0
    return bodies, cols, tf, sensor.astype(np.uint8)


def mixed_queries(rng, s, n, kinds=(0, 1, SHAPE_CAPSULE)):
    """n query shapes near the colliders, kinds mixed lane by lane; the last three sit by the far collider."""
    pos_c = np.stack(s.pos, 1).astype(float)
    shape = rng.choice(np.array(kinds, np.uint8), n)
    he = rng.uniform(0.15, 0.6, (n, 3))
    he[::9, 1] = 0.0                                   # h == 0 capsules (balls) and flat cuboids
    pos = pos_c[rng.integers(0, s.n, n)] + rng.normal(size=(n, 3)) * np.choose(np.arange(n) % 3, [0.3, 0.9, 2.0])[:, None]
    pos[-3:] = FAR + rng.normal(size=(3, 3)) * 0.7
    rot = random_unit_quats(rng, n)
    rot[::4] = I
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[-3:] = (FAR - pos[-3:]) / np.linalg.norm(FAR - pos[-3:], axis=1, keepdims=True)
    md = np.where(rng.random(n) < 0.3, rng.uniform(0.5, 4, n), np.inf)
    return shape, he, pos, rot, d, md


def with_invalid(q):
    """The batch with invalid capsules planted among the valid lanes."""
    shape, he, pos, rot, d, md = (np.array(x) for x in q)
    shape[[3, 20, 41, 64, 70]] = SHAPE_CAPSULE
    he[3, 0] = -0.1; he[20, 1] = -0.2; he[41, 0] = np.nan; he[64, 1] = np.inf; pos[70, 2] = np.nan
    shape[50] = 2                                       # kind 2 stays invalid
    he[5, 2] = np.nan; shape[5] = SHAPE_CAPSULE         # z is not read: still valid
    return shape, he, pos, rot, d, md


def check_all(sq, s, q, sensor, what, caps=(0, 1, 3, 64), ks=(1, 4), **flt):
    """Every stateless entry point of one batch against the brute force; returns (intersection counts, closest hits, contact counts)."""
    shape, he, pos, rot, d, md = q
    ex = flt.get("excluded", ())
    kw = dict(mask=flt.get("mask"), excluded=flt.get("excluded"))
    with np.errstate(all="ignore"):
        for cap in caps:
            same_ids(sq.shape_intersections(shape, he, pos, rot, cap, **kw), C.shape_intersections(s, shape, he, pos, rot, cap, flt.get("mask"), ex), f"{what}: intersections cap={cap}")
        closest, many = C.cast_queries(s, shape, he, pos, rot, d, ks, md, flt.get("mask"), ex)
        assert C.last_rounds.size == 0 or C.last_rounds.max() < C.ROUNDS, "a pair of the set reaches the Newton round cap"
        got = sq.cast_shapes(shape, he, pos, rot, d, md, **kw)
        same_records(got, closest, f"{what}: cast_shapes")
        for k in ks:
            h, cnt = sq.shape_hits(shape, he, pos, rot, d, k, md, **kw)
            same_records(h, many[k][0], f"{what}: shape_hits k={k}")
            assert np.array_equal(cnt, many[k][1]), f"{what}: shape_hits k={k} counts"
        pred = np.where(np.arange(len(shape)) % 2, 0.25, 0.0)
        lists = C.contact_lists(s, shape, he, pos, rot, pred, mask=flt.get("mask"), excluded=ex, sensor=sensor, skip_sensors=flt.get("skip_sensors", False))
        for cap in caps:
            rec, cnt = sq.shape_contacts(shape, he, pos, rot, pred, cap, skip_sensors=flt.get("skip_sensors", False), **kw)
            want = CR.pad(lists, cap, 32 if s.dt == np.float32 else 64)
            same_records(rec, want[0], f"{what}: shape_contacts cap={cap}")
            assert np.array_equal(cnt, want[1]), f"{what}: shape_contacts cap={cap} counts"
    ids, icnt = sq.shape_intersections(shape, he, pos, rot, 64, **kw)
    return icnt, got, np.array([len(l) for l in lists]), lists


def assert_capsules_seen(shape, icnt, closest, ccnt):
    cap = shape == SHAPE_CAPSULE
    assert (icnt[cap] > 0).sum() >= 3 and (closest["collider"][cap] != MISS).sum() >= 3 and (ccnt[cap] > 0).sum() >= 3
    assert (icnt[~cap] > 0).any() or cap.all()


# ---- the smallest trees ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colliders", [1, 2])
def test_smallest_trees(n_colliders):
    pos = [[0.0, -0.5, 0.0], [1.5, 1.0, 0.5]][:n_colliders]
    cols = dict(entity_index=np.arange(40, 40 + n_colliders, dtype=np.uint32), body=np.arange(n_colliders, dtype=np.int32),
                shape=np.array([R.SHAPE_CUBOID, R.SHAPE_BALL][:n_colliders], np.uint8), half_extents=np.array([[3, 0.5, 3], [0.75, 0, 0]][:n_colliders], float))
    rng = np.random.default_rng(n_colliders)
    n = 70
    shape = rng.choice(np.array([0, 1, SHAPE_CAPSULE, SHAPE_CAPSULE], np.uint8), n)
    he = rng.uniform(0.2, 0.5, (n, 3))
    qpos = np.c_[rng.uniform(-2, 2, n), rng.uniform(-0.2, 2.0, n), rng.uniform(-2, 2, n)]
    rot = random_unit_quats(rng, n)
    vel = rng.normal(size=(n, 3)) * 4
    d = vel / np.linalg.norm(vel, axis=1, keepdims=True)
    own = np.where(rng.random(n) < 0.2, 40, MISS).astype(np.uint32)
    for bits in (32, 64):
        w = world_of(bits, SC.bodies_of(pos, [I] * n_colliders), cols)
        sq = SpatialQuery(w)
        sq.update()
        s = snapshot_of(w, cols)
        icnt, closest, ccnt, _ = check_all(sq, s, (shape, he, qpos, rot, d, np.full(n, np.inf)), None, f"{n_colliders} colliders f{bits}", caps=(1, 3), ks=(4,))
        assert_capsules_seen(shape, icnt, closest, ccnt)
        info = {}
        with np.errstate(all="ignore"):
            want = C.cast_moves(s, shape, he, qpos, rot, vel * 0.25, 0.05, own, info=info)
            same_records(sq.cast_moves(shape, he, qpos, rot, vel * 0.25, 0.05, self_entity=own), want, "cast_moves")
            ws, wh = C.move_and_slide(s, shape, he, qpos, rot, vel, **MS.CFG, hit_cap=3, self_entity=own)
        gs, gh = sq.move_and_slide(shape, he, qpos, rot, vel, **MS.CFG, hit_cap=3, self_entity=own)
        same_records(gs, ws, "move_and_slide: slides"); same_records(gh, wh, "move_and_slide: hit log")
        cap = shape == SHAPE_CAPSULE
        assert (want["collider"][cap] != MISS).sum() >= 5 and (gs["hit_count"][cap] > 0).sum() >= 5


# ---- the mixed scene ---------------------------------------------------------------------------------------------------------------------------------
def world_40(bits):
    bodies, cols, tf, sensor = scene_40()
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    return w, sq, snapshot_of(w, cols, tf), cols, sensor


@pytest.mark.parametrize("bits", [32, 64])
def test_mixed_batch_of_100(bits):
    """100 queries that mix capsules with balls and cuboids in one call, invalid capsules among them: caps 0 / 1 / 3 / 64, max_hits 1 and 4."""
    w, sq, s, cols, sensor = world_40(bits)
    rng = np.random.default_rng(100 + bits)
    q = with_invalid(mixed_queries(rng, s, 100))
    icnt, closest, ccnt, _ = check_all(sq, s, q, sensor, f"mixed f{bits}")
    assert_capsules_seen(q[0], icnt, closest, ccnt)
    bad = [3, 20, 41, 64, 70, 50]
    assert not icnt[bad].any() and (closest["collider"][bad] == MISS).all() and not ccnt[bad].any()
    cap = q[0] == SHAPE_CAPSULE
    assert (icnt[cap] > 0).sum() >= 10 and (ccnt[cap] > 0).sum() >= 10 and (closest["collider"][cap] != MISS).sum() >= 15
    assert closest["collider"][-3:].tolist().count(11) >= 1          # the far collider is hit from nearby
    st = sq.stats()
    assert st.nodes_visited > 0 and st.leaves_visited > 0


@pytest.mark.parametrize("bits", [32, 64])
def test_no_capsule_and_capsules_only(bits):
    w, sq, s, cols, sensor = world_40(bits)
    rng = np.random.default_rng(200 + bits)
    plain = mixed_queries(rng, s, 100, kinds=(0, 1))
    check_all(sq, s, plain, sensor, f"no capsule f{bits}", caps=(3,), ks=(4,))
    only = mixed_queries(rng, s, 100, kinds=(SHAPE_CAPSULE,))
    icnt, closest, ccnt, _ = check_all(sq, s, only, sensor, f"capsules only f{bits}", caps=(3,), ks=(4,))
    assert (icnt > 0).sum() >= 20 and (closest["collider"] != MISS).sum() >= 30 and (ccnt > 0).sum() >= 20


@pytest.mark.parametrize("bits", [32, 64])
def test_filters_and_sensors(bits):
    w, sq, s, cols, sensor = world_40(bits)
    rng = np.random.default_rng(300 + bits)
    q = mixed_queries(rng, s, 100)
    base = check_all(sq, s, q, sensor, "unfiltered", caps=(64,), ks=(4,))
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), 100)
    excluded = np.array([203, 210, 225], np.uint32)
    flt = check_all(sq, s, q, sensor, "filtered", caps=(64,), ks=(4,), mask=mask, excluded=excluded, skip_sensors=True)
    cap = q[0] == SHAPE_CAPSULE
    assert (flt[0][cap] != base[0][cap]).sum() >= 5 and (flt[2][cap] != base[2][cap]).sum() >= 3
    assert sensor.sum() >= 3 and not any(np.isin(l["collider"], np.nonzero(sensor)[0]).any() for l in flt[3])


@pytest.mark.parametrize("bits", [32, 64])
def test_device_pointers_equal_host_pointers(bits):
    import torch
    w, sq, s, cols, sensor = world_40(bits)
    rng = np.random.default_rng(400 + bits)
    shape, he, pos, rot, d, md = mixed_queries(rng, s, 100)
    dev = torch.device("cuda", 0)
    dt = DT[bits]
    T = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(np.asarray(a, t) if t else a)).to(dev)
    ts, th, tp, tr, td, tm = T(shape), T(he, dt), T(pos, dt), T(rot, dt), T(d, dt), T(md, dt)
    ids, cnt = sq.shape_intersections(ts, th, tp, tr, 3)
    hi, hc = sq.shape_intersections(shape, he, pos, rot, 3)
    assert ids.is_cuda and np.array_equal(ids.cpu().numpy().view(np.uint32).reshape(hi.shape), hi) and np.array_equal(cnt.cpu().numpy().view(np.uint32), hc)
    ct = sq.cast_shapes(ts, th, tp, tr, td, tm)
    host = sq.cast_shapes(shape, he, pos, rot, d, md)
    same_records(ct.cpu().numpy().reshape(-1).view(sq.shape_hit_dtype), host, "device pointers: cast_shapes")
    rec, rc = sq.shape_contacts(ts, th, tp, tr, T(np.full(100, 0.25), dt), 3)
    hr, hrc = sq.shape_contacts(shape, he, pos, rot, np.full(100, 0.25), 3)
    same_records(rec.cpu().numpy().reshape(-1).view(sq.shape_contact_dtype).reshape(hr.shape), hr, "device pointers: shape_contacts")
    assert np.array_equal(rc.cpu().numpy().view(np.uint32), hrc)
    mv = d * 0.8
    mt = sq.cast_moves(ts, th, tp, tr, T(mv, dt), T(np.full(100, 0.05), dt))
    mh = sq.cast_moves(shape, he, pos, rot, mv, np.full(100, 0.05))
    same_records(mt.cpu().numpy().reshape(-1).view(sq.move_hit_dtype), mh, "device pointers: cast_moves")
    ht, hcnt = sq.shape_hits(ts, th, tp, tr, td, 4, tm)
    hh, hhc = sq.shape_hits(shape, he, pos, rot, d, 4, md)
    same_records(ht.cpu().numpy().reshape(-1).view(sq.shape_hit_dtype).reshape(hh.shape), hh, "device pointers: shape_hits")
    assert np.array_equal(hcnt.cpu().numpy().view(np.uint32), hhc)
    dp = sq.depenetrate(ts, th, tp, tr, **DEPEN)
    same_records(dp.cpu().numpy().reshape(-1).view(sq.depenetration_dtype), sq.depenetrate(shape, he, pos, rot, **DEPEN), "device pointers: depenetrate")
    vel = d * 6.0
    st, sht = sq.move_and_slide(ts, th, tp, tr, T(vel, dt), **MS.CFG, hit_cap=3)
    sh, shh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=3)
    same_records(st.cpu().numpy().reshape(-1).view(sq.slide_dtype), sh, "device pointers: move_and_slide slides")
    same_records(sht.cpu().numpy().reshape(-1).view(sq.slide_hit_dtype).reshape(shh.shape), shh, "device pointers: move_and_slide hit log")
    cap = shape == SHAPE_CAPSULE
    assert (hhc[cap] > 1).sum() >= 5 and (sh["hit_count"][cap] > 0).sum() >= 5
    assert (host["collider"][cap] != MISS).sum() >= 10 and (hc[cap] > 0).sum() >= 5 and (mh["collider"][cap] != MISS).sum() >= 5


@pytest.mark.parametrize("bits", [32, 64])
def test_depenetrate_on_the_devices_own_records(bits):
    w, sq, s, cols, sensor = world_40(bits)
    rng = np.random.default_rng(500 + bits)
    shape, he, pos, rot, _, _ = mixed_queries(rng, s, 100)
    rec, cnt = sq.shape_contacts(shape, he, pos, rot, DEPEN["skin_width"], MAX_HITS, skip_sensors=True)
    want = CR.depenetrations(rec, cnt, DEPEN["skin_width"], DEPEN["max_depenetration_error"], DEPEN["penetration_rejection_threshold"], DEPEN["iterations"], bits)
    got = sq.depenetrate(shape, he, pos, rot, **DEPEN, skip_sensors=True)
    same_records(got, want, "depenetrate")
    cap = shape == SHAPE_CAPSULE
    assert (np.abs(got["fixup"][cap]).max(1) > 0).sum() >= 5 and (got["count"][cap] > 0).sum() >= 8
    # and the records themselves are the brute force's
    with np.errstate(all="ignore"):
        lists = C.contact_lists(s, shape, he, pos, rot, DEPEN["skin_width"], sensor=sensor, skip_sensors=True)
    same_records(rec, CR.pad(lists, MAX_HITS, bits)[0], "the contacts of the depenetration")


# ---- cast_moves and move_and_slide -----------------------------------------------------------------------------------------------------------------------
def room(bits):
    bodies, cols, sensor = MS.room()
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    return w, sq, snapshot_of(w, cols), sensor


@pytest.mark.parametrize("bits", [32, 64])
def test_cast_moves_origin_penetration_rule(bits):
    """Capsules sunk into the room's floor: on the way out the floor is ignored, on the way in it blocks at distance 0 with the contact's normal."""
    w, sq, s, sensor = room(bits)
    rng = np.random.default_rng(600 + bits)
    n = 64
    shape = np.full(n, SHAPE_CAPSULE, np.uint8); shape[::8] = rng.integers(0, 2, len(shape[::8]))
    he = np.c_[rng.uniform(0.3, 0.45, n), rng.uniform(0.2, 0.5, n), rng.uniform(0.3, 0.45, n)]
    rot = random_unit_quats(rng, n); rot[::2] = I
    pos = np.c_[rng.uniform(-5.5, -3.5, n), rng.uniform(0.05, 0.3, n), rng.uniform(-5.5, -3.5, n)]
    up = np.arange(n) % 4 < 2
    mv = np.c_[rng.normal(size=n) * 0.3, np.where(up, 1.0, -1.0) * rng.uniform(0.5, 1.5, n), rng.normal(size=n) * 0.3]
    pos[40:48, 1] = -0.2                                   # the whole core below the floor's top: cores crossing
    info = {}
    with np.errstate(all="ignore"):
        want = C.cast_moves(s, shape, he, pos, rot, mv, 0.05, sensor=sensor, info=info)
    assert C.last_rounds.max() < C.ROUNDS
    got = sq.cast_moves(shape, he, pos, rot, mv, 0.05)
    same_records(got, want, "cast_moves")
    cap = shape == SHAPE_CAPSULE
    assert (info["ignored"][cap] > 0).sum() >= 15 and (info["blocked"][cap] > 0).sum() >= 15
    blocked = cap & (got["collider"] == 0) & (got["collision_distance"] > 0) & (info["blocked"] > 0)
    assert blocked.sum() >= 10 and (got["distance"][blocked] == 0).all() and (got["normal1"][blocked][:, 1] > 0.9).all()


def slide_cfg():
    return dict(MS.CFG)


@pytest.mark.parametrize("bits", [32, 64])
def test_move_and_slide_along_a_floor_into_a_wall(bits):
    w, sq, s, sensor = room(bits)
    rng = np.random.default_rng(700 + bits)
    n = 16
    shape = np.full(n, SHAPE_CAPSULE, np.uint8)
    he = np.tile([0.4, 0.5, 0.0], (n, 1))                  # the reference character: Collider::capsule(0.4, 1.0)
    pos = np.c_[rng.uniform(4.0, 5.0, n), 0.9 + rng.uniform(0.0, 0.05, n), rng.uniform(-4, 4, n)]
    rot = np.tile(I, (n, 1))
    vel = np.c_[rng.uniform(6, 12, n), -rng.uniform(0.5, 2, n), rng.normal(size=n)]
    with np.errstate(all="ignore"):
        ws, wh = C.move_and_slide(s, shape, he, pos, rot, vel, **slide_cfg(), hit_cap=6, sensor=sensor)
    gs, gh = sq.move_and_slide(shape, he, pos, rot, vel, **slide_cfg(), hit_cap=6)
    same_records(gs, ws, "slides"); same_records(gh, wh, "hit log")
    # they end against the wall (its face at x = 6) on the floor, sliding along both
    assert (gs["hit_count"] >= 2).all() and (gs["position"][:, 0] < 6.0 - 0.4 + 1e-3).all() and (gs["position"][:, 0] > 5.0).all()
    assert (gs["position"][:, 1] > 0.9 - 1e-3).all() and (np.abs(gs["projected_velocity"][:, 0]) < 1e-3).all()
    assert set(gh["collider"][gh["collider"] != MISS]) >= {0, 1}


@pytest.mark.parametrize("bits", [32, 64])
def test_move_and_slide_up_against_a_box_corner(bits):
    w, sq, s, sensor = room(bits)
    rng = np.random.default_rng(800 + bits)
    n = 16
    shape = np.full(n, SHAPE_CAPSULE, np.uint8)
    he = np.tile([0.4, 0.5, 0.0], (n, 1))
    crate = np.array([-2.5, 0.5, 3.0])                     # the rotated crate of the room, half extents 0.5
    ang = rng.uniform(0, 2 * np.pi, n)
    pos = crate + np.c_[np.cos(ang) * 2.0, np.full(n, 0.45), np.sin(ang) * 2.0]
    rot = random_unit_quats(rng, n); rot[::2] = I
    aim = crate + np.c_[rng.normal(size=n) * 0.2, np.zeros(n), rng.normal(size=n) * 0.2] - pos
    vel = aim / np.linalg.norm(aim, axis=1, keepdims=True) * rng.uniform(6, 10, n)[:, None]
    with np.errstate(all="ignore"):
        ws, wh = C.move_and_slide(s, shape, he, pos, rot, vel, **slide_cfg(), hit_cap=6, sensor=sensor)
    gs, gh = sq.move_and_slide(shape, he, pos, rot, vel, **slide_cfg(), hit_cap=6)
    same_records(gs, ws, "slides"); same_records(gh, wh, "hit log")
    assert (gh["collider"] == 8).any(1).sum() >= 10 and (gs["iterations_run"] >= 2).sum() >= 10


# ---- a body-anchored capsule ShapeCaster -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_body_anchored_capsule_caster_over_two_steps(bits):
    bodies, cols, tf = layered_compound_scene()
    shapes = caster_set(91, bodies, cols, tf, hit_cap=4, shapes=True, rich=True)
    n = len(shapes["shape"])
    cap = np.arange(n) % 3 != 0
    shapes["shape"] = np.where(cap, SHAPE_CAPSULE, shapes["shape"]).astype(np.uint8)
    body = cap & (np.arange(n) % 2 == 0)
    shapes["anchor_kind"] = np.where(body, BODY, shapes["anchor_kind"]).astype(np.uint8)
    shapes["anchor"] = np.where(body, np.arange(n) % len(bodies["position"]), shapes["anchor"]).astype(np.uint32)
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    w.pipeline_enable()
    sq = SpatialQuery(w)
    poses = []
    for step in range(3):
        with C.patched():
            (hits, count), = run_and_check(w, sq, cols, tf, shapes=shapes, what=f"step {step}")
        poses.append(sq.caster_poses(CASTER_SHAPE)[0].copy())
        if step == 0:
            assert (count[cap] > 0).sum() >= 15 and (count[body] > 0).sum() >= 5
        w.step()
    assert (poses[0][body] != poses[1][body]).any(1).sum() >= 5 and (poses[1][body] != poses[2][body]).any(1).sum() >= 5
