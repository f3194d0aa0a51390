"""GPU: the spatial queries against Triangle COLLIDERS (avn_spatial_triangle_colliders_set; include/avian_mi355x_spatial.h, "queries against triangle
colliders") through every entry point, against the brute force of tests/spatial_triangle_collider_reference.py, tolerance 0: every byte of every record
and every count, f32 and f64.  The world is tests/spatial_triangle_set.py's scene -- scenes.trimesh_drop with 32 faces of a bumpy mesh on a moved and tilted
static body and 18 boxes, balls and capsules -- uploaded with native triangles and stepped four times in the closed loop; some colliders are children with a
ColliderTransform, some sensors, there are three membership layers and one body's pose is NaN.  A call holds 512 queries of all three query kinds aimed at
faces, shared edges and vertices, so both launches of every CTRI kernel run, over more than one wave."""
import functools

import numpy as np
import pytest

from avian_amd import scenes
from avian_amd.spatial_query import MAX_HITS, MISS, SHAPE_CAPSULE, SpatialQuery
from helpers import F, hip_lib, random_unit_quats
import spatial_capsule_collider_reference as CC
import spatial_contact_reference as CR
import spatial_move_scenes as MS
import spatial_query_reference as R
import spatial_triangle_collider_reference as TC
import spatial_triangle_set as TS
from test_gpu_spatial_capsule_colliders import DEPEN, host_of, to_device
from test_gpu_spatial_casters import compare, upload
from test_gpu_spatial_contacts import mixed_scene, world_of
from test_gpu_spatial_query import same_ids, same_records, snapshot_of

pytestmark = pytest.mark.gpu

N = TS.N
TRI = TS.TRI
NAN_BODY = 5            # a dynamic body whose position is made NaN after the steps: its collider is never a candidate
STATE = 6               # AVN_ERR_STATE


# ---- the world ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    sc = TS.scene()
    cols = sc.collider_kwargs(native_triangles=True)
    n = len(cols["shape"])
    nf = sc.n_faces
    rng = np.random.default_rng(5)
    cols["entity_index"] = np.arange(300, 300 + n, dtype=np.uint32)
    cols["memberships"] = (1 << rng.integers(0, 3, n)).astype(np.uint32)
    flags = np.where(rng.random(n) < 0.1, F.COLLIDER_SENSOR, 0).astype(np.uint8)
    cols["collider_flags"] = flags
    child = (np.arange(n) % 6 == 2) & (np.arange(n) >= nf)          # (the bodies' colliders; the faces get their frame from body 0's pose)
    tf = dict(is_child=child.astype(np.uint8), translation=rng.uniform(-0.2, 0.2, (n, 3)), rotation=random_unit_quats(rng, n))
    tri = cols["shape"] == TRI
    assert n == 50 and nf == 32 and tri.sum() == 32 and child.sum() >= 2 and ((flags != 0) & tri).sum() >= 2 and len(set(cols["memberships"][tri])) == 3
    return sc, cols, tf, (flags != 0).astype(np.uint8)


def stepped_world(bits, triangle_colliders=True, capsule_colliders=True, host=None, steps=4):
    """The scene stepped four times; then body NAN_BODY's position becomes NaN (the poses go through a download and an upload unchanged)."""
    sc, cols, tf, sensor = scene()
    if host is not None:
        cols = dict(cols, shape=np.where(np.arange(len(cols["shape"])) == host, F.SHAPE_HOST, cols["shape"]).astype(np.uint8))
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**cols); w.collider_transforms_upload(**tf)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction, restitution=0.0)
    if host is None and steps:
        w.pipeline_enable()
        for _ in range(steps):
            w.step()
    b = w.bodies_download()
    b["position"][NAN_BODY, 1] = np.nan
    w.bodies_upload(**dict(sc.body_kwargs(), **b))
    sq = SpatialQuery(w, capsule_colliders=capsule_colliders, triangle_colliders=triangle_colliders)
    sq.update()
    return w, sq, reference_snapshot(w, cols, tf), cols, tf, sensor


def reference_snapshot(w, cols, tf):
    s = snapshot_of(w, {k: v for k, v in cols.items() if k != "triangles"}, tf)
    return TC.with_triangles(s, cols["triangles"]["vertices"], cols["triangles"]["edge_flags"])


def on_faces(s, colliders):
    c = np.asarray(colliders)
    return (c != MISS) & (s.shape == TRI)[np.where(c == MISS, 0, c)]


# ---- every entry point, byte for byte; each test is one kind of launch, so that they can be run alone, narrowest first ------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_update_snapshots_the_faces_as_candidates(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    st = sq.stats()
    assert st.valid == 1 and st.colliders == 50 and st.host_skipped == 0
    # one straight-down ray per face centre: the face (or a body lying on it) answers
    sc = scene()[0]
    c = TS.faces_of(sc).mean(1)
    o = c + [0.0, 3.0, 0.0]
    d = np.tile([0.0, -1.0, 0.0], (len(c), 1))
    got = sq.cast_rays(o, d)
    same_records(got, TC.cast_rays(s, o, d), "centre rays")
    assert on_faces(s, got["collider"]).sum() >= 20


@pytest.mark.parametrize("bits", [32, 64])
def test_rays(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(1)
    o, d, md, solid = TS.rays_of(rng, scene()[0])
    mask = np.random.default_rng(1000 + bits).choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), N)
    ex = np.array([305, 333], np.uint32)
    closest, many = TC.ray_queries(s, o, d, (2, 8), md, solid, mask, ex)
    got = sq.cast_rays(o, d, md, solid, mask=mask, excluded=ex)
    same_records(got, closest, "cast_rays")
    for k in (2, 8):
        h, c = sq.ray_hits(o, d, k, md, solid, mask=mask, excluded=ex)
        same_records(h, many[k][0], f"ray_hits k={k}")
        assert np.array_equal(c, many[k][1])
    plain = sq.cast_rays(o, d, md, solid)
    same_records(plain, TC.cast_rays(s, o, d, md, solid), "cast_rays, no filter")
    face = on_faces(s, plain["collider"])
    up = d[:, 1] > 0
    assert face.sum() >= 200 and (face & up).sum() >= 40 and (face & ~up).sum() >= 100      # both sides
    assert (sq.ray_hits(o, d, 8, md, solid)[1] > 1).sum() >= 20                             # a shared edge or a vertex: more than one face
    assert not (plain["collider"] == 32 + NAN_BODY - 1).any() and (plain["collider"][[77, 78]] == MISS).all()   # the NaN body's collider; the non-finite rays
    to, td, tm, tsol = to_device(bits, o, d, md, solid)
    same_records(host_of(sq.cast_rays(to, td, tm, tsol), sq.hit_dtype, (N,)), plain, "device pointers: cast_rays")


@pytest.mark.parametrize("bits", [32, 64])
def test_points_boxes_and_projections(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(2)
    sc = scene()[0]
    p, face, kind = TS.targets(rng, sc, N)
    pts = p + rng.normal(size=(N, 3)) * np.choose(np.arange(N) % 4, [0.0, 0.0, 0.05, 0.5])[:, None]
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), N)
    ex = np.array([305, 333], np.uint32)
    for cap in (2, 16):
        same_ids(sq.point_intersections(pts, cap, mask=mask), TC.point_intersections(s, pts, cap, mask), f"points cap={cap}")
    lo = pts - rng.uniform(0.05, 0.6, (N, 3)); hi = pts + rng.uniform(0.05, 0.6, (N, 3))
    for cap in (3, 32):
        same_ids(sq.aabb_intersections(lo, hi, cap, excluded=ex), TC.aabb_intersections(s, lo, hi, cap, None, ex), f"aabbs cap={cap}")
    ids, cnt = sq.aabb_intersections(lo, hi, 32)
    assert on_faces(s, ids).sum() >= 1000 and (cnt > 3).sum() >= 100
    psolid = (np.arange(N) % 2).astype(np.uint8)
    pr = sq.project_points(pts, psolid, mask=mask)
    same_records(pr, TC.project_points(s, pts, psolid, mask), "project_points")
    plain = sq.project_points(pts, psolid)
    same_records(plain, TC.project_points(s, pts, psolid), "project_points, no filter")
    assert on_faces(s, plain["collider"]).sum() >= 300
    tp, ts = to_device(bits, pts, psolid)
    same_records(host_of(sq.project_points(tp, ts), sq.projection_dtype, (N,)), plain, "device pointers: project_points")


def shapes(seed=3):
    return TS.shapes_of(np.random.default_rng(seed), scene()[0])


@pytest.mark.parametrize("bits", [32, 64])
def test_shape_intersections(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    shape, he, pos, rot, d, md = shapes()
    mask = np.random.default_rng(2000 + bits).choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), N)
    ex = np.array([310, 344], np.uint32)
    for cap in (2, 32):
        same_ids(sq.shape_intersections(shape, he, pos, rot, cap, mask=mask, excluded=ex), TC.shape_intersections(s, shape, he, pos, rot, cap, mask, ex), f"intersections cap={cap}")
    ids, cnt = sq.shape_intersections(shape, he, pos, rot, 32)
    same_ids((ids, cnt), TC.shape_intersections(s, shape, he, pos, rot, 32), "intersections, no filter")
    for kind in (0, 1, SHAPE_CAPSULE):
        assert on_faces(s, ids[shape == kind]).sum() >= 40, kind
    assert (cnt[[200, 300, 400]] == 0).all()
    ts, th, tp, tr = to_device(bits, shape, he, pos, rot)
    di, dc = sq.shape_intersections(ts, th, tp, tr, 32)
    assert np.array_equal(host_of(di, np.uint32, ids.shape), ids) and np.array_equal(host_of(dc, np.uint32, cnt.shape), cnt)


@pytest.mark.parametrize("bits", [32, 64])
def test_shape_casts(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    q = shapes()
    shape, he, pos, rot, d, md = q
    mask = np.random.default_rng(2500 + bits).choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), N)
    ex = np.array([310, 344], np.uint32)
    TC.reset_rounds(); CC.reset_rounds()
    closest, many = TC.cast_queries(s, shape, he, pos, rot, d, (1, 4), md, mask, ex)
    plain, _ = TC.cast_queries(s, shape, he, pos, rot, d, (), md)
    assert TC.last_rounds < TC.ROUNDS and CC.last_rounds < CC.ROUNDS, "a pair of the set reaches the Newton round cap"
    same_records(sq.cast_shapes(shape, he, pos, rot, d, md, mask=mask, excluded=ex), closest, "cast_shapes")
    for k in (1, 4):
        h, cnt = sq.shape_hits(shape, he, pos, rot, d, k, md, mask=mask, excluded=ex)
        same_records(h, many[k][0], f"shape_hits k={k}")
        assert np.array_equal(cnt, many[k][1]), f"shape_hits k={k} counts"
    got = sq.cast_shapes(shape, he, pos, rot, d, md)
    same_records(got, plain, "cast_shapes, no filter")
    face = on_faces(s, got["collider"])
    for kind in (0, 1, SHAPE_CAPSULE):
        lanes = (shape == kind) & face
        assert lanes.sum() >= 60 and (lanes & (got["distance"] > 0)).sum() >= 30 and (lanes & (got["distance"] == 0)).sum() >= 5, kind
    assert not (got["collider"][[200, 300, 400]] != MISS).any()
    ts, th, tp, tr, td, tm = to_device(bits, *q)
    same_records(host_of(sq.cast_shapes(ts, th, tp, tr, td, tm), sq.shape_hit_dtype, (N,)), got, "device pointers: cast_shapes")


@pytest.mark.parametrize("bits", [32, 64])
def test_shape_contacts_and_depenetrate(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    shape, he, pos, rot, d, md = shapes()
    mask = np.random.default_rng(2700 + bits).choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), N)
    pred = np.where(np.arange(N) % 2, 0.25, 0.0)
    for kw, what in ((dict(mask=mask, excluded=np.array([310, 344], np.uint32), skip_sensors=True), "filtered"), (dict(), "plain")):
        lists = TC.contact_lists_of(s, shape, he, pos, rot, pred, mask=kw.get("mask"), excluded=kw.get("excluded", ()), sensor=sensor, skip_sensors=kw.get("skip_sensors", False))
        for cap in (2, MAX_HITS):
            rec, cnt = sq.shape_contacts(shape, he, pos, rot, pred, cap, **kw)
            want = CR.pad(lists, cap, bits)
            same_records(rec, want[0], f"{what}: shape_contacts cap={cap}")
            assert np.array_equal(cnt, want[1]), f"{what}: shape_contacts cap={cap} counts"
    for kind in (0, 1, SHAPE_CAPSULE):
        assert sum(on_faces(s, l["collider"]).sum() for l, k in zip(lists, shape) if k == kind) >= 40, kind
    lists = TC.contact_lists_of(s, shape, he, pos, rot, DEPEN["skin_width"], sensor=sensor, skip_sensors=True)
    rec, cnt = CR.pad(lists, MAX_HITS, bits)
    want = CR.depenetrations(rec, cnt, DEPEN["skin_width"], DEPEN["max_depenetration_error"], DEPEN["penetration_rejection_threshold"], DEPEN["iterations"], bits)
    dp = sq.depenetrate(shape, he, pos, rot, **DEPEN, skip_sensors=True)
    same_records(dp, want, "depenetrate")
    assert (np.abs(dp["fixup"]).max(1) > 0).sum() >= 50
    ts, th, tp, tr = to_device(bits, shape, he, pos, rot)
    rec, rc = sq.shape_contacts(ts, th, tp, tr, to_device(bits, np.full(N, 0.25))[0], 4)
    hr, hrc = sq.shape_contacts(shape, he, pos, rot, np.full(N, 0.25), 4)
    same_records(host_of(rec, sq.shape_contact_dtype, hr.shape), hr, "device pointers: shape_contacts")
    assert np.array_equal(host_of(rc, np.uint32, hrc.shape), hrc)
    same_records(host_of(sq.depenetrate(ts, th, tp, tr, **DEPEN), sq.depenetration_dtype, (N,)), sq.depenetrate(shape, he, pos, rot, **DEPEN), "device pointers: depenetrate")


@pytest.mark.parametrize("bits", [32, 64])
def test_cast_moves_move_and_slide_and_project_velocities(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(3000 + bits)
    shape, he, pos, rot, d, md = shapes()
    own = np.where(rng.random(N) < 0.2, 300 + rng.integers(32, s.n, N), MISS).astype(np.uint32)
    mv = d * rng.uniform(0.2, 2.0, N)[:, None]
    info = {}
    want = TC.cast_moves(s, shape, he, pos, rot, mv, 0.05, own, sensor=sensor, info=info)
    got = sq.cast_moves(shape, he, pos, rot, mv, 0.05, self_entity=own)
    same_records(got, want, "cast_moves")
    face = on_faces(s, got["collider"])
    assert face.sum() >= 200 and (info["blocked"] > 0).sum() >= 10 and (info["ignored"] + info["no_contact"] > 0).sum() >= 1
    for kind in (0, 1, SHAPE_CAPSULE):
        assert (face & (shape == kind)).sum() >= 40, kind
    vel = d * rng.uniform(2, 8, N)[:, None]
    ws, wh = TC.move_and_slide(s, shape, he, pos, rot, vel, **MS.CFG, hit_cap=4, self_entity=own, sensor=sensor)
    gs, gh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=4, self_entity=own)
    same_records(gs, ws, "move_and_slide: slides"); same_records(gh, wh, "move_and_slide: hit log")
    assert on_faces(s, gh["collider"]).sum() >= 200 and (gs["hit_count"] > 1).sum() >= 30
    # project_velocities reads no snapshot: the same bytes as a world without the switch gives
    normals = np.zeros((N, 4, 3), np.float32); normals[:, 0] = gh["normal"][:, 0]; normals[:, 1] = [0.0, 1.0, 0.0]
    counts = np.full(N, 2, np.uint32)
    pv = sq.project_velocities(vel, normals, counts)
    w2, sq2, *_ = stepped_world(bits, triangle_colliders=False, steps=0)
    assert np.array_equal(pv.view(np.uint8), sq2.project_velocities(vel, normals, counts).view(np.uint8))
    ts, th, tp, tr, tm, tv = to_device(bits, shape, he, pos, rot, mv, vel)
    same_records(host_of(sq.cast_moves(ts, th, tp, tr, tm, to_device(bits, np.full(N, 0.05))[0]), sq.move_hit_dtype, (N,)),
                 sq.cast_moves(shape, he, pos, rot, mv, np.full(N, 0.05)), "device pointers: cast_moves")
    st, sht = sq.move_and_slide(ts, th, tp, tr, tv, **MS.CFG, hit_cap=4)
    sh, shh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=4)
    same_records(host_of(st, sq.slide_dtype, (N,)), sh, "device pointers: slides"); same_records(host_of(sht, sq.slide_hit_dtype, shh.shape), shh, "device pointers: hit log")


@pytest.mark.parametrize("bits", [32, 64])
def test_ray_and_shape_casters_through_casters_run(bits):
    """512 ray casters and 512 shape casters of the three kinds anchored on bodies, colliders and the world; the run snapshots with the switch on."""
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(4000 + bits)
    o, d, md, solid = TS.rays_of(np.random.default_rng(1), scene()[0])
    o = np.nan_to_num(o); d = np.nan_to_num(d, posinf=1.0)
    shape, he, pos, rot, sd, smd = shapes()
    kind = rng.choice(np.array([0, 1, 2], np.uint8), N, p=[0.6, 0.2, 0.2])
    anchor = np.where(kind == 1, rng.integers(0, 19, N), rng.integers(0, s.n, N)).astype(np.uint32)
    local = kind != 0
    max_hits = np.array([1, 2, 3, 64], np.uint32)[np.arange(N) % 4]
    own = np.where(kind == 2, 300 + anchor, MISS).astype(np.uint32)      # a caster anchored on a collider -- a face among them -- ignores that collider's entity
    down = np.tile(np.array([0.05, -1.0, 0.02], np.float32), (N, 1))
    rays = dict(anchor_kind=kind, anchor=anchor, origin=np.where(local[:, None], rng.normal(scale=0.3, size=(N, 3)) + [0, 0.5, 0], o),
                direction=np.where(local[:, None], down, d.astype(np.float32)), max_distance=np.where(np.isinf(md), 6.0, md), max_hits=max_hits, hit_cap=4, solid=solid,
                self_entity=own, mask=rng.choice(np.array([1, 6, 0xFFFFFFFF], np.uint32), N))
    shapes_ = dict(anchor_kind=kind, anchor=anchor, origin=np.where(local[:, None], rng.normal(scale=0.3, size=(N, 3)) + [0, 0.8, 0], pos),
                   direction=np.where(local[:, None], down, sd.astype(np.float32)), max_distance=np.where(np.isinf(smd), 6.0, smd), max_hits=max_hits, hit_cap=4, shape=shape,
                   half_extents=he, shape_rotation=rot, self_entity=own)
    upload(sq, rays, False); upload(sq, shapes_, True)
    sq.casters_run()
    bodies = w.bodies_download()
    (hr, cr), (hs, cs) = compare(sq, TC.ray_casters(s, bodies, rays), TC.shape_casters(s, bodies, shapes_), f"casters f{bits}")
    for hits, count, several in ((hr, cr, 10), (hs, cs, 40)):       # (a ray meets a second collider only through a shared edge or under a body)
        assert on_faces(s, hits["collider"]).sum() >= 120 and (count > 1).sum() >= several
    on_own_face = (kind == 2) & (anchor < 32)
    assert on_own_face.sum() >= 40 and not (hr["entity"][on_own_face] == own[on_own_face, None]).any() and not (hs["entity"][on_own_face] == own[on_own_face, None]).any()
    assert sq.stats().host_skipped == 0


# ---- the switch --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_the_switch_off_on_and_flipped_without_an_update(bits):
    """Off: today's answers -- AVN_ERR_STATE without the skip flag, no face ever returned with it, host_skipped counts them.  Flipped on: the snapshot is
    invalid until the next update.  On: the reference with the faces as candidates; off again: the old answers byte for byte."""
    w, sq, s, cols, tf, sensor = stepped_world(bits, triangle_colliders=False)
    o, d, md, solid = TS.rays_of(np.random.default_rng(1), scene()[0])
    shape, he, pos, rot, sd, smd = shapes()
    off = TC.without_triangles(s)
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d, md, solid)
    assert e.value.status == STATE and "AVN_SHAPE_TRIANGLE" in str(e.value) and sq.stats().host_skipped == 32
    want_r = CC.cast_rays(off, o, d, md, solid)
    want_c = CC.cast_queries(off, shape, he, pos, rot, sd, (), smd)[0]
    got_r = sq.cast_rays(o, d, md, solid, skip_host_shapes=True)
    got_c = sq.cast_shapes(shape, he, pos, rot, sd, smd, skip_host_shapes=True)
    same_records(got_r, want_r, "switch off: cast_rays"); same_records(got_c, want_c, "switch off: cast_shapes")
    assert not on_faces(s, got_r["collider"]).any() and not on_faces(s, got_c["collider"]).any()
    sq.set_triangle_colliders(True)
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d, md, solid, skip_host_shapes=True)
    assert e.value.status == STATE                                   # the snapshot is invalidated
    sq.update()
    assert sq.stats().host_skipped == 0
    on_r = sq.cast_rays(o, d, md, solid)
    same_records(on_r, TC.cast_rays(s, o, d, md, solid), "switch on: cast_rays")
    assert on_faces(s, on_r["collider"]).sum() >= 200
    sq.set_triangle_colliders(False)
    sq.update()
    same_records(sq.cast_rays(o, d, md, solid, skip_host_shapes=True), got_r, "switch off again: cast_rays")
    same_records(sq.cast_shapes(shape, he, pos, rot, sd, smd, skip_host_shapes=True), got_c, "switch off again: cast_shapes")
    assert sq.stats().host_skipped == 32


@pytest.mark.parametrize("capsules, triangles", [(False, False), (True, False), (False, True), (True, True)])
def test_the_four_combinations_of_the_capsule_and_the_triangle_switch(capsules, triangles):
    w, sq, s, cols, tf, sensor = stepped_world(32, triangle_colliders=triangles, capsule_colliders=capsules)
    o, d, md, solid = TS.rays_of(np.random.default_rng(1), scene()[0])
    shape, he, pos, rot, sd, smd = shapes()
    ncap = int((s.shape == SHAPE_CAPSULE).sum())
    assert ncap == 6 and sq.stats().host_skipped == (0 if capsules else ncap) + (0 if triangles else 32)
    seen = s if triangles else TC.without_triangles(s)
    seen = seen if capsules else CC.without_capsules(seen)
    skip = not (capsules and triangles)
    if skip:
        with pytest.raises(F.AvnError) as e:
            sq.cast_rays(o, d, md, solid)
        assert e.value.status == STATE and ("AVN_SHAPE_TRIANGLE" in str(e.value)) == (not triangles)
    got = sq.cast_rays(o, d, md, solid, skip_host_shapes=skip)
    same_records(got, TC.cast_rays(seen, o, d, md, solid), "cast_rays")
    same_records(sq.cast_shapes(shape, he, pos, rot, sd, smd, skip_host_shapes=skip), TC.cast_queries(seen, shape, he, pos, rot, sd, (), smd)[0], "cast_shapes")
    rec, cnt = sq.shape_contacts(shape, he, pos, rot, 0.25, 4, skip_host_shapes=skip)
    want = TC.shape_contacts(seen, shape, he, pos, rot, 0.25, 4)
    same_records(rec, want[0], "shape_contacts"); assert np.array_equal(cnt, want[1])
    hit = got["collider"][got["collider"] != MISS]
    assert ((s.shape[hit] == TRI).sum() >= 200) == triangles and ((s.shape[hit] == SHAPE_CAPSULE).sum() >= 1) == capsules


def test_a_host_shape_keeps_its_rule_with_the_switch_on():
    w, sq, s, cols, tf, sensor = stepped_world(32, host=40)
    o, d, md, solid = TS.rays_of(np.random.default_rng(1), scene()[0])
    assert sq.stats().host_skipped == 1
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d, md, solid)
    assert e.value.status == STATE and "AVN_SHAPE_TRIANGLE" not in str(e.value)
    hosted = reference_snapshot(w, dict(cols, shape=np.where(np.arange(s.n) == 40, R.SHAPE_HOST, cols["shape"])), tf)
    got = sq.cast_rays(o, d, md, solid, skip_host_shapes=True)
    same_records(got, TC.cast_rays(hosted, o, d, md, solid), "one host shape, the switch on")
    assert not (got["collider"] == 40).any() and on_faces(s, got["collider"]).sum() >= 200


@pytest.mark.parametrize("bits", [32, 64])
def test_a_triangle_free_world_is_byte_identical_with_the_switch_on(bits):
    bodies, cols = mixed_scene(seed=4, n=40)
    rng = np.random.default_rng(7000 + bits)
    answers = []
    for on in (False, True):
        w = world_of(bits, bodies, cols)
        sq = SpatialQuery(w, triangle_colliders=on)
        sq.update()
        if not answers:
            s = snapshot_of(w, cols)
            pos_c = np.stack(s.pos, 1).astype(float)
            o = pos_c[rng.integers(0, s.n, N)] + rng.normal(size=(N, 3)) * 2; d = rng.normal(size=(N, 3)); solid = (np.arange(N) % 2).astype(np.uint8)
            shape = rng.choice(np.array([0, 1, SHAPE_CAPSULE], np.uint8), N); he = rng.uniform(0.1, 0.45, (N, 3))
            pos = pos_c[rng.integers(0, s.n, N)] + rng.normal(size=(N, 3)) * 0.7; rot = random_unit_quats(rng, N); sd = rng.normal(size=(N, 3))
        a = [sq.cast_rays(o, d, None, solid), sq.ray_hits(o, d, 4, None, solid)[0], sq.project_points(o, solid), sq.shape_intersections(shape, he, pos, rot, 8)[0],
             sq.cast_shapes(shape, he, pos, rot, sd), sq.shape_contacts(shape, he, pos, rot, 0.2, 8)[0], sq.cast_moves(shape, he, pos, rot, sd, 0.05),
             sq.move_and_slide(shape, he, pos, rot, sd * 4, **MS.CFG, hit_cap=3)[0], sq.depenetrate(shape, he, pos, rot, **DEPEN)]
        answers.append(a)
        assert sq.stats().host_skipped == 0
    names = ("cast_rays", "ray_hits", "project_points", "shape_intersections", "cast_shapes", "shape_contacts", "cast_moves", "move_and_slide", "depenetrate")
    for name, x, y in zip(names, *answers):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    assert (answers[0][0]["collider"] != MISS).sum() >= 50


def test_a_triangle_table_upload_after_an_update_invalidates_the_snapshot():
    w, sq, s, cols, tf, sensor = stepped_world(32)
    o, d, md, solid = TS.rays_of(np.random.default_rng(1), scene()[0])
    before = sq.cast_rays(o, d, md, solid)
    tri = cols["triangles"]
    moved = np.asarray(tri["vertices"], np.float64).copy()
    moved[:32, 1::3] -= 0.5                                           # every face half a unit lower in body 0's frame
    w.collider_triangles_upload(moved, tri["edge_flags"])
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d, md, solid)
    assert e.value.status == STATE
    sq.update()
    after = sq.cast_rays(o, d, md, solid)
    lowered = reference_snapshot(w, dict(cols, triangles=dict(vertices=moved, edge_flags=tri["edge_flags"])), tf)
    same_records(after, TC.cast_rays(lowered, o, d, md, solid), "after the new table")
    assert (after["distance"] != before["distance"]).sum() >= 150


# ---- a character -------------------------------------------------------------------------------------------------------------------------------------
def flat_mesh_world(bits, all_edges):
    sc = scenes.trimesh_drop(n_boxes=0, n_balls=1, n_capsules=0, nx=4, nz=4, all_edges=all_edges, seed=2)
    sc.position[1] = [0.0, 30.0, 0.0]                                  # (the one body the scene needs, far above the walk)
    cols = sc.collider_kwargs(native_triangles=True)
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64))
    sq = SpatialQuery(w, triangle_colliders=True)
    sq.update()
    return w, sq, reference_snapshot(w, cols, None)


@pytest.mark.parametrize("bits", [32, 64])
def test_a_capsule_character_walks_over_the_interior_edges_of_a_flat_mesh(bits):
    """64 capsule characters are walked by move_and_slide across a flat 4 x 4-quad mesh, pressed down onto it, over interior edges and vertices: with the
    adjacency's edge flags every slide normal the device logs is the face normal (0, 1, 0) and the characters keep their height within the project's band,
    32 eps (|position| + size + distance); the reference shows that the same walk over faces that all carry ALL_EDGES does log tilted normals."""
    dt = np.float32 if bits == 32 else np.float64
    w, sq, s = flat_mesh_world(bits, all_edges=False)
    rng = np.random.default_rng(8000)
    n = 64
    r, h = 0.3, 0.4
    shape = np.full(n, SHAPE_CAPSULE, np.uint8)
    he = np.tile([r, h, 0.0], (n, 1))
    start = np.c_[rng.uniform(-1.5, -1.2, n), np.full(n, r + h + 0.02), rng.uniform(-1.1, 1.1, n)]
    rot = np.tile(TS.I, (n, 1))
    vel = np.c_[rng.uniform(1.6, 2.2, n), np.full(n, -0.5), rng.uniform(-0.4, 0.4, n)]      # 0.25 s a step: five steps stay over the mesh's interior
    rest = r + h + MS.CFG["skin_width"]
    pos = start.copy()
    walked = np.zeros(n)
    for step in range(5):
        ws, wh = TC.move_and_slide(s, shape, he, pos, rot, vel, **MS.CFG, hit_cap=6)
        gs, gh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=6)
        same_records(gs, ws, f"step {step}: slides"); same_records(gh, wh, f"step {step}: hit log")
        logged = gh["collider"] != MISS
        nrm = gh["normal"][logged].astype(float)
        assert logged.any(1).all() and (nrm == [0.0, 1.0, 0.0]).all(), f"step {step}: a tilted slide normal {nrm[(nrm != [0.0, 1.0, 0.0]).any(1)][:3]}"
        new = gs["position"].astype(float)
        walked += np.linalg.norm(new - pos, axis=1)
        pos = new
        band = 32 * np.finfo(dt).eps * (np.abs(pos).sum(1) + (r + h) + 4.0 + walked)
        assert (np.abs(pos[:, 1] - rest) <= band).all(), f"step {step}: heights {pos[:, 1].min()} .. {pos[:, 1].max()}, band {band.max()}"
    assert (walked > 1.5).all() and (np.abs(pos[:, [0, 2]]) < 1.7).all()
    crossed = np.floor(pos[:, 0] + 2.0) - np.floor(start[:, 0] + 2.0)
    assert (crossed >= 2).all()                                       # every character crossed at least two of the mesh's x = const edge lines (and their diagonals)
    # the same walk over a bag of isolated triangles, by the reference: the interior edges do tilt normals
    sc7 = scenes.trimesh_drop(n_boxes=0, n_balls=1, n_capsules=0, nx=4, nz=4, all_edges=True, seed=2)
    s7 = TC.with_triangles(s, s.tri_vertices.reshape(s.n, 9), sc7.edge_flags)
    tilted = 0
    pos = start.copy()
    for step in range(5):
        ws, wh = TC.move_and_slide(s7, shape, he, pos, rot, vel, **MS.CFG, hit_cap=6)
        nrm = wh["normal"][wh["collider"] != MISS].astype(float)
        tilted += int((nrm != [0.0, 1.0, 0.0]).any(1).sum())
        pos = ws["position"].astype(float)
    assert tilted >= 20, tilted
