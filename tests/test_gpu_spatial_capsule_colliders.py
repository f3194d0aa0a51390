"""GPU: the spatial queries against Capsule COLLIDERS (avn_spatial_capsule_colliders_set; include/avian_mi355x_spatial.h, "queries against capsule
colliders") through every entry point, against the brute force of tests/spatial_capsule_collider_reference.py, tolerance 0: every byte of every
record and every count, f32 and f64.  The world is scenes.capsule_drop with 72 capsules among 128 boxes and balls (200 colliders with the
ground), some colliders children with a ColliderTransform, some sensors, three layers, stepped on the device first.  A call holds 512 queries
of all three query kinds, so both the CAPSULE second launch and the CCAP instantiations run, over more than one wave."""
import functools

import numpy as np
import pytest

from avian_amd import scenes
from avian_amd.spatial_query import MAX_HITS, MISS, SHAPE_CAPSULE, SpatialQuery
from helpers import F, hip_lib, random_unit_quats
import spatial_capsule_collider_reference as CC
import spatial_capsule_reference as C
import spatial_contact_reference as CR
import spatial_move_scenes as MS
import spatial_query_reference as R
import spatial_scenes as SC
from test_gpu_spatial_casters import compare, upload
from test_gpu_spatial_contacts import mixed_scene, world_of
from test_gpu_spatial_query import same_ids, same_records, snapshot_of

pytestmark = pytest.mark.gpu

I = [0.0, 0.0, 0.0, 1.0]
DT = {32: np.float32, 64: np.float64}
N = 512
NAN_BODY = 17          # a capsule's body whose position is made NaN after the steps: never a candidate
DEPEN = dict(skin_width=0.05, max_depenetration_error=1e-4, penetration_rejection_threshold=0.3, iterations=16)


# ---- the world ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    sc = scenes.capsule_drop(72, seed=3, n_boxes=64, n_balls=63)
    n = sc.n
    rng = np.random.default_rng(5)
    cols = sc.collider_kwargs()
    cols["entity_index"] = np.arange(300, 300 + n, dtype=np.uint32)
    cols["memberships"] = (1 << rng.integers(0, 3, n)).astype(np.uint32)
    cols["memberships"][0] = 0xFFFFFFFF
    flags = np.where(rng.random(n) < 0.1, F.COLLIDER_SENSOR, 0).astype(np.uint8)
    flags[0] = 0
    cols["collider_flags"] = flags
    child = (np.arange(n) % 6 == 2)
    tf = dict(is_child=child.astype(np.uint8), translation=rng.uniform(-0.2, 0.2, (n, 3)), rotation=random_unit_quats(rng, n))
    caps = sc.shape == SHAPE_CAPSULE
    assert n == 200 and caps.sum() == 72 and caps[NAN_BODY] and (child & caps).sum() >= 8 and ((flags != 0) & caps).sum() >= 3
    assert (cols["memberships"][caps] != 1).sum() >= 20
    return sc, cols, tf, (flags != 0).astype(np.uint8)


def stepped_world(bits, capsule_colliders=True, host=None):
    """The scene stepped four times; then body NAN_BODY's position becomes NaN (the poses go through a download and an upload unchanged)."""
    sc, cols, tf, sensor = scene()
    if host is not None:
        cols = dict(cols, shape=np.where(np.arange(sc.n) == host, F.SHAPE_HOST, cols["shape"]).astype(np.uint8))
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**cols); w.collider_transforms_upload(**tf)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction, restitution=0.0)
    if host is None:
        w.pipeline_enable()
        for _ in range(4):
            w.step()
    b = w.bodies_download()
    assert (b["position"][1:] != np.asarray(sc.position, w.dtype)[1:]).any() or host is not None
    b["position"][NAN_BODY, 1] = np.nan
    w.bodies_upload(**dict(sc.body_kwargs(), **b))
    sq = SpatialQuery(w, capsule_colliders=capsule_colliders)
    sq.update()
    return w, sq, snapshot_of(w, cols, tf), cols, tf, sensor


def axis_of(s, c):
    q = [float(x[c]) for x in s.rot]
    x, y, z, w = q
    return np.array([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)])


# ---- the queries ------------------------------------------------------------------------------------------------------------------------------------
def rays_of(rng, s):
    """512 rays: random ones aimed at colliders, rays along capsule axes through the end caps, origins inside capsules (solid and not)."""
    pos_c = np.stack(s.pos, 1).astype(float)
    caps = np.nonzero((s.shape == SHAPE_CAPSULE) & np.isfinite(pos_c).all(1))[0]
    tgt = rng.integers(1, s.n, N)
    d = rng.normal(size=(N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.nan_to_num(pos_c[tgt]) + rng.normal(size=(N, 3)) * 0.15 - d * rng.uniform(0.5, 4, N)[:, None]
    for k, c in enumerate(caps[:40]):
        a = axis_of(s, c)
        o[k] = pos_c[c] - a * 3.0; d[k] = a                       # along the axis, through both end caps
    for k, c in enumerate(caps[:40]):
        o[64 + k] = pos_c[c] + axis_of(s, c) * 0.2 * (k % 3 - 1)  # the origin inside, on the core
        o[128 + k] = pos_c[c] + rng.normal(size=3) * 0.08         # inside, off the core
    for k, c in enumerate(caps[:6]):
        d[64 + k] = axis_of(s, c)                                 # inside and parallel to the axis: the exit is a cap
    solid = (np.arange(N) % 2).astype(np.uint8)
    md = np.where(rng.random(N) < 0.25, rng.uniform(0.3, 3, N), np.inf)
    return o, d, md, solid


def shapes_of(rng, s):
    """512 query shapes of the three kinds near the colliders; capsules parallel to capsule colliders; starts that overlap; h = 0; invalid lanes."""
    pos_c = np.nan_to_num(np.stack(s.pos, 1).astype(float))
    rot_c = np.stack(s.rot, 1).astype(float)
    caps = np.nonzero(s.shape == SHAPE_CAPSULE)[0]
    shape = rng.choice(np.array([0, 1, SHAPE_CAPSULE], np.uint8), N)
    he = rng.uniform(0.1, 0.45, (N, 3))
    he[::9, 1] = 0.0
    tgt = rng.integers(1, s.n, N)
    if len(caps):
        tgt[:96] = caps[np.arange(96) % len(caps)]                # the first 96 lanes are aimed at capsule colliders
    pos = pos_c[tgt] + rng.normal(size=(N, 3)) * np.choose(np.arange(N) % 3, [0.2, 0.7, 1.5])[:, None]
    rot = random_unit_quats(rng, N)
    rot[::4] = I
    par = np.arange(0, 96, 3)
    shape[par] = SHAPE_CAPSULE; rot[par] = rot_c[tgt[par]]        # a query capsule parallel to the collider capsule it is aimed at
    d = pos_c[tgt] - pos + rng.normal(size=(N, 3)) * 0.2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = np.arange(N) % 3 == 2
    pos[far] -= d[far] * 1.5
    md = np.where(rng.random(N) < 0.3, rng.uniform(0.5, 4, N), np.inf)
    shape[[200, 300]] = SHAPE_CAPSULE; he[200, 0] = -0.1; he[300, 1] = np.nan; shape[400] = 2      # invalid lanes
    # the parallel lanes: tilted by 0 (exactly parallel) .. 4 mrad against their collider and set beside it at a surface gap of -3 .. +3 mm, the axes
    # converging or crossing -- where sp_seg_seg's parallel rule (f32: up to 2.8 mrad) alone would over-estimate the distance
    he_c = np.stack(s.he, 1).astype(float)
    for j, k in enumerate(par):
        th = TILTS[j % len(TILTS)] * (1 if j % 2 else -1)
        ax = np.array([0.0, 0.0, 1.0]) if j % 4 < 2 else np.array([1.0, 0.0, 0.0])
        rot[k] = qmul_np(rot_c[tgt[k]], list(ax * np.sin(th / 2)) + [np.cos(th / 2)])
        he[k, 1] = max(he[k, 1], 0.3)
        side = qrot_np(rot_c[tgt[k]], np.array([1.0, 0.0, 0.0]))
        gap = (-3e-3, -1e-3, -2e-4, 2e-4, 1e-3, 3e-3)[j % 6]
        off = 0.0 if j % 8 == 7 else he[k, 0] + he_c[tgt[k], 0] + gap + abs(np.sin(th)) * min(he[k, 1], he_c[tgt[k], 1])
        pos[k] = pos_c[tgt[k]] + side * off
        if j % 3 == 0 and off:
            pos[k] += side * 1.5; d[k] = -side                       # a cast from 1.5 m away straight at it
    return shape, he, pos, rot, d, md


TILTS = (0.0, 1e-7, 1e-4, 2e-4, 1e-3, 2e-3, 2.8e-3, 4e-3)


def qmul_np(l, r):
    lx, ly, lz, lw = l
    rx, ry, rz, rw = r
    return [lw * rx + lx * rw + ly * rz - lz * ry, lw * ry - lx * rz + ly * rw + lz * rx, lw * rz + lx * ry - ly * rx + lz * rw, lw * rw - lx * rx - ly * ry - lz * rz]


def qrot_np(q, v):
    b = np.asarray(q[:3], float)
    return v * (q[3] * q[3] - b @ b) + b * (2 * (v @ b)) + np.cross(b, v) * (2 * q[3])


def to_device(bits, *arrays):
    import torch
    dev = torch.device("cuda", 0)
    out = []
    for a in arrays:
        a = np.asarray(a)
        a = a if a.dtype in (np.uint8, np.uint32) else a.astype(DT[bits])
        out.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    return out


def host_of(t, dtype, shape):
    return t.cpu().numpy().reshape(-1).view(dtype).reshape(shape)


# ---- every entry point, byte for byte ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_rays_points_boxes_and_projections(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(1000 + bits)
    o, d, md, solid = rays_of(rng, s)
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), N)
    ex = np.array([305, 333, 371], np.uint32)
    closest, many = CC.ray_queries(s, o, d, (2, 8), md, solid, mask, ex)
    got = sq.cast_rays(o, d, md, solid, mask=mask, excluded=ex)
    same_records(got, closest, "cast_rays")
    for k in (2, 8):
        h, c = sq.ray_hits(o, d, k, md, solid, mask=mask, excluded=ex)
        same_records(h, many[k][0], f"ray_hits k={k}")
        assert np.array_equal(c, many[k][1]) and (c > k).sum() >= (3 if k == 2 else 0)
    caps = s.shape == SHAPE_CAPSULE
    on_cap = (got["collider"] != MISS) & caps[np.where(got["collider"] == MISS, 0, got["collider"])]
    assert on_cap.sum() >= 100 and on_cap[:40].sum() >= 8             # the axis rays hit end caps (the others are masked out or out of range)
    inside = np.arange(64, 168)
    zero_n = (got["distance"] == 0) & (got["normal"] == 0).all(1) & (got["collider"] != MISS)
    assert (zero_n[inside] & (solid[inside] == 1)).sum() >= 15 and ((got["distance"][inside] > 0) & (solid[inside] == 0) & on_cap[inside]).sum() >= 15
    assert not (got["collider"] == NAN_BODY).any() and not np.isin(many[8][0]["collider"], [NAN_BODY]).any()
    # device pointers: the same bytes
    to, td, tm, tsol = to_device(bits, o, d, md, solid)
    same_records(host_of(sq.cast_rays(to, td, tm, tsol), sq.hit_dtype, (N,)), sq.cast_rays(o, d, md, solid), "device pointers: cast_rays")
    # points and boxes
    pos_c = np.nan_to_num(np.stack(s.pos, 1).astype(float))
    pts = pos_c[rng.integers(1, s.n, N)] + rng.normal(size=(N, 3)) * np.choose(np.arange(N) % 2, [0.1, 0.5])[:, None]
    for cap in (2, 16):
        same_ids(sq.point_intersections(pts, cap, mask=mask), CC.point_intersections(s, pts, cap, mask), f"points cap={cap}")
    ids, cnt = sq.point_intersections(pts, 16)
    assert caps[ids[ids != MISS]].sum() >= 50
    lo = pts - rng.uniform(0.05, 0.6, (N, 3)); hi = pts + rng.uniform(0.05, 0.6, (N, 3))
    for cap in (3, 32):
        same_ids(sq.aabb_intersections(lo, hi, cap, excluded=ex), CC.aabb_intersections(s, lo, hi, cap, None, ex), f"aabbs cap={cap}")
    box_ids, box_cnt = sq.aabb_intersections(lo, hi, 32)
    assert caps[box_ids[box_ids != MISS]].sum() >= 200 and (box_cnt > 3).sum() >= 20
    psolid = (np.arange(N) % 2).astype(np.uint8)
    pr = sq.project_points(pts, psolid, mask=mask)
    same_records(pr, CC.project_points(s, pts, psolid, mask), "project_points")
    assert (caps[pr["collider"] % s.n] & (pr["collider"] != MISS)).sum() >= 80 and (pr["is_inside"] != 0).sum() >= 40
    tp, ts = to_device(bits, pts, psolid)
    same_records(host_of(sq.project_points(tp, ts), sq.projection_dtype, (N,)), sq.project_points(pts, psolid), "device pointers: project_points")


def check_shape_calls(sq, s, q, sensor, what, **flt):
    """test_gpu_spatial_capsule.check_all's comparisons with this module's reference."""
    shape, he, pos, rot, d, md = q
    n = len(shape)
    mask, ex = flt.get("mask"), flt.get("excluded", ())
    kw = dict(mask=mask, excluded=flt.get("excluded"))
    for cap in (2, 32):
        same_ids(sq.shape_intersections(shape, he, pos, rot, cap, **kw), CC.shape_intersections(s, shape, he, pos, rot, cap, mask, ex), f"{what}: intersections cap={cap}")
    CC.reset_rounds()
    closest, many = CC.cast_queries(s, shape, he, pos, rot, d, (1, 4), md, mask, ex)
    assert CC.last_rounds < CC.ROUNDS and (C.last_rounds.size == 0 or C.last_rounds.max() < C.ROUNDS), "a pair of the set reaches the Newton round cap"
    got = sq.cast_shapes(shape, he, pos, rot, d, md, **kw)
    same_records(got, closest, f"{what}: cast_shapes")
    for k in (1, 4):
        h, cnt = sq.shape_hits(shape, he, pos, rot, d, k, md, **kw)
        same_records(h, many[k][0], f"{what}: shape_hits k={k}")
        assert np.array_equal(cnt, many[k][1]), f"{what}: shape_hits k={k} counts"
    pred = np.where(np.arange(n) % 2, 0.25, 0.0)
    skip = flt.get("skip_sensors", False)
    lists = CC.contact_lists(s, shape, he, pos, rot, pred, mask=mask, excluded=ex, sensor=sensor, skip_sensors=skip)
    bits = 32 if s.dt == np.float32 else 64
    for cap in (2, MAX_HITS):
        rec, cnt = sq.shape_contacts(shape, he, pos, rot, pred, cap, skip_sensors=skip, **kw)
        want = CR.pad(lists, cap, bits)
        same_records(rec, want[0], f"{what}: shape_contacts cap={cap}")
        assert np.array_equal(cnt, want[1]), f"{what}: shape_contacts cap={cap} counts"
    return got, many[4][1], lists


@pytest.mark.parametrize("bits", [32, 64])
def test_shape_intersections_casts_and_contacts(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(2000 + bits)
    q = shapes_of(rng, s)
    shape = q[0]
    got, cnt4, lists = check_shape_calls(sq, s, q, sensor, f"f{bits}")
    caps = s.shape == SHAPE_CAPSULE
    hit = got["collider"] != MISS
    on_cap = hit & caps[got["collider"] % s.n]
    for kind in (0, 1, SHAPE_CAPSULE):
        lanes = (shape == kind) & on_cap
        assert lanes.sum() >= 15 and (lanes & (got["distance"] > 0)).sum() >= 8 and (lanes & (got["distance"] == 0)).sum() >= 2, kind
        assert sum(caps[l["collider"]].sum() for l, k in zip(lists, shape) if k == kind) >= 10, kind
    assert (cnt4 > 4).sum() >= 10 and not hit[[200, 300, 400]].any()
    assert not any((l["collider"] == NAN_BODY).any() for l in lists) and not (got["collider"] == NAN_BODY).any()
    # filtered, sensors skipped: the first 128 lanes (the ones aimed at capsule colliders among them)
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), 128)
    flt = check_shape_calls(sq, s, tuple(x[:128] for x in q), sensor, f"f{bits} filtered", mask=mask, excluded=np.array([310, 344], np.uint32), skip_sensors=True)
    assert not any(np.isin(l["collider"], np.nonzero(sensor)[0]).any() for l in flt[2])
    # device pointers
    shape, he, pos, rot, d, md = q
    ts, th, tp, tr, td, tm = to_device(bits, *q)
    same_records(host_of(sq.cast_shapes(ts, th, tp, tr, td, tm), sq.shape_hit_dtype, (N,)), got, "device pointers: cast_shapes")
    ids, c = sq.shape_intersections(ts, th, tp, tr, 8)
    hi, hc = sq.shape_intersections(shape, he, pos, rot, 8)
    assert np.array_equal(host_of(ids, np.uint32, hi.shape), hi) and np.array_equal(host_of(c, np.uint32, hc.shape), hc)
    rec, rc = sq.shape_contacts(ts, th, tp, tr, to_device(bits, np.full(N, 0.25))[0], 4)
    hr, hrc = sq.shape_contacts(shape, he, pos, rot, np.full(N, 0.25), 4)
    same_records(host_of(rec, sq.shape_contact_dtype, hr.shape), hr, "device pointers: shape_contacts")
    assert np.array_equal(host_of(rc, np.uint32, hrc.shape), hrc)


@pytest.mark.parametrize("bits", [32, 64])
def test_depenetrate_and_cast_moves(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(3000 + bits)
    shape, he, pos, rot, d, md = shapes_of(rng, s)
    caps = s.shape == SHAPE_CAPSULE
    # depenetrate: the device's own loop over the brute force's records
    lists = CC.contact_lists(s, shape, he, pos, rot, DEPEN["skin_width"], sensor=sensor, skip_sensors=True)
    rec, cnt = CR.pad(lists, MAX_HITS, bits)
    want = CR.depenetrations(rec, cnt, DEPEN["skin_width"], DEPEN["max_depenetration_error"], DEPEN["penetration_rejection_threshold"], DEPEN["iterations"], bits)
    dp = sq.depenetrate(shape, he, pos, rot, **DEPEN, skip_sensors=True)
    same_records(dp, want, "depenetrate")
    assert (np.abs(dp["fixup"]).max(1) > 0).sum() >= 50
    own = np.where(rng.random(N) < 0.2, 300 + rng.integers(1, s.n, N), MISS).astype(np.uint32)
    mv = d * rng.uniform(0.2, 2.0, N)[:, None]
    info = {}
    want = CC.cast_moves(s, shape, he, pos, rot, mv, 0.05, own, sensor=sensor, info=info)
    got = sq.cast_moves(shape, he, pos, rot, mv, 0.05, self_entity=own)
    same_records(got, want, "cast_moves")
    on_cap = (got["collider"] != MISS) & caps[got["collider"] % s.n]
    assert on_cap.sum() >= 60 and (info["blocked"] > 0).sum() >= 10 and (info["ignored"] > 0).sum() >= 10
    for kind in (0, 1, SHAPE_CAPSULE):
        assert (on_cap & (shape == kind)).sum() >= 10, kind
    ts, th, tp, tr, tm = to_device(bits, shape, he, pos, rot, mv)
    same_records(host_of(sq.cast_moves(ts, th, tp, tr, tm, to_device(bits, np.full(N, 0.05))[0]), sq.move_hit_dtype, (N,)),
                 sq.cast_moves(shape, he, pos, rot, mv, np.full(N, 0.05)), "device pointers: cast_moves")
    same_records(host_of(sq.depenetrate(ts, th, tp, tr, **DEPEN), sq.depenetration_dtype, (N,)), sq.depenetrate(shape, he, pos, rot, **DEPEN), "device pointers: depenetrate")


@pytest.mark.parametrize("bits", [32, 64])
def test_move_and_slide(bits):
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(3500 + bits)
    shape, he, pos, rot, d, md = shapes_of(rng, s)
    caps = s.shape == SHAPE_CAPSULE
    own = np.where(rng.random(N) < 0.2, 300 + rng.integers(1, s.n, N), MISS).astype(np.uint32)
    vel = d * rng.uniform(2, 8, N)[:, None]
    ws, wh = CC.move_and_slide(s, shape, he, pos, rot, vel, **MS.CFG, hit_cap=4, self_entity=own, sensor=sensor)
    gs, gh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=4, self_entity=own)
    same_records(gs, ws, "move_and_slide: slides"); same_records(gh, wh, "move_and_slide: hit log")
    logged = gh["collider"][gh["collider"] != MISS]
    assert caps[logged].sum() >= 60 and (gs["hit_count"] > 1).sum() >= 30
    # device pointers
    ts, th, tp, tr, tv = to_device(bits, shape, he, pos, rot, vel)
    st, sht = sq.move_and_slide(ts, th, tp, tr, tv, **MS.CFG, hit_cap=4)
    sh, shh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=4)
    same_records(host_of(st, sq.slide_dtype, (N,)), sh, "device pointers: slides"); same_records(host_of(sht, sq.slide_hit_dtype, shh.shape), shh, "device pointers: hit log")


@pytest.mark.parametrize("bits", [32, 64])
def test_ray_and_shape_casters_through_casters_run(bits):
    """512 ray casters and 512 shape casters of the three kinds anchored on bodies, colliders and the world; the run snapshots with the switch on."""
    w, sq, s, cols, tf, sensor = stepped_world(bits)
    rng = np.random.default_rng(4000 + bits)
    o, d, md, solid = rays_of(rng, s)
    shape, he, pos, rot, sd, smd = shapes_of(rng, s)
    kind = rng.choice(np.array([0, 1, 2], np.uint8), N, p=[0.6, 0.2, 0.2])
    anchor = np.where(kind == 1, rng.integers(0, s.n, N), rng.integers(0, s.n, N)).astype(np.uint32)
    local = kind != 0
    max_hits = np.array([1, 2, 3, 64], np.uint32)[np.arange(N) % 4]
    own = np.where(kind == 1, 300 + anchor, MISS).astype(np.uint32)
    rays = dict(anchor_kind=kind, anchor=anchor, origin=np.where(local[:, None], rng.normal(scale=0.3, size=(N, 3)), o), direction=d.astype(np.float32),
                max_distance=np.where(np.isinf(md), 6.0, md), max_hits=max_hits, hit_cap=4, solid=solid, self_entity=own,
                mask=rng.choice(np.array([1, 6, 0xFFFFFFFF], np.uint32), N))
    shapes = dict(anchor_kind=kind, anchor=anchor, origin=np.where(local[:, None], rng.normal(scale=0.3, size=(N, 3)), pos), direction=sd.astype(np.float32),
                  max_distance=np.where(np.isinf(smd), 6.0, smd), max_hits=max_hits, hit_cap=4, shape=shape, half_extents=he, shape_rotation=rot, self_entity=own)
    upload(sq, rays, False); upload(sq, shapes, True)
    sq.casters_run()
    bodies = w.bodies_download()
    (hr, cr), (hs, cs) = compare(sq, CC.ray_casters(s, bodies, rays), CC.shape_casters(s, bodies, shapes), f"casters f{bits}")
    caps = s.shape == SHAPE_CAPSULE
    for hits, count in ((hr, cr), (hs, cs)):
        got = hits["collider"][hits["collider"] != MISS]
        assert caps[got].sum() >= 80 and (count > 1).sum() >= 40 and NAN_BODY not in got
    assert sq.stats().host_skipped == 0


# ---- the switch --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_the_switch(bits):
    """Off: today's answers -- AVN_ERR_STATE without the skip flag, no capsule ever returned with it, host_skipped counts them.  Flipped on: the
    snapshot is invalid until the next update.  On: the reference with capsule candidates; off again: the old answers byte for byte."""
    w, sq, s, cols, tf, sensor = stepped_world(bits, capsule_colliders=False)
    rng = np.random.default_rng(5000 + bits)
    o, d, md, solid = rays_of(rng, s)
    shape, he, pos, rot, sd, smd = shapes_of(rng, s)
    caps = s.shape == SHAPE_CAPSULE
    off = CC.without_capsules(s)
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d, md, solid)
    assert e.value.status == 6 and sq.stats().host_skipped == 72   # AVN_ERR_STATE
    with np.errstate(all="ignore"):
        want_r = R.cast_rays(off, o, d, md, solid)
        want_c = C.cast_queries(off, shape, he, pos, rot, sd, (), smd)[0]
    got_r = sq.cast_rays(o, d, md, solid, skip_host_shapes=True)
    got_c = sq.cast_shapes(shape, he, pos, rot, sd, smd, skip_host_shapes=True)
    same_records(got_r, want_r, "switch off: cast_rays"); same_records(got_c, want_c, "switch off: cast_shapes")
    assert not caps[got_r["collider"][got_r["collider"] != MISS]].any() and not caps[got_c["collider"][got_c["collider"] != MISS]].any()
    sq.set_capsule_colliders(True)
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d, md, solid, skip_host_shapes=True)
    assert e.value.status == 6                                      # the snapshot is invalidated
    sq.update()
    assert sq.stats().host_skipped == 0
    on_r = sq.cast_rays(o, d, md, solid)
    same_records(on_r, CC.cast_rays(s, o, d, md, solid), "switch on: cast_rays")
    assert caps[on_r["collider"][on_r["collider"] != MISS]].sum() >= 100
    sq.set_capsule_colliders(False)
    sq.update()
    same_records(sq.cast_rays(o, d, md, solid, skip_host_shapes=True), got_r, "switch off again: cast_rays")
    same_records(sq.cast_shapes(shape, he, pos, rot, sd, smd, skip_host_shapes=True), got_c, "switch off again: cast_shapes")
    assert sq.stats().host_skipped == 72


def test_a_host_shape_keeps_its_rule_with_the_switch_on():
    w, sq, s, cols, tf, sensor = stepped_world(32, host=5)
    rng = np.random.default_rng(6000)
    o, d, md, solid = rays_of(rng, s)
    assert sq.stats().host_skipped == 1
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d, md, solid)
    assert e.value.status == 6
    host = R.Snapshot(w.bodies_download(), dict(cols, shape=np.where(np.arange(s.n) == 5, R.SHAPE_HOST, cols["shape"])), tf, w.dtype)
    got = sq.cast_rays(o, d, md, solid, skip_host_shapes=True)
    same_records(got, CC.cast_rays(host, o, d, md, solid), "one host shape, the switch on")
    assert not (got["collider"] == 5).any() and (s.shape == SHAPE_CAPSULE)[got["collider"][got["collider"] != MISS]].sum() >= 100


@pytest.mark.parametrize("bits", [32, 64])
def test_a_capsule_free_world_is_byte_identical_with_the_switch_on(bits):
    bodies, cols = mixed_scene(seed=4, n=40)
    rng = np.random.default_rng(7000 + bits)
    answers = []
    for on in (False, True):
        w = world_of(bits, bodies, cols)
        sq = SpatialQuery(w, capsule_colliders=on)
        sq.update()
        s = snapshot_of(w, cols)
        if not answers:
            o, d, md, solid = rays_of(rng, s)
            shape, he, pos, rot, sd, smd = shapes_of(rng, s)
        a = [sq.cast_rays(o, d, md, solid), sq.ray_hits(o, d, 4, md, solid)[0], sq.project_points(o, solid), sq.shape_intersections(shape, he, pos, rot, 8)[0],
             sq.cast_shapes(shape, he, pos, rot, sd, smd), sq.shape_contacts(shape, he, pos, rot, 0.2, 8)[0], sq.cast_moves(shape, he, pos, rot, sd, 0.05),
             sq.move_and_slide(shape, he, pos, rot, sd * 4, **MS.CFG, hit_cap=3)[0], sq.depenetrate(shape, he, pos, rot, **DEPEN)]
        answers.append(a)       # (the arrays as the calls returned them: a copy of a record array need not keep its padding bytes)
        assert sq.stats().host_skipped == 0
    names = ("cast_rays", "ray_hits", "project_points", "shape_intersections", "cast_shapes", "shape_contacts", "cast_moves", "move_and_slide", "depenetrate")
    for name, x, y in zip(names, *answers):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    assert (answers[0][0]["collider"] != MISS).sum() >= 50


# ---- a character -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_a_capsule_character_slides_along_a_lying_and_a_standing_capsule(bits):
    """Capsule characters walk along +x over a floor into a capsule lying along z and, further on, a standing one: they end outside both, having slid."""
    dt = DT[bits]
    lying = [0.7071067811865476, 0.0, 0.0, 0.7071067811865476]      # the axis (0, 1, 0) -> (0, 0, 1): lies along z
    items = [(R.SHAPE_CUBOID, [20.0, 0.5, 20.0], [0.0, -0.5, 0.0], I), (SHAPE_CAPSULE, [0.5, 3.0, 0.0], [3.0, 0.5, 0.0], lying),
             (SHAPE_CAPSULE, [0.5, 1.0, 0.0], [-1.0, 1.5, 4.0], I)]
    cols = dict(entity_index=np.arange(600, 603, dtype=np.uint32), body=np.arange(3, dtype=np.int32), shape=np.array([i[0] for i in items], np.uint8),
                half_extents=np.array([i[1] for i in items], float))
    w = world_of(bits, SC.bodies_of([i[2] for i in items], [i[3] for i in items]), cols)
    sq = SpatialQuery(w, capsule_colliders=True)
    sq.update()
    s = snapshot_of(w, cols)
    rng = np.random.default_rng(8000 + bits)
    n = 64
    shape = np.full(n, SHAPE_CAPSULE, np.uint8)
    he = np.tile([0.4, 0.5, 0.0], (n, 1))
    pos = np.c_[np.full(n, 0.5), 1.0 + rng.uniform(0.0, 0.05, n), rng.uniform(-2.0, 2.0, n)]     # (clear of the floor: the first sweep meets the capsule)
    pos[n // 2:] = np.c_[np.full(n // 2, -3.5), 1.0 + rng.uniform(0.0, 0.05, n // 2), 4.0 + rng.uniform(-0.6, 0.6, n // 2)]
    rot = np.tile(I, (n, 1))
    vel = np.c_[rng.uniform(6, 10, n), np.zeros(n), rng.uniform(1.0, 3.0, n) * np.where(rng.random(n) < 0.5, -1, 1)]
    CC.reset_rounds()
    ws, wh = CC.move_and_slide(s, shape, he, pos, rot, vel, **MS.CFG, hit_cap=6)
    assert CC.last_rounds < CC.ROUNDS
    gs, gh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=6)
    same_records(gs, ws, "slides"); same_records(gh, wh, "hit log")
    end = gs["position"].astype(float)
    # every character ends outside BOTH capsules: the exact distance of the cores (rational arithmetic on the device's own end position) minus the
    # radii is >= -band, band = 32 eps (|pos_q| + size_q + |pos_c| + size_c + distance)
    from test_spatial_capsule_colliders_cpu import Capsule, band_of, core_d2
    import spatial_exact_geometry as X
    cols_x = [Capsule(it[2], it[3], it[1][0], it[1][1], dt) for it in items[1:]]
    for i in range(n):
        q = Capsule(end[i], I, 0.4, 0.5, dt)
        for cap in cols_x:
            band = band_of(dt, q, cap, float(np.linalg.norm(end[i] - pos[i])))
            assert X.sqrt_q(core_d2(cap, SHAPE_CAPSULE, q)) - (q.r + cap.r) >= -band, (i, end[i])
    # they slid: a character whose first sweep hit capsule c at p_hit went on from there, along the surface -- the part of (end - p_hit)
    # perpendicular to the hit normal is centimetres, where a character that stopped at its first hit would have none
    speed = np.linalg.norm(vel.astype(np.float32).astype(float), axis=1)
    for k, c in enumerate((1, 2)):
        lanes = np.arange(n // 2) + k * (n // 2)
        first = gh[lanes, 0]
        hit = (first["collider"] == c) & (first["kind"] == 0) & (first["iteration"] == 0)
        assert hit.sum() >= n // 8, (c, hit.sum())
        slid = []
        for i, h in zip(lanes[hit], first[hit]):
            p_hit = pos[i] + vel[i] / speed[i] * float(h["distance"])
            m = end[i] - p_hit
            nrm = h["normal"].astype(float)
            slid.append(np.linalg.norm(m - nrm * (m @ nrm)))
            assert slid[-1] > 1e-3 and gs["iterations_run"][i] >= 2, (i, slid[-1])      # (> 0 by far more than band, about 5e-5 here in f32)
        assert np.median(slid) > 0.1, (c, np.median(slid))                              # a near head-on hit slides little, most slide far
