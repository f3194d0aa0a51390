"""GPU: avn_spatial_project_points and avn_spatial_shape_intersections against a brute-force pass of the numpy restatement
(tests/spatial_shape_reference.py) over every collider, tolerance 0: every record byte, every id and every count."""
import numpy as np
import pytest

from avian_amd import scenes
from avian_amd.spatial_query import SpatialQuery, MISS
from compound_helpers import compound_scene, compound_world
from helpers import F, hip_lib, random_unit_quats
import spatial_query_reference as R
import spatial_scenes as SC
import spatial_shape_cases as CASES
import spatial_shape_reference as S
from test_gpu_spatial_query import same_ids, same_records, snapshot_of

pytestmark = pytest.mark.gpu


def world_of(bits, bodies, cols, tf):
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))
    w.bodies_upload(**bodies)
    w.colliders_upload(**cols)
    w.collider_transforms_upload(**tf)
    return w


def queries(rng, s, n, he_hi=0.9):
    """n points (a quarter inside colliders, both solid values) and n query shapes of both kinds near the colliders."""
    pos = np.stack(s.pos, 1).astype(float)
    near = pos[rng.integers(0, s.n, n)]
    pts = near + rng.normal(scale=1.0, size=(n, 3))
    pts[: n // 4] = near[: n // 4] + rng.normal(scale=0.05, size=(n // 4, 3))
    solid = (rng.random(n) < 0.5).astype(np.uint8)
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.1, he_hi, (n, 3))
    qpos = near + rng.normal(scale=0.8, size=(n, 3))
    rot = random_unit_quats(rng, n)
    rot[: n // 8] = [0, 0, 0, 1]
    return pts, solid, shape, he, qpos, rot


def check_both(sq, s, rng, n, caps, mask=None, excluded=(), skip=False, he_hi=0.9):
    pts, solid, shape, he, qpos, rot = queries(rng, s, n, he_hi)
    kw = dict(mask=mask, excluded=excluded)
    ref = S.project_points(s, pts, solid, **kw)
    got = sq.project_points(pts, solid, skip_host_shapes=skip, **kw)
    same_records(got, ref, "project_points")
    hits, _ = S.shape_pairs(s, shape, he, qpos, rot)
    cand = R._masks(s, n, mask, excluded, np.ones(n, bool))
    for cap in caps:
        same_ids(sq.shape_intersections(shape, he, qpos, rot, cap, skip_host_shapes=skip, **kw), R._ids(hits & cand, cap), f"shape_intersections cap={cap}")
    return pts, solid, got, (hits & cand).sum(1)


@pytest.mark.parametrize("bits", [32, 64])
def test_mixed_scene_against_brute_force(bits):
    rng = np.random.default_rng(bits)
    bodies, cols, tf = compound_scene(seed=3, n_bodies=40)
    cols = dict(cols, memberships=(1 << rng.integers(0, 3, len(cols["shape"]))).astype(np.uint32))
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    assert s.n > 60 and (s.shape == R.SHAPE_BALL).any()
    pts, solid, got, counts = check_both(sq, s, rng, 130, (0, 4, 64), he_hi=1.5)
    assert (got["is_inside"] == 1).sum() >= 10 and (got["collider"] != MISS).all() and counts.max() > 4 and (counts == 0).any()
    # solid = 1: is_inside and the collider agree with point_intersections on the same snapshot
    ids, cnt = sq.point_intersections(pts, 4)
    sol = solid == 1
    assert np.array_equal(got["is_inside"][sol] == 1, cnt[sol] > 0)
    inside = sol & (cnt > 0)
    assert inside.sum() >= 5 and np.array_equal(got["collider"][inside], ids[inside, 0]) and (got["distance"][inside] == 0).all()
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), 130)
    excluded = rng.choice(cols["entity_index"], 12, replace=False)
    check_both(sq, s, rng, 130, (0, 4, 64), mask=mask, excluded=excluded, he_hi=1.5)


@pytest.mark.parametrize("n_colliders", [1, 2])
def test_smallest_trees(n_colliders):
    rng = np.random.default_rng(n_colliders)
    pos = [[0.5, 1.0, -0.25], [1.5, 1.25, 0.5]][:n_colliders]
    rot = random_unit_quats(rng, n_colliders)
    cols = dict(entity_index=np.arange(40, 40 + n_colliders, dtype=np.uint32), body=np.arange(n_colliders, dtype=np.int32),
                shape=np.array([R.SHAPE_CUBOID, R.SHAPE_BALL][:n_colliders], np.uint8), half_extents=np.array([[0.5, 0.75, 1.0], [0.75, 0, 0]][:n_colliders], float))
    tf = dict(is_child=np.zeros(n_colliders, np.uint8), translation=np.zeros((n_colliders, 3)), rotation=np.tile([0.0, 0, 0, 1], (n_colliders, 1)))
    w = world_of(32, SC.bodies_of(pos, rot), cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    _, _, got, counts = check_both(sq, s, rng, 70, (0, 1, 2))
    assert counts.max() >= 1 and (got["collider"] != MISS).all()


@pytest.mark.parametrize("bits", [32, 64])
def test_crafted_cases(bits):
    dt = np.float32 if bits == 32 else np.float64
    bodies, cols, tf = CASES.world()
    w = world_of(bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    pts, solid = CASES.projection_arrays()
    got = sq.project_points(pts, solid)
    want = CASES.expected_projections(dt)
    for i, case in enumerate(CASES.PROJECTIONS):
        assert got[i] == want[i], f"{case[0]}: device {got[i]} expected {want[i]}"
    same_records(got, S.project_points(s, pts, solid), "crafted projections")
    shape, he, pos, rot, want = CASES.shape_arrays(dt)
    ids, cnt = sq.shape_intersections(shape, he, pos, rot, 4)
    for i, case in enumerate(CASES.shape_cases(dt)):
        assert list(ids[i, :cnt[i]]) == want[i] and cnt[i] == len(want[i]), f"{case[0]}: device {ids[i]} expected {want[i]}"
    same_ids((ids, cnt), S.shape_intersections(s, shape, he, pos, rot, 4), "crafted shapes")


def test_resting_box_pile_ties_and_culling():
    sc = scenes.box_stack(12, 10, 12)
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); cols = sc.collider_kwargs(); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    w.pipeline_enable()
    for _ in range(5):
        w.step()
    w.synchronize()
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    C, n = s.n, 256
    assert C > 1400
    rng = np.random.default_rng(8)
    pos = np.stack(s.pos, 1).astype(float)
    centres = pos[rng.integers(1, C, n)]
    pts = centres + rng.normal(scale=0.6, size=(n, 3))
    pts[:64] = centres[:64] + np.array([0.0, 0.5, 0.0]) * rng.choice([-1.0, 1.0], (64, 1))   # on the face two resting boxes share
    solid = (rng.random(n) < 0.5).astype(np.uint8)
    same_records(sq.project_points(pts, solid), S.project_points(s, pts, solid), "pile: project_points")
    st = sq.stats()
    per_point = st.leaves_visited / n
    assert st.leaves_visited < n * C, f"{per_point:.0f} exact tests per projection: the tree does not cull"
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.1, 0.75, (n, 3))
    rot = random_unit_quats(rng, n); rot[:96] = [0, 0, 0, 1]
    qpos = centres + rng.normal(scale=0.5, size=(n, 3))
    qpos[:48] = centres[:48] + [1.0, 0, 0]; he[:48] = 0.5; shape[:48] = R.SHAPE_CUBOID   # the box a neighbour would be: zero separations
    same_ids(sq.shape_intersections(shape, he, qpos, rot, 16), S.shape_intersections(s, shape, he, qpos, rot, 16), "pile: shape_intersections")
    st = sq.stats()
    per_shape = st.leaves_visited / n
    assert st.leaves_visited < n * C, f"{per_shape:.0f} exact tests per shape: the tree does not cull"
    print(f"box_stack(12, 10, 12), {C} colliders: {per_point:.1f} exact tests per projection, {per_shape:.1f} per shape query")


def test_far_scene():
    rng = np.random.default_rng(21)
    bodies, cols, tf = SC.far_scene(7, n_bodies=24, spread=10.0, centre=(3000.0, -2000.0, 1000.0))
    w = world_of(32, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    _, _, got, counts = check_both(sq, s, rng, 130, (8,), he_hi=2.0)
    assert (got["collider"] != MISS).all() and counts.max() >= 2


def test_non_finite_and_invalid_queries_leave_the_other_lanes_alone():
    rng = np.random.default_rng(31)
    bodies, cols, tf = compound_scene(seed=5, n_bodies=30)
    w = compound_world(hip_lib(), 32, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    n = 64
    pts, solid, shape, he, qpos, rot = queries(rng, s, n, 1.5)
    pts[3] = [np.nan, 0, 0]; pts[17, 1] = np.inf; pts[40, 2] = -np.inf
    with np.errstate(all="ignore"):
        ref = S.project_points(s, pts, solid)
        got = sq.project_points(pts, solid)
    same_records(got, ref, "non-finite points")
    bad = [3, 17, 40]
    assert (got["collider"][bad] == MISS).all() and (got["entity"][bad] == MISS).all() and (got["distance"][bad] == 0).all() and (got["point"][bad] == 0).all()
    assert (np.delete(got["collider"], bad) != MISS).all()
    shape = shape.copy()
    qpos[2, 0] = np.nan; rot[9, 3] = np.inf; he[12] = [np.nan, 0.5, 0.5]; shape[12] = R.SHAPE_CUBOID
    he[20, 1] = -0.25; shape[20] = R.SHAPE_CUBOID; he[21, 0] = -0.5; shape[21] = R.SHAPE_BALL; shape[33] = 2; he[34] = [0.5, np.inf, 0.5]; shape[34] = R.SHAPE_CUBOID
    he[35] = [0.5, np.nan, -1.0]; shape[35] = R.SHAPE_BALL    # a ball's y and z are not read: a valid query
    with np.errstate(all="ignore"):
        ref = S.shape_intersections(s, shape, he, qpos, rot, 8)
        got = sq.shape_intersections(shape, he, qpos, rot, 8)
    same_ids(got, ref, "invalid query shapes")
    bad = [2, 9, 12, 20, 21, 33, 34]
    assert (got[1][bad] == 0).all() and (got[0][bad] == MISS).all() and np.delete(got[1], bad).sum() > 20


def test_device_pointers_equal_host_pointers():
    import torch
    rng = np.random.default_rng(11)
    bodies, cols, tf = compound_scene(seed=5, n_bodies=30)
    for bits, dt in ((32, np.float32), (64, np.float64)):
        w = compound_world(hip_lib(), bits, bodies, cols, tf)
        sq = SpatialQuery(w)
        sq.update()
        s = snapshot_of(w, cols, tf)
        n = 130
        pts, solid, shape, he, qpos, rot = (np.ascontiguousarray(a.astype(dt) if a.dtype == np.float64 else a) for a in queries(rng, s, n, 1.5))
        mask = rng.choice(np.array([1, 0xFFFFFFFF], np.uint32), n)
        excluded = cols["entity_index"][:5]
        dev = torch.device("cuda", 0)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        i32 = lambda a: T(a.view(np.int32))
        pt = sq.project_points(T(pts), T(solid), mask=i32(mask), excluded=i32(excluded))
        assert pt.dtype == torch.uint8 and tuple(pt.shape) == (n, sq.projection_dtype.itemsize)
        same_records(pt.cpu().numpy().reshape(-1).view(sq.projection_dtype), sq.project_points(pts, solid, mask=mask, excluded=excluded), "device pointers: project_points")
        for cap in (0, 4):
            it, ct = sq.shape_intersections(T(shape), T(he), T(qpos), T(rot), cap, mask=i32(mask), excluded=i32(excluded))
            ih, ch = sq.shape_intersections(shape, he, qpos, rot, cap, mask=mask, excluded=excluded)
            assert np.array_equal(it.cpu().numpy().view(np.uint32).reshape(n, cap), ih) and np.array_equal(ct.cpu().numpy().view(np.uint32), ch)
        assert ch.sum() > 20


def test_status_codes():
    sc = scenes.box_stack(4, 4, 4)
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); cols = sc.collider_kwargs(); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    sq = SpatialQuery(w)
    p = np.array([[0.3, 20.0, 0.3]])
    shape, he, rot = np.array([1], np.uint8), np.array([[0.5, 0, 0]]), np.array([[0, 0, 0, 1.0]])
    calls = (lambda: sq.project_points(p), lambda: sq.shape_intersections(shape, he, p, rot, 4))
    for call in calls:                       # before update()
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.update()
    for call in calls:
        call()
    w.colliders_upload(**cols)               # the tables changed: update again
    for call in calls:
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.update()
    # null arrays
    import ctypes as C
    from avian_amd import spatial_query as Q
    pin = Q.avn_spatial_solid_points(); pin.count = 1
    rec = np.zeros(1, sq.projection_dtype)
    pout = Q.avn_spatial_projections_out(rec.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_project_points(w.handle, C.byref(pin), C.byref(pout)) == 1
    sin = Q.avn_spatial_shapes(); sin.count = 1
    cnt = np.zeros(1, np.uint32)
    sout = Q.avn_spatial_ids_out(None, cnt.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_shape_intersections(w.handle, C.byref(sin), 0, C.byref(sout)) == 1
    assert sq.dll.avn_spatial_project_points(w.handle, None, C.byref(pout)) == 1
    assert sq.dll.avn_spatial_shape_intersections(w.handle, C.byref(sin), 0, None) == 1
    # a cap without an id array
    s8, h, r = shape.ctypes.data_as(Q.vp), np.zeros((1, 3), np.float32), np.array([[0, 0, 0, 1]], np.float32)
    sin.shape, sin.half_extents, sin.position, sin.rotation = s8, h.ctypes.data_as(Q.vp), h.ctypes.data_as(Q.vp), r.ctypes.data_as(Q.vp)
    assert sq.dll.avn_spatial_shape_intersections(w.handle, C.byref(sin), 4, C.byref(sout)) == 1
    assert sq.dll.avn_spatial_shape_intersections(w.handle, C.byref(sin), 0, C.byref(sout)) == 0


def test_host_shapes_need_the_skip_flag():
    from host_shape_helpers import capsule_world, capsule_scene
    w, _, _ = capsule_world(hip_lib(), 32)
    for _ in range(3):
        w.step()
    w.synchronize()
    _, cols, _, _ = capsule_scene()
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    rng = np.random.default_rng(9)
    n = 96
    pts = rng.uniform([-1, -1, -1], [8, 5, 8], (n, 3)); solid = (rng.random(n) < 0.5).astype(np.uint8)
    shape = (rng.random(n) < 0.5).astype(np.uint8); he = rng.uniform(0.2, 1.0, (n, 3)); rot = random_unit_quats(rng, n)
    for call in (lambda: sq.project_points(pts, solid), lambda: sq.shape_intersections(shape, he, pts, rot, 8)):
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    host = np.nonzero(s.shape == R.SHAPE_HOST)[0]
    got = sq.project_points(pts, solid, skip_host_shapes=True)
    same_records(got, S.project_points(s, pts, solid), "host shapes skipped: project_points")
    assert sq.stats().host_skipped == len(host) > 0 and not np.isin(got["collider"], host).any()
    ids, cnt = sq.shape_intersections(shape, he, pts, rot, 8, skip_host_shapes=True)
    same_ids((ids, cnt), S.shape_intersections(s, shape, he, pts, rot, 8), "host shapes skipped: shape_intersections")
    assert not np.isin(ids, host).any() and cnt.sum() > 0
