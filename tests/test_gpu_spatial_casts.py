"""GPU: avn_spatial_cast_shapes and avn_spatial_shape_hits against a brute-force pass of the numpy restatement
(tests/spatial_cast_reference.py) over every collider, tolerance 0: every record byte and every count."""
import numpy as np
import pytest

from avian_amd import scenes
from avian_amd.spatial_query import SpatialQuery, MISS
from compound_helpers import compound_scene, compound_world
from helpers import F, hip_lib, random_unit_quats
import spatial_cast_reference as CR
import spatial_query_reference as R
import spatial_scenes as SC
from test_gpu_spatial_query import same_records, snapshot_of
from test_gpu_spatial_shapes import world_of

pytestmark = pytest.mark.gpu


def casts(rng, s, n, he_hi=0.9, reach=6.0):
    """n casts of both kinds: shapes a few units from a collider and aimed at it, a quarter starting inside one, an eighth aimed away;
    a third with a finite range around the distance to the target."""
    pos = np.stack(s.pos, 1).astype(float)
    target = pos[rng.integers(0, s.n, n)]
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(1.0, reach, n)
    dist[: n // 4] = rng.uniform(0.0, 0.05, n // 4)            # starting inside (or touching) the target
    qpos = target - d * dist[:, None] + rng.normal(scale=0.3, size=(n, 3))
    d[n // 4: n // 4 + n // 8] *= -1.0                         # aimed away
    d[-3:] = [[1, 0, 0], [0, -1, 0], [0, 0, 1]]                # zero direction components
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.1, he_hi, (n, 3))
    he[n // 2: n // 2 + 4, 0] = 0.0                            # zero-radius balls and plates
    rot = random_unit_quats(rng, n)
    rot[: n // 8] = [0, 0, 0, 1]
    md = np.full(n, np.inf)
    cut = rng.random(n) < 0.33
    md[cut] = dist[cut] * rng.uniform(0.5, 1.5, cut.sum())
    return shape, he, qpos, rot, d, md


def check(sq, s, q, ks, mask=None, excluded=(), skip=False):
    shape, he, qpos, rot, d, md = q
    kw = dict(max_distance=md, mask=mask, excluded=excluded)
    with np.errstate(all="ignore"):
        closest, many = CR.cast_queries(s, shape, he, qpos, rot, d, ks, **kw)
    got = sq.cast_shapes(shape, he, qpos, rot, d, skip_host_shapes=skip, **kw)
    same_records(got, closest, "cast_shapes")
    for k in ks:
        hits, cnt = sq.shape_hits(shape, he, qpos, rot, d, k, skip_host_shapes=skip, **kw)
        assert np.array_equal(cnt, many[k][1]), f"shape_hits k={k}: counts differ at {np.nonzero(cnt != many[k][1])[0][:8]}"
        same_records(hits.reshape(-1), many[k][0].reshape(-1), f"shape_hits k={k}")
    return got, (many[max(ks)][1] if ks else None)


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
    q = casts(rng, s, 130, he_hi=1.5)
    got, counts = check(sq, s, q, (1, 4, 64))
    hit = got["collider"] != MISS
    assert (~hit).sum() >= 3 and (hit & (got["distance"] == 0)).sum() >= 10 and (got["distance"] > 0).sum() >= 30 and counts.max() > 4
    assert (got["normal1"][hit & (got["distance"] == 0)] == 0).all() and (got["point1"][~hit] == 0).all()
    pairs = {(int(a), int(b)) for a, b in zip(q[0][hit], s.shape[got["collider"][hit]])}
    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}, f"pair kinds hit: {pairs}"
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), 130)
    excluded = rng.choice(cols["entity_index"], 12, replace=False)
    check(sq, s, q, (1, 4, 64), mask=mask, excluded=excluded)


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
    got, counts = check(sq, s, casts(rng, s, 70), (1, 2))
    assert counts.max() == n_colliders and (got["collider"] != MISS).sum() > 20


def test_far_scene_and_culling():
    rng = np.random.default_rng(21)
    bodies, cols, tf = SC.far_scene(7, n_bodies=24, spread=10.0, centre=(3000.0, -2000.0, 1000.0))
    w = world_of(32, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    q = casts(rng, s, 130, he_hi=2.0, reach=12.0)
    got, counts = check(sq, s, q, (8,))
    assert (got["collider"] != MISS).sum() > 60 and counts.max() >= 2
    sq.cast_shapes(*q[:5], max_distance=q[5])
    st = sq.stats()
    assert 0 < st.leaves_visited < 130 * s.n, f"{st.leaves_visited / 130:.0f} exact tests per cast of {s.n} colliders: the tree does not cull"


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
        shape, he, qpos, rot, d, md = (np.ascontiguousarray(a.astype(dt) if a.dtype == np.float64 else a) for a in casts(rng, s, n, 1.5))
        mask = rng.choice(np.array([1, 0xFFFFFFFF], np.uint32), n)
        excluded = cols["entity_index"][:5]
        dev = torch.device("cuda", 0)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        i32 = lambda a: T(a.view(np.int32))
        hd = sq.shape_hit_dtype
        ct = sq.cast_shapes(T(shape), T(he), T(qpos), T(rot), T(d), max_distance=T(md), mask=i32(mask), excluded=i32(excluded))
        assert ct.dtype == torch.uint8 and tuple(ct.shape) == (n, hd.itemsize)
        host = sq.cast_shapes(shape, he, qpos, rot, d, max_distance=md, mask=mask, excluded=excluded)
        same_records(ct.cpu().numpy().reshape(-1).view(hd), host, "device pointers: cast_shapes")
        assert (host["collider"] != MISS).sum() > 40
        ht, nt = sq.shape_hits(T(shape), T(he), T(qpos), T(rot), T(d), 4, max_distance=T(md), mask=i32(mask), excluded=i32(excluded))
        hh, nh = sq.shape_hits(shape, he, qpos, rot, d, 4, max_distance=md, mask=mask, excluded=excluded)
        same_records(ht.cpu().numpy().reshape(-1).view(hd), hh.reshape(-1), "device pointers: shape_hits")
        assert np.array_equal(nt.cpu().numpy().view(np.uint32), nh)


def test_status_codes():
    sc = scenes.box_stack(4, 4, 4)
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); cols = sc.collider_kwargs(); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    sq = SpatialQuery(w)
    p = np.array([[0.3, 20.0, 0.3]])
    shape, he, rot, d = np.array([1], np.uint8), np.array([[0.5, 0, 0]]), np.array([[0, 0, 0, 1.0]]), np.array([[0, -1.0, 0]])
    calls = (lambda: sq.cast_shapes(shape, he, p, rot, d), lambda: sq.shape_hits(shape, he, p, rot, d, 4))
    for call in calls:                       # before update()
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.update()
    assert calls[0]()["collider"][0] != MISS and calls[1]()[1][0] >= 4
    w.colliders_upload(**cols)               # the tables changed: update again
    for call in calls:
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.update()
    for k in (0, 65):
        with pytest.raises(F.AvnError) as e:
            sq.shape_hits(shape, he, p, rot, d, k)
        assert e.value.status == 1
    # null arrays and arguments
    import ctypes as C
    from avian_amd import spatial_query as Q
    cin = Q.avn_spatial_shape_casts(); cin.count = 1
    rec = np.zeros(4, sq.shape_hit_dtype); cnt = np.zeros(1, np.uint32)
    out = Q.avn_spatial_shape_hits_out(rec.ctypes.data_as(Q.vp), cnt.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_cast_shapes(w.handle, C.byref(cin), C.byref(out)) == 1
    assert sq.dll.avn_spatial_shape_hits(w.handle, C.byref(cin), 4, C.byref(out)) == 1
    assert sq.dll.avn_spatial_cast_shapes(w.handle, None, C.byref(out)) == 1
    assert sq.dll.avn_spatial_cast_shapes(w.handle, C.byref(cin), None) == 1


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
    q = casts(rng, s, 96, 1.0)
    for call in (lambda: sq.cast_shapes(*q[:5]), lambda: sq.shape_hits(*q[:5], 8)):
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    host = np.nonzero(s.shape == R.SHAPE_HOST)[0]
    got, counts = check(sq, s, q, (8,), skip=True)
    assert sq.stats().host_skipped == len(host) > 0 and not np.isin(got["collider"], host).any() and counts.sum() > 0


def test_non_finite_and_invalid_casts_leave_the_other_lanes_alone():
    rng = np.random.default_rng(31)
    bodies, cols, tf = compound_scene(seed=5, n_bodies=30)
    w = compound_world(hip_lib(), 32, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    n = 64
    shape, he, qpos, rot, d, md = casts(rng, s, n, 1.5)
    md[:] = np.inf
    d[:] = (np.stack(s.pos, 1).astype(float)[rng.integers(0, s.n, n)] - qpos)   # every cast aimed at a collider's centre
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shape = shape.copy()
    qpos[2, 0] = np.nan; rot[9, 3] = np.inf; he[12] = [np.nan, 0.5, 0.5]; shape[12] = R.SHAPE_CUBOID
    he[20, 1] = -0.25; shape[20] = R.SHAPE_CUBOID; he[21, 0] = -0.5; shape[21] = R.SHAPE_BALL; shape[33] = 2; he[34] = [0.5, np.inf, 0.5]; shape[34] = R.SHAPE_CUBOID
    d[40, 1] = np.nan; d[41, 0] = np.inf; md[42] = np.nan; qpos[43] = [3e38, 0, 0]; he[43] = [3e38, 1, 1]; shape[43] = R.SHAPE_CUBOID; rot[43] = [0, 0, 0, 1]   # a non-finite AABB
    he[35] = [0.5, np.nan, -1.0]; shape[35] = R.SHAPE_BALL    # a ball's y and z are not read: a valid query
    md[36] = -np.inf                                           # legal, and nothing is within it
    bad = [2, 9, 12, 20, 21, 33, 34, 40, 41, 42, 43]
    got, counts = check(sq, s, (shape, he, qpos, rot, d, md), (8,))
    assert (got["collider"][bad + [36]] == MISS).all() and (counts[bad + [36]] == 0).all()
    assert got[bad].tobytes() == got[bad[:1]].tobytes() * len(bad)   # misses, byte for byte
    assert (np.delete(got["collider"], bad + [36]) != MISS).all()
