"""GPU: the device spatial queries (include/avian_mi355x_spatial.h) against a brute-force pass of the numpy restatement
(tests/spatial_query_reference.py) over every collider, tolerance 0: collider index, entity, distance and normal bit for bit."""
import numpy as np
import pytest

from avian_amd import scenes
from avian_amd.spatial_query import SpatialQuery, MISS
from compound_helpers import compound_scene, compound_world
from helpers import F, hip_lib
import spatial_query_reference as R

pytestmark = pytest.mark.gpu


def same_records(dev, ref, what):
    assert dev.dtype == ref.dtype and dev.shape == ref.shape, what
    if not np.array_equal(dev.view(np.uint8), ref.view(np.uint8)):
        bad = np.nonzero((dev.view(np.uint8).reshape(dev.shape + (-1,)) != ref.view(np.uint8).reshape(ref.shape + (-1,))).any(axis=-1))
        i = tuple(x[0] for x in bad)
        raise AssertionError(f"{what}: {len(bad[0])} records differ, first at {i}: device {dev[i]} reference {ref[i]}")


def same_ids(dev, ref, what):
    for a, b, k in zip(dev, ref, ("ids", "counts")):
        if not np.array_equal(a, b):
            i = np.nonzero(a != b)[0][0]
            raise AssertionError(f"{what}: {k} differ first at query {i}: device {a[i]} reference {b[i]}")


def snapshot_of(w, cols, tf=None):
    return R.Snapshot(w.bodies_download(), cols, tf, w.dtype)


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def mixed_rays(rng, s, n):
    """Random rays plus crafted ones: origins inside shapes (both solid values), axis-parallel rays (zero direction components), grazing rays
    along the ground slab's top face and onto its corner, max_distance cut-offs."""
    pos = np.stack(s.pos, 1).astype(float)
    lo, hi = pos.min(0) - 3, pos.max(0) + 3
    o = rng.uniform(lo, hi, (n, 3))
    d = unit(rng.normal(size=(n, 3)))
    md = np.where(rng.random(n) < 0.3, rng.uniform(0.5, 6, n), np.inf)
    solid = (rng.random(n) < 0.5).astype(np.uint8)
    k = n // 4
    o[:k] = pos[rng.integers(0, len(pos), k)]                      # inside a collider
    ax = rng.integers(0, 3, k)
    d[k:2 * k] = 0; d[np.arange(k, 2 * k), ax] = rng.choice([-1.0, 1.0], k)   # axis-parallel
    g = 8
    o[2 * k:2 * k + g] = np.c_[np.full(g, -40.0), np.zeros(g), rng.uniform(-5, 5, g)]; d[2 * k:2 * k + g] = [1, 0, 0]   # grazing the slab's top face y = 0
    o[2 * k + g:2 * k + 2 * g] = [-40, 0, -40]; d[2 * k + g:2 * k + 2 * g] = unit(np.array([[1.0, 0, 1.0]]))[0]        # onto the slab's top corner edge
    return o, d, md, solid


def check_all(w, sq, s, rng, n_rays, n_pts, ks, mask=None, excluded=(), skip=False):
    o, d, md, solid = mixed_rays(rng, s, n_rays)
    kw = dict(mask=mask, excluded=excluded)
    closest, many = R.ray_queries(s, o, d, ks, md, solid, **kw)
    same_records(sq.cast_rays(o, d, md, solid, skip_host_shapes=skip, **kw), closest, "cast_rays")
    for k in ks:
        h, c = sq.ray_hits(o, d, k, md, solid, skip_host_shapes=skip, **kw)
        same_records(h, many[k][0], f"ray_hits k={k}")
        assert np.array_equal(c, many[k][1]), f"ray_hits k={k}: counts"
    pos = np.stack(s.pos, 1).astype(float)
    pts = np.concatenate([pos[rng.integers(0, len(pos), n_pts // 2)] + rng.normal(scale=0.3, size=(n_pts // 2, 3)),
                          rng.uniform(pos.min(0) - 1, pos.max(0) + 1, (n_pts - n_pts // 2, 3))])
    pmask = None if mask is None else mask[:n_pts]
    same_ids(sq.point_intersections(pts, 8, mask=pmask, excluded=excluded, skip_host_shapes=skip), R.point_intersections(s, pts, 8, mask=pmask, excluded=excluded), "points")
    c = rng.uniform(pos.min(0) - 1, pos.max(0) + 1, (n_pts, 3)); ext = rng.uniform(0, 2, (n_pts, 3))
    same_ids(sq.aabb_intersections(c - ext, c + ext, 16, mask=pmask, excluded=excluded, skip_host_shapes=skip),
             R.aabb_intersections(s, c - ext, c + ext, 16, mask=pmask, excluded=excluded), "aabbs")
    return o, d, md, solid


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
    check_all(w, sq, s, rng, 512, 256, (1, 4, 64))
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), 512)
    excluded = rng.choice(cols["entity_index"], 12, replace=False)
    check_all(w, sq, s, rng, 512, 256, (1, 4, 64), mask=mask, excluded=excluded)
    st = sq.stats()
    assert st.valid == 1 and st.colliders == s.n and st.nodes == 2 * s.n - 1 and st.host_skipped == 0
    with pytest.raises(F.AvnError) as e:
        sq.ray_hits(np.zeros((1, 3)), np.array([[0, 0, 1.0]]), 65)
    assert e.value.status == 1


def test_cfg2_after_closed_loop_steps():
    sc = scenes.box_stack(50, 40, 50)
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); cols = sc.collider_kwargs(); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    w.pipeline_enable()
    for _ in range(20):
        w.step()
    w.synchronize()
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    C = s.n
    assert C > 100_000
    rng = np.random.default_rng(2)
    pos = np.stack(s.pos, 1).astype(float)
    n = 1024
    o = pos[rng.integers(1, C, n)] + rng.normal(scale=0.7, size=(n, 3))
    d = unit(rng.normal(size=(n, 3)))
    md = rng.uniform(0.2, 2.0, n)     # sensor-like short rays
    solid = (rng.random(n) < 0.5).astype(np.uint8)
    closest, many = R.ray_queries(s, o, d, (4,), md, solid, chunk=8)
    same_records(sq.cast_rays(o, d, md, solid), closest, "cfg2 cast_rays")
    st = sq.stats()
    assert st.leaves_visited / n < 0.01 * C, f"{st.leaves_visited / n:.0f} exact tests per short ray: the tree does not cull"
    h, c = sq.ray_hits(o, d, 4, md, solid)
    same_records(h, many[4][0], "cfg2 ray_hits k=4"); assert np.array_equal(c, many[4][1])
    pts = pos[rng.integers(1, C, n)] + rng.normal(scale=0.5, size=(n, 3))
    same_ids(sq.point_intersections(pts, 8), R.point_intersections(s, pts, 8), "cfg2 points")
    ext = rng.uniform(0, 1.5, (n, 3))
    same_ids(sq.aabb_intersections(pts - ext, pts + ext, 32), R.aabb_intersections(s, pts - ext, pts + ext, 32), "cfg2 aabbs")
    assert (closest["collider"] != MISS).sum() > n // 4


def test_snapshot_rules():
    sc = scenes.box_stack(4, 4, 4)
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); cols = sc.collider_kwargs(); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    sq = SpatialQuery(w)
    o, d = np.array([[0.3, 20.0, 0.3]]), np.array([[0, -1.0, 0]])
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d)
    assert e.value.status == 6
    sq.update()
    sq.cast_rays(o, d)
    w.colliders_upload(**cols)
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d)
    assert e.value.status == 6
    assert sq.stats().valid == 0
    # steps without an update: the queries keep answering against the snapshot's poses
    sc2 = scenes.falling_grid(4)
    w2 = F.World(hip_lib(), F.default_config(32, substeps=4))
    w2.bodies_upload(**sc2.body_kwargs()); cols2 = sc2.collider_kwargs(); w2.colliders_upload(**cols2)
    w2.existing_pairs_upload(np.zeros(0, np.uint64)); w2.collider_materials_upload(friction=0.5)
    w2.pipeline_enable()
    sq2 = SpatialQuery(w2)
    sq2.update()
    s_then = snapshot_of(w2, cols2)
    for _ in range(10):
        w2.step()
    w2.synchronize()
    s_now = snapshot_of(w2, cols2)
    assert not np.array_equal(s_then.pos[1], s_now.pos[1]), "the bodies must have moved"
    rng = np.random.default_rng(5)
    pos = np.stack(s_then.pos, 1)
    o = pos[rng.integers(1, s_then.n, 256)] + rng.normal(scale=0.2, size=(256, 3)) + [0, 3, 0]
    d = np.tile([0, -1.0, 0], (256, 1))
    got = sq2.cast_rays(o, d)
    same_records(got, R.cast_rays(s_then, o, d), "after steps: the snapshot's poses")
    sq2.update()
    same_records(sq2.cast_rays(o, d), R.cast_rays(s_now, o, d), "after a new update: the current poses")


def test_host_shapes_need_the_skip_flag():
    from host_shape_helpers import capsule_world, capsule_scene
    w, _, _ = capsule_world(hip_lib(), 32)
    for _ in range(3):
        w.step()
    w.synchronize()
    _, cols, _, _ = capsule_scene()
    sq = SpatialQuery(w)
    sq.update()
    rng = np.random.default_rng(9)
    o = rng.uniform([-1, -1, -1], [8, 5, 8], (128, 3)); d = unit(rng.normal(size=(128, 3)))
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d)
    assert e.value.status == 6
    s = snapshot_of(w, cols)
    closest, many = R.ray_queries(s, o, d, (8,))
    got = sq.cast_rays(o, d, skip_host_shapes=True)
    same_records(got, closest, "host shapes skipped: cast_rays")
    h, c = sq.ray_hits(o, d, 8, skip_host_shapes=True)
    same_records(h, many[8][0], "host shapes skipped: ray_hits")
    host = np.nonzero(s.shape == R.SHAPE_HOST)[0]
    assert not np.isin(got["collider"], host).any() and not np.isin(h["collider"], host).any()
    ids, cnt = sq.point_intersections(o, 4, skip_host_shapes=True)
    same_ids((ids, cnt), R.point_intersections(s, o, 4), "host shapes skipped: points")
    assert sq.stats().host_skipped == len(host) == 24


def test_queries_between_steps_change_nothing():
    sc = scenes.box_stack(10, 10, 10)
    worlds = []
    for _ in range(2):
        w = F.World(hip_lib(), F.default_config(32, substeps=4))
        w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**sc.collider_kwargs())
        w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
        w.pipeline_enable()
        worlds.append(w)
    plain, queried = worlds
    sq = SpatialQuery(queried)
    rng = np.random.default_rng(4)
    o = rng.uniform([-1, 0, -1], [11, 11, 11], (256, 3)); d = unit(rng.normal(size=(256, 3)))
    from test_gpu_graph import compare_step
    for s in range(30):
        plain.step(); queried.step()
        sq.update()
        sq.cast_rays(o, d); sq.ray_hits(o, d, 4); sq.point_intersections(o, 4); sq.aabb_intersections(o - 0.5, o + 0.5, 4)
        compare_step(s, plain, queried, check_rows=(s % 10 == 9))


def test_device_pointers_equal_host_pointers():
    import torch
    rng = np.random.default_rng(11)
    bodies, cols, tf = compound_scene(seed=5, n_bodies=30)
    w = compound_world(hip_lib(), 32, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    n = 300
    pos = np.array([bodies["position"][b] for b in cols["body"]])
    o = rng.uniform(pos.min(0) - 2, pos.max(0) + 2, (n, 3)).astype(np.float32); d = unit(rng.normal(size=(n, 3))).astype(np.float32)
    md = np.where(rng.random(n) < 0.5, 4.0, np.inf).astype(np.float32); solid = (rng.random(n) < 0.5).astype(np.uint8)
    excluded = cols["entity_index"][:5]
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    recs = lambda t, shape: t.cpu().numpy().reshape(-1).view(sq.hit_dtype).reshape(shape)
    same_records(recs(sq.cast_rays(T(o), T(d), T(md), T(solid), excluded=T(excluded.astype(np.int32))), (n,)),
                 sq.cast_rays(o, d, md, solid, excluded=excluded), "device pointers: cast_rays")
    ht, ct = sq.ray_hits(T(o), T(d), 4, T(md), T(solid))
    hh, ch = sq.ray_hits(o, d, 4, md, solid)
    same_records(recs(ht, (n, 4)), hh, "device pointers: ray_hits")
    assert np.array_equal(ct.cpu().numpy().view(np.uint32), ch)
    it, ct = sq.point_intersections(T(o), 4)
    ih, ch = sq.point_intersections(o, 4)
    assert np.array_equal(it.cpu().numpy().view(np.uint32), ih) and np.array_equal(ct.cpu().numpy().view(np.uint32), ch)
    it, ct = sq.aabb_intersections(T(o - 1), T(o + 1), 8)
    ih, ch = sq.aabb_intersections(o - 1, o + 1, 8)
    assert np.array_equal(it.cpu().numpy().view(np.uint32), ih) and np.array_equal(ct.cpu().numpy().view(np.uint32), ch)
