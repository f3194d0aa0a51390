"""GPU: avn_spatial_shape_contacts and avn_spatial_depenetrate against the brute force of tests/spatial_contact_reference.py (filter, AABB
precondition, the CPU oracle's contact_manifolds, the last-maximum fold), tolerance 0: every byte of every record and every count."""
import numpy as np
import pytest

from avian_amd.spatial_query import MAX_HITS, MISS, SpatialQuery
from compound_helpers import compound_scene, compound_world
from helpers import F, hip_lib, random_unit_quats
import spatial_contact_reference as CR
import spatial_query_reference as R
import spatial_scenes as SC
from test_gpu_spatial_query import same_records, snapshot_of

pytestmark = pytest.mark.gpu

I = [0.0, 0.0, 0.0, 1.0]
CFG = dict(skin_width=0.05, max_depenetration_error=1e-4, penetration_rejection_threshold=0.5, iterations=16)


def world_of(bits, bodies, cols, tf=None):
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))
    w.bodies_upload(**bodies)
    w.colliders_upload(**cols)
    if tf is not None:
        w.collider_transforms_upload(**tf)
    return w


def mixed_scene(seed=4, n=40):
    """n balls and cuboids in a box of side 6, one collider per body, three layers, a few sensors."""
    rng = np.random.default_rng(seed)
    ball = rng.random(n) < 0.4
    he = rng.uniform(0.3, 0.8, (n, 3))
    he[ball, 1:] = 0
    cols = dict(entity_index=np.arange(200, 200 + n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=ball.astype(np.uint8), half_extents=he,
                memberships=(1 << rng.integers(0, 3, n)).astype(np.uint32), collider_flags=np.where(rng.random(n) < 0.2, F.COLLIDER_SENSOR, 0).astype(np.uint8))
    rot = random_unit_quats(rng, n)
    rot[: n // 5] = I
    return SC.bodies_of(rng.uniform(-3, 3, (n, 3)), rot), cols


def queries(rng, s, n, size=0.9, reach=0.8):
    """n query shapes of both kinds: a third overlapping colliders, a third near them, a third far away; predictions 0 .. reach, some exactly 0."""
    pos = np.stack(s.pos, 1).astype(float)
    near = pos[rng.integers(0, s.n, n)]
    scale = np.choose(np.arange(n) % 3, [0.3, 1.0, 0.0])[:, None]
    qpos = near + rng.normal(size=(n, 3)) * scale + np.where(scale == 0, 25.0, 0.0)
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.1, size, (n, 3))
    rot = random_unit_quats(rng, n)
    rot[: n // 8] = I
    pred = rng.uniform(0, reach, n)
    pred[rng.random(n) < 0.15] = 0.0
    return shape, he, qpos, rot, pred


def check(sq, s, q, caps=(MAX_HITS,), sensor=None, depenetrate=True, **kw):
    """shape_contacts at every cap and depenetrate against the brute force; returns the true counts."""
    shape, he, qpos, rot, pred = q
    dev_kw = dict(mask=kw.get("mask"), excluded=kw.get("excluded"), skip_sensors=kw.get("skip_sensors", False), skip_host_shapes=kw.get("skip_host_shapes", False))
    with np.errstate(all="ignore"):
        lists = CR.contact_lists(s, shape, he, qpos, rot, pred, mask=kw.get("mask"), excluded=kw.get("excluded", ()), sensor=sensor, skip_sensors=kw.get("skip_sensors", False))
    bits = sq.bits
    for cap in caps:
        rec, cnt = sq.shape_contacts(shape, he, qpos, rot, pred, cap, **dev_kw)
        ref, rcnt = CR.pad(lists, cap, bits)
        assert np.array_equal(cnt, rcnt), f"cap={cap}: counts differ first at query {np.nonzero(cnt != rcnt)[0][:1]}: device {cnt[cnt != rcnt][:1]} reference {rcnt[cnt != rcnt][:1]}"
        same_records(rec, ref, f"shape_contacts cap={cap}")
    if depenetrate:
        same_depenetration(sq, shape, he, qpos, rot, CFG, dev_kw)
    return np.array([len(l) for l in lists])


def same_depenetration(sq, shape, he, qpos, rot, cfg, dev_kw):
    """depenetrate == the numpy restatement over the device's own contact records at prediction skin_width."""
    rec, cnt = sq.shape_contacts(shape, he, qpos, rot, cfg["skin_width"], MAX_HITS, **dev_kw)
    got = sq.depenetrate(shape, he, qpos, rot, **cfg, **dev_kw)
    want = CR.depenetrations(rec, cnt, cfg["skin_width"], cfg["max_depenetration_error"], cfg["penetration_rejection_threshold"], cfg["iterations"], sq.bits)
    same_records(got, want, "depenetrate")
    return got


@pytest.mark.parametrize("n_colliders", [1, 2])
def test_smallest_trees(n_colliders):
    rng = np.random.default_rng(n_colliders)
    pos = [[0.5, 1.0, -0.25], [1.5, 1.25, 0.5]][:n_colliders]
    cols = dict(entity_index=np.arange(40, 40 + n_colliders, dtype=np.uint32), body=np.arange(n_colliders, dtype=np.int32),
                shape=np.array([R.SHAPE_CUBOID, R.SHAPE_BALL][:n_colliders], np.uint8), half_extents=np.array([[0.5, 0.75, 1.0], [0.75, 0, 0]][:n_colliders], float))
    for bits in (32, 64):
        w = world_of(bits, SC.bodies_of(pos, random_unit_quats(np.random.default_rng(3), n_colliders)), cols)
        sq = SpatialQuery(w)
        sq.update()
        s = snapshot_of(w, cols)
        counts = check(sq, s, queries(rng, s, 70), (0, 1, 2))
        assert counts.max() == n_colliders and (counts == 0).any()


@pytest.mark.parametrize("bits", [32, 64])
def test_mixed_scene_against_brute_force(bits):
    rng = np.random.default_rng(bits)
    bodies, cols = mixed_scene()
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    assert s.n == 40 and (s.shape == R.SHAPE_BALL).any() and (s.shape == R.SHAPE_CUBOID).any()
    q = queries(rng, s, 100)                       # two blocks, the second a partial wave
    counts = check(sq, s, q, (0, 1, 3, MAX_HITS))    # the truncated records are a prefix of the full list, the count unchanged
    assert counts.max() > 3 and (counts == 0).sum() >= 30 and (counts > 0).sum() >= 30
    # filters: layer masks, excluded entities, sensors in reach with the flag off and on
    mask = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF], np.uint32), 100)
    excluded = rng.choice(cols["entity_index"], 8, replace=False)
    filtered = check(sq, s, q, (3, MAX_HITS), mask=mask, excluded=excluded)
    assert 0 < filtered.sum() < counts.sum()
    sensor = cols["collider_flags"] & F.COLLIDER_SENSOR
    assert sensor.any()
    kept = check(sq, s, q, (MAX_HITS,), sensor=sensor, skip_sensors=False)
    skipped = check(sq, s, q, (MAX_HITS,), sensor=sensor, skip_sensors=True)
    assert np.array_equal(kept, counts) and 0 < skipped.sum() < counts.sum()
    rec, _ = sq.shape_contacts(*q, MAX_HITS, skip_sensors=True)
    assert not np.isin(rec["collider"], np.nonzero(sensor)[0]).any()


@pytest.mark.parametrize("bits", [32, 64])
def test_compound_scene_child_colliders(bits):
    rng = np.random.default_rng(5 + bits)
    bodies, cols, tf = compound_scene(seed=3, n_bodies=24)
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    assert s.n > 40 and tf["is_child"].any()
    counts = check(sq, s, queries(rng, s, 100, size=0.6, reach=0.4), (4, MAX_HITS))
    assert counts.max() >= 3 and counts.max() <= MAX_HITS


def test_far_scene():
    rng = np.random.default_rng(21)
    bodies, cols, tf = SC.far_scene(7, n_bodies=24, spread=10.0, centre=(3000.0, -2000.0, 1000.0))
    for bits in (32, 64):
        w = world_of(bits, bodies, cols, tf)
        sq = SpatialQuery(w)
        sq.update()
        s = snapshot_of(w, cols, tf)
        counts = check(sq, s, queries(rng, s, 100, size=2.0, reach=2.0), (8,))
        assert counts.max() >= 2


@pytest.mark.parametrize("bits", [32, 64])
def test_depenetrate_truncation_flag(bits):
    """70 small balls overlapping one query ball: more contacts than AVN_SPATIAL_MAX_HITS."""
    rng = np.random.default_rng(70)
    n = 70
    d = rng.normal(size=(n, 3))
    pos = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2, 0.9, (n, 1))
    cols = dict(entity_index=np.arange(n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=np.full(n, R.SHAPE_BALL, np.uint8),
                half_extents=np.c_[np.full(n, 0.125), np.zeros((n, 2))])
    w = world_of(bits, SC.bodies_of(pos, np.tile(I, (n, 1))), cols)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    q = (np.array([R.SHAPE_BALL, R.SHAPE_BALL], np.uint8), np.array([[1.0, 0, 0], [0.25, 0, 0]]), np.array([[0.0, 0, 0], [0, 5.0, 0]]), np.tile(I, (2, 1)), np.array([0.05, 0.05]))
    counts = check(sq, s, q, (0, 3, MAX_HITS), depenetrate=False)
    assert list(counts) == [n, 0]
    cfg = dict(CFG, penetration_rejection_threshold=10.0)
    got = same_depenetration(sq, *q[:4], cfg, {})
    assert list(got["count"]) == [n, 0] and list(got["truncated"]) == [1, 0] and got["iterations_run"][0] >= 1 and np.abs(got["fixup"][0]).max() > 0
    assert (got["fixup"][1] == 0).all() and got["iterations_run"][1] == 1     # no contact: one pass with no error


def test_device_pointers_equal_host_pointers():
    import torch
    rng = np.random.default_rng(11)
    bodies, cols = mixed_scene()
    for bits, dt in ((32, np.float32), (64, np.float64)):
        w = world_of(bits, bodies, cols)
        sq = SpatialQuery(w)
        sq.update()
        s = snapshot_of(w, cols)
        n = 100
        shape, he, qpos, rot, pred = (np.ascontiguousarray(a.astype(dt) if a.dtype == np.float64 else a) for a in queries(rng, s, n))
        mask = rng.choice(np.array([1, 0xFFFFFFFF], np.uint32), n)
        excluded = cols["entity_index"][:5]
        dev = torch.device("cuda", 0)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        i32 = lambda a: T(a.view(np.int32))
        for cap in (0, 4):
            rt, ct = sq.shape_contacts(T(shape), T(he), T(qpos), T(rot), T(pred), cap, mask=i32(mask), excluded=i32(excluded), skip_sensors=True)
            rh, ch = sq.shape_contacts(shape, he, qpos, rot, pred, cap, mask=mask, excluded=excluded, skip_sensors=True)
            assert rt.dtype == torch.uint8 and tuple(rt.shape) == (n, cap, sq.shape_contact_dtype.itemsize)
            same_records(rt.cpu().numpy().reshape(-1).view(sq.shape_contact_dtype).reshape(n, cap), rh, "device pointers: shape_contacts")
            assert np.array_equal(ct.cpu().numpy().view(np.uint32), ch)
        assert ch.sum() > 20
        dt_ = sq.depenetrate(T(shape), T(he), T(qpos), T(rot), **CFG, mask=i32(mask), excluded=i32(excluded))
        dh = sq.depenetrate(shape, he, qpos, rot, **CFG, mask=mask, excluded=excluded)
        same_records(dt_.cpu().numpy().reshape(-1).view(sq.depenetration_dtype), dh, "device pointers: depenetrate")
        assert np.abs(dh["fixup"]).max() > 0


def test_invalid_queries_leave_the_other_lanes_alone():
    rng = np.random.default_rng(31)
    bodies, cols = mixed_scene()
    w = world_of(32, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    n = 64
    shape, he, qpos, rot, pred = queries(rng, s, n)
    qpos[:] = np.stack(s.pos, 1)[rng.integers(0, s.n, n)] + rng.normal(scale=0.3, size=(n, 3))   # most valid queries have contacts
    shape = shape.copy()
    qpos[2, 0] = np.nan; rot[9, 3] = np.inf; he[12] = [np.nan, 0.5, 0.5]; shape[12] = R.SHAPE_CUBOID
    he[20, 1] = -0.25; shape[20] = R.SHAPE_CUBOID; he[21, 0] = -0.5; shape[21] = R.SHAPE_BALL; shape[33] = 2
    pred[40] = np.nan; pred[41] = np.inf; pred[42] = -0.125; pred[43] = -np.inf
    he[35] = [0.5, np.nan, -1.0]; shape[35] = R.SHAPE_BALL    # a ball's y and z are not read: a valid query
    pred[36] = 0.0
    bad = [2, 9, 12, 20, 21, 33, 40, 41, 42, 43]
    with np.errstate(all="ignore"):
        counts = check(sq, s, (shape, he, qpos, rot, pred), (0, 8))
        rec, cnt = sq.shape_contacts(shape, he, qpos, rot, pred, 8)
        dep = sq.depenetrate(shape, he, qpos, rot, **CFG)
    assert (cnt[bad] == 0).all() and (rec["collider"][bad] == MISS).all() and np.delete(cnt, bad).sum() > 40 and np.array_equal(cnt, counts)
    assert (dep["count"][[2, 9, 12, 20, 21, 33]] == 0).all() and (dep["fixup"][[2, 9, 12, 20, 21, 33]] == 0).all()


def test_status_codes():
    import ctypes as C
    from avian_amd import spatial_query as Q
    bodies, cols = mixed_scene()
    w = world_of(32, bodies, cols)
    sq = SpatialQuery(w)
    shape, he, p, rot = np.array([1], np.uint8), np.array([[0.5, 0, 0]]), np.array([[0.3, 0.2, 0.3]]), np.array([I])
    calls = (lambda: sq.shape_contacts(shape, he, p, rot, 0.1, 4), lambda: sq.depenetrate(shape, he, p, rot, **CFG))
    for call in calls:                       # before update()
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.update()
    for call in calls:
        call()
    w.colliders_upload(**cols)               # the tables changed: a stale snapshot
    for call in calls:
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.update()
    with pytest.raises(F.AvnError) as e:     # cap above AVN_SPATIAL_MAX_HITS
        sq.shape_contacts(shape, he, p, rot, 0.1, MAX_HITS + 1)
    assert e.value.status == 1
    sq.shape_contacts(shape, he, p, rot, 0.1, MAX_HITS)
    # null arguments and null arrays
    qin = Q.avn_spatial_shape_contact_queries(); qin.count = 1
    cnt = np.zeros(1, np.uint32)
    rec = np.zeros(4, sq.shape_contact_dtype)
    out = Q.avn_spatial_shape_contacts_out(rec.ctypes.data_as(Q.vp), cnt.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_shape_contacts(w.handle, C.byref(qin), 4, C.byref(out)) == 1
    assert sq.dll.avn_spatial_shape_contacts(w.handle, None, 4, C.byref(out)) == 1
    assert sq.dll.avn_spatial_shape_contacts(w.handle, C.byref(qin), 4, None) == 1
    s8, h, r, pd = shape.ctypes.data_as(Q.vp), np.zeros((1, 3), np.float32), np.array([I], np.float32), np.zeros(1, np.float32)
    qin.shape, qin.half_extents, qin.position, qin.rotation = s8, h.ctypes.data_as(Q.vp), h.ctypes.data_as(Q.vp), r.ctypes.data_as(Q.vp)
    assert sq.dll.avn_spatial_shape_contacts(w.handle, C.byref(qin), 4, C.byref(out)) == 1          # no prediction array
    qin.prediction_distance = pd.ctypes.data_as(Q.vp)
    nout = Q.avn_spatial_shape_contacts_out(None, cnt.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_shape_contacts(w.handle, C.byref(qin), 4, C.byref(nout)) == 1         # a cap without a record array
    assert sq.dll.avn_spatial_shape_contacts(w.handle, C.byref(qin), 0, C.byref(nout)) == 0
    assert sq.dll.avn_spatial_shape_contacts(w.handle, C.byref(qin), 4, C.byref(out)) == 0
    sin = Q.avn_spatial_shapes(); sin.count = 1
    cfg = Q.avn_spatial_depenetration_config(0.05, 1e-4, 0.5, 4)
    drec = np.zeros(1, sq.depenetration_dtype)
    dout = Q.avn_spatial_depenetrations_out(drec.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_depenetrate(w.handle, C.byref(sin), C.byref(cfg), C.byref(dout)) == 1
    assert sq.dll.avn_spatial_depenetrate(w.handle, C.byref(sin), None, C.byref(dout)) == 1
    sin.shape, sin.half_extents, sin.position, sin.rotation = s8, h.ctypes.data_as(Q.vp), h.ctypes.data_as(Q.vp), r.ctypes.data_as(Q.vp)
    assert sq.dll.avn_spatial_depenetrate(w.handle, C.byref(sin), C.byref(cfg), C.byref(Q.avn_spatial_depenetrations_out(None))) == 1
    assert sq.dll.avn_spatial_depenetrate(w.handle, C.byref(sin), C.byref(cfg), C.byref(dout)) == 0


def test_host_shapes_need_the_skip_flag():
    from host_shape_helpers import capsule_world, capsule_scene
    w, _, _ = capsule_world(hip_lib(), 32)
    w.synchronize()
    _, cols, _, _ = capsule_scene()
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    rng = np.random.default_rng(9)
    q = queries(rng, s, 64)
    for call in (lambda: sq.shape_contacts(*q, 8), lambda: sq.depenetrate(*q[:4], **CFG)):
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    host = np.nonzero(s.shape == R.SHAPE_HOST)[0]
    counts = check(sq, s, q, (8,), skip_host_shapes=True)
    rec, _ = sq.shape_contacts(*q, 8, skip_host_shapes=True)
    assert sq.stats().host_skipped == len(host) > 0 and not np.isin(rec["collider"], host).any() and counts.sum() > 0


@pytest.mark.parametrize("bits", [32, 64])
def test_depenetrate_known_scenes(bits):
    """iterations = 0 answers zero records; a ball pressed into a floor ends up skin_width above it."""
    cols = dict(entity_index=np.array([7], np.uint32), body=np.zeros(1, np.int32), shape=np.array([R.SHAPE_CUBOID], np.uint8), half_extents=np.array([[5.0, 0.5, 5.0]]))
    w = world_of(bits, SC.bodies_of([[0, -0.5, 0]], [I]), cols)
    sq = SpatialQuery(w)
    sq.update()
    shape, he, pos, rot = np.array([R.SHAPE_BALL], np.uint8), np.array([[0.5, 0, 0]]), np.array([[0.25, 0.3, -0.5]]), np.array([I])
    zero = sq.depenetrate(shape, he, pos, rot, **dict(CFG, iterations=0))
    assert zero.tobytes() == bytes(zero.nbytes) and sq.stats().nodes_visited == 0
    skin, max_error = 0.01, 1e-4
    got = sq.depenetrate(shape, he, pos, rot, skin_width=skin, max_depenetration_error=max_error, penetration_rejection_threshold=1.0, iterations=8)
    assert got["count"][0] == 1 and got["truncated"][0] == 0 and got["iterations_run"][0] == 2
    assert got["fixup"][0][0] == 0 and got["fixup"][0][2] == 0 and abs(got["fixup"][0][1] - 0.21) < 1e-6
    rec, cnt = sq.shape_contacts(shape, he, pos + got["fixup"].astype(float), rot, 0.1, 1)
    assert cnt[0] == 1 and rec["penetration"][0, 0] <= -skin + max_error
