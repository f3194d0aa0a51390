"""GPU: avn_spatial_project_velocities, avn_spatial_cast_moves and avn_spatial_move_and_slide against the numpy restatement of
tests/spatial_move_reference.py, tolerance 0: every byte of every record, f32 and f64.  The scenes, seeds and the populations that keep the
comparison from being empty are those of tests/test_spatial_moves_cpu.py, asserted again here on the reference's side."""
import numpy as np
import pytest

from avian_amd.spatial_query import MAX_HITS, MAX_PLANES, MAX_SLIDE_ITERATIONS, MISS, SpatialQuery
from compound_helpers import compound_scene, compound_world
from helpers import F, hip_lib, random_unit_quats
import spatial_move_reference as M
import spatial_move_scenes as MS
import spatial_query_reference as R
import spatial_scenes as SC
from test_gpu_spatial_contacts import world_of
from test_gpu_spatial_query import same_records, snapshot_of
from test_spatial_moves_cpu import MOVE_SEED, NORMALS, SLIDE_SEED, slide_populations

pytestmark = pytest.mark.gpu

I = MS.I
DT = {32: np.float32, 64: np.float64}
CAPACITY = 4      # AVN_ERR_CAPACITY


def room_world(bits, centre=(0.0, 0.0, 0.0)):
    bodies, cols, sensor = MS.room(centre)
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    return w, sq, snapshot_of(w, cols), cols, sensor


def check_moves(sq, s, q, sensor=None, **kw):
    """cast_moves == the restatement; returns (records, the reference's overlap counters)."""
    shape, he, pos, rot, mv, skin, own = q
    info = {}
    with np.errstate(all="ignore"):
        want = M.cast_moves(s, shape, he, pos, rot, mv, skin, own, mask=kw.get("mask"), excluded=kw.get("excluded", ()), sensor=sensor, info=info)
    got = sq.cast_moves(shape, he, pos, rot, mv, skin, self_entity=own, mask=kw.get("mask"), excluded=kw.get("excluded"), skip_host_shapes=kw.get("skip_host_shapes", False))
    same_records(got, want, "cast_moves")
    return got, info


def check_slide(sq, s, chars, cfg, hit_cap, sensor=None, **kw):
    """move_and_slide == the restatement, slide records and hit log; returns (slides, hits, the reference's info)."""
    shape, he, pos, rot, vel, own = chars
    info = {}
    with np.errstate(all="ignore"):
        want, want_hits = M.move_and_slide(s, shape, he, pos, rot, vel, **cfg, hit_cap=hit_cap, self_entity=own, mask=kw.get("mask"), excluded=kw.get("excluded", ()),
                                           sensor=sensor, info=info)
    got, hits = sq.move_and_slide(shape, he, pos, rot, vel, **cfg, hit_cap=hit_cap, self_entity=own, mask=kw.get("mask"), excluded=kw.get("excluded"))
    same_records(got, want, f"move_and_slide {cfg} hit_cap={hit_cap}: slides")
    same_records(hits, want_hits, f"move_and_slide {cfg} hit_cap={hit_cap}: hit log")
    return got, hits, info


# ---- project_velocities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_project_velocities(bits):
    dt = DT[bits]
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))          # no bodies, no snapshot: the call needs neither
    sq = SpatialQuery(w)
    rng = np.random.default_rng(bits)
    n, stride = 100, 9                                                   # two blocks, the second a partial wave
    nrm = rng.normal(size=(n, stride, 3))
    nrm[:, :, 1] = np.abs(nrm[:, :, 1])                                  # planes that face up, so that cones of several planes are common
    nrm[::7, 0] = [0, 1, 0]; nrm[::7, 1] = [-1, 0, 0]; nrm[::7, 2] = [0, 0, -1]      # axis planes: exact zeros, ties and -0.0
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    cnt = rng.integers(0, stride + 1, n).astype(np.uint32)
    cnt[::7] = np.arange(len(cnt[::7])) % 4
    cnt[3] = stride + 5                                                  # above the stride: read as the stride
    vel = rng.normal(size=(n, 3)) * 3
    vel[::7] = np.array([[1, -1, 1], [0, -1, 0], [1, -1, 0], [-0.0, -2, 0.0]])[np.arange(len(vel[::7])) % 4]
    vel[10] = [np.nan, 1, 0]; vel[11] = [1, -np.inf, 0]; nrm[12, 0, 2] = np.nan; cnt[12] = 3; nrm[13, 5, 0] = np.inf; cnt[13] = 5     # 13: beyond its count
    with np.errstate(all="ignore"):
        want = M.project_velocities(vel, nrm, cnt, dt)
        got = sq.project_velocities(vel, nrm, cnt)
    assert got.dtype == dt and got.tobytes() == want.tobytes(), f"first at {np.nonzero((got.view(np.uint8) != want.view(np.uint8)).reshape(n, -1).any(1))[0][:4]}"
    v = vel.astype(dt)
    changed = (got != v).any(1)
    assert changed.sum() >= 40 and (~changed).sum() >= 15 and ((got == 0).all(1) & np.signbit(got).all(1)).sum() >= 1
    assert np.array_equal(got[[10, 11, 12]], v[[10, 11, 12]], equal_nan=True)
    # the reference's own 17 normals, all of them at once (stride 17)
    vs = rng.normal(size=(64, 3))
    nn = np.tile(np.array(NORMALS, np.float32)[None], (64, 1, 1))
    got = sq.project_velocities(vs, nn)
    want = M.project_velocities(vs, nn, np.full(64, 17), dt)
    assert got.tobytes() == want.tobytes() and (-(got @ np.array(NORMALS, dt).T) <= M.DOT_EPSILON).all()
    # limits and null arrays
    with pytest.raises(F.AvnError) as e:
        sq.project_velocities(vs, np.zeros((64, MAX_PLANES + 1, 3), np.float32))
    assert e.value.status == 1
    assert sq.project_velocities(vs, np.zeros((64, 0, 3), np.float32)).tobytes() == vs.astype(dt).tobytes()      # no planes: unchanged


# ---- cast_moves ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colliders", [1, 2])
def test_smallest_trees(n_colliders):
    pos = [[0.0, -0.5, 0.0], [1.5, 1.0, 0.5]][:n_colliders]
    cols = dict(entity_index=np.arange(40, 40 + n_colliders, dtype=np.uint32), body=np.arange(n_colliders, dtype=np.int32),
                shape=np.array([R.SHAPE_CUBOID, R.SHAPE_BALL][:n_colliders], np.uint8), half_extents=np.array([[3, 0.5, 3], [0.75, 0, 0]][:n_colliders], float))
    rng = np.random.default_rng(n_colliders)
    n = 70
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.2, 0.5, (n, 3))
    qpos = np.c_[rng.uniform(-2, 2, n), rng.uniform(-0.2, 2.0, n), rng.uniform(-2, 2, n)]
    rot = random_unit_quats(rng, n)
    vel = rng.normal(size=(n, 3)) * 4
    own = np.where(rng.random(n) < 0.2, 40, MISS).astype(np.uint32)
    for bits in (32, 64):
        w = world_of(bits, SC.bodies_of(pos, [I] * n_colliders), cols)
        sq = SpatialQuery(w)
        sq.update()
        s = snapshot_of(w, cols)
        got, info = check_moves(sq, s, (shape, he, qpos, rot, vel * 0.25, 0.05, own))
        assert (got["collider"] == MISS).sum() >= 10 and (got["collider"] != MISS).sum() >= 10 and info["ignored"].sum() >= 3 and info["blocked"].sum() >= 3
        out, _, sinfo = check_slide(sq, s, (shape, he, qpos, rot, vel, own), MS.CFG, 3)
        assert (out["hit_count"] > 0).sum() >= 10 and (out["hit_count"] == 0).sum() >= 10 and len(set(out["iterations_run"])) >= 3


@pytest.mark.parametrize("bits", [32, 64])
def test_cast_moves_in_the_room(bits):
    w, sq, s, cols, sensor = room_world(bits)
    q = MS.moves(MOVE_SEED)                                              # 100 moves: two blocks, the second a partial wave
    got, info = check_moves(sq, s, q, sensor)
    # the populations of tests/test_spatial_moves_cpu.py
    assert (got["collider"] == MISS).sum() >= 15 and (got["collider"] != MISS).sum() >= 40
    assert (info["ignored"] > 0).sum() >= 8 and (info["blocked"] > 0).sum() >= 8 and (info["no_contact"] > 0).sum() >= 1
    assert got["collider"][5] != 11 and not (got["collider"] == 10).any() and len(set(got["collider"])) >= 6
    # masks and the shared excluded list
    rng = np.random.default_rng(bits)
    mask = rng.choice(np.array([1, 2, 3, 0xFFFFFFFF], np.uint32), 100)
    filtered, _ = check_moves(sq, s, q, sensor, mask=mask, excluded=np.array([100, 107], np.uint32))
    assert (filtered["collider"] != got["collider"]).sum() >= 10 and not np.isin(filtered["collider"], [0, 7]).any()


@pytest.mark.parametrize("bits", [32, 64])
def test_room_far_from_the_origin(bits):
    centre = (1000.0, -2000.0, 1500.0)
    w, sq, s, cols, sensor = room_world(bits, centre)
    got, info = check_moves(sq, s, MS.moves(MOVE_SEED, centre=centre), sensor)
    assert (got["collider"] != MISS).sum() >= 40 and (info["ignored"] > 0).sum() >= 5 and (info["blocked"] > 0).sum() >= 5
    out, _, sinfo = check_slide(sq, s, MS.characters(SLIDE_SEED, centre=centre), MS.CFG, 4, sensor)
    p = slide_populations(out, sinfo)
    assert p["never_hit"] >= 10 and p["one_plane"] >= 5 and p["more_planes"] >= 5, p


# ---- move_and_slide -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_move_and_slide_in_the_room(bits):
    w, sq, s, cols, sensor = room_world(bits)
    chars = MS.characters(SLIDE_SEED)
    out, hits, info = check_slide(sq, s, chars, MS.CFG, 4, sensor)
    p = slide_populations(out, info)
    assert p["never_hit"] >= 10 and p["one_plane"] >= 10 and p["more_planes"] >= 10 and p["leaving"] >= 5 and p["blocked"] >= 5 and p["no_contact"] >= 1, p
    assert info["live"][0] == 100 and info["live"][-1] >= 5 and (out["hit_count"] > 4).any() and (out["iterations_run"] == 4).any()
    assert (hits["kind"][hits["collider"] != MISS] == 1).any() and not np.isin(hits["collider"], [10]).any() and not (hits["collider"][5] == 11).any()
    moved = np.abs(out["position"] - chars[2].astype(DT[bits])).max(1)
    assert (moved > 0.5).sum() >= 30
    # iterations 0 and 1, max_planes 1, hit_cap 0 / 2 / 64, initial planes
    o0, _, _ = check_slide(sq, s, chars, dict(MS.CFG, move_and_slide_iterations=0), 0, sensor)
    assert (o0["iterations_run"] == 0).all() and (o0["hit_count"] == 0).all() and (o0["position"] != chars[2].astype(DT[bits])).any()      # the depenetrations alone
    o1, _, _ = check_slide(sq, s, chars, dict(MS.CFG, move_and_slide_iterations=1), 2, sensor)
    assert o1["iterations_run"].max() == 1 and (o1["hit_count"] >= 2).any() and (o1["hit_count"] <= out["hit_count"]).all()
    om, hm, im = check_slide(sq, s, chars, dict(MS.CFG, max_planes=1), MAX_HITS, sensor)
    assert im["max_planes"].max() == 1 and (om["projected_velocity"] != out["projected_velocity"]).any() and (hm["collider"][:, 8:] == MISS).all()
    planes = np.array([[0, 1, 0], [0.6, 0, -0.8]], np.float32)
    op, _, ip = check_slide(sq, s, chars, dict(MS.CFG, planes=planes), 4, sensor)
    assert ip["max_planes"].max() >= 4 and (op["projected_velocity"] != out["projected_velocity"]).any()
    # no depenetration at all: depenetration_iterations = 0
    check_slide(sq, s, chars, dict(MS.CFG, depenetration_iterations=0), 4, sensor)
    # masks and the shared excluded list
    rng = np.random.default_rng(bits)
    mask = rng.choice(np.array([1, 2, 3, 0xFFFFFFFF], np.uint32), 100)
    of, _, _ = check_slide(sq, s, chars, MS.CFG, 4, sensor, mask=mask, excluded=np.array([107, 100], np.uint32))
    assert (of["position"] != out["position"]).any(1).sum() >= 10
    st = sq.stats()
    assert st.nodes_visited > 0 and st.leaves_visited > 0


@pytest.mark.parametrize("bits", [32, 64])
def test_compound_scene_child_colliders(bits):
    rng = np.random.default_rng(5 + bits)
    bodies, cols, tf = compound_scene(seed=3, n_bodies=24)
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols, tf)
    assert s.n > 40 and tf["is_child"].any()
    n = 100
    near = np.stack(s.pos, 1).astype(float)[rng.integers(0, s.n, n)]
    pos = near + rng.normal(size=(n, 3)) * np.choose(np.arange(n) % 3, [0.4, 1.2, 3.0])[:, None]
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.1, 0.5, (n, 3))
    rot = random_unit_quats(rng, n)
    vel = rng.normal(size=(n, 3)) * 5
    own = np.where(rng.random(n) < 0.3, s.entity[rng.integers(0, s.n, n)], MISS).astype(np.uint32)
    got, info = check_moves(sq, s, (shape, he, pos, rot, vel * 0.25, rng.uniform(0, 0.1, n), own))
    assert (got["collider"] != MISS).sum() >= 30 and (got["collider"] == MISS).sum() >= 10 and info["ignored"].sum() >= 3 and info["blocked"].sum() >= 3
    out, _, sinfo = check_slide(sq, s, (shape, he, pos, rot, vel, own), MS.CFG, 6)
    assert (sinfo["max_planes"] >= 2).sum() >= 5 and (out["hit_count"] == 0).sum() >= 5


@pytest.mark.parametrize("bits", [32, 64])
def test_many_colliders_overlapping_at_the_start(bits):
    """Small balls inside one query ball: 60 of them go through the pending list of AVN_SPATIAL_MAX_HITS slots, 70 are more than it holds."""
    rng = np.random.default_rng(70)
    for n, fits in ((60, True), (70, False)):
        d = rng.normal(size=(n, 3))
        pos = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2, 0.9, (n, 1))
        cols = dict(entity_index=np.arange(n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=np.full(n, R.SHAPE_BALL, np.uint8),
                    half_extents=np.c_[np.full(n, 0.125), np.zeros((n, 2))])
        w = world_of(bits, SC.bodies_of(pos, np.tile(I, (n, 1))), cols)
        sq = SpatialQuery(w)
        sq.update()
        s = snapshot_of(w, cols)
        q = (np.array([R.SHAPE_BALL] * 3, np.uint8), np.array([[1.0, 0, 0], [0.25, 0, 0], [1.0, 0, 0]]), np.array([[0.0, 0, 0], [0, 5.0, 0], [0.0, 0, 0]]), np.tile(I, (3, 1)),
             np.array([[0.5, 0.25, 0], [0, 1.0, 0], [0, 0, 0]]), 0.05, None)
        if fits:
            got, info = check_moves(sq, s, q)
            assert info["ignored"][0] + info["blocked"][0] + info["no_contact"][0] == n and info["ignored"][0] >= 10 and info["blocked"][0] >= 10
            assert got["collider"][0] != MISS and got["distance"][0] == 0 and got["collider"][1] == MISS and got["collider"][2] != MISS
        else:
            with pytest.raises(F.AvnError) as e:
                sq.cast_moves(*q[:6])
            assert e.value.status == CAPACITY
            sq.cast_moves(q[0][1:2], q[1][1:2], q[2][1:2], q[3][1:2], q[4][1:2], 0.05)      # the world is usable afterwards


def test_device_pointers_equal_host_pointers():
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda a: T(np.ascontiguousarray(a).view(np.int32))
    for bits, dt in ((32, np.float32), (64, np.float64)):
        w, sq, s, cols, sensor = room_world(bits)
        shape, he, pos, rot, mv, skin, own = (np.ascontiguousarray(a.astype(dt) if a.dtype == np.float64 else a) for a in MS.moves(MOVE_SEED))
        n = len(shape)
        mask = np.where(np.arange(n) % 3 == 0, 1, 0xFFFFFFFF).astype(np.uint32)
        excluded = np.array([107], np.uint32)
        ht = sq.cast_moves(T(shape), T(he), T(pos), T(rot), T(mv), T(skin), self_entity=i32(own), mask=i32(mask), excluded=i32(excluded))
        hh = sq.cast_moves(shape, he, pos, rot, mv, skin, self_entity=own, mask=mask, excluded=excluded)
        assert ht.dtype == torch.uint8 and tuple(ht.shape) == (n, sq.move_hit_dtype.itemsize)
        same_records(ht.cpu().numpy().reshape(-1).view(sq.move_hit_dtype), hh, "device pointers: cast_moves")
        assert (hh["collider"] != MISS).sum() > 30
        vel = (mv * 4).astype(dt)
        for cap in (0, 3):
            st, lt = sq.move_and_slide(T(shape), T(he), T(pos), T(rot), T(vel), **MS.CFG, hit_cap=cap, self_entity=i32(own), mask=i32(mask), excluded=i32(excluded))
            sh, lh = sq.move_and_slide(shape, he, pos, rot, vel, **MS.CFG, hit_cap=cap, self_entity=own, mask=mask, excluded=excluded)
            same_records(st.cpu().numpy().reshape(-1).view(sq.slide_dtype), sh, "device pointers: move_and_slide")
            same_records(lt.cpu().numpy().reshape(-1).view(sq.slide_hit_dtype).reshape(n, cap), lh, "device pointers: hit log")
        assert (sh["hit_count"] > 0).sum() > 30
        nrm = np.tile(np.array(NORMALS[:5], np.float32)[None], (n, 1, 1))
        cnt = (np.arange(n) % 6).astype(np.uint32)
        vt = sq.project_velocities(T(vel), T(nrm), i32(cnt))
        assert vt.cpu().numpy().tobytes() == sq.project_velocities(vel, nrm, cnt).tobytes()


def test_invalid_queries_leave_the_other_lanes_alone():
    w, sq, s, cols, sensor = room_world(32)
    shape, he, pos, rot, vel, own = MS.characters(SLIDE_SEED, 64)
    shape = shape.copy()
    pos[2, 0] = np.nan; rot[9, 3] = np.inf; he[12] = [np.nan, 0.5, 0.5]; shape[12] = R.SHAPE_CUBOID
    he[20, 1] = -0.25; shape[20] = R.SHAPE_CUBOID; he[21, 0] = -0.5; shape[21] = R.SHAPE_BALL; shape[33] = 2
    he[35] = [0.5, np.nan, -1.0]; shape[35] = R.SHAPE_BALL    # a ball's y and z are not read: a valid character
    bad = [2, 9, 12, 20, 21, 33]
    vel[40] = [np.nan, 1, 0]; vel[41] = [0, -np.inf, 0]; vel[42] = 0.0; vel[43] = [1e-6, 0, 0]      # no movement: only the depenetrations
    with np.errstate(all="ignore"):
        out, hits, info = check_slide(sq, s, (shape, he, pos, rot, vel, own), MS.CFG, 2, sensor)
    assert np.array_equal(out["position"][bad], pos[bad].astype(np.float32), equal_nan=True) and np.array_equal(out["projected_velocity"][bad], vel[bad].astype(np.float32))
    assert (out["iterations_run"][bad + [40, 41, 42, 43]] == 0).all() and (out["hit_count"][bad] == 0).all() and (hits["collider"][bad] == MISS).all()
    assert np.array_equal(out["projected_velocity"][[40, 41]], vel[[40, 41]].astype(np.float32), equal_nan=True)
    assert (np.delete(out["hit_count"], bad) > 0).sum() > 25 and out["iterations_run"][35] > 0
    mv = vel * 0.25
    skin = np.full(64, 0.05)
    skin[50] = np.nan; skin[51] = np.inf; skin[52] = -0.125; mv[53] = [0, np.inf, 0]
    with np.errstate(all="ignore"):
        got, _ = check_moves(sq, s, (shape, he, pos, rot, mv, skin, own), sensor)
    assert (got["collider"][bad + [40, 41, 50, 51, 52, 53]] == MISS).all() and (got["collider"] != MISS).sum() > 25


def test_status_codes():
    import ctypes as C
    from avian_amd import spatial_query as Q
    bodies, cols, sensor = MS.room()
    w = world_of(32, bodies, cols)
    sq = SpatialQuery(w)
    shape, he, p, rot, v = np.array([1], np.uint8), np.array([[0.5, 0, 0]]), np.array([[0.3, 0.7, 0.3]]), np.array([I]), np.array([[0, -1.0, 0]])
    calls = (lambda: sq.cast_moves(shape, he, p, rot, v, 0.05), lambda: sq.move_and_slide(shape, he, p, rot, v, **MS.CFG))
    for call in calls:                       # before update()
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.project_velocities(v, np.array([[[0, 1, 0]]], np.float32))       # needs no snapshot
    sq.update()
    for call in calls:
        call()
    w.colliders_upload(**cols)               # the tables changed: a stale snapshot
    for call in calls:
        with pytest.raises(F.AvnError) as e:
            call()
        assert e.value.status == 6
    sq.update()
    for bad in (dict(move_and_slide_iterations=MAX_SLIDE_ITERATIONS + 1), dict(max_planes=MAX_PLANES + 1), dict(planes=np.zeros((MAX_PLANES + 1, 3), np.float32)), dict(hit_cap=MAX_HITS + 1)):
        with pytest.raises(F.AvnError) as e:
            sq.move_and_slide(shape, he, p, rot, v, **dict(MS.CFG, **bad))
        assert e.value.status == 1, bad
    sq.move_and_slide(shape, he, p, rot, v, **dict(MS.CFG, move_and_slide_iterations=MAX_SLIDE_ITERATIONS, max_planes=MAX_PLANES, planes=np.tile([[0, 1, 0]], (MAX_PLANES, 1)), hit_cap=MAX_HITS))
    # null arguments and null arrays
    qin = Q.avn_spatial_moves(); qin.count = 1
    rec = np.zeros(1, sq.move_hit_dtype)
    out = Q.avn_spatial_move_hits_out(rec.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_cast_moves(w.handle, C.byref(qin), C.byref(out)) == 1
    assert sq.dll.avn_spatial_cast_moves(w.handle, None, C.byref(out)) == 1
    assert sq.dll.avn_spatial_cast_moves(w.handle, C.byref(qin), None) == 1
    cin = Q.avn_spatial_characters(); cin.count = 1
    cfg = Q.avn_spatial_move_and_slide_config(0.25, 0.05, 1e-4, 0.3, 0.999, None, 0, 20, 4, 16)
    srec = np.zeros(1, sq.slide_dtype)
    sout = Q.avn_spatial_slides_out(srec.ctypes.data_as(Q.vp), None)
    assert sq.dll.avn_spatial_move_and_slide(w.handle, C.byref(cin), C.byref(cfg), 0, C.byref(sout)) == 1
    assert sq.dll.avn_spatial_move_and_slide(w.handle, C.byref(cin), None, 0, C.byref(sout)) == 1
    s8, h, r = shape.ctypes.data_as(Q.vp), np.array([[0.5, 0, 0]], np.float32), np.array([I], np.float32)
    pp, vv = np.array([[0.3, 0.7, 0.3]], np.float32), np.array([[0, -1, 0]], np.float32)
    cin.shape, cin.half_extents, cin.position, cin.rotation, cin.velocity = s8, h.ctypes.data_as(Q.vp), pp.ctypes.data_as(Q.vp), r.ctypes.data_as(Q.vp), vv.ctypes.data_as(Q.vp)
    assert sq.dll.avn_spatial_move_and_slide(w.handle, C.byref(cin), C.byref(cfg), 2, C.byref(sout)) == 1          # a hit_cap without a hit array
    assert sq.dll.avn_spatial_move_and_slide(w.handle, C.byref(cin), C.byref(cfg), 0, C.byref(sout)) == 0
    cfg.n_planes = 1                                                                                                 # planes announced, none given
    assert sq.dll.avn_spatial_move_and_slide(w.handle, C.byref(cin), C.byref(cfg), 0, C.byref(sout)) == 1
    vin = Q.avn_spatial_velocity_projections(); vin.count = 1
    vout = Q.avn_spatial_velocities_out(vv.ctypes.data_as(Q.vp))
    assert sq.dll.avn_spatial_project_velocities(w.handle, C.byref(vin), C.byref(vout)) == 1
    assert sq.dll.avn_spatial_project_velocities(w.handle, C.byref(vin), None) == 1


def test_host_shapes_need_the_skip_flag():
    from host_shape_helpers import capsule_world, capsule_scene
    w, _, _ = capsule_world(hip_lib(), 32)
    w.synchronize()
    _, cols, _, _ = capsule_scene()
    sq = SpatialQuery(w)
    sq.update()
    s = snapshot_of(w, cols)
    rng = np.random.default_rng(9)
    n = 64
    pos = np.stack(s.pos, 1).astype(float)[rng.integers(0, s.n, n)] + rng.normal(size=(n, 3))
    q = ((rng.random(n) < 0.5).astype(np.uint8), rng.uniform(0.1, 0.5, (n, 3)), pos, random_unit_quats(rng, n), rng.normal(size=(n, 3)), 0.05, None)
    with pytest.raises(F.AvnError) as e:
        sq.cast_moves(*q[:6])
    assert e.value.status == 6
    with pytest.raises(F.AvnError) as e:
        sq.move_and_slide(*q[:4], q[4] * 4, **MS.CFG)
    assert e.value.status == 6
    host = np.nonzero(s.shape == R.SHAPE_HOST)[0]
    got, _ = check_moves(sq, s, q, skip_host_shapes=True)
    assert sq.stats().host_skipped == len(host) > 0 and not np.isin(got["collider"], host).any() and (got["collider"] != MISS).sum() > 5
