"""GPU: the persistent casters (avn_spatial_*_casters_upload, avn_spatial_casters_run and their getters; include/avian_mi355x_spatial.h
"Casters") against the numpy restatement of tests/spatial_caster_reference.py, tolerance 0: every byte of every record, every count and every
re-aimed pose, f32 and f64.  The scenes, caster sets and the populations that keep the comparison from being empty are those of
tests/test_spatial_casters_cpu.py."""
import functools

import numpy as np
import pytest

from avian_amd import scenes
from avian_amd.spatial_query import CASTER_RAY, CASTER_SHAPE, MISS, SpatialQuery
from compound_helpers import compound_world
from helpers import F, hip_lib, random_unit_quats
import spatial_caster_reference as CA
import spatial_query_reference as R
import spatial_scenes as SC
from test_gpu_spatial_contacts import world_of
from test_gpu_spatial_query import same_records
from test_spatial_casters_cpu import (BODY, CASTER_SEED, COLLIDER, GAUNTLET_KS, WORLD, caster_set, gauntlet_casters, gauntlet_scene, layered_compound_scene, unit)

pytestmark = pytest.mark.gpu

I = [0.0, 0.0, 0.0, 1.0]
DT = {32: np.float32, 64: np.float64}
BAD_ARG, CAPACITY, STATE = 1, 4, 6
FAR = (1000.0, -2000.0, 1500.0)


def upload(sq, c, shapes):
    kw = dict(anchor_kind=c["anchor_kind"], anchor=c["anchor"], max_distance=c["max_distance"], max_hits=c["max_hits"], hit_cap=c["hit_cap"], enabled=c.get("enabled"),
              mask=c.get("mask"), self_entity=c.get("self_entity"), excluded=c.get("excluded"))
    if shapes:
        sq.shape_casters_upload(c["shape"], c["half_extents"], c["origin"], c["shape_rotation"], c["direction"], **kw)
    else:
        sq.ray_casters_upload(c["origin"], c["direction"], solid=c["solid"], **kw)


def same_poses(got, want, what):
    for g, w, name in zip(got, want, ("origins", "directions", "rotations")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: re-aimed {name} differ first at {np.nonzero((g != w).any(1))[0][:4]}"


def compare(sq, rays=None, shapes=None, what=""):
    """The device's records, counts and poses of the last run against (records, counts, poses...) of the reference."""
    out = []
    for want, kind, getter in ((rays, CASTER_RAY, sq.ray_caster_hits), (shapes, CASTER_SHAPE, sq.shape_caster_hits)):
        if want is None:
            continue
        hits, count = getter()
        same_records(hits, want[0], f"{what} {'shape' if kind else 'ray'} casters: records")
        assert np.array_equal(count, want[1]), f"{what}: counts differ first at {np.nonzero(count != want[1])[0][:4]}"
        same_poses(sq.caster_poses(kind), want[2:], what)
        out.append((hits, count))
    return out


def run_and_check(w, sq, cols, tf, rays=None, shapes=None, what="", **run_kw):
    """Upload, run, and compare with the reference built from a fresh bodies_download."""
    if rays is not None:
        upload(sq, rays, False)
    if shapes is not None:
        upload(sq, shapes, True)
    sq.casters_run(**run_kw)
    bodies = w.bodies_download()
    s = R.Snapshot(bodies, cols, tf, w.dtype)
    return compare(sq, None if rays is None else CA.ray_casters(s, bodies, rays), None if shapes is None else CA.shape_casters(s, bodies, shapes), what)


# ---- the compound scene: one reference per (bits, hit_cap, shift), shared by the tests below -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compound_case(bits, hit_cap, shift=(0.0, 0.0, 0.0), plain=False):
    bodies, cols, tf = layered_compound_scene(shift)
    s = R.Snapshot(bodies, cols, tf, DT[bits])          # (bodies_download returns the uploaded poses rounded to the world's scalar: the same snapshot)
    rays = caster_set(CASTER_SEED, bodies, cols, tf, hit_cap=hit_cap, rich=not plain)
    shapes = caster_set(CASTER_SEED + 1, bodies, cols, tf, hit_cap=hit_cap, shapes=True, rich=not plain)
    b = {k: np.asarray(bodies[k], DT[bits]) for k in ("position", "rotation")}
    return bodies, cols, tf, rays, shapes, CA.ray_casters(s, b, rays), CA.shape_casters(s, b, shapes)


def compound_run(bits, hit_cap, shift=(0.0, 0.0, 0.0), plain=False):
    bodies, cols, tf, rays, shapes, want_r, want_s = compound_case(bits, hit_cap, shift, plain)
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    upload(sq, rays, False); upload(sq, shapes, True)
    sq.casters_run()
    return w, sq, compound_case(bits, hit_cap, shift, plain)


@pytest.mark.parametrize("hit_cap", [64, 3])
@pytest.mark.parametrize("bits", [32, 64])
def test_compound_scene(bits, hit_cap):
    w, sq, (bodies, cols, tf, rays, shapes, want_r, want_s) = compound_run(bits, hit_cap)
    (hr, cr), (hs, cs) = compare(sq, want_r, want_s, f"f{bits} hit_cap {hit_cap}")
    for hits, count, c in ((hr, cr, rays), (hs, cs, shapes)):
        off = c["enabled"] == 0
        assert off.sum() == 11 and not count[off].any() and (hits[off]["collider"] == MISS).all()
        assert (count == 0).sum() >= 15 and (count >= 1).sum() >= 30 and (count >= 2).sum() >= 8
        k = np.minimum(c["max_hits"], hit_cap)
        filled = (hits["collider"] != MISS).sum(1)
        assert np.array_equal(filled, np.minimum(count, k)) and (count[k == 1] <= 1).all()
        if hit_cap == 3:
            assert (count > 3).any(), "some list must be cut by hit_cap"
    st = sq.stats()
    assert st.valid == 1 and st.colliders == 124 and st.leaves_visited > 0 and st.nodes_visited > st.leaves_visited


@pytest.mark.parametrize("bits", [32, 64])
def test_compound_scene_far_from_the_origin(bits):
    w, sq, (bodies, cols, tf, rays, shapes, want_r, want_s) = compound_run(bits, 64, FAR)
    (hr, cr), (hs, cs) = compare(sq, want_r, want_s, f"f{bits} far")
    assert (cr >= 1).sum() >= 25 and (cs >= 1).sum() >= 25


@pytest.mark.parametrize("bits", [32, 64])
def test_populations_with_and_without_ignore_self(bits):
    """The plain set of the CPU test: 39 hits with ignore_self, 78 answers change without it."""
    bodies, cols, tf = layered_compound_scene()
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    (h1, c1), = run_and_check(w, sq, cols, tf, rays=caster_set(CASTER_SEED, bodies, cols, tf), what="ignore_self")
    (h0, c0), = run_and_check(w, sq, cols, tf, rays=caster_set(CASTER_SEED, bodies, cols, tf, ignore_self=False), what="hits itself")
    assert c1.sum() >= 25 and (c1 == 0).sum() >= 25 and (h1[:, 0].view(np.uint8).reshape(100, -1) != h0[:, 0].view(np.uint8).reshape(100, -1)).any(1).sum() >= 30


# ---- the smallest trees and launches ---------------------------------------------------------------------------------------------------------------------
def small_casters(rng, n, n_bodies, shapes):
    kind = rng.choice(np.array([WORLD, BODY, COLLIDER], np.uint8), n)
    c = dict(anchor_kind=kind, anchor=rng.integers(0, n_bodies, n).astype(np.uint32), origin=np.c_[rng.uniform(-2, 2, n), rng.uniform(0.5, 2.5, n), rng.uniform(-2, 2, n)],
             direction=unit(rng.normal(size=(n, 3)) + [0, -1.5, 0]).astype(np.float32), max_distance=np.where(rng.random(n) < 0.5, np.inf, rng.uniform(1, 4, n)),
             max_hits=np.array([1, 2], np.uint32)[np.arange(n) % 2], hit_cap=2, self_entity=np.where(rng.random(n) < 0.3, 40, MISS).astype(np.uint32))
    if shapes:
        he = rng.uniform(0.1, 0.3, (n, 3)); ball = rng.random(n) < 0.5; he[ball, 1:] = 0
        c.update(shape=ball.astype(np.uint8), half_extents=he, shape_rotation=random_unit_quats(rng, n))
    else:
        c["solid"] = (rng.random(n) < 0.5).astype(np.uint8)
    return c


@pytest.mark.parametrize("n_casters", [1, 65])          # one lane; two blocks, the second with one live lane
@pytest.mark.parametrize("n_colliders", [1, 2])
def test_smallest_trees(n_colliders, n_casters):
    pos = [[0.0, -0.5, 0.0], [1.5, 1.0, 0.5]][:n_colliders]
    rot = [I, [0.0, np.sqrt(0.5), 0.0, np.sqrt(0.5)]][:n_colliders]
    cols = dict(entity_index=np.arange(40, 40 + n_colliders, dtype=np.uint32), body=np.arange(n_colliders, dtype=np.int32),
                shape=np.array([R.SHAPE_CUBOID, R.SHAPE_BALL][:n_colliders], np.uint8), half_extents=np.array([[3, 0.5, 3], [0.75, 0, 0]][:n_colliders], float))
    rng = np.random.default_rng(10 * n_colliders + n_casters)
    rays, shapes = small_casters(rng, n_casters, n_colliders, False), small_casters(rng, n_casters, n_colliders, True)
    for bits in (32, 64):
        w = world_of(bits, SC.bodies_of(pos, rot), cols)
        (hr, cr), (hs, cs) = run_and_check(w, SpatialQuery(w), cols, None, rays, shapes, f"f{bits} {n_colliders} colliders {n_casters} casters")
        if n_casters > 1:
            assert (cr > 0).sum() >= 10 and (cr == 0).sum() >= 5 and (cs > 0).sum() >= 10 and (cs == 0).sum() >= 5


@pytest.mark.parametrize("bits", [32, 64])
def test_gauntlet(bits):
    bodies, cols = gauntlet_scene()
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    (hr, cr), (hs, cs) = run_and_check(w, sq, cols, None, gauntlet_casters(True), gauntlet_casters(True, True), f"f{bits} gauntlet")
    for hits, count in ((hr, cr), (hs, cs)):
        assert list(count) == [1, 8, 8, 8, 8]
        for i, k in enumerate(GAUNTLET_KS):
            assert list(hits[i]["collider"][:min(k, 8)]) == list(range(min(k, 8))) and (hits[i]["collider"][min(k, 8):] == MISS).all()
    (hr, cr), (hs, cs) = run_and_check(w, sq, cols, None, gauntlet_casters(False), gauntlet_casters(False, True), f"f{bits} gauntlet without ignore_self")
    for hits, count in ((hr, cr), (hs, cs)):
        assert list(count) == [1, 9, 9, 9, 9] and (hits[:, 0]["collider"] == 8).all() and (hits[:, 0]["distance"] == 0).all()


@pytest.mark.parametrize("bits", [32, 64])
def test_a_body_with_a_nan_position(bits):
    bodies, cols, tf = layered_compound_scene()
    bodies = dict(bodies, position=bodies["position"].copy())
    bodies["position"][7, 1] = np.nan
    rays = caster_set(CASTER_SEED, bodies, cols, tf, hit_cap=4)
    rays["anchor"][:6] = 7
    rays["max_hits"] = np.array([1, 4], np.uint32)[np.arange(100) % 2]
    shapes = caster_set(CASTER_SEED + 1, bodies, cols, tf, hit_cap=4, shapes=True)
    shapes["anchor"][:6] = 7
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    with np.errstate(all="ignore"):
        (hr, cr), (hs, cs) = run_and_check(w, sq, cols, tf, rays, shapes, f"f{bits} NaN body")
    for hits, count, c in ((hr, cr, rays), (hs, cs, shapes)):
        on_nan = c["anchor"] == 7
        assert on_nan.sum() >= 6 and not count[on_nan].any() and (hits[on_nan]["collider"] == MISS).all()
        assert (count[~on_nan] > 0).sum() >= 25
        assert not np.isin(hits["collider"], np.nonzero(cols["body"] == 7)[0]).any()
    assert np.isnan(sq.caster_poses(CASTER_RAY)[0][:6, 1]).all()


# ---- checks that run the world ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_after_closed_loop_steps_the_run_takes_a_new_snapshot(bits):
    bodies, cols, tf, rays, shapes, want_r, want_s = compound_case(bits, 64)
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    w.pipeline_enable()
    sq = SpatialQuery(w)
    upload(sq, rays, False); upload(sq, shapes, True)
    sq.casters_run()
    compare(sq, want_r, want_s, "before the steps")
    before = sq.caster_poses(CASTER_RAY), sq.caster_poses(CASTER_SHAPE)
    for _ in range(5):
        w.step()
    sq.casters_run()                                    # no update() of the caller's: the run snapshots
    now = w.bodies_download()
    s = R.Snapshot(now, cols, tf, w.dtype)
    compare(sq, CA.ray_casters(s, now, rays), CA.shape_casters(s, now, shapes), "after five steps")
    after = sq.caster_poses(CASTER_RAY), sq.caster_poses(CASTER_SHAPE)
    moving = rays["anchor_kind"] != WORLD
    assert (before[0][0][moving] != after[0][0][moving]).any(1).sum() >= 60 and (before[0][1][moving] != after[0][1][moving]).any(1).sum() >= 60
    assert (before[1][2] != after[1][2]).any(1).sum() >= 60
    assert np.array_equal(before[0][0][~moving], after[0][0][~moving])


@pytest.mark.parametrize("bits", [32, 64])
def test_casters_run_between_steps_changes_nothing(bits):
    sc = scenes.box_stack(6, 6, 6)
    worlds = []
    for _ in range(2):
        w = F.World(hip_lib(), F.default_config(bits, substeps=4))
        w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**sc.collider_kwargs())
        w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
        w.pipeline_enable()
        worlds.append(w)
    plain, cast = worlds
    sq = SpatialQuery(cast)
    rng = np.random.default_rng(4)
    n, nb = 96, plain.n_bodies
    kw = dict(anchor_kind=np.full(n, BODY, np.uint8), anchor=rng.integers(0, nb, n).astype(np.uint32), max_hits=np.array([1, 4], np.uint32)[np.arange(n) % 2], hit_cap=4)
    d = unit(rng.normal(size=(n, 3))).astype(np.float32)
    sq.ray_casters_upload(np.zeros((n, 3)), d, **kw)
    sq.shape_casters_upload(np.ones(n, np.uint8), np.full((n, 3), 0.2), np.zeros((n, 3)), np.tile(I, (n, 1)), d, **kw)
    from test_gpu_graph import compare_step
    hit = 0
    for s in range(12):
        plain.step(); cast.step()
        sq.casters_run()
        if s % 4 == 3:
            hit += int((sq.ray_caster_hits()[1] > 0).sum()) + int((sq.shape_caster_hits()[1] > 0).sum())
        compare_step(s, plain, cast, check_rows=(s % 6 == 5))
    assert hit > 100


# ---- cross-checks ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_the_batched_queries_answer_the_same_from_the_device_poses(bits):
    """Not the restatement: casters without exclusions, their own re-aimed poses fed to cast_rays / ray_hits / cast_shapes / shape_hits."""
    dt = DT[bits]
    bodies, cols, tf = layered_compound_scene()
    rays = caster_set(CASTER_SEED, bodies, cols, tf, hit_cap=64, rich=True)
    shapes = caster_set(CASTER_SEED + 1, bodies, cols, tf, hit_cap=64, shapes=True, rich=True)
    for c in (rays, shapes):
        del c["excluded"], c["enabled"]
        c["self_entity"] = np.full(100, MISS, np.uint32)
    w = compound_world(hip_lib(), bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    upload(sq, rays, False); upload(sq, shapes, True)
    sq.casters_run()
    hr, cr = sq.ray_caster_hits(); hs, cs = sq.shape_caster_hits()
    ro, rd = sq.caster_poses(CASTER_RAY)
    so, sd, srot = sq.caster_poses(CASTER_SHAPE)
    assert (cr > 0).sum() >= 30 and (cs > 0).sum() >= 30
    for k in (1, 2, 3, 64):
        i = np.nonzero(rays["max_hits"] == k)[0]
        a = (ro[i], rd[i].astype(dt), rays["max_distance"][i], rays["solid"][i], rays["mask"][i])
        j = np.nonzero(shapes["max_hits"] == k)[0]
        b = (shapes["shape"][j], shapes["half_extents"][j], so[j], srot[j], sd[j].astype(dt))
        if k == 1:
            same_records(np.ascontiguousarray(hr[i, 0]), sq.cast_rays(*a), "cast_rays from the casters' poses")
            same_records(np.ascontiguousarray(hs[j, 0]), sq.cast_shapes(*b, shapes["max_distance"][j], shapes["mask"][j]), "cast_shapes from the casters' poses")
            assert np.array_equal(cr[i], hr[i, 0]["collider"] != MISS) and np.array_equal(cs[j], hs[j, 0]["collider"] != MISS)
            assert (hr[i, 1:]["collider"] == MISS).all() and (hs[j, 1:]["collider"] == MISS).all()
        else:
            h, cnt = sq.ray_hits(a[0], a[1], k, *a[2:])
            same_records(np.ascontiguousarray(hr[i, :k]), h, f"ray_hits k={k} from the casters' poses"); assert np.array_equal(cr[i], cnt)
            h, cnt = sq.shape_hits(*b, k, shapes["max_distance"][j], shapes["mask"][j])
            same_records(np.ascontiguousarray(hs[j, :k]), h, f"shape_hits k={k} from the casters' poses"); assert np.array_equal(cs[j], cnt)
            assert (hr[i, k:]["collider"] == MISS).all() and (hs[j, k:]["collider"] == MISS).all()


@pytest.mark.parametrize("bits", [32, 64])
def test_device_pointer_getters_equal_host_getters(bits):
    import torch
    w, sq, _ = compound_run(bits, 64)
    for kind, getter, rec in ((CASTER_RAY, sq.ray_caster_hits, sq.hit_dtype), (CASTER_SHAPE, sq.shape_caster_hits, sq.shape_hit_dtype)):
        hh, ch = getter()
        ht, ct = getter(device=True)
        assert ht.is_cuda and ct.is_cuda
        same_records(ht.cpu().numpy().reshape(-1).view(rec).reshape(hh.shape), hh, "device pointers: records")
        assert np.array_equal(ct.cpu().numpy().view(np.uint32), ch)
        for a, b in zip(sq.caster_poses(kind, device=True), sq.caster_poses(kind)):
            assert a.is_cuda and a.cpu().numpy().tobytes() == b.tobytes()
    assert sq.stats().leaves_visited > 0


# ---- statuses ------------------------------------------------------------------------------------------------------------------------------------------------
def status_of(fn, *a, **kw):
    with pytest.raises(F.AvnError) as e:
        fn(*a, **kw)
    return e.value.status


def test_status_codes():
    bodies, cols = gauntlet_scene()
    w = world_of(32, bodies, cols)
    sq = SpatialQuery(w)
    rays, shapes = gauntlet_casters(True), gauntlet_casters(True, True)
    upload(sq, rays, False); upload(sq, shapes, True)
    sq.update()
    # a getter before any run
    assert status_of(sq.ray_caster_hits) == STATE and status_of(sq.shape_caster_hits) == STATE and status_of(sq.caster_poses, CASTER_RAY) == STATE
    sq.casters_run()
    assert list(sq.ray_caster_hits()[1]) == [1, 8, 8, 8, 8]
    # a getter after a table change
    w.colliders_upload(**cols)
    assert status_of(sq.ray_caster_hits) == STATE and status_of(sq.caster_poses, CASTER_SHAPE) == STATE
    sq.update()
    assert status_of(sq.shape_caster_hits) == STATE, "a plain update does not bring the old run's results back"
    sq.casters_run()
    assert list(sq.shape_caster_hits()[1]) == [1, 8, 8, 8, 8]
    # a new definition drops the results
    upload(sq, rays, False)
    assert status_of(sq.ray_caster_hits) == STATE
    # hit_cap 0 and 65, an out-of-range anchor, an unknown anchor kind, bad flags
    assert status_of(upload, sq, dict(rays, hit_cap=0), False) == BAD_ARG and status_of(upload, sq, dict(shapes, hit_cap=65), True) == BAD_ARG
    assert status_of(upload, sq, dict(rays, anchor=np.full(5, 9, np.uint32)), False) == BAD_ARG
    assert status_of(upload, sq, dict(shapes, anchor_kind=np.full(5, COLLIDER, np.uint8), anchor=np.full(5, 9, np.uint32)), True) == BAD_ARG
    assert status_of(upload, sq, dict(rays, anchor_kind=np.full(5, 3, np.uint8)), False) == BAD_ARG
    assert sq.dll.avn_spatial_casters_run(w.handle, 1) == BAD_ARG
    # a rejected upload of another count and hit_cap leaves the tables, and the sizes of the getters' answers, as they were
    sq.casters_run()
    before = sq.ray_caster_hits(), sq.shape_caster_hits(), sq.caster_poses(CASTER_RAY), sq.caster_poses(CASTER_SHAPE)
    two = lambda c, **kw: dict({k: (v[:2] if isinstance(v, np.ndarray) else v) for k, v in c.items()}, **kw)
    assert status_of(upload, sq, two(rays, hit_cap=0), False) == BAD_ARG and status_of(upload, sq, two(shapes, hit_cap=65), True) == BAD_ARG
    assert status_of(upload, sq, two(rays, hit_cap=2, anchor=np.full(2, 9, np.uint32)), False) == BAD_ARG
    assert status_of(upload, sq, two(shapes, hit_cap=2, anchor_kind=np.full(2, 3, np.uint8)), True) == BAD_ARG
    sq.casters_run()
    after = sq.ray_caster_hits(), sq.shape_caster_hits(), sq.caster_poses(CASTER_RAY), sq.caster_poses(CASTER_SHAPE)
    assert after[0][0].shape == after[1][0].shape == (5, 64) and after[2][0].shape == (5, 3) and after[3][2].shape == (5, 4)
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
    assert list(after[0][1]) == [1, 8, 8, 8, 8] and list(after[1][1]) == [1, 8, 8, 8, 8]
    # count == 0 clears a kind: the run still answers the other one
    sq.ray_casters_upload(np.zeros((0, 3)), np.zeros((0, 3), np.float32))
    sq.casters_run()
    assert sq.ray_caster_hits()[0].shape == (0, 1) and list(sq.shape_caster_hits()[1]) == [1, 8, 8, 8, 8]
    upload(sq, rays, False)
    # an anchor that no longer fits after a smaller bodies_upload (body 8 leaves with its collider)
    keep = np.arange(9) < 8
    w.bodies_upload(**{k: v[keep] for k, v in bodies.items()})
    w.colliders_upload(**{k: v[keep] for k, v in cols.items()})
    assert status_of(sq.casters_run) == STATE
    sq.update()                                          # the tables themselves are fine
    assert sq.cast_rays(np.zeros((1, 3)), np.array([[1.0, 0, 0]]))[0]["collider"] == 0
    # with no casters at all the run is the update
    sq.ray_casters_upload(np.zeros((0, 3)), np.zeros((0, 3), np.float32))
    sq.shape_casters_upload(np.zeros(0, np.uint8), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 4)), np.zeros((0, 3), np.float32))
    w.colliders_upload(**{k: v[keep] for k, v in cols.items()})
    assert sq.stats().valid == 0
    sq.casters_run()
    assert sq.stats().valid == 1 and sq.cast_rays(np.zeros((1, 3)), np.array([[1.0, 0, 0]]))[0]["collider"] == 0


def test_despawn_drops_the_definitions():
    from test_gpu_despawn import despawn_both
    sc = scenes.box_stack(3, 3, 3)
    bodies, cols = sc.body_kwargs(), sc.collider_kwargs()
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    w.bodies_upload(**bodies); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    w.pipeline_enable()
    for _ in range(3):
        w.step()
    sq = SpatialQuery(w)
    n = 8
    sq.ray_casters_upload(np.zeros((n, 3)), np.tile(np.float32([0, -1, 0]), (n, 1)), anchor_kind=np.full(n, BODY, np.uint8), anchor=np.arange(w.n_bodies - n, w.n_bodies, dtype=np.uint32))
    sq.casters_run()
    assert (sq.ray_caster_hits()[1] == 1).all() and sq.stats().leaves_visited > 0
    despawn_both([w], bodies, cols, [5])
    sq.casters_run()                                     # the anchors would name other bodies now: no caster is left, the run is the update
    sq.ray_caster_hits()
    st = sq.stats()
    assert st.valid == 1 and st.nodes_visited == 0 and st.leaves_visited == 0


def test_host_shapes_need_the_skip_flag():
    from host_shape_helpers import capsule_scene, capsule_world
    w, _, _ = capsule_world(hip_lib(), 32)
    for _ in range(3):
        w.step()
    _, cols, _, _ = capsule_scene()
    sq = SpatialQuery(w)
    rng = np.random.default_rng(9)
    n = 64
    rays = dict(anchor_kind=np.full(n, WORLD, np.uint8), anchor=np.zeros(n, np.uint32), origin=rng.uniform([-1, -1, -1], [8, 5, 8], (n, 3)),
                direction=unit(rng.normal(size=(n, 3))).astype(np.float32), max_distance=np.full(n, np.inf), max_hits=np.array([1, 8], np.uint32)[np.arange(n) % 2], hit_cap=8,
                solid=np.ones(n, np.uint8))
    upload(sq, rays, False)
    assert status_of(sq.casters_run) == STATE
    (hits, count), = run_and_check(w, sq, cols, None, rays, None, "host shapes skipped", skip_host_shapes=True)
    host = np.nonzero(np.asarray(cols["shape"]) == R.SHAPE_HOST)[0]
    assert len(host) == 24 and not np.isin(hits["collider"], host).any() and (count > 0).sum() >= 20
