"""CPU: the caster definitions of include/avian_mi355x_spatial.h ("Casters") through their numpy restatement (tests/spatial_caster_reference.py):
the library's exports and struct layouts, hand-computed re-aiming cases compared with ==, the order of the shape-rotation product, the rounding
of the direction through float in an f64 world, the gauntlet that truncates the hit lists, and the populations the GPU test relies on.  The
scenes and caster sets of tests/test_gpu_spatial_casters.py are built here."""
import ctypes
import os
import re

import numpy as np
import pytest

from avian_amd import spatial_query as Q
from compound_helpers import compound_scene
from helpers import hip_lib, random_unit_quats
import spatial_caster_reference as CA
import spatial_query_reference as R
import spatial_scenes as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I = [0.0, 0.0, 0.0, 1.0]
DT = {32: np.float32, 64: np.float64}
MISS = R.MISS
WORLD, BODY, COLLIDER = CA.WORLD, CA.BODY, CA.COLLIDER
CASTER_SEED = 11
NEW_SYMBOLS = ["avn_spatial_ray_casters_upload", "avn_spatial_shape_casters_upload", "avn_spatial_casters_run", "avn_spatial_ray_caster_hits_get",
               "avn_spatial_shape_caster_hits_get", "avn_spatial_caster_poses_get"]


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- scenes and caster sets (shared with the GPU test) -------------------------------------------------------------------------------------------
def gauntlet_scene():
    """Eight static walls of half extents (0.1, 1, 1) at x = 1 .. 8 and body 8 at the origin with a ball of its own (entity 108)."""
    pos = [[float(x), 0.0, 0.0] for x in range(1, 9)] + [[0.0, 0.0, 0.0]]
    cols = dict(entity_index=np.arange(100, 109, dtype=np.uint32), body=np.arange(9, dtype=np.int32), shape=np.array([R.SHAPE_CUBOID] * 8 + [R.SHAPE_BALL], np.uint8),
                half_extents=np.array([[0.1, 1, 1]] * 8 + [[0.25, 0, 0]], float))
    return SC.bodies_of(pos, [I] * 9), cols


GAUNTLET_KS = [1, 2, 3, 8, 64]


def gauntlet_casters(ignore_self, shapes=False):
    """Five casters on body 8 along +x, max_distance 20, max_hits 1, 2, 3, 8, 64, hit_cap 64."""
    n = len(GAUNTLET_KS)
    c = dict(anchor_kind=np.full(n, BODY, np.uint8), anchor=np.full(n, 8, np.uint32), origin=np.zeros((n, 3)), direction=np.tile(np.float32([1, 0, 0]), (n, 1)),
             max_distance=np.full(n, 20.0), max_hits=np.array(GAUNTLET_KS, np.uint32), hit_cap=64,
             self_entity=np.full(n, 108 if ignore_self else MISS, np.uint32))
    if shapes:
        c.update(shape=np.full(n, R.SHAPE_CUBOID, np.uint8), half_extents=np.full((n, 3), 0.125),
                 shape_rotation=np.tile(I, (n, 1)))
    else:
        c["solid"] = np.ones(n, np.uint8)
    return c


def layered_compound_scene(shift=(0.0, 0.0, 0.0)):
    """compound_scene(seed=3, n_bodies=40), 124 colliders, with memberships in three layers; optionally moved as a whole."""
    bodies, cols, tf = compound_scene(seed=3, n_bodies=40)
    rng = np.random.default_rng(3)
    cols = dict(cols, memberships=(1 << rng.integers(0, 3, len(cols["shape"]))).astype(np.uint32))
    bodies = dict(bodies, position=bodies["position"] + np.asarray(shift, float))
    return bodies, cols, tf


def own_entities(cols, tf, n_bodies):
    """Per body the entity of its own (non-child) collider."""
    own = np.full(n_bodies, MISS, np.uint32)
    for c in range(len(cols["shape"])):
        if not tf["is_child"][c]:
            own[cols["body"][c]] = cols["entity_index"][c]
    return own


def caster_set(seed, bodies, cols, tf, n=100, hit_cap=1, shapes=False, rich=False, ignore_self=True):
    """n casters on the compound scene.  Plain: body anchors drawn uniformly, local origins normal(scale 0.2) with every fifth exactly 0, unit
    float32 directions, max_distance uniform in 0.5 .. 6, max_hits 1, ignore_self for all or none.  Rich adds: anchors of all three kinds (caster 1
    on a child collider), max_hits cycling 1, 2, 3, 64 inside every wave, masks, excluded lists of length 0, 1 and 5, ignore_self mixed, every ninth
    caster disabled, both values of solid, a few infinite ranges."""
    rng = np.random.default_rng(seed)
    nb, nc = len(bodies["position"]), len(cols["shape"])
    anchor = rng.integers(0, nb, n).astype(np.uint32)
    origin = rng.normal(scale=0.2, size=(n, 3)); origin[::5] = 0
    direction = unit(rng.normal(size=(n, 3))).astype(np.float32)
    md = rng.uniform(0.5, 6, n)
    own = own_entities(cols, tf, nb)[anchor]
    kind = np.full(n, BODY, np.uint8)
    c = dict(anchor_kind=kind, anchor=anchor, origin=origin, direction=direction, max_distance=md, max_hits=np.ones(n, np.uint32), hit_cap=hit_cap,
             self_entity=own if ignore_self else np.full(n, MISS, np.uint32))
    if shapes:
        ball = np.arange(n) % 2 == 0
        he = rng.uniform(0.1, 0.3, (n, 3)); he[ball, 1:] = 0
        c.update(shape=ball.astype(np.uint8), half_extents=he, shape_rotation=random_unit_quats(rng, n))
    else:
        c["solid"] = np.ones(n, np.uint8)
    if rich:
        kind[:] = rng.choice(np.array([WORLD, BODY, COLLIDER], np.uint8), n, p=[0.2, 0.5, 0.3])
        kind[1] = COLLIDER
        col = rng.integers(0, nc, n)
        col[1] = int(np.nonzero(tf["is_child"])[0][3])                      # a child collider
        anchor[kind == COLLIDER] = col[kind == COLLIDER]
        own[kind == COLLIDER] = cols["entity_index"][col[kind == COLLIDER]]
        w = kind == WORLD
        anchor[w] = 0; own[w] = MISS
        origin[w] = bodies["position"][rng.integers(1, nb, int(w.sum()))] + rng.normal(scale=0.5, size=(int(w.sum()), 3))
        c["max_hits"] = np.array([1, 2, 3, 64], np.uint32)[np.arange(n) % 4]
        c["max_distance"] = md = np.where(np.arange(n) % 7 == 3, np.inf, md)
        c["self_entity"] = np.where(rng.random(n) < 0.6, own, MISS).astype(np.uint32)
        c["mask"] = rng.choice(np.array([1, 2, 4, 3, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32), n)
        c["excluded"] = [rng.choice(cols["entity_index"], [0, 1, 5][i % 3], replace=False).astype(np.uint32) for i in range(n)]
        en = np.ones(n, np.uint8); en[8::9] = 0
        c["enabled"] = en
        if not shapes:
            c["solid"] = (rng.random(n) < 0.5).astype(np.uint8)
    return c


def snapshot(bodies, cols, tf, dt):
    return R.Snapshot(bodies, cols, tf, dt)


# ---- exports and layouts ---------------------------------------------------------------------------------------------------------------------------
def test_caster_entry_points_are_exported_and_laid_out():
    text = open(os.path.join(REPO, "include", "avian_mi355x_spatial.h")).read()
    declared = set(re.findall(r"AVN_API\s+avn_status\s+(avn_spatial_\w+)\s*\(", text))
    dll = ctypes.CDLL(hip_lib().path)
    for name in NEW_SYMBOLS:
        assert name in declared and name in Q.SYMBOLS and hasattr(dll, name), f"{hip_lib().path} does not export {name}"
    P = ctypes.sizeof(ctypes.c_void_p)
    rc, sc, po = Q.avn_spatial_ray_casters, Q.avn_spatial_shape_casters, Q.avn_spatial_caster_poses_out
    assert {rc, sc, po} <= set(Q.STRUCTS)
    assert ctypes.sizeof(rc) == 8 + 12 * P and ctypes.sizeof(sc) == 8 + 14 * P and ctypes.sizeof(po) == 3 * P
    assert [f[0] for f in rc._fields_] == ["count", "hit_cap", "anchor_kind", "anchor", "origin", "direction", "max_distance", "max_hits", "solid", "enabled", "mask",
                                           "self_entity", "excluded_offset", "excluded"]
    assert [f[0] for f in sc._fields_] == ["count", "hit_cap", "anchor_kind", "anchor", "origin", "direction", "max_distance", "max_hits", "shape", "half_extents",
                                           "shape_rotation", "enabled", "mask", "self_entity", "excluded_offset", "excluded"]
    assert rc.hit_cap.offset == 4 and rc.anchor_kind.offset == 8 and sc.shape.offset == 8 + 6 * P and po.rotation.offset == 2 * P
    # the header's field order is the binding's
    for cls in (rc, sc, po):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cls.__name__, cls.__name__), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in cls._fields_], cls.__name__
    assert (Q.ANCHOR_WORLD, Q.ANCHOR_BODY, Q.ANCHOR_COLLIDER, Q.CASTER_RAY, Q.CASTER_SHAPE) == (0, 1, 2, 0, 1)
    for name, value in (("AVN_SPATIAL_ANCHOR_WORLD", 0), ("AVN_SPATIAL_ANCHOR_BODY", 1), ("AVN_SPATIAL_ANCHOR_COLLIDER", 2), ("AVN_SPATIAL_CASTER_RAY", 0), ("AVN_SPATIAL_CASTER_SHAPE", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name


# ---- known answers of the re-aiming -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_reaim_known_answers(bits):
    dt = DT[bits]
    # body 0 at (1, 2, 3) turned 180 degrees about z; body 1 carries a child collider moved by (0, 4, 0) and turned 180 degrees about x
    bodies = SC.bodies_of([[1, 2, 3], [8, 0, 0]], [[0, 0, 1, 0], I])
    cols = dict(entity_index=np.array([7, 9], np.uint32), body=np.array([0, 1], np.int32), shape=np.array([R.SHAPE_BALL] * 2, np.uint8), half_extents=np.array([[0.5, 0, 0]] * 2, float))
    tf = dict(is_child=np.array([0, 1], np.uint8), translation=np.array([[0, 0, 0], [0, 4, 0]], float), rotation=np.array([I, [1, 0, 0, 0]], float))
    s = snapshot(bodies, cols, tf, dt)
    kind = np.array([BODY, WORLD, COLLIDER], np.uint8)
    go, gd, grot = CA.reaim(s, bodies, kind, [0, 0, 1], [[1, 0, 0], [1, 0, 0], [0, 1, 2]], np.float32([[1, 0, 0], [1, 0, 0], [0, 0, 1]]), [[0, 0, 0, 1]] * 3)
    assert go.dtype == dt and gd.dtype == np.float32 and grot.dtype == dt
    assert (go[0] == [0, 2, 3]).all() and (gd[0] == [-1, 0, 0]).all()                  # the issue's case, exact
    assert (grot[0] == [0, 0, 1, 0]).all()                                             # identity * rot
    assert (go[1] == [1, 0, 0]).all() and (gd[1] == [1, 0, 0]).all() and (grot[1] == I).all()      # a world anchor: unchanged
    # the child collider sits at (8, 4, 0) turned 180 degrees about x: (0, 1, 2) -> (0, -1, -2), +z -> -z
    assert (go[2] == [8, 3, -2]).all() and (gd[2] == [0, 0, -1]).all()


def textbook_qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


@pytest.mark.parametrize("bits", [32, 64])
def test_shape_rotation_is_on_the_left(bits):
    dt = DT[bits]
    h = np.sqrt(0.5)
    rot = np.array([0, 0, h, h])            # the body: 90 degrees about z
    sr = np.array([h, 0, 0, h])             # the shape: 90 degrees about x
    bodies = SC.bodies_of([[0, 0, 0]], [rot])
    cols = dict(entity_index=np.array([1], np.uint32), body=np.array([0], np.int32), shape=np.array([R.SHAPE_BALL], np.uint8), half_extents=np.array([[0.5, 0, 0]], float))
    s = snapshot(bodies, cols, None, dt)
    _, _, grot = CA.reaim(s, bodies, [BODY], [0], [[0, 0, 0]], np.float32([[1, 0, 0]]), [sr])
    want = textbook_qmul(sr.astype(dt).astype(float), rot.astype(dt).astype(float))
    reverse = textbook_qmul(rot.astype(dt).astype(float), sr.astype(dt).astype(float))
    eps = float(np.finfo(dt).eps)
    assert np.abs(grot[0].astype(float) - want).max() <= 4 * eps
    assert np.abs(want - reverse).max() > 0.9 and np.abs(grot[0].astype(float) - reverse).max() > 0.9      # (0.5, 0.5, 0.5, 0.5) against (0.5, -0.5, 0.5, 0.5)


def test_direction_is_rounded_through_float_in_an_f64_world():
    dt = np.float64
    rng = np.random.default_rng(5)
    rot = random_unit_quats(rng, 1)[0]
    bodies = SC.bodies_of([[0.5, -1, 2]], [rot])
    cols = dict(entity_index=np.array([1], np.uint32), body=np.array([0], np.int32), shape=np.array([R.SHAPE_BALL], np.uint8), half_extents=np.array([[0.5, 0, 0]], float))
    s = snapshot(bodies, cols, None, dt)
    d = unit(rng.normal(size=(8, 3))).astype(np.float32)
    _, gd, _ = CA.reaim(s, bodies, [BODY] * 8, [0] * 8, np.zeros((8, 3)), d)
    q = tuple(np.full(8, x) for x in rot)
    full = np.stack(R.qrot(q, tuple(d[:, i].astype(dt) for i in range(3)), dt), 1)     # the rotation in f64, not rounded
    assert gd.dtype == np.float32 and np.array_equal(gd, full.astype(np.float32))
    assert (gd.astype(dt) != full).any(1).all(), "every direction must have lost bits to the rounding"
    assert np.abs(gd.astype(dt) - full).max() <= 2.0 ** -24
    # not the f32 rotation either: the product is taken in the world's scalar
    f32 = np.stack(R.qrot(tuple(x.astype(np.float32) for x in q), tuple(d[:, i] for i in range(3)), np.float32), 1)
    assert (f32 != gd).any()
    # and not renormalised
    assert (np.linalg.norm(gd.astype(dt), axis=1) != 1).any()


# ---- the gauntlet: truncation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("shapes", [False, True])
def test_gauntlet(bits, shapes):
    bodies, cols = gauntlet_scene()
    s = snapshot(bodies, cols, None, DT[bits])
    run = (lambda c: CA.shape_casters(s, bodies, c)[:2]) if shapes else (lambda c: CA.ray_casters(s, bodies, c)[:2])
    hits, count = run(gauntlet_casters(True, shapes))
    assert hits.shape == (5, 64) and list(count) == [1, 8, 8, 8, 8]
    for i, k in enumerate(GAUNTLET_KS):
        m = min(k, 8)
        assert list(hits[i]["collider"][:m]) == list(range(m)) and (hits[i]["collider"][m:] == MISS).all() and (hits[i]["entity"][m:] == MISS).all()
        assert not hits[i][m:].view(np.uint8).reshape(64 - m, -1)[:, 8:].any()             # slots past the answer: ids MISS, zeros
        if i:
            p = min(GAUNTLET_KS[i - 1], 8)
            assert hits[i - 1][:p].tobytes() == hits[i][:p].tobytes(), "each list is the prefix of the next"
    reach = 0.125 if shapes else 0.0
    # the walls' near faces, less the cast shape's reach: a few roundings of coordinates <= 8
    assert np.abs(hits[4]["distance"][:8] - (np.arange(1, 9) - 0.1 - reach)).max() <= 64 * float(np.finfo(DT[bits]).eps)
    # without ignore_self the caster's own collider comes first, at distance 0
    hits, count = run(gauntlet_casters(False, shapes))
    assert list(count) == [1, 9, 9, 9, 9]
    assert (hits[:, 0]["collider"] == 8).all() and (hits[:, 0]["entity"] == 108).all() and (hits[:, 0]["distance"] == 0).all()
    assert list(hits[3]["collider"][:9]) == [8, 0, 1, 2, 3, 4, 5, 6, MISS] and list(hits[4]["collider"][:10]) == [8, 0, 1, 2, 3, 4, 5, 6, 7, MISS]


# ---- populations of the random scene ------------------------------------------------------------------------------------------------------------------
def ray_populations(bits):
    bodies, cols, tf = layered_compound_scene()
    s = snapshot(bodies, cols, tf, DT[bits])
    assert s.n == 124
    with_self = CA.ray_casters(s, bodies, caster_set(CASTER_SEED, bodies, cols, tf))
    without = CA.ray_casters(s, bodies, caster_set(CASTER_SEED, bodies, cols, tf, ignore_self=False))
    return with_self, without


@pytest.mark.parametrize("bits", [32, 64])
def test_populations_of_the_random_scene(bits):
    (hits, count, _, _), (hits0, count0, _, _) = ray_populations(bits)
    hit = hits[:, 0]["collider"] != MISS
    changed = (hits[:, 0].view(np.uint8).reshape(100, -1) != hits0[:, 0].view(np.uint8).reshape(100, -1)).any(1)
    print(f"f{bits}: {hit.sum()} hit, {(~hit).sum()} miss, {changed.sum()} change without ignore_self")
    assert hit.sum() >= 25 and (~hit).sum() >= 25 and changed.sum() >= 30
    assert np.array_equal(count, hit.astype(np.uint32))


def test_the_rich_caster_sets_cover_every_feature():
    """The sets the GPU test compares: every anchor kind, every k, both filters, disabled casters, and answers of every length."""
    bodies, cols, tf = layered_compound_scene()
    s = snapshot(bodies, cols, tf, np.float32)
    for shapes in (False, True):
        c = caster_set(CASTER_SEED + shapes, bodies, cols, tf, hit_cap=64, shapes=shapes, rich=True)
        assert set(c["anchor_kind"]) == {WORLD, BODY, COLLIDER} and tf["is_child"][c["anchor"][1]] and c["anchor_kind"][1] == COLLIDER
        assert sorted(set(len(e) for e in c["excluded"])) == [0, 1, 5] and (c["self_entity"] == MISS).sum() >= 20 and (c["self_entity"] != MISS).sum() >= 20
        for wave in (slice(0, 64), slice(64, 100)):
            assert set(c["max_hits"][wave]) == {1, 2, 3, 64}
        hits, count = (CA.shape_casters if shapes else CA.ray_casters)(s, bodies, c)[:2]
        on = c["enabled"] != 0
        assert (~on).sum() == 11 and not count[~on].any() and (hits[~on]["collider"] == MISS).all()
        print(f"shapes={shapes}: counts {np.bincount(count)}")
        assert (count == 0).sum() >= 15 and (count >= 1).sum() >= 30 and (count >= 2).sum() >= 8
        # truncation by hit_cap 3: the same answers cut to three slots (nearest-k is a prefix)
        h3, c3 = (CA.shape_casters if shapes else CA.ray_casters)(s, bodies, dict(c, hit_cap=3))[:2]
        assert h3.tobytes() == np.ascontiguousarray(hits[:, :3]).tobytes()
        many = c["max_hits"] > 1
        assert np.array_equal(c3[many], count[many])
