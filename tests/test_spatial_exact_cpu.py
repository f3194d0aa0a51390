"""CPU: the numpy restatement of the spatial queries' exact tests (tests/spatial_query_reference.py, the device's operation order) against
exact rational geometry (tests/spatial_exact_geometry.py), the tree's padding property, the far-field ball regression and the non-finite
contract (include/avian_mi355x_spatial.h)."""
import numpy as np
import pytest

import spatial_exact_geometry as X
import spatial_query_reference as R
import spatial_scenes as S

CASES = [(32, np.float32, 1e4), (64, np.float64, 1e9)]   # (bits, dtype, farthest ray origin)
N_RAYS = 800


def far_field(bits, dt, far, n=N_RAYS):
    bodies, cols, tf = S.far_scene(bits)
    s = R.Snapshot(bodies, cols, tf, dt)
    o, d, md, solid, target, aim = S.aimed_rays(bits, s, n, 1.0, far)
    return s, S.exact_colliders(bodies, cols, tf, dt), o.astype(dt), d.astype(dt), md.astype(dt), solid, target, aim.astype(dt)


def pick(a, idx):
    return tuple(np.asarray(x)[idx] for x in a)


@pytest.mark.parametrize("bits,dt,far", CASES)
def test_rays_against_exact_geometry(bits, dt, far):
    s, ex, o, d, md, solid, tg, _ = far_field(bits, dt, far)
    hit, toi, nrm = R.ray_exact(s.shape[tg], pick(s.he, tg), pick(s.pos, tg), pick(s.rot, tg), tuple(o.T), tuple(d.T), md, solid != 0, dt)
    decided = hits = misses = compared = 0
    for i in range(len(o)):
        c = ex[tg[i]]
        a = X.ray(c, o[i], d[i], float(md[i]), bool(solid[i]))
        band, tb, nb = X.bound(bits, o[i], c, a.toi or 0, a.half_chord)
        if a.margin() <= band:
            continue
        decided += 1
        what = f"ray {i} -> collider {tg[i]} (shape {c.shape}, he {[float(h) for h in c.he]}): exact {a}, float hit {hit[i]} toi {toi[i]}"
        assert bool(hit[i]) == a.hit, f"decision differs outside the band {band:.3g}: {what}"
        hits += a.hit
        misses += not a.hit
        if a.hit and all(a.margin(k) is None or a.margin(k) > band for k in ("inside", "face")):
            compared += 1
            assert abs(float(toi[i]) - float(a.toi)) <= tb, f"distance off by {abs(float(toi[i]) - float(a.toi)):.3g} > {tb:.3g}: {what}"
            err = max(abs(float(nrm[k][i]) - float(a.normal[k])) for k in range(3))
            assert err <= nb, f"normal off by {err:.3g} > {nb:.3g}: {what}"
    assert decided >= 0.6 * len(o), f"only {decided} of {len(o)} rays decided outside the band"
    assert hits >= 0.2 * decided and misses >= 0.1 * decided and compared >= 0.2 * decided, (hits, misses, compared)


@pytest.mark.parametrize("bits,dt,far", CASES)
def test_points_and_boxes_against_exact_geometry(bits, dt, far):
    s, ex, _, _, _, _, tg, aim = far_field(bits, dt, far)
    rng = np.random.default_rng(bits)
    ins = R.point_exact(s.shape[tg], pick(s.he, tg), pick(s.pos, tg), pick(s.rot, tg), tuple(aim.T), dt)
    ext = rng.uniform(0, 0.05, aim.shape)
    centre = aim + rng.uniform(-1, 1, aim.shape) * rng.uniform(0, 2, (len(aim), 1))   # around the aimed surface point, some clear of the AABB
    lo, hi = (centre - ext).astype(dt), (centre + ext).astype(dt)
    over = R.aabb_exact(s.shape[tg], pick(s.he, tg), pick(s.pos, tg), pick(s.rot, tg), tuple(lo.T), tuple(hi.T), dt)
    n_p = n_b = inside = overlap = 0
    for i in range(len(aim)):
        c = ex[tg[i]]
        band = X.bound(bits, aim[i], c)[0]
        a = X.point(c, aim[i])
        if a.margin() > band:
            n_p += 1
            inside += a.hit
            assert bool(ins[i]) == a.hit, f"point {i} in collider {tg[i]}: exact {a}, float {ins[i]}"
        b = X.aabb(c, lo[i], hi[i])
        if b.margin() > band:
            n_b += 1
            overlap += b.hit
            assert bool(over[i]) == b.hit, f"box {i} on collider {tg[i]}: exact {b}, float {over[i]}"
    assert n_p >= 0.5 * len(aim) and n_b >= 0.5 * len(aim), (n_p, n_b)
    assert 0.1 * n_p <= inside <= 0.9 * n_p and 0.1 * n_b <= overlap <= 0.9 * n_b, (inside, n_p, overlap, n_b)


@pytest.mark.parametrize("bits,dt,far", CASES)
def test_padding_property(bits, dt, far):
    """Every (ray, collider) pair the float exact test accepts enters the collider's padded leaf box no later than its distance (the node
    test of k_sp_query with the closest hit's bound), and every point the float test accepts lies in the point node test's box: the tree
    never culls an answer, so the device equals brute force."""
    s, _, o, d, md, solid, _, aim = far_field(bits, dt, far)
    lo, hi = R.leaf_boxes(s)
    col = lambda a: tuple(x[None, :] for x in a)
    row = lambda a: tuple(np.asarray(a)[:, k][:, None] for k in range(3))
    hit, toi, _ = R.ray_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), row(o), row(d), md[:, None], (solid != 0)[:, None], dt)
    entry = R.ray_box(row(o), row(d), col(lo), col(hi), toi, dt)
    bad = np.argwhere(hit & ~(entry <= toi))
    assert hit.sum() > 0.5 * len(o)
    assert not len(bad), f"{len(bad)} accepted pairs lie outside the padded leaf box, first ray {bad[0][0]} collider {bad[0][1]}: toi {toi[tuple(bad[0])]}, entry {entry[tuple(bad[0])]}"
    pin = R.point_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), row(aim), dt)
    assert pin.sum() > 0.1 * len(aim)
    assert not (pin & ~R.point_box(row(aim), col(lo), col(hi), dt)).any()


@pytest.mark.parametrize("bits,dt,x", [(32, np.float32, 1000.0), (64, np.float64, 1e8)])
def test_far_grazing_ball_is_a_miss(bits, dt, x):
    """A unit ball at (x, 0, 0) and a ray along +x at y = 1.0125: it misses by 0.0125.  Parry's discriminant b^2 - a c reported a hit at
    distance x with normal (0, 1, 0), outside the padded leaf box, so the device (which culls it) and brute force disagreed."""
    bodies = S.bodies_of([[x, 0, 0]], [S.IDENTITY])
    cols = dict(entity_index=np.array([5], np.uint32), body=np.array([0], np.int32), shape=np.array([R.SHAPE_BALL], np.uint8), half_extents=np.array([[1.0, 0, 0]]))
    s = R.Snapshot(bodies, cols, None, dt)
    o, d = np.array([[0.0, 1.0125, 0]], dt), np.array([[1.0, 0, 0]], dt)
    ex = X.ray(X.Collider(R.SHAPE_BALL, (1, 0, 0), (x, 0, 0), S.IDENTITY), o[0], d[0])
    assert not ex.hit and ex.margin() > X.bound(bits, o[0], X.Collider(R.SHAPE_BALL, (1, 0, 0), (x, 0, 0), S.IDENTITY))[0]
    assert R.cast_rays(s, o, d)[0]["collider"] == R.MISS
    lo, hi = R.leaf_boxes(s)
    assert R.ray_box(tuple(o.T), tuple(d.T), lo, hi, dt(np.inf), dt)[0] == np.inf   # the tree culls it too
    # just inside the silhouette it is a hit, with the right distance
    o2 = np.array([[0.0, 0.9875, 0]], dt)
    h = R.cast_rays(s, o2, d)[0]
    ex2 = X.ray(X.Collider(R.SHAPE_BALL, (1, 0, 0), (x, 0, 0), S.IDENTITY), o2[0], d[0])
    assert ex2.hit and h["collider"] == 0 and abs(float(h["distance"]) - float(ex2.toi)) <= X.bound(bits, o2[0], X.Collider(R.SHAPE_BALL, (1, 0, 0), (x, 0, 0), S.IDENTITY), ex2.toi, ex2.half_chord)[1]


def nonfinite_scene(dt):
    """Four unit cubes on the x axis and a ball; colliders 1 (NaN position), 2 (inf position) and 3 (NaN rotation, a ball: its AABB
    ignores the rotation) are not finite."""
    pos = np.array([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [6, 0, 0], [9, 0, 0]], float)
    rot = np.tile(S.IDENTITY, (5, 1))
    rot[3] = [np.nan, 0, 0, 1]
    cols = dict(entity_index=np.arange(5, dtype=np.uint32), body=np.arange(5, dtype=np.int32),
                shape=np.array([0, 0, 0, 1, 0], np.uint8), half_extents=np.array([[0.5] * 3, [0.5] * 3, [0.5] * 3, [0.5, 0, 0], [0.5] * 3]))
    return R.Snapshot(S.bodies_of(pos, rot), cols, None, dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_non_finite_contract_of_the_reference(dt):
    s = nonfinite_scene(dt)
    assert list(s.candidates()) == [True, False, False, False, True]
    lo, hi = R.leaf_boxes(s)
    assert all(np.isinf(x[1:4]).all() for x in lo + hi)
    # a ray along +x through everything: only the finite cuboids, nearest first
    h, cnt = R.ray_hits(s, np.array([[-5.0, 0, 0]]), np.array([[1.0, 0, 0]]), 8)
    assert cnt[0] == 2 and list(h[0]["collider"][:3]) == [0, 4, R.MISS]
    # non-finite queries: a miss / count 0 whatever the scene
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])
    ok = np.array([[-5.0, 0, 0]] * 3)
    dirs = np.array([[1.0, 0, 0]] * 3)
    assert (R.cast_rays(s, bad, dirs)["collider"] == R.MISS).all()
    assert (R.cast_rays(s, ok, bad)["collider"] == R.MISS).all()
    assert (R.ray_hits(s, bad, dirs, 4)[1] == 0).all()
    assert (R.point_intersections(s, bad, 4)[1] == 0).all()
    assert (R.aabb_intersections(s, np.full((1, 3), -np.inf), np.full((1, 3), np.inf), 4)[1] == 0).all()
    assert (R.aabb_intersections(s, np.full((1, 3), -1.0), np.array([[1.0, 1, np.nan]]), 4)[1] == 0).all()
    # finite queries reach only the finite colliders, a box over everything included
    assert list(R.aabb_intersections(s, np.full((1, 3), -1e30), np.full((1, 3), 1e30), 8)[0][0][:3]) == [0, 4, R.MISS]
    # a hit needs a finite distance: a non-solid ray with a zero direction from inside a cuboid has no exit
    h = R.cast_rays(s, np.array([[0.1, 0, 0]]), np.zeros((1, 3)), solid=np.array([0], np.uint8))
    assert h[0]["collider"] == R.MISS
    h = R.cast_rays(s, np.array([[0.1, 0, 0]]), np.zeros((1, 3)), solid=np.array([1], np.uint8))
    assert h[0]["collider"] == 0 and h[0]["distance"] == 0
