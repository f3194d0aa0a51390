"""GPU: the device spatial queries at their edges, against a brute-force pass of the numpy restatement (tests/spatial_query_reference.py)
at tolerance 0 and, on a sample, against exact geometry (tests/spatial_exact_geometry.py): far-field scenes, LBVH build edges (sizes around
the sort's and the workgroups' boundaries, degenerate and extreme centres), query edges, and the non-finite contract of
include/avian_mi355x_spatial.h.  The worlds here are only uploaded, updated and queried, never stepped."""
import numpy as np
import pytest

from avian_amd.spatial_query import SpatialQuery, MISS
from helpers import F, hip_lib, random_unit_quats
from test_gpu_spatial_query import same_records, same_ids
import spatial_exact_geometry as X
import spatial_query_reference as R
import spatial_scenes as S

pytestmark = pytest.mark.gpu


def world_of(bits, bodies, cols, tf=None):
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))
    w.bodies_upload(**bodies)
    w.colliders_upload(**cols)
    if tf is not None:
        w.collider_transforms_upload(**tf)
    return w


def check_queries(sq, s, o, d, md, solid, pts, lo, hi, ks=(8,), cap=8, chunk=16):
    """The four queries of the device equal brute force, bit for bit."""
    closest, many = R.ray_queries(s, o, d, ks, md, solid, chunk=chunk)
    same_records(sq.cast_rays(o, d, md, solid), closest, "cast_rays")
    for k in ks:
        h, c = sq.ray_hits(o, d, k, md, solid)
        same_records(h, many[k][0], f"ray_hits k={k}")
        assert np.array_equal(c, many[k][1]), f"ray_hits k={k}: counts"
    same_ids(sq.point_intersections(pts, cap), R.point_intersections(s, pts, cap, chunk=4 * chunk), "points")
    same_ids(sq.aabb_intersections(lo, hi, cap), R.aabb_intersections(s, lo, hi, cap), "aabbs")
    return closest


# ---- far field ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,far", [(32, 1e4), (64, 1e9)])
def test_far_field_against_brute_force_and_exact_geometry(bits, far):
    dt = np.float32 if bits == 32 else np.float64
    bodies, cols, tf = S.far_scene(bits)
    w = world_of(bits, bodies, cols, tf)
    sq = SpatialQuery(w)
    sq.update()
    s = R.Snapshot(w.bodies_download(), cols, tf, dt)
    o, d, md, solid, tg, aim = S.aimed_rays(bits, s, 768, 1.0, far)
    rng = np.random.default_rng(bits)
    ext = rng.uniform(0, 0.05, aim.shape)
    centre = aim + rng.uniform(-1, 1, aim.shape) * rng.uniform(0, 2, (len(aim), 1))
    check_queries(sq, s, o, d, md, solid, aim, centre - ext, centre + ext, ks=(1, 8))
    # a sample against exact geometry: the aimed collider is in the device's hit list exactly when geometry says so (outside the band),
    # with the distance and normal within the bound
    ex = S.exact_colliders(bodies, cols, tf, dt)
    n = 256
    h, cnt = sq.ray_hits(o[:n], d[:n], 64, md[:n], solid[:n])
    o_, d_, md_ = o.astype(dt), d.astype(dt), md.astype(dt)
    decided = 0
    for i in range(n):
        c = ex[tg[i]]
        a = X.ray(c, o_[i], d_[i], float(md_[i]), bool(solid[i]))
        band, tb, nb = X.bound(bits, o_[i], c, a.toi or 0, a.half_chord)
        if a.margin() <= band or cnt[i] > 64:
            continue
        decided += 1
        row = h[i][h[i]["collider"] == tg[i]]
        assert len(row) == int(a.hit), f"ray {i}, collider {tg[i]}: exact {a}, device {h[i][:cnt[i]]}"
        if a.hit and all(a.margin(k) is None or a.margin(k) > band for k in ("inside", "face")):
            assert abs(float(row[0]["distance"]) - float(a.toi)) <= tb, f"ray {i}: device {row[0]}, exact {a}"
            assert max(abs(float(row[0]["normal"][k]) - float(a.normal[k])) for k in range(3)) <= nb, f"ray {i}: device {row[0]}, exact {a}"
    assert decided > n // 2


# ---- build edges ------------------------------------------------------------------------------------------------------------------------------
def layout(kind, n, rng):
    """Centres and half extents of n colliders."""
    size = np.full(n, 0.5)
    if kind == "identical":
        c = np.tile([1.0, 2.0, 3.0], (n, 1))
    elif kind == "collinear":
        c = np.arange(n)[:, None] * np.array([1.5, 0.75, 0.375])
    elif kind == "coplanar":
        m = int(np.ceil(np.sqrt(n)))
        c = np.c_[np.arange(n) % m, np.arange(n) // m, np.zeros(n)] * 1.5
    elif kind == "exponential":   # one axis, spacing growing geometrically: the Morton codes crowd into the first cells
        c = np.c_[np.expm1(np.arange(n) * (80.0 / max(n, 1))), np.zeros(n), np.zeros(n)]
    elif kind == "clusters":      # scales 1e-3 and 1e4 in one scene
        half = n // 2
        c = np.r_[rng.uniform(-1e-3, 1e-3, (half, 3)), rng.uniform(-1e4, 1e4, (n - half, 3)) + [5e4, 0, 0]]
        size = np.r_[np.full(half, 1e-4), np.full(n - half, 1.0)]
    elif kind == "huge":          # f64 centres beyond FLT_MAX: k_sp_morton sees them as inf
        c = np.c_[3.5e38 + np.arange(n) * 4e35, rng.uniform(-1e36, 1e36, (n, 2))]
        size = np.full(n, 1e35)
    else:
        raise ValueError(kind)
    return c, size


def build_scene(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    c, size = layout(kind, n, rng)
    shape = (np.arange(n) % 3 == 2).astype(np.uint8)   # every third a ball
    he = np.where(shape[:, None] == R.SHAPE_BALL, size[:, None] * [1, 0, 0], size[:, None] * rng.uniform(0.3, 1.0, (n, 3)))
    rot = random_unit_quats(rng, n) if n else np.zeros((0, 4))
    cols = dict(entity_index=np.arange(n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=shape, half_extents=he)
    return S.bodies_of(c, rot), cols


BUILD_CASES = ([(32, k, n) for k in ("identical", "collinear", "coplanar", "exponential", "clusters") for n in (1, 2, 3, 255, 256, 257, 8192, 8193)]
               + [(32, k, n) for k in ("collinear", "clusters") for n in (262144, 262145)]
               + [(64, "huge", n) for n in (1, 2, 3, 257, 8193)] + [(64, "clusters", 8193)])


@pytest.mark.parametrize("bits,kind,n", BUILD_CASES)
def test_build_edges(bits, kind, n):
    dt = np.float32 if bits == 32 else np.float64
    bodies, cols = build_scene(kind, n, seed=n)
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    st = sq.stats()
    assert st.valid == 1 and st.colliders == n and st.nodes == 2 * n - 1
    s = R.Snapshot(bodies, cols, None, dt)
    nq = 32 if n > 100_000 else 160
    pos = np.stack(s.pos, 1).astype(float)
    scale = float(np.abs(pos).max()) + 1.0
    o, d, md, solid, _, aim = S.aimed_rays(n + 1, s, nq, 1.0, 1e3 if kind != "huge" else 1e37)
    rng = np.random.default_rng(n)
    ext = np.abs(rng.normal(size=(nq, 3))) * (0.5 if kind != "huge" else 1e35)
    check_queries(sq, s, o, d, md, solid, aim, aim - ext, aim + ext, ks=(8,), chunk=4 if n > 100_000 else 16)
    if n >= 255 and kind not in ("identical",):
        sq.point_intersections(aim, 8)
        per_query = sq.stats().leaves_visited / nq
        assert per_query < n / 4, f"{per_query:.0f} exact tests per point query of {n} colliders (scale {scale:.3g}): the tree does not cull"


def test_empty_collider_table():
    """n = 0: either the upload refuses it cleanly or the queries all miss."""
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    bodies = S.bodies_of(np.zeros((1, 3)), [S.IDENTITY])
    w.bodies_upload(**bodies)
    cols = dict(entity_index=np.zeros(0, np.uint32), body=np.zeros(0, np.int32), shape=np.zeros(0, np.uint8), half_extents=np.zeros((0, 3)))
    try:
        w.colliders_upload(**cols)
    except F.AvnError as e:
        assert e.status in (1, 6), e
        return
    sq = SpatialQuery(w)
    sq.update()
    st = sq.stats()
    assert st.colliders == 0 and st.nodes == 0
    o, d = np.zeros((3, 3)), np.tile([1.0, 0, 0], (3, 1))
    assert (sq.cast_rays(o, d)["collider"] == MISS).all()
    assert (sq.ray_hits(o, d, 4)[1] == 0).all()
    assert (sq.point_intersections(o, 4)[1] == 0).all() and (sq.aabb_intersections(o - 1, o + 1, 4)[1] == 0).all()


# ---- query edges ------------------------------------------------------------------------------------------------------------------------------
def edge_scene():
    """A row of 100 unit cubes on y = 10 (more hits than AVN_SPATIAL_MAX_HITS), a unit cube at the origin, a zero-extent cuboid at
    (3, 0, 0), a zero-radius ball at (5, 0, 0), a plate (zero thickness) at (7, 0, 0) and a rotated cube."""
    row = np.c_[np.arange(100) * 1.0, np.full(100, 10.0), np.zeros(100)]
    pos = np.r_[row, [[0, 0, 0], [3, 0, 0], [5, 0, 0], [7, 0, 0], [0, -4, 0]]]
    rot = np.tile(S.IDENTITY, (len(pos), 1))
    rot[-1] = random_unit_quats(np.random.default_rng(1), 1)[0]
    he = np.r_[np.full((100, 3), 0.5), [[0.5, 0.5, 0.5], [0, 0, 0], [0, 0, 0], [0, 0.5, 0.5], [0.5, 0.5, 0.5]]]
    shape = np.zeros(len(pos), np.uint8)
    shape[102] = R.SHAPE_BALL
    cols = dict(entity_index=np.arange(len(pos), dtype=np.uint32), body=np.arange(len(pos), dtype=np.int32), shape=shape, half_extents=he)
    return S.bodies_of(pos, rot), cols


def edge_rays():
    o, d = [], []
    for y in (10.0, 10.5, 10.25):                       # along the row: 100 hits, on a face line, inside
        o.append([-5, y, 0]); d.append([1, 0, 0])
    for x0 in (-0.5, 0.5):                              # starting exactly on the faces of the origin cube, in, out and along
        for dd in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1]):
            o.append([x0, 0.25, 0]); d.append(dd)
    o.append([0.5, 0.5, 0.5]); d.append([1, 0, 0])      # on a corner
    for x in (3.0, 5.0, 7.0):                           # through the zero-extent cuboid, the zero ball, the plate: head on and from the side
        o.append([x, -3, 0]); d.append([0, 1, 0])
        o.append([x, 0, -3]); d.append([0, 0, 1])
    o.append([-2, 0, 0]); d.append([1, 0, 0])            # along the axis through all of them
    o.append([0, -4, 0]); d.append([0, 1, 0])           # from the rotated cube's centre
    return np.array(o, float), np.array(d, float)


@pytest.mark.parametrize("bits", [32, 64])
def test_query_edges(bits):
    dt = np.float32 if bits == 32 else np.float64
    bodies, cols = edge_scene()
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    s = R.Snapshot(bodies, cols, None, dt)
    o, d = edge_rays()
    k = len(o)
    for md in (np.inf, 0.0, -1.0, 4.5):
        for solid in (0, 1):
            mdv, sv = np.full(k, md), np.full(k, solid, np.uint8)
            closest = check_queries(sq, s, o, d, mdv, sv, o, o - 0.25, o + 0.25, ks=(1, 64))
            if md < 0:
                assert (closest["collider"] == MISS).all()
    h, c = sq.ray_hits(o[:1], d[:1], 64)
    assert c[0] == 100 and (h[0]["collider"] != MISS).all() and list(h[0]["collider"][:3]) == [0, 1, 2]
    # 0, 1, 63 and 65 queries; cap = 0 (counts only)
    rng = np.random.default_rng(bits)
    for n in (0, 1, 63, 65):
        p = rng.uniform([-2, -5, -1], [100, 11, 1], (n, 3))
        dirs = rng.normal(size=(n, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True) if n else 1
        check_queries(sq, s, p, dirs, np.full(n, np.inf), np.ones(n, np.uint8), p, p - 1, p + 1, ks=(1, 64))
        for cap in (0, 1):
            ids, cnt = sq.point_intersections(p, cap)
            ri, rc = R.point_intersections(s, p, cap)
            assert ids.shape == (n, cap) and np.array_equal(cnt, rc) and np.array_equal(ids, ri)
            ids, cnt = sq.aabb_intersections(p - 1, p + 1, cap)
            ri, rc = R.aabb_intersections(s, p - 1, p + 1, cap)
            assert ids.shape == (n, cap) and np.array_equal(cnt, rc) and np.array_equal(ids, ri)
    # two identical cuboids at one pose (colliders 1 and 2) with a third (collider 0) behind them, 65 rays (a second, partial wave): the
    # closest hit is the lower index of the two at the equal distance, whichever of them the traversal reaches first
    pos = np.array([[3.0, 0, 0], [0, 0, 0], [0, 0, 0]])
    cols = dict(entity_index=np.arange(3, dtype=np.uint32), body=np.arange(3, dtype=np.int32), shape=np.zeros(3, np.uint8), half_extents=np.full((3, 3), 0.5))
    bodies = S.bodies_of(pos, np.tile(S.IDENTITY, (3, 1)))
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    s = R.Snapshot(bodies, cols, None, dt)
    o = np.c_[np.full(65, -5.0), rng.uniform(-0.4, 0.4, (65, 2))]
    d = np.tile([1.0, 0, 0], (65, 1))
    closest = check_queries(sq, s, o, d, np.full(65, np.inf), np.ones(65, np.uint8), o, o - 1, o + 1, ks=(1, 3))
    assert (closest["collider"] == 1).all() and (sq.cast_rays(o, d)["collider"] == 1).all()
    assert (sq.cast_rays(o + [10.0, 0, 0], -d)["collider"] == 0).all()


# ---- non-finite ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_non_finite_colliders_and_queries(bits):
    dt = np.float32 if bits == 32 else np.float64
    bodies, cols, tf = S.far_scene(100 + bits, n_bodies=40)
    bad_pos = {3: np.nan, 11: np.inf, 20: -np.inf}
    bad_rot = (7, 29)
    sick = {k: np.array(v, copy=True) for k, v in bodies.items()}
    for b, v in bad_pos.items():
        sick["position"][b, b % 3] = v
    for b in bad_rot:
        sick["rotation"][b, 1] = np.nan
    bad_bodies = np.array(sorted(set(bad_pos) | set(bad_rot)))
    bad_cols = np.isin(cols["body"], bad_bodies)
    assert bad_cols.sum() >= 5 and (np.asarray(cols["shape"])[bad_cols] == R.SHAPE_BALL).any()
    ones = np.ones(len(cols["shape"]), np.uint32)
    w_sick = world_of(bits, sick, dict(cols, memberships=ones), tf)
    w_ref = world_of(bits, bodies, dict(cols, memberships=np.where(bad_cols, 0, ones).astype(np.uint32)), tf)
    sqs, sqr = SpatialQuery(w_sick), SpatialQuery(w_ref)
    sqs.update(); sqr.update()
    s = R.Snapshot(sick, dict(cols, memberships=ones), tf, dt)
    assert not s.candidates()[bad_cols].any()
    o, d, md, solid, _, aim = S.aimed_rays(bits, R.Snapshot(bodies, cols, tf, dt), 512, 1.0, 100.0)
    lo, hi = aim - 0.7, aim + 0.7
    check_queries(sqs, s, o, d, md, solid, aim, lo, hi, ks=(1, 8))
    same_records(sqs.cast_rays(o, d, md, solid), sqr.cast_rays(o, d, md, solid), "non-finite colliders = memberships 0: cast_rays")
    for a, b in zip(sqs.ray_hits(o, d, 8, md, solid), sqr.ray_hits(o, d, 8, md, solid)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "non-finite colliders = memberships 0: ray_hits"
    same_ids(sqs.point_intersections(aim, 8), sqr.point_intersections(aim, 8), "non-finite colliders = memberships 0: points")
    same_ids(sqs.aabb_intersections(lo, hi, 8), sqr.aabb_intersections(lo, hi, 8), "non-finite colliders = memberships 0: aabbs")
    everything = sqs.aabb_intersections(np.full((1, 3), -1e30), np.full((1, 3), 1e30), 256)
    assert everything[1][0] == (~bad_cols).sum() and not np.isin(everything[0][0], np.nonzero(bad_cols)[0]).any()
    # non-finite queries: a miss / count 0 without traversing
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]])
    good = np.tile(np.stack(s.pos, 1)[np.nonzero(~bad_cols)[0][0]].astype(float), (4, 1))
    unit = np.tile([1.0, 0, 0], (4, 1))
    for oo, dd in ((bad, unit), (good, bad)):
        assert (sqs.cast_rays(oo, dd)["collider"] == MISS).all()
        h, c = sqs.ray_hits(oo, dd, 4)
        assert (c == 0).all() and (h["collider"] == MISS).all()
    assert sqs.stats().leaves_visited == 0 and sqs.stats().nodes_visited == 0
    assert (sqs.point_intersections(bad, 4)[1] == 0).all()
    assert (sqs.aabb_intersections(bad, good + 1, 4)[1] == 0).all() and (sqs.aabb_intersections(good - 1, bad, 4)[1] == 0).all()
    assert (sqs.aabb_intersections(np.full((1, 3), -np.inf), np.full((1, 3), np.inf), 4)[1] == 0).all()
    assert sqs.stats().nodes_visited == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_single_non_finite_collider(bits):
    bodies = S.bodies_of([[np.nan, 0, 0]], [S.IDENTITY])
    cols = dict(entity_index=np.array([1], np.uint32), body=np.array([0], np.int32), shape=np.array([R.SHAPE_BALL], np.uint8), half_extents=np.array([[1.0, 0, 0]]))
    w = world_of(bits, bodies, cols)
    sq = SpatialQuery(w)
    sq.update()
    assert sq.stats().nodes == 1
    o, d = np.array([[-5.0, 0, 0], [0, 0, 0]]), np.array([[1.0, 0, 0], [1.0, 0, 0]])
    assert (sq.cast_rays(o, d)["collider"] == MISS).all()
    assert (sq.ray_hits(o, d, 4)[1] == 0).all()
    assert (sq.point_intersections(o, 4)[1] == 0).all()
    assert (sq.aabb_intersections(np.full((1, 3), -1e30), np.full((1, 3), 1e30), 4)[1] == 0).all()
