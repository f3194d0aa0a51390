"""CPU: the shape-cast restatement (tests/spatial_cast_reference.py, which the device is compared with bit for bit on the GPU) against answers
worked out by hand, against exact rational geometry (tests/spatial_cast_exact_geometry.py), and the tree's padding property."""
import numpy as np
import pytest

from compound_helpers import compound_scene
from helpers import random_unit_quats
import spatial_cast_exact_geometry as XC
import spatial_cast_reference as CR
import spatial_query_reference as R
import spatial_scenes as SC

MISS = R.MISS
ID = [0.0, 0.0, 0.0, 1.0]
S2, S3 = np.sqrt(0.5), np.sqrt(1.0 / 3.0)
DTYPES = [np.float32, np.float64]


def snap(dt, shape, he, pos, rot=None):
    n = len(shape)
    rot = np.tile(ID, (n, 1)) if rot is None else np.asarray(rot, float)
    cols = dict(body=np.arange(n), half_extents=np.asarray(he, float), shape=np.asarray(shape), entity_index=np.arange(n) + 100)
    return R.Snapshot(dict(position=np.asarray(pos, float), rotation=rot), cols, None, dt)


def one(dt, col, query, d, md=np.inf):
    """The record of one cast against one collider: col = (shape, he, pos[, rot]), query = (shape, he, pos[, rot])."""
    s = snap(dt, [col[0]], [col[1]], [col[2]], None if len(col) < 4 else [col[3]])
    d = np.asarray(d, float); d = d / np.linalg.norm(d)
    return CR.cast_shapes(s, [query[0]], [query[1]], [query[2]], [ID if len(query) < 4 else query[3]], [d], [md])[0]


def close(a, b, dt, k=64):
    return np.allclose(np.asarray(a, float), np.asarray(b, float), rtol=0, atol=k * np.finfo(dt).eps * 8)


CUBE1 = (0, [1, 1, 1])          # a cube of half extent 1 ("unit" in the hand-computed cases below)
BALL1 = (1, [1, 0, 0])


@pytest.mark.parametrize("dt", DTYPES)
def test_hand_computed_answers(dt):
    # a unit ball from the origin along +x at a cube of half extent 1 centred at x = 5: the face at x = 4, the ball's front at x = 1
    r = one(dt, CUBE1 + ([5, 0, 0],), BALL1 + ([0, 0, 0],), [1, 0, 0])
    assert r["collider"] == 0 and r["entity"] == 100 and r["distance"] == 3
    assert list(r["point1"]) == [4, 0, 0] and list(r["point2"]) == [4, 0, 0] and list(r["normal1"]) == [-1, 0, 0] and list(r["normal2"]) == [1, 0, 0]
    # ball / ball head-on: centres 6 apart, radii 1 and 0.5
    r = one(dt, BALL1 + ([6, 0, 0],), (1, [0.5, 0, 0], [0, 0, 0]), [1, 0, 0])
    assert r["distance"] == 4.5 and list(r["point1"]) == [5, 0, 0] and list(r["point2"]) == [5, 0, 0] and list(r["normal1"]) == [-1, 0, 0]
    # ball / ball grazing: the centre's line passes at 1.5 = r1 + r2 exactly (a hit at the tangent point), at 1.5 + 1e-3 a miss
    r = one(dt, BALL1 + ([6, 1.5, 0],), (1, [0.5, 0, 0], [0, 0, 0]), [1, 0, 0])
    assert r["collider"] == 0 and close(r["distance"], 6, dt) and close(r["normal1"], [0, -1, 0], dt)
    assert one(dt, BALL1 + ([6, 1.501, 0],), (1, [0.5, 0, 0], [0, 0, 0]), [1, 0, 0])["collider"] == MISS
    # a unit ball onto the cube's edge x = y = 1 at 45 degrees: the centre stops sqrt(2) + 1 from the origin, having started at 5 sqrt(2)
    r = one(dt, CUBE1 + ([0, 0, 0],), BALL1 + ([5, 5, 0],), [-1, -1, 0])
    assert close(r["distance"], 4 * np.sqrt(2) - 1, dt) and close(r["point1"], [1, 1, 0], dt) and close(r["point2"], [1, 1, 0], dt)
    assert close(r["normal1"], [S2, S2, 0], dt) and close(r["normal2"], [-S2, -S2, 0], dt)
    # ... and onto the corner (1, 1, 1) along the diagonal
    r = one(dt, CUBE1 + ([0, 0, 0],), BALL1 + ([5, 5, 5],), [-1, -1, -1])
    assert close(r["distance"], 4 * np.sqrt(3) - 1, dt) and close(r["point1"], [1, 1, 1], dt) and close(r["normal1"], [S3, S3, S3], dt)
    # the same two with the roles swapped (a cube cast at a ball): the record's sides swap
    r = one(dt, BALL1 + ([5, 5, 5],), CUBE1 + ([0, 0, 0],), [1, 1, 1])
    assert close(r["distance"], 4 * np.sqrt(3) - 1, dt) and close(r["normal1"], [-S3, -S3, -S3], dt) and close(r["normal2"], [S3, S3, S3], dt)
    p = 5 - S3
    assert close(r["point1"], [p, p, p], dt) and close(r["point2"], [p, p, p], dt)
    # cube / cube face-on, the query smaller and off-centre so that its support vertex (+y, +z) lies on the collider's face
    r = one(dt, CUBE1 + ([5, 0, 0],), (0, [0.5, 0.25, 0.25], [0, 0.5, -0.5]), [1, 0, 0])
    assert r["distance"] == 3.5 and list(r["normal1"]) == [-1, 0, 0] and list(r["point1"]) == [4, 0.75, -0.25] and list(r["point2"]) == [4, 0.75, -0.25]
    # parallel faces whose support vertex lies off the other face: the witnesses are clipped to the overlap of the two faces.  A cube of half
    # extent 3 face-on at a cube of half extent 1; then two unit cubes offset by 1.5 in y (faces overlapping for 0.5 <= y <= 1)
    r = one(dt, CUBE1 + ([7, 0, 0],), (0, [3, 3, 3], [0, 0, 0]), [1, 0, 0])
    assert r["distance"] == 3 and list(r["point1"]) == list(r["point2"]) and r["point1"][0] == 6 and abs(r["point1"][1]) <= 1 and abs(r["point1"][2]) <= 1
    r = one(dt, CUBE1 + ([5, 0, 0],), CUBE1 + ([0, 1.5, 0],), [1, 0, 0])
    assert r["distance"] == 3 and list(r["point1"]) == list(r["point2"]) and r["point1"][0] == 4 and 0.5 <= r["point1"][1] <= 1 and abs(r["point1"][2]) <= 1
    # cube / cube edge to edge: the query turned 45 degrees about z, the collider 45 degrees about y, approaching along x.  The query's
    # vertical edge leads at x = +sqrt(2) of its centre, the collider's edge along y faces it at x = 10 - sqrt(2)
    qz = [0, 0, np.sin(np.pi / 8), np.cos(np.pi / 8)]
    qy = [0, np.sin(np.pi / 8), 0, np.cos(np.pi / 8)]
    r = one(dt, CUBE1 + ([10, 0, 0], qy), CUBE1 + ([0, 0, 0], qz), [1, 0, 0])
    assert close(r["distance"], 10 - 2 * np.sqrt(2), dt, 256) and close(r["normal1"], [-1, 0, 0], dt, 256)
    assert close(r["point1"], [10 - np.sqrt(2), 0, 0], dt, 256) and close(r["point2"], [10 - np.sqrt(2), 0, 0], dt, 256)
    # a parallel slide that misses: 2.001 apart sideways, half extents 1 + 1
    assert one(dt, CUBE1 + ([5, 2.001, 0],), CUBE1 + ([0, 0, 0],), [1, 0, 0])["collider"] == MISS
    assert one(dt, CUBE1 + ([5, 1.999, 0],), CUBE1 + ([0, 0, 0],), [1, 0, 0])["distance"] == 3
    # an initial overlap, every pair kind: distance 0, everything else 0
    for col, q in ((CUBE1, CUBE1), (CUBE1, BALL1), (BALL1, CUBE1), (BALL1, BALL1)):
        r = one(dt, col + ([0.5, 0.25, 0],), q + ([0, 0, 0],), [1, 0, 0])
        assert r["collider"] == 0 and r["distance"] == 0 and r.tobytes()[12 if dt == np.float32 else 16:] == bytes(r.dtype.itemsize - (12 if dt == np.float32 else 16))
    # max_distance: inclusive at the exact distance, a miss just below; behind the shape: a miss
    assert one(dt, CUBE1 + ([5, 0, 0],), BALL1 + ([0, 0, 0],), [1, 0, 0], 3.0)["distance"] == 3
    assert one(dt, CUBE1 + ([5, 0, 0],), BALL1 + ([0, 0, 0],), [1, 0, 0], 2.999)["collider"] == MISS
    assert one(dt, CUBE1 + ([5, 0, 0],), BALL1 + ([0, 0, 0],), [-1, 0, 0])["collider"] == MISS
    m = one(dt, CUBE1 + ([5, 0, 0],), CUBE1 + ([0, 0, 0],), [-1, 0, 0])
    assert m["collider"] == MISS and m["entity"] == MISS and m.tobytes()[8:] == bytes(m.dtype.itemsize - 8)


def scene_casts(seed, s, n, he_hi, reach):
    """Casts aimed at colliders from `reach` away: both kinds, a fifth starting inside, a fifth with a finite range."""
    rng = np.random.default_rng(seed)
    pos = np.stack(s.pos, 1).astype(float)
    target = pos[rng.integers(0, s.n, n)]
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(1.0, reach, n)
    dist[: n // 5] = rng.uniform(0, 0.05, n // 5)
    qpos = target - d * dist[:, None] + rng.normal(scale=0.4, size=(n, 3))
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.1, he_hi, (n, 3))
    rot = random_unit_quats(rng, n)
    md = np.full(n, np.inf)
    cut = rng.random(n) < 0.2
    md[cut] = dist[cut] * rng.uniform(0.5, 1.5, cut.sum())
    return shape, he, qpos, rot, d, md


def scenes(dt):
    yield "compound", R.Snapshot(*compound_scene(seed=3, n_bodies=40), dt), 1.5, 6.0
    yield "far", R.Snapshot(*SC.far_scene(7, n_bodies=24, spread=10.0, centre=(3000.0, -2000.0, 1000.0)), dt), 2.0, 12.0


@pytest.mark.parametrize("dt", DTYPES)
def test_padding_property_on_the_leaf_boxes(dt):
    """The tree never culls a pair the exact test accepts: for every (cast, collider) hit, the node test's entry into that collider's leaf
    box is <= the computed distance, and the query's own range never culls it either."""
    for name, s, he_hi, reach in scenes(dt):
        shape, he, qpos, rot, d, md = scene_casts(5, s, 200, he_hi, reach)
        with np.errstate(all="ignore"):
            hit, toi, _, _, _, ok = CR.cast_pairs(s, shape, he, qpos, rot, d, md)
            _, hev, posv, rotv, dv, mdv = CR.cast_valid(shape, he, qpos, rot, d, md, dt)
            centre, hw = CR.cast_box(shape, hev, posv, rotv, dt)
            lo, hi = R.leaf_boxes(s)
            q = lambda t: tuple(x[:, None] for x in t)
            col = lambda t: tuple(x[None, :] for x in t)
            entry = CR.node_entry(q(centre), q(hw), tuple(dv[:, i][:, None] for i in range(3)), col(lo), col(hi), mdv[:, None], dt)
        assert ok.all() and hit.sum() > 300 and (hit & (toi > 0)).sum() > 100, name
        assert not (hit & (entry > toi)).any(), f"{name}: {(hit & (entry > toi)).sum()} hits lie behind their leaf box's entry"


@pytest.mark.parametrize("dt", DTYPES)
def test_zero_radius_ball_casts_agree_with_rays(dt):
    """A ball of radius 0 is a point: its cast answers cast_rays (solid) in collider and, within the band, in distance.  The two paths round
    differently (nalgebra's isometry arithmetic against the ray's conjugate rotation), so this is not a bitwise comparison."""
    eps = np.finfo(dt).eps
    for name, s, he_hi, reach in scenes(dt):
        shape, he, qpos, rot, d, md = scene_casts(9, s, 200, he_hi, reach)
        shape[:] = R.SHAPE_BALL; he[:] = 0
        with np.errstate(all="ignore"):
            cast = CR.cast_shapes(s, shape, he, qpos, rot, d, md)
            ray = R.cast_rays(s, qpos, d, md, np.ones(len(d), np.uint8))
        scale = np.abs(qpos).max(1) + np.abs(np.stack(s.pos, 1)).max() + 2.0 + ray["distance"]
        band = XC.BAND_EPS * eps * scale
        both = (cast["collider"] != MISS) & (ray["collider"] != MISS)
        # the same collider, and a miss exactly where the ray misses.  (Two colliders within the band of each other, or a ray grazing within
        # it, could legitimately answer differently on the two paths; these seeded sets hold no such ray, so the agreement is exact here.)
        assert both.sum() > 100 and np.array_equal(cast["collider"], ray["collider"]), f"{name}: rays {np.nonzero(cast['collider'] != ray['collider'])[0]} differ"
        assert (np.abs(cast["distance"] - ray["distance"])[both] <= band[both]).all(), name


@pytest.mark.parametrize("dt", DTYPES)
def test_nearest_k_is_a_prefix_of_the_sorted_list(dt):
    name, s, he_hi, reach = next(scenes(dt))
    q = scene_casts(13, s, 64, he_hi, reach)
    with np.errstate(all="ignore"):
        closest, many = CR.cast_queries(s, *q[:5], (1, 3, 64), max_distance=q[5])
    full, count = many[64]
    assert count.max() > 3 and count.max() <= 64
    for k in (1, 3):
        rec, cnt = many[k]
        assert np.array_equal(cnt, count) and rec.tobytes() == np.ascontiguousarray(full[:, :k]).tobytes()
    assert closest.tobytes() == np.ascontiguousarray(full[:, 0]).tobytes()
    dist, idx = full["distance"], full["collider"].astype(np.int64)
    for r in range(len(count)):
        m = min(int(count[r]), 64)
        assert (idx[r, m:] == MISS).all() and (np.diff(dist[r, :m]) >= 0).all()
        ties = np.diff(dist[r, :m]) == 0
        assert (np.diff(idx[r, :m])[ties] > 0).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_parallel_faces_turned_about_the_normal(dt):
    """Parallel faces whose edges are NOT parallel: a cuboid of half extent 3 turned 30 degrees about x lands face-on on a cube of half extent
    1 at x = 7.  The header's two rounds of clamps C(Q(C(p))) / Q(point1) are pinned here as documented: the distance and the normal are the
    face contact's, each witness lies on its own shape's contact face, and the two coincide wherever the first clamp already lands in the
    overlap of the two faces (the query's face covering the collider's corner).  Where the overlap is a sliver at the collider's edge they do
    not: point2 is the query face's nearest point to point1, and as the faces do overlap that is nearer than the collider's face is wide
    (2 sqrt(2)); it is NOT within the band, which is the gap the header and DESIGN.md 4.4.6 state."""
    a = np.pi / 12
    turn = [np.sin(a), 0, 0, np.cos(a)]
    c30, s30 = np.cos(np.pi / 6), np.sin(np.pi / 6)
    tol = 64 * np.finfo(dt).eps * 8

    def faces(off):
        r = one(dt, CUBE1 + ([7, 0, 0],), (0, [3, 3, 3], off, turn), [1, 0, 0])
        assert r["collider"] == 0 and r["distance"] == 3 and list(r["normal1"]) == [-1, 0, 0] and list(r["normal2"]) == [1, 0, 0]
        p1, p2 = np.asarray(r["point1"], float), np.asarray(r["point2"], float)
        assert p1[0] == 6 and abs(p1[1]) <= 1 and abs(p1[2]) <= 1                       # on the collider's face
        y, z = p2[1] - off[1], p2[2] - off[2]                                            # ... and on the query's, in its own frame
        assert abs(p2[0] - 6) <= tol and abs(c30 * y + s30 * z) <= 3 + tol and abs(-s30 * y + c30 * z) <= 3 + tol
        return p1, p2

    for off in ([0, 0, 0], [0, 2.5, 0], [0, 3.2, 1.0], [0, 3.5, 2.0], [0, 2.0, 3.4], [0, 3.0, 3.0]):
        p1, p2 = faces(off)
        assert np.abs(p1 - p2).max() <= tol, off
    p1, p2 = faces([0, 3.3, -2.2])
    assert np.linalg.norm(p1 - p2) <= 2 * np.sqrt(2)


# ---- the restatement against exact geometry ---------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v)


def crafted_pairs(seed, n, centre):
    """n (collider, cast) pairs around `centre`, one collider per cast: balls onto faces, edges and corners of cuboids (both roles), cuboid
    pairs with random, equal and quarter-turned rotations, ball pairs (some grazing within 1 %); an eighth start overlapping, an eighth are aimed past the collider,
    a fifth have a finite range around the distance."""
    rng = np.random.default_rng(seed)
    cs, ch, cp, cr = [], [], [], []          # collider shape, half extents, position, rotation
    qs, qh, qp, qr, qd, md = [], [], [], [], [], []
    for i in range(n):
        kind = ("ball-cuboid", "cuboid-ball", "cuboid-cuboid", "cuboid-cuboid", "parallel", "ball-ball")[i % 6]
        pos = np.asarray(centre, float) + rng.uniform(-3, 3, 3)
        rot = random_unit_quats(rng, 1)[0]
        he = rng.uniform(0.2, 1.5, 3)
        r = rng.uniform(0.1, 1.0)
        dist = rng.uniform(0.5, 6.0)
        mode = rng.random()                  # < 1/8 overlapping at the start, < 1/4 aimed past, else aimed at the feature
        if kind in ("ball-cuboid", "cuboid-ball"):
            # the cuboid's frame: a feature point and a normal inside that feature's cone
            sg = rng.choice([-1.0, 1.0], 3)
            feat = i // 6 % 3                # 0 face, 1 edge, 2 corner
            free = rng.permutation(3)
            w = np.zeros(3); local = sg * he
            if feat == 0:
                w[free[0]] = 1; local[free[1]] *= rng.uniform(-0.8, 0.8); local[free[2]] *= rng.uniform(-0.8, 0.8)
            elif feat == 1:
                a = rng.uniform(0.2, np.pi / 2 - 0.2); w[free[0]] = np.cos(a); w[free[1]] = np.sin(a); local[free[2]] *= rng.uniform(-0.8, 0.8)
            else:
                w = _unit(rng.uniform(0.3, 1.0, 3))
            nl = sg * w
            dl = _unit(-nl + rng.normal(scale=0.15, size=3))
            to_w = lambda v: np.array(R.qrot(tuple(rot), tuple(v), np.float64))
            impact = pos + to_w(local + nl * r)               # the ball's centre at the impact
            d = to_w(dl)
            if mode < 0.125:
                dist = -rng.uniform(0.05, 0.5) * r
            start = impact - d * dist + (to_w(np.cross(dl, nl) if feat else _unit(np.cross(dl, rng.normal(size=3)))) * 4.0 if 0.125 <= mode < 0.25 else 0)
            if kind == "ball-cuboid":
                cs.append(0); ch.append(he); cp.append(pos); cr.append(rot)
                qs.append(1); qh.append([r, 0, 0]); qp.append(start); qr.append(random_unit_quats(rng, 1)[0]); qd.append(d)
            else:                            # the cuboid is cast at the ball: the same geometry seen from the ball
                cs.append(1); ch.append([r, 0, 0]); cp.append(start); cr.append(random_unit_quats(rng, 1)[0])
                qs.append(0); qh.append(he); qp.append(pos); qr.append(rot); qd.append(-d)
        else:
            d = _unit(rng.normal(size=3))
            if kind == "ball-ball":
                cs.append(1); ch.append([r, 0, 0]); qs.append(1); qh.append([rng.uniform(0.1, 1.0), 0, 0]); qrot = random_unit_quats(rng, 1)[0]
                reach = r + qh[-1][0]
            else:
                cs.append(0); ch.append(he); qs.append(0); qh.append(rng.uniform(0.2, 1.5, 3))
                if kind == "parallel":       # the same rotation, or a quarter turn about a local axis composed onto it
                    turn = [[0, 0, 0, 1.0], [np.sqrt(0.5), 0, 0, np.sqrt(0.5)], [0, np.sqrt(0.5), 0, np.sqrt(0.5)]][i // 6 % 3]
                    qrot = np.array(R.qmul(tuple(rot), tuple(turn), np.float64))
                else:
                    qrot = random_unit_quats(rng, 1)[0]
                reach = np.linalg.norm(he) * 0.6 + np.linalg.norm(qh[-1]) * 0.6
            cp.append(pos); cr.append(rot); qr.append(qrot); qd.append(d)
            side = _unit(np.cross(d, rng.normal(size=3)))
            if mode < 0.125:
                qp.append(pos + side * rng.uniform(0, 0.3) * reach)
            elif mode < 0.25:
                qp.append(pos - d * (dist + reach) + side * reach * 4.0)
            elif mode < 0.4 and kind == "ball-ball":     # grazing: the centre's line within +-1 % of the sum of the radii
                qp.append(pos - d * (dist + reach) + side * reach * (1 + rng.uniform(-0.01, 0.01)))
            else:
                qp.append(pos - d * (dist + reach) + side * rng.uniform(0, 0.5) * reach)
        md.append(np.inf if rng.random() > 0.2 else abs(dist) * rng.uniform(0.5, 1.5))
    A = lambda x, t=float: np.asarray(x, t)
    return (A(cs, np.uint8), A(ch), A(cp), A(cr)), (A(qs, np.uint8), A(qh), A(qp), A(qr), A(qd), A(md))


def pair_records(dt, cols, q):
    """The restatement's record of cast i against collider i alone."""
    cshape, che, cpos, crot = cols
    s = snap(dt, cshape, che, cpos, crot)
    with np.errstate(all="ignore"):
        hit, toi, p1, p2, n1, ok = CR.cast_pairs(s, *q)
    i = np.arange(len(cshape))
    assert ok.all()
    return hit[i, i], toi[i, i], np.stack([x[i, i] for x in p1], 1), np.stack([x[i, i] for x in p2], 1), np.stack([x[i, i] for x in n1], 1)


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (300.0, -200.0, 100.0)], ids=["origin", "far"])
@pytest.mark.parametrize("dt", DTYPES)
def test_restatement_against_exact_geometry(dt, centre):
    bits = 32 if dt == np.float32 else 64
    n = 240
    cols, q = crafted_pairs(17, n, centre)
    rd = lambda a: np.asarray(a, float).astype(dt).astype(float)     # the values the world holds
    cols = (cols[0],) + tuple(rd(a) for a in cols[1:])
    q = (q[0],) + tuple(rd(a) for a in q[1:])
    hit, toi, p1, p2, n1 = pair_records(dt, cols, q)
    classes = dict.fromkeys(XC.CLASSES, 0)
    undecided, worst_d, worst_w, checked_w, parallel = 0, 0.0, 0.0, 0, 0
    for i in range(n):
        col = XC.Collider(cols[0][i], cols[1][i], cols[2][i], cols[3][i])
        qs = XC.Shape(q[0][i], q[1][i], q[2][i], q[3][i])
        d, md = q[4][i], q[5][i]
        ex = XC.cast(qs, d, col, md)
        classes[ex.cls] += 1
        _, band = XC.scale_of(bits, qs, col, ex.toi if ex.hit else toi[i])
        dec_hit, dec_start = XC.decided(qs, d, col, md, band)
        if bool(hit[i]) != ex.hit:
            assert dec_hit is None, f"pair {i}: computed hit={hit[i]} exact {ex}, decided {dec_hit}"
            undecided += 1
            continue
        if not ex.hit:
            continue
        if (toi[i] == 0) != ex.overlap:
            assert dec_start is None, f"pair {i}: computed distance {toi[i]} exact {ex}, decided {dec_start}"
            undecided += 1
            continue
        if ex.overlap:
            assert not p1[i].any() and not p2[i].any() and not n1[i].any()
            continue
        bound = XC.distance_bound(band, ex, qs, col)
        err = abs(float(ex.toi) - float(toi[i]))
        worst_d = max(worst_d, err / bound)
        assert err <= bound, f"pair {i} ({ex.cls}): distance {toi[i]} exact {float(ex.toi)}: off by {err / bound:.2f} bounds"
        if dec_hit is None:
            continue
        rec = dict(point1=p1[i], point2=p2[i], normal1=n1[i], distance=toi[i])
        e = {k: float(v) for k, v in XC.witness_errors(rec, qs, d, col).items()}
        wband = (bound + err) / (float(ex.sin2) if ex.sin2 and ex.cls != "parallel-face" else 1.0)
        checked_w += 1
        parallel += ex.cls == "parallel-face"
        worst_w = max(worst_w, e["on1"] / wband, e["on2"] / wband, e["apart"] / (2 * wband), e["separation"] / wband, e["plane1"] / wband, e["plane2"] / wband)
        assert max(e["on1"], e["on2"], e["separation"], e["plane1"], e["plane2"]) <= wband and e["apart"] <= 2 * wband and e["unit"] <= XC.BAND_EPS * np.finfo(dt).eps, \
            f"pair {i} ({ex.cls}): witness errors {e} against {wband}"
    assert parallel >= 10
    print(f"{dt.__name__} {centre}: classes {classes}, undecided {undecided}/{n}, worst distance error {worst_d:.2f} bounds, worst witness error {worst_w:.2f} bounds ({checked_w} checked)")
    assert all(v >= 10 for v in classes.values()), classes
    assert undecided <= 0.02 * n
    assert worst_d <= 1 and worst_w <= 1
    # the recorded figures stay true: a set or a restatement that drifts past four times WORST_OBSERVED has to be looked at and re-recorded
    assert worst_d <= 4 * XC.WORST_OBSERVED["distance"] and worst_w <= 4 * XC.WORST_OBSERVED["witness"]
    assert undecided / n <= XC.WORST_OBSERVED["undecided_fraction"] + 0.02


@pytest.mark.parametrize("dt", DTYPES)
def test_invalid_casts_answer_a_miss(dt):
    """The per-query rule of the header: a kind that is neither Ball nor Cuboid, a negative half extent, a non-finite pose, size, direction or
    AABB, or a NaN max_distance answers a miss; +inf as max_distance is legal and -inf reaches nothing."""
    s = snap(dt, [0], [[1, 1, 1]], [[5, 0, 0]])
    base = dict(shape=1, he=[1.0, 0, 0], pos=[0.0, 0, 0], rot=list(ID), d=[1.0, 0, 0], md=np.inf)
    big = float(np.finfo(dt).max) * 0.9
    cases = [({}, True), (dict(md=3.0), True), (dict(md=-np.inf), False), (dict(md=np.nan), False), (dict(shape=2), False), (dict(he=[-1.0, 0, 0]), False),
             (dict(shape=0, he=[1.0, -0.5, 1.0]), False), (dict(he=[1.0, np.nan, -1.0]), True), (dict(he=[np.inf, 0, 0]), False), (dict(pos=[np.nan, 0, 0]), False),
             (dict(rot=[0, 0, 0, np.inf]), False), (dict(d=[1.0, np.nan, 0]), False), (dict(d=[np.inf, 0, 0]), False),
             (dict(shape=0, he=[big, 1, 1], pos=[big, 0, 0]), False)]
    q = [dict(base, **c) for c, _ in cases]
    col = lambda k: [x[k] for x in q]
    with np.errstate(all="ignore"):
        closest, many = CR.cast_queries(s, np.array(col("shape"), np.uint8), col("he"), col("pos"), col("rot"), col("d"), (2,), max_distance=col("md"))
    want = np.array([w for _, w in cases])
    assert np.array_equal(closest["collider"] != MISS, want) and np.array_equal(many[2][1] == 1, want)
    assert (closest["distance"][want] == 3).all()
    miss = closest[~want]
    assert miss.tobytes() == miss[:1].tobytes() * len(miss)
