"""CPU: the triangle collider's definitions (tests/triangle_collider_reference.py) against geometry that does not share their algorithm, the
interior-edge rule on a tessellated square, triangle_colliders' adjacency flags, and a mesh scene on the oracle with its triangles hosted."""
import numpy as np
import pytest

import triangle_collider_reference as TR
from avian_amd import scenes
from avian_amd.trimesh import triangle_colliders
from helpers import F, oracle_lib, random_unit_quats

CUB, BALL, CAP, TRI = TR.SHAPE_CUBOID, TR.SHAPE_BALL, TR.SHAPE_CAPSULE, TR.SHAPE_TRIANGLE
COMBOS = [(TRI, BALL), (BALL, TRI), (TRI, CAP), (CAP, TRI), (TRI, CUB), (CUB, TRI)]
N_SAMPLES = 2001
I4 = [0.0, 0.0, 0.0, 1.0]
# The tolerances are those of test_capsule_collider_cpu.py::test_reference_against_sampled_geometry: depths to 1e-12 (plus the sampling bound where a
# segment is sampled), directions and witness points to TOL = 1e-9 (positions are O(10), float64).  That test skips no finite row; neither does this one:
# every row either has the manifold the exact geometry asks for, or has none where the exact geometry says there is none.
TOL = 1e-9
DEPTH_TOL = 1e-12


# ---- exact geometry in float64 that shares nothing with the reference's algorithm -----------------------------------------------------------
def qrot(q, v):
    u = q[..., :3]
    return v + 2.0 * np.cross(u, np.cross(u, v) + q[..., 3:4] * v)


def qinv(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def point_segment(p, a, b):
    d = b - a
    t = np.clip(((p - a) * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0)
    return np.linalg.norm(p - (a + d * t[..., None]), axis=-1)


def point_triangle(p, tri):
    """Exact distance of the points p [k, 3] to the triangle: the distance to its plane where the projection lies inside (three half-plane tests),
    else the smallest distance to the three edges -- not Ericson's region walk."""
    a, b, c = tri
    n = np.cross(b - a, c - a); n = n / np.linalg.norm(n)
    h = (p - a) @ n
    q = p - h[:, None] * n
    inside = np.ones(len(p), bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= ((q - u) @ np.cross(n, v - u)) >= 0.0
    edges = np.minimum(np.minimum(point_segment(p, a, b), point_segment(p, b, c)), point_segment(p, c, a))
    return np.where(inside, np.abs(h), edges)


def world_triangle(v, pos, rot):
    return pos + qrot(np.asarray(rot, np.float64), np.asarray(v, np.float64).reshape(3, 3))


def box_corners(he, pos, rot):
    s = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    return pos + qrot(np.asarray(rot, np.float64), s * he)


def overlap_along(d, tri_w, corners, tri_first):
    """How far the two convex hulls overlap along the unit direction d that points from shape 1 to shape 2 (negative: apart), from supports alone."""
    pt, pb = tri_w @ d, corners @ d
    return (pt.max() - pb.min()) if tri_first else (pb.max() - pt.min())


def expected_cuboid(tri_w, he, po, ro, pred):
    """What the definition must answer for a triangle (all edges real) and a cuboid, computed another way: in float64 arrays in the box's frame, the
    depth by ENUMERATING the corners a clipped polygon can have (the incident polygon's own corners and every crossing of one of its edges with a side
    plane of the reference feature, kept where they lie over the reference feature) instead of clipping plane after plane.
    None: no manifold -- an axis separates beyond the prediction distance, or no such corner lies within it (a manifold holds only what lies over its
    reference feature, as for two cuboids).  Else (d, depth, least overlap of the 13 axes): d the world direction from the box towards the triangle."""
    inv = qinv(ro)
    v = qrot(inv, tri_w - po)
    edges = [v[(k + 1) % 3] - v[k] for k in range(3)]
    N = np.cross(edges[0], v[2] - v[0]); N /= np.linalg.norm(N)
    E = np.eye(3)
    axes = [("face", i, E[i]) for i in range(3)] + [("tri", 0, N)]
    for k in range(3):
        for i in range(3):
            c = np.cross(E[i], edges[k])
            if np.linalg.norm(c) > 1e-15 * np.linalg.norm(edges[k]):
                axes.append(("edge", k, c / np.linalg.norm(c)))
    best = None
    sat_min = np.inf
    for what, idx, L in axes:
        p = v @ L
        rb = np.abs(L) @ he
        sp, sm = p.min() - rb, -p.max() - rb
        sep, d = (sp, L) if sp >= sm else (sm, -L)
        if sep > pred:
            return None
        sat_min = min(sat_min, -sep)
        if what == "face":
            pd = v @ d
            low = v[pd == pd.min()]
            if len(low) < 3 and not any(all(abs(x[j]) <= he[j] for j in range(3) if j != idx) for x in low):
                continue   # the triangle's lowest feature lies beside the box face: it carries no contact
        if what == "edge" and v[(idx + 2) % 3] @ d < v[idx] @ d:
            continue       # the vertex opposite to the edge is lower along the axis: the edge carries no contact
        if best is None or sep > best[0]:
            best = (sep, d, what, idx)
    sep, d, what, idx = best
    tol = 1e-12
    if what == "edge":
        dists = [sep]
    elif what == "face":
        sg = 1.0 if d[idx] > 0 else -1.0
        others = [j for j in range(3) if j != idx]
        cand = list(v)
        for k in range(3):
            for j in others:
                for h in (-he[j], he[j]):
                    a, b = v[k][j] - h, v[(k + 1) % 3][j] - h
                    if a * b < 0.0:
                        cand.append(v[k] + edges[k] * (a / (a - b)))
        dists = [sg * x[idx] - he[idx] for x in cand if all(abs(x[j]) <= he[j] + tol for j in others)]
    else:
        ax = int(np.argmax(np.abs(d)))   # the box's face towards the triangle
        sg = 1.0 if d[ax] > 0 else -1.0
        o1, o2 = [j for j in range(3) if j != ax]
        quad = []
        for s1_, s2_ in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
            x = np.zeros(3); x[ax] = sg * he[ax]; x[o1] = s1_ * he[o1]; x[o2] = s2_ * he[o2]
            quad.append(x)
        planes = [(np.cross(N, edges[k]), v[k]) for k in range(3)]
        cand = list(quad)
        for m_ in range(4):
            P, Q = quad[m_], quad[(m_ + 1) % 4]
            for mk, vk in planes:
                a, b = (P - vk) @ mk, (Q - vk) @ mk
                if a * b < 0.0:
                    cand.append(P + (Q - P) * (a / (a - b)))
        dists = [d @ (v[0] - x) for x in cand if all((x - vk) @ mk >= -tol for mk, vk in planes)]
    dists = [x for x in dists if x <= pred]
    if not dists:
        return None
    return qrot(np.asarray(ro, np.float64), d), -min(dists), sat_min


def segment_crosses_triangle(a, b, tri):
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    da, db = (a - tri[0]) @ n, (b - tri[0]) @ n
    if da * db >= 0.0:
        return False
    x = a + (b - a) * (da / (da - db))
    return all(((x - u) @ np.cross(n, v - u)) >= 0.0 for u, v in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])))


# ---- samplers ----------------------------------------------------------------------------------------------------------------------------------
def random_triangles(rng, n):
    """Local triangles with edges of 0.4 .. 2.5 and no angle under ~8 degrees (the sampler keeps the reference away from the degenerate triangles the
    upload refuses, so no row has to be skipped)."""
    out = np.zeros((n, 9))
    for i in range(n):
        while True:
            v = rng.uniform(-1.2, 1.2, (3, 3))
            e = np.array([v[1] - v[0], v[2] - v[1], v[0] - v[2]])
            l = np.linalg.norm(e, axis=1)
            area2 = np.linalg.norm(np.cross(e[0], -e[2]))
            if l.min() > 0.4 and area2 > 0.15 * l.max() ** 2:
                break
        out[i] = v.reshape(9)
    return out


def random_pairs(rng, k1, k2, n):
    """Random poses from far apart to deep overlap: (shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction, vertices1, vertices2, flags1, flags2)."""
    def he(kind):
        h = rng.uniform(0.1, 1.0, (n, 3))
        if kind == CAP:
            h[:, 0] = rng.uniform(0.05, 0.4, n); h[:, 2] = 0.0
        if kind == TRI:
            h[:] = 0.0
        return h
    sep = rng.uniform(0.0, 2.0, (n, 1)) * random_unit_quats(rng, n)[:, :3]
    base = rng.uniform(-5, 5, (n, 3))
    flags = lambda: np.full(n, 7, np.uint8)
    return (np.full(n, k1), he(k1), base, random_unit_quats(rng, n), np.full(n, k2), he(k2), base + sep, random_unit_quats(rng, n), rng.uniform(0.0, 0.3, n),
            random_triangles(rng, n), random_triangles(rng, n), flags(), flags())


BIG = [-2.0, 0.0, -2.0, -2.0, 0.0, 3.0, 3.0, 0.0, -2.0]      # a large face in the plane y = 0, normal +y; its vertex a = (-2, 0, -2), edge ab along z at x = -2
SMALL = [-0.2, 0.0, -0.2, -0.2, 0.0, 0.3, 0.3, 0.0, -0.2]
UPRIGHT = [-2.0, -2.0, 0.0, 3.0, -2.0, 0.0, -2.0, 3.0, 0.0]  # a face in the plane z = 0, which holds the axis of a capsule standing at z = 0


def constructed_pairs():
    """Constructed cases, float64 rows, each with the triangle as shape 1 and as shape 2."""
    s = np.sqrt(0.5)
    Z90 = [0.0, 0.0, s, s]           # local y -> world -x: a capsule lying along x
    tilt = [np.sin(0.35), 0.0, 0.0, np.cos(0.35)]
    corner = list(np.array([0.3, 0.1, 0.4, 0.86]) / np.linalg.norm([0.3, 0.1, 0.4, 0.86]))
    rows = []

    def both(kind, he, pos, rot, tri, pred, flags=7):
        z9 = tri if kind == TRI else [0.0] * 9   # (the other shape's vertices are not read unless it is a triangle too)
        rows.append((TRI, [0, 0, 0], [0, 0, 0], I4, kind, he, pos, rot, pred, tri, z9, flags, 7))
        rows.append((kind, he, pos, rot, TRI, [0, 0, 0], [0, 0, 0], I4, pred, z9, tri, 7, flags))
    ball, cap, box = [0.3, 0, 0], [0.2, 0.5, 0.0], [0.4, 0.3, 0.5]
    for flags in (7, 0):
        both(BALL, ball, [0.2, 0.25, 0.3], I4, BIG, 0.05, flags)                 # over the face
        both(BALL, ball, [-2.1, 0.2, 0.5], I4, BIG, 0.05, flags)                 # over edge ab
        both(BALL, ball, [-2.1, 0.15, -2.1], I4, BIG, 0.05, flags)               # over vertex a
        both(BALL, ball, [0.2, -0.25, 0.3], I4, BIG, 0.05, flags)                # under the face: the triangle is two-sided
        both(CAP, cap, [0.2, 0.2 + 0.01, 0.3], Z90, BIG, 0.05, flags)            # lying on the face: two points
        both(CAP, cap, [-2.0, 0.15, 0.3], Z90, BIG, 0.05, flags)                 # lying across edge ab: clipped at the edge
        both(CAP, cap, [0.2, 0.6, 0.3], I4, BIG, 0.05, flags)                    # standing on the face
        both(CAP, cap, [0.2, 0.1, 0.3], I4, BIG, 0.05, flags)                    # its core crossing the face
        both(CAP, cap, [-2.15, 0.1, 0.5], tilt, BIG, 0.05, flags)                # beside edge ab
        both(CUB, box, [0.2, 0.3 - 0.01, 0.3], I4, BIG, 0.05, flags)             # flat on a face larger than it
        both(CUB, box, [0.0, 0.3 - 0.01, 0.0], I4, SMALL, 0.05, flags)           # flat on a face smaller than it
        both(CUB, box, [0.2, 0.55, 0.3], corner, BIG, 0.05, flags)               # a corner on the face
        both(CUB, box, [-2.0 - 0.3, 0.25, 0.5], [0.0, 0.0, np.sin(0.4), np.cos(0.4)], BIG, 0.05, flags)   # box edge (along z) beside / along edge ab
        both(CUB, box, [-2.0 - 0.25, 0.3, 0.5], [np.sin(0.3) * s, np.sin(0.3) * s, 0.0, np.cos(0.3)], BIG, 0.05, flags)   # a box edge across edge ab
        both(CUB, box, [-2.0, 0.25, 0.4], I4, BIG, 0.05, flags)                  # straddling edge ab
    both(BALL, ball, [0.2, 0.0, 0.3], I4, BIG, 0.05)                             # centre exactly on the plane: no manifold
    both(CAP, cap, [0.2, 0.0, 0.0], I4, UPRIGHT, 0.05)                           # the core in the triangle's plane: no manifold
    both(CUB, box, [0.2, 0.0, 0.3], I4, BIG, 0.05)                               # centre on the plane: deep overlap
    both(BALL, ball, [0.2, 0.3 + 0.5, 0.3], I4, BIG, 0.5)                        # prediction exactly at the acceptance boundary
    both(TRI, [0, 0, 0], [0.1, 0.05, 0.1], I4, BIG, 0.5)                         # two triangles: no manifold (not built)
    cols = list(zip(*rows))
    A = lambda k, dt=np.float64: np.array(cols[k], dt)
    return (A(0, np.int64), A(1), A(2), A(3), A(4, np.int64), A(5), A(6), A(7), A(8), A(9), A(10), A(11, np.uint8), A(12, np.uint8))


def _swap(b):
    return (b[4], b[5], b[6], b[7], b[0], b[1], b[2], b[3], b[8], b[10], b[9], b[12], b[11])


def _check_against_exact_geometry(batch, label):
    """Every row with all flags set: the manifold's normal and deepest penetration against the exact geometry above.  Returns the manifolds seen."""
    m, ms = TR.manifolds(*batch, np.float64), TR.manifolds(*_swap(batch), np.float64)
    s1, he1, p1, r1, s2, he2, p2, r2, pred, v1, v2, f1, f2 = batch
    n_manifolds = 0
    for i in range(len(s1)):
        k1, k2 = int(s1[i]), int(s2[i])
        if k1 == TRI and k2 == TRI:
            assert m["point_count"][i] == 0
            continue
        tri_first = k1 == TRI
        if (f1[i] if tri_first else f2[i]) != 7:
            continue   # (the interior-edge rule has its own test)
        tri_w = world_triangle(v1[i], p1[i], r1[i]) if tri_first else world_triangle(v2[i], p2[i], r2[i])
        ko, heo, po, ro = (k2, he2[i], p2[i], r2[i]) if tri_first else (k1, he1[i], p1[i], r1[i])
        pc = int(m["point_count"][i])
        assert pc == ms["point_count"][i], f"{label} row {i}: swapped point count"
        nrm = m["normal"][i]
        pen = m["penetration"][i, :pc]
        to_other = 1.0 if tri_first else -1.0   # nrm * to_other points from the triangle towards the other shape
        if ko == CUB:
            corners = box_corners(heo, po, ro)
            exp = expected_cuboid(tri_w, heo, po, ro, pred[i])
            if pc == 0:
                assert exp is None, f"{label} row {i}: no manifold, expected depth {exp}"
                continue
            assert exp is not None, f"{label} row {i}: a manifold where a separating axis or an empty clipped polygon was expected"
            n_manifolds += 1
            assert abs(np.linalg.norm(nrm) - 1.0) < 1e-12
            deepest = pen.max()
            d_exp, depth_exp, sat_min = exp
            assert np.allclose(nrm * to_other, -d_exp, atol=TOL, rtol=0), f"{label} row {i}: normal {nrm} vs the expected axis {d_exp}"
            assert abs(deepest - depth_exp) <= DEPTH_TOL, f"{label} row {i}: depth {deepest} vs the deepest corner over the reference feature {depth_exp}"
            # no point is deeper than the hulls overlap along the normal, from supports alone
            assert deepest <= overlap_along(nrm, tri_w, corners, tri_first) + DEPTH_TOL, f"{label} row {i}: a point deeper than the hulls overlap"
            # the 13 axes are all there is: no direction whatever has a smaller overlap than the least of theirs (overlapping hulls)
            if sat_min > 0.0:
                d = np.random.default_rng(i).normal(size=(4000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
                pt, pb = tri_w @ d.T, corners @ d.T
                ov = (pt.max(0) - pb.min(0)) if tri_first else (pb.max(0) - pt.min(0))
                assert sat_min <= ov.min() + DEPTH_TOL, f"{label} row {i}: a direction with a smaller overlap than any of the 13 axes"
        else:
            r = float(heo[0])
            if ko == BALL:
                d_s, bound, crossing = point_triangle(po[None], tri_w)[0], 0.0, False
                core = po[None]
            else:
                t = np.linspace(-1.0, 1.0, N_SAMPLES)[:, None]
                core = po + qrot(np.asarray(ro), t * np.array([0.0, heo[1], 0.0]))
                d_s, bound = point_triangle(core, tri_w).min(), 2.0 * heo[1] / (2.0 * (N_SAMPLES - 1))
                crossing = segment_crosses_triangle(core[0], core[-1], tri_w)
            if pc == 0:
                assert d_s - r > pred[i] - bound - 1e-9 or d_s <= bound + 1e-9, f"{label} row {i}: no manifold at core distance {d_s}"
                continue
            n_manifolds += 1
            assert abs(np.linalg.norm(nrm) - 1.0) < 1e-12
            deepest = pen.max()
            if crossing:
                assert deepest >= r - DEPTH_TOL, f"{label} row {i}: a crossing core penetrates by at least the radius"
            else:
                assert d_s - bound - r - DEPTH_TOL <= -deepest <= d_s - r + DEPTH_TOL, f"{label} row {i}: depth {deepest} vs exact core distance {d_s}"
                # the normal: stepping the deepest point's core point against it approaches the triangle
                k = int(np.argmax(pen))
                surf = p1[i] + m["anchor1"][i, k]
                core_pt = surf + nrm * to_other * (r - pen[k] * 0.5) if not tri_first else surf + nrm * (-pen[k] * 0.5 + r)
                assert abs(point_triangle(core_pt[None], tri_w)[0] - (r - pen[k])) <= TOL or pc == 2, f"{label} row {i}: the point's own depth"
                if ko == BALL:
                    foot = po - nrm * to_other * d_s   # the centre's foot along the normal
                    assert point_triangle(foot[None], tri_w)[0] <= TOL, f"{label} row {i}: the normal does not point from the closest point to the centre"
        assert np.allclose(ms["normal"][i], -nrm, atol=TOL, rtol=0), f"{label} row {i}: swapping the shapes negates the normal"
        assert abs(ms["penetration"][i, :pc].max() - pen.max()) <= DEPTH_TOL, f"{label} row {i}: swapping keeps the depth"
        for k in range(pc):
            assert np.allclose(m["anchor2"][i, k], m["anchor1"][i, k] + (p1[i] - p2[i]), atol=1e-12, rtol=0)
        ids = [(int(m["feature_id1"][i, k]), int(m["feature_id2"][i, k])) for k in range(pc)]
        assert len(set(ids)) == pc, f"{label} row {i}: the points have distinct feature ids {ids}"
    return n_manifolds


@pytest.mark.parametrize("k1,k2", COMBOS)
def test_reference_against_exact_geometry(k1, k2):
    """2 000 random pairs per kind combination in float64, all flags set."""
    rng = np.random.default_rng(200 + 10 * k1 + k2)
    assert _check_against_exact_geometry(random_pairs(rng, k1, k2, 2000), f"{k1}-{k2}") > 300


def test_reference_on_the_constructed_cases():
    b = constructed_pairs()
    assert _check_against_exact_geometry(b, "constructed") > 20
    m = TR.manifolds(*b, np.float64)
    s1, s2, pc = b[0], b[4], m["point_count"]
    other = np.where(s1 == TRI, s2, s1)
    assert ((other == CAP) & (pc == 2)).sum() >= 4, "a capsule lying on a face gets two points"
    assert ((other == CUB) & (pc == 4)).sum() >= 4 and ((other == CUB) & (pc == 3)).sum() >= 2, "a cuboid flat on a larger face gets its 4 corners, on a smaller one the face's 3"
    assert ((other == CUB) & (pc == 1)).sum() >= 2, "an edge - edge contact is one point"
    centre_on_plane = [i for i in range(len(pc)) if (other[i] == BALL and b[2][i][1] == 0.0 and b[6][i][1] == 0.0) or (other[i] == CAP and b[2][i][2] == 0.0 and b[6][i][2] == 0.0)]
    assert len(centre_on_plane) == 4 and (pc[centre_on_plane] == 0).all()
    assert (pc[(s1 == TRI) & (s2 == TRI)] == 0).all()
    # each case with the triangle as shape 1 and as shape 2: the same points, the normal negated
    for i in range(0, len(pc), 2):
        assert pc[i] == pc[i + 1] and np.allclose(m["normal"][i], -m["normal"][i + 1], atol=1e-12)


# ---- the interior-edge property ------------------------------------------------------------------------------------------------------------------
def _square_batch(kind, he, pos, rot, tri, flags):
    n, f = len(pos), len(tri)
    rep = lambda a: np.repeat(np.asarray(a, np.float64)[None], n * f, axis=0)
    P, R_ = np.repeat(pos, f, axis=0), np.repeat(rot, f, axis=0)
    V, Fl = np.tile(tri.reshape(f, 9), (n, 1)), np.tile(flags, n)
    z = np.zeros((n * f, 3))
    return (np.full(n * f, TRI), z, z, rep(I4), np.full(n * f, kind), rep(he), P, R_, np.full(n * f, 0.05), V, np.zeros((n * f, 9)), Fl, np.full(n * f, 7, np.uint8))


@pytest.mark.parametrize("kind,he", [(BALL, [0.3, 0.0, 0.0]), (CAP, [0.2, 0.4, 0.0]), (CUB, [0.12, 0.1, 0.14])])
def test_interior_edges_of_a_tessellated_square_raise_no_tilted_normals(kind, he):
    """A flat 4 x 4-quad square (spacing 0.5: every coordinate a power-of-two fraction), identity pose, flags from triangle_colliders: at 500 random
    poses above it -- straddling interior edges and vertices -- every manifold normal is vertical to 4 eps and the deepest penetration is the one
    against ONE cuboid whose top face is the square.  With all flags set at least one case has a tilted normal: the flags do something."""
    gv, gi = scenes.trimesh_ground(4, 4, 0.5)
    tri, flags = triangle_colliders(gv, gi)
    assert len(tri) == 32 and (flags[[1, 3, 5]] != 7).all()
    rng = np.random.default_rng(300 + kind)
    n = 500
    lowest = 0.3 if kind == BALL else (0.2 if kind == CAP else 0.1)    # the centre's height when the shape just rests on the square
    # every shape with its prediction distance stays inside the square's boundary (|x|, |z| = 1), whose edges are real
    span = 0.3 if kind == CAP else 0.55
    pos = np.stack([rng.uniform(-span, span, n), rng.uniform(lowest - 0.08, lowest + 0.02, n), rng.uniform(-span, span, n)], axis=1)
    pos[:40, 0] = rng.integers(-1, 2, 40) * (0.25 if kind == CAP else 0.5)    # exactly over interior edges (x = 0, +-0.5) or a quad's middle ...
    pos[20:60, 2] = rng.integers(-1, 2, 40) * (0.25 if kind == CAP else 0.5)   # ... and interior vertices
    rot = random_unit_quats(rng, n)
    if kind != BALL:                                                  # lying / flat, tilted by up to ~6 degrees, turned freely about y
        yaw = rng.uniform(0, np.pi, n); lean = rng.uniform(-0.1, 0.1, n)
        base = np.array([0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5)]) if kind == CAP else np.array(I4)
        for i in range(n):
            qy = np.array([0.0, np.sin(yaw[i] / 2), 0.0, np.cos(yaw[i] / 2)]); ql = np.array([np.sin(lean[i] / 2), 0.0, 0.0, np.cos(lean[i] / 2)])
            mul = lambda a, b: np.concatenate([a[3] * b[:3] + b[3] * a[:3] + np.cross(a[:3], b[:3]), [a[3] * b[3] - a[:3] @ b[:3]]])
            rot[i] = mul(qy, mul(ql, base))
    eps = np.finfo(np.float64).eps
    m = TR.manifolds(*_square_batch(kind, he, pos, rot, tri, flags), np.float64)
    pc = m["point_count"].reshape(n, 32)
    nrm = m["normal"].reshape(n, 32, 3)
    deepest = np.where(np.arange(16)[None, None] < pc[..., None], m["penetration"].reshape(n, 32, 16), -np.inf).max(-1)   # [n, 32]
    touching = pc > 0
    assert touching.any(1).sum() > 300 and (touching.sum(1) >= 2).sum() > 100, "the poses straddle edges: many touch several faces"
    assert (np.abs(nrm[touching][:, [0, 2]]) <= 4 * eps).all(), "an interior edge or vertex tilted a normal"
    assert (nrm[touching][:, 1] > 0).all()
    # one cuboid whose top face is the square, through the oracle's / the capsule reference's own manifolds
    slab = ([CUB], [[1.0, 0.5, 1.0]], [[0.0, -0.5, 0.0]], [I4])
    oracle = F.World(oracle_lib(), F.default_config(64))
    for i in range(n):   # every pose, none dropped: so close to the middle of its top face the slab answers with that face
        if kind == CAP:
            import capsule_collider_reference as CC
            ref = CC.manifolds(*slab, [CAP], [he], [pos[i]], [rot[i]], 0.05, np.float64)
        else:
            ref = oracle.contact_manifolds(*slab, [kind], [he], [pos[i]], [rot[i]], 0.05)
        rpc = int(ref["point_count"][0])
        if rpc == 0:
            assert not touching[i].any() or deepest[i].max() <= -0.05 + TOL, f"pose {i}: the square touches where the slab does not"
            continue
        assert abs(ref["normal"][0][1] - 1.0) <= 1e-12, f"pose {i}: the slab's own normal is not its top face's"
        assert touching[i].any() and abs(ref["penetration"][0, :rpc].max() - deepest[i].max()) <= TOL, f"pose {i}: deepest penetration against the square"
    # the control: the same poses against a bag of isolated triangles
    m7 = TR.manifolds(*_square_batch(kind, he, pos, rot, tri, np.full(32, 7, np.uint8)), np.float64)
    t7 = m7["point_count"] > 0
    assert (np.abs(m7["normal"][t7][:, [0, 2]]) > 1e-3).any(), "with all flags set some normal is tilted"


# ---- triangle_colliders' adjacency ---------------------------------------------------------------------------------------------------------------
def test_triangle_colliders_flags_follow_the_adjacency():
    # a flat grid: the boundary set, everything inside clear
    gv, gi = scenes.trimesh_ground(3, 3, 1.0)
    tri, flags = triangle_colliders(gv, gi)
    assert tri.shape == (18, 3, 3)
    for f in range(18):
        for k in range(3):
            a, b = tri[f, k], tri[f, (k + 1) % 3]
            on_boundary = any(abs(a[c]) == 1.5 and abs(b[c]) == 1.5 and a[c] == b[c] for c in (0, 2))
            assert bool(flags[f] & (1 << k)) == on_boundary, (f, k)
    # a ridge (convex) and a valley (concave): two faces sharing the edge (0,0,0)-(0,0,1)
    for y, shared_set in ((-0.3, True), (0.3, False), (0.0, False)):
        v = np.array([[0, 0, 0], [0, 0, 1], [1, y, 0], [-1, y, 0]], np.float64)
        _, fl = triangle_colliders(v, [[0, 1, 2], [1, 0, 3]])          # both normals point up
        assert [bool(fl[0] & 1), bool(fl[1] & 1)] == [shared_set, shared_set], (y, fl)
        assert (fl & 6 == 6).all(), "the open boundary is set"
    # an edge shared by three faces is set
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [-1, 0, 0], [0, 1, 0]], np.float64)
    _, fl = triangle_colliders(v, [[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    assert (fl & 1 == 1).all()


def test_kind_four_is_no_collider_kind_yet():
    """No backend has the triangle kind: the upload refuses it (the device would read it as a cuboid); a MeshScene uploads its faces as host shapes."""
    sc = scenes.trimesh_drop(n_boxes=1, n_balls=1, n_capsules=1, nx=2, nz=2)
    w = F.World(oracle_lib(), F.default_config(32))
    w.bodies_upload(**sc.body_kwargs())
    with pytest.raises(ValueError):
        w.colliders_upload(**dict(sc.collider_kwargs(), shape=sc.col_shape))
    cols = sc.collider_kwargs()
    assert (cols["shape"][sc.col_shape == TRI] == F.SHAPE_HOST).all() and (cols["shape"][sc.col_shape != TRI] == sc.col_shape[sc.col_shape != TRI]).all()
    w.colliders_upload(**cols)


# ---- the oracle-hosted scene ------------------------------------------------------------------------------------------------------------------
SCENE = dict(n_boxes=8, n_balls=8, n_capsules=8, nx=8, nz=8, spacing=1.0, seed=3)   # 128 triangles, 24 bodies
STEPS = 100


def bumps(x, z):
    """A bumpy ground whose border rises (from |x|, |z| = 3 on): what rolls stays on the mesh."""
    up = lambda t: 0.6 * np.maximum(np.abs(t) - 3.0, 0.0) ** 2
    return 0.15 * np.sin(1.3 * x) * np.cos(0.9 * z) + up(x) + up(z)


def hosted_world(lib, bits):
    """The trimesh_drop scene with its triangles held as AVN_SHAPE_HOST and answered by the reference callbacks -- and its capsules too, answered by the
    capsule collider's reference: the oracle has neither kind."""
    sc = scenes.trimesh_drop(**SCENE, height_fn=bumps)
    cols = sc.collider_kwargs(host_capsules=True)
    assert not (cols["shape"] == TRI).any() and (cols["shape"] == F.SHAPE_HOST).sum() == 128 + 8
    host = TR.MeshHost(cols["entity_index"], sc.col_shape, sc.col_half_extents, sc.vertices, sc.edge_flags)
    w = F.World(lib, F.default_config(bits, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction, restitution=0.0)
    w.host_shapes_set(host.aabb, host.manifolds)
    w.pipeline_enable()
    return w, host, sc


def lowest_points(sc, bodies):
    """Per dynamic body the world position of its lowest point (ball: centre - r; capsule: its lower cap; cuboid: its lowest corner)."""
    out = np.zeros((sc.n - 1, 3))
    for k in range(1, sc.n):
        p, q, he, kind = bodies["position"][k].astype(np.float64), bodies["rotation"][k].astype(np.float64), sc.half_extents[k], sc.shape[k]
        if kind == BALL:
            out[k - 1] = p - [0, he[0], 0]
        elif kind == CAP:
            ends = p + qrot(q, np.array([[0, -he[1], 0], [0, he[1], 0]], np.float64))
            out[k - 1] = ends[np.argmin(ends[:, 1])] - [0, he[0], 0]
        else:
            c = box_corners(he, p, q)
            out[k - 1] = c[np.argmin(c[:, 1])]
    return out


def test_oracle_hosted_mesh_scene_covers_every_pair_kind_and_comes_to_rest():
    """24 bodies on a bumpy 8 x 8-quad ground on the oracle, the 128 triangles AVN_SHAPE_HOST answered by the reference: every pair kind occurs in the
    first STEPS steps, the bodies come to rest on the ground, none sinks more than 0.03 (the capsule rest test's bound) under the
    surface.  At rest means what it means in the capsule rest test -- every body lies on the ground --: nothing here resists rolling, so the balls and the
    capsules keep rolling slowly between the bumps (observed: under 1 m/s) while the cuboids stand still."""
    w, host, sc = hosted_world(oracle_lib(), 32)
    for step in range(300):
        w.step()
        if step == STEPS - 1:
            at_steps = dict(host.kinds)
    assert not w.host_shape_errors()
    count = lambda kinds, pcs: sum(v for (k, c), v in at_steps.items() if k == kinds and c in pcs)
    got = {"triangle-ball": count((BALL, TRI), (1,)), "triangle-capsule, one point": count((CAP, TRI), (1,)), "triangle-capsule, two points": count((CAP, TRI), (2,)),
           "triangle-cuboid, one point": count((CUB, TRI), (1,)), "triangle-cuboid, several points": count((CUB, TRI), tuple(range(2, 9)))}
    print("manifold queries by pair kind over", STEPS, "steps:", got)
    for k, v in got.items():
        assert v >= 20, f"{k}: {v} queries with a manifold"
    b = w.bodies_download()
    assert np.isfinite(b["position"]).all()
    low = lowest_points(sc, b)
    depth = sc.surface_height(low[:, 0], low[:, 2]) - low[:, 1]
    print("deepest lowest point under the surface:", depth.max(), " fastest body:", np.abs(b["linear_velocity"]).max())
    assert (np.abs(low[:, [0, 2]]) < 4.0).all(), "every body is still over the mesh"
    assert (depth <= 0.03).all(), "no body sank into the ground"
    assert (depth >= -0.45).all() and np.median(depth) > -0.05, "every body lies on the ground or leans on a neighbour"
    speed = np.linalg.norm(b["linear_velocity"][1:], axis=1)
    assert speed.max() < 2.0 and np.median(speed[sc.shape[1:] == CUB]) < 0.05, "nothing was thrown about; the cuboids stand still"
