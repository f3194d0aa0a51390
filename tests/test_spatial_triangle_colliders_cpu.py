"""tests/spatial_triangle_collider_reference.py -- the numpy definition of the spatial queries against triangle colliders, which the device is held to bit for
bit (tests/test_gpu_spatial_triangle_colliders.py, tests/test_spatial_triangle_host.py) -- held to exact rational geometry inside the project's band: band_of of
tests/test_spatial_capsule_cpu.py, 32 eps (|query position| + query size + |collider position| + collider size + distance).  No GPU, no library.

Rays: a reported hit point lies on the triangle within band, a reported miss is an exact miss of the triangle shrunk by band (both sides, through vertices and
edges, parallel to the plane, coplanar).  Projection and the three intersections are decided correctly whenever the exact gap is more than 2 band from the
threshold.  Casts of the three query kinds, aimed as aimed_casts aims them: the exact query grown by band touches the triangle at the reported distance and
shrunk by band does not at distance - band (never an over-estimate); the witnesses lie on their shapes; a grazing pass is only required not to over-estimate.
The largest Newton round count over the random set is recorded and must stay below the cap.  Contacts equal the deepest point of
triangle_collider_reference.manifold with the query as shape 1; over the interior of a flat tessellated square every query kind gets the face normal, an
isolated triangle with ALL_EDGES tilts it.  Every triangle lies inside its leaf box."""
from fractions import Fraction as Q
from types import SimpleNamespace

import numpy as np
import pytest

from avian_amd import scenes
from helpers import random_unit_quats
import spatial_contact_reference as CR
import spatial_exact_geometry as X
import spatial_query_reference as R
import spatial_scenes as SC
import spatial_triangle_collider_reference as TC
import triangle_collider_reference as T
from test_spatial_capsule_cpu import band_of, exact_seg_box_d2

DTYPES = [np.float32, np.float64]
CUB, BALL, CAP, TRI = 0, 1, 3, 4
I = [0.0, 0.0, 0.0, 1.0]
MISS = 0xFFFFFFFF


# ---- exact geometry (Fractions) ------------------------------------------------------------------------------------------------------------------
def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def closest_q(a, b, c, p):
    """Ericson 5.1.5 in exact arithmetic: the closest point of the triangle to p."""
    ab, ac, ap = X.sub(b, a), X.sub(c, a), X.sub(p, a)
    d1, d2 = X.dot(ab, ap), X.dot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        return a
    bp = X.sub(p, b)
    d3, d4 = X.dot(ab, bp), X.dot(ac, bp)
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return X.add(a, X.scale(ab, d1 / (d1 - d3)))
    cp = X.sub(p, c)
    d5, d6 = X.dot(ab, cp), X.dot(ac, cp)
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return X.add(a, X.scale(ac, d2 / (d2 - d6)))
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return X.add(b, X.scale(X.sub(c, b), (d4 - d3) / ((d4 - d3) + (d5 - d6))))
    den = va + vb + vc
    return X.add(a, X.add(X.scale(ab, vb / den), X.scale(ac, vc / den)))


def point_d2(tri, p):
    e = X.sub(p, closest_q(*tri, p))
    return X.dot(e, e)


def seg_seg_d2(p1, u1, p2, u2):
    """The exact squared distance of two segments (Ericson 5.1.9 in rationals)."""
    r = X.sub(p1, p2)
    a, e, f = X.dot(u1, u1), X.dot(u2, u2), X.dot(u2, r)
    clamp = lambda x: min(max(x, Q(0)), Q(1))
    if a == 0 and e == 0:
        s = t = Q(0)
    elif a == 0:
        s, t = Q(0), clamp(f / e)
    else:
        c = X.dot(u1, r)
        if e == 0:
            t, s = Q(0), clamp(-c / a)
        else:
            b = X.dot(u1, u2)
            den = a * e - b * b
            s = clamp((b * f - c * e) / den) if den != 0 else Q(0)
            t = (b * s + f) / e
            if t < 0:
                t, s = Q(0), clamp(-c / a)
            elif t > 1:
                t, s = Q(1), clamp((b - c) / a)
    d = X.sub(X.add(p1, X.scale(u1, s)), X.add(p2, X.scale(u2, t)))
    return X.dot(d, d)


def seg_d2(tri, A, u):
    """The exact squared distance of the segment A + s u from the triangle."""
    a, b, c = tri
    n = cross(X.sub(b, a), X.sub(c, a))
    B = X.add(A, u)
    da, db = X.dot(n, X.sub(A, a)), X.dot(n, X.sub(B, a))
    if da * db < 0:
        P = X.add(A, X.scale(u, da / (da - db)))
        if closest_q(a, b, c, P) == P:
            return Q(0)
    best = min(point_d2(tri, A), point_d2(tri, B))
    for v, w in ((a, b), (b, c), (c, a)):
        best = min(best, seg_seg_d2(A, u, v, X.sub(w, v)))
    return best


def box_overlaps(tri, he, pos, rot):
    """Exact SAT of the triangle and the box (he at pos with the rotation of the -- not necessarily unit -- quaternion rot): True when no axis separates."""
    m = X.rotation(rot)
    v = [X.mul_t(m, X.sub(p, pos)) for p in tri]      # the vertices in the box's frame
    if any(h < 0 for h in he):
        return False
    e = [X.sub(v[1], v[0]), X.sub(v[2], v[1]), X.sub(v[0], v[2])]
    unit = [(Q(1), Q(0), Q(0)), (Q(0), Q(1), Q(0)), (Q(0), Q(0), Q(1))]
    axes = unit + [cross(e[0], e[1])] + [cross(ek, ui) for ek in e for ui in unit]
    for L in axes:
        if L == (0, 0, 0):
            continue
        p = [X.dot(L, x) for x in v]
        rb = sum(abs(L[i]) * he[i] for i in range(3))
        if min(p) > rb or max(p) < -rb:
            return False
    return True


class Tri:
    """A triangle collider at a pose: exact world vertices; `size` its largest local coordinate."""

    def __init__(self, verts, pos, rot, dt):
        f = lambda x: [float(dt(y)) for y in x]
        self.local = np.array([f(v) for v in verts])
        self.pos_f, self.rot_f = f(pos), f(rot)
        self.pos = X.vec(self.pos_f)
        m = X.rotation(X.vec(self.rot_f))
        self.w = tuple(X.add(X.mul(m, X.vec(v)), self.pos) for v in self.local)
        self.size = float(np.abs(self.local).max())


def query(kind, he, pos, rot, dt):
    f = lambda x: [float(dt(y)) for y in x]
    he, pos, rot = f(he), f(pos), f(rot)
    o = SimpleNamespace(kind=kind, he=X.vec(he), pos=X.vec(pos), rot=X.vec(rot))
    o.size = float(he[0]) if kind == BALL else (float(he[0] + he[1]) if kind == CAP else float(np.linalg.norm(he)))
    if kind == CAP:
        hv = X.mul(X.rotation(o.rot), (Q(0), o.he[1], Q(0)))
        o.a, o.u = X.sub(o.pos, hv), X.scale(hv, 2)
    return o


def touches(qs, tri: Tri, shift, grow):
    """The exact query shape, translated by `shift` and grown by `grow` (a ball's and a capsule's radius, a cuboid's half extents), touches the triangle."""
    if qs.kind == BALL:
        r = qs.he[0] + grow
        return r >= 0 and point_d2(tri.w, X.add(qs.pos, shift)) <= r * r
    if qs.kind == CAP:
        r = qs.he[0] + grow
        return r >= 0 and seg_d2(tri.w, X.add(qs.a, shift), qs.u) <= r * r
    return box_overlaps(tri.w, tuple(h + grow for h in qs.he), X.add(qs.pos, shift), qs.rot)


def snapshot(tris, dt, flags=None):
    """A Snapshot of triangle colliders, one static body each, with its triangle table."""
    n = len(tris)
    cols = dict(entity_index=np.arange(500, 500 + n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=np.full(n, TRI, np.uint8), half_extents=np.zeros((n, 3)))
    s = R.Snapshot(SC.bodies_of([t.pos_f for t in tris], [t.rot_f for t in tris]), cols, None, dt)
    return TC.with_triangles(s, np.array([t.local for t in tris]).reshape(n, 9), flags)


def random_tris(rng, n, dt, spread=2.0):
    out = []
    for k in range(n):
        v = rng.normal(size=(3, 3)) * rng.choice([0.4, 1.0, 2.0])
        rot = I if k % 3 == 0 else list(random_unit_quats(rng, 1)[0])
        out.append(Tri(v, rng.normal(size=3) * spread, rot, dt))
    return out


def on_tri(rng, t: Tri, where):
    """A float point of the triangle: inside it (0), on an edge (1), at a vertex (2)."""
    w = rng.dirichlet([1.0, 1.0, 1.0])
    if where == 1:
        w[2] = 0.0; w /= w.sum()
    if where == 2:
        w = np.eye(3)[rng.integers(0, 3)]
    return w @ np.array([[float(x) for x in v] for v in t.w])


# ---- the array closest point is the scalar definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_the_array_closest_point_is_the_scalar_one_bit_for_bit(dt):
    rng = np.random.default_rng(1)
    n = 3000
    tri = rng.normal(size=(n, 3, 3)).astype(dt)
    p = (rng.normal(size=(n, 3)) * 1.5).astype(dt)
    p[::7] = tri[::7, 1]                                        # on a vertex
    p[1::7] = ((tri[1::7, 0].astype(np.float64) + tri[1::7, 2]) / 2).astype(dt)   # near an edge
    cols = lambda a: tuple(a[:, j] for j in range(3))
    with np.errstate(all="ignore"):
        pt, rg = TC.closest_point(cols(tri[:, 0]), cols(tri[:, 1]), cols(tri[:, 2]), cols(p), dt)
    seen = set()
    for i in range(n):
        S_ = lambda a: tuple(dt(x) for x in a)
        with np.errstate(all="ignore"):
            q, r = T.closest_point(S_(tri[i, 0]), S_(tri[i, 1]), S_(tri[i, 2]), S_(p[i]), dt)
        assert r == rg[i] and all(np.array([q[j]], dt).tobytes() == np.array([pt[j][i]], dt).tobytes() for j in range(3)), i
        seen.add(int(r))
    assert seen == set(range(7))


# ---- rays ----------------------------------------------------------------------------------------------------------------------------------------------
def edge_margin2(tri, p):
    """The squared distance of a point of the triangle's plane from the triangle's boundary."""
    a, b, c = tri
    return min(seg_seg_d2(p, (Q(0),) * 3, v, X.sub(w, v)) for v, w in ((a, b), (b, c), (c, a)))


@pytest.mark.parametrize("dt", DTYPES)
def test_rays_against_exact_geometry(dt):
    rng = np.random.default_rng(11)
    tris = random_tris(rng, 40, dt)
    s = snapshot(tris, dt)
    n = 600
    tgt = rng.integers(0, len(tris), n)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        t = tris[tgt[i]]
        p = on_tri(rng, t, i % 3)
        d[i] = rng.normal(size=3); d[i] /= np.linalg.norm(d[i])
        if i % 10 == 9:                                        # parallel to the plane, a tenth of a unit or more off it
            a, b, c = (np.array([float(x) for x in v]) for v in t.w)
            nrm = np.cross(b - a, c - a); nrm /= np.linalg.norm(nrm)
            d[i] = (b - a) / np.linalg.norm(b - a)
            p = p + nrm * rng.uniform(0.1, 0.5) * (1 if i % 20 == 9 else -1)
        o[i] = p - d[i] * rng.uniform(0.0 if i % 7 == 0 else 0.3, 3.0)
        if i % 5 == 4:
            o[i] += rng.normal(size=3) * 0.3                   # a near miss or a hit somewhere else
    o, d = o.astype(dt), d.astype(dt)
    hits, miss, sides = 0, 0, set()
    for i in range(n):
        t = tris[tgt[i]]
        one = snapshot([t], dt)
        got = TC.cast_rays(one, o[i:i + 1], d[i:i + 1])[0]
        oq, dq = X.vec(o[i]), X.vec(d[i])
        a, b, c = t.w
        nq = cross(X.sub(b, a), X.sub(c, a))
        den = X.dot(nq, dq)
        tq = X.dot(nq, X.sub(a, oq)) / den if den != 0 else None
        qs = SimpleNamespace(pos=oq, size=0.0)
        if got["collider"] != MISS:
            hits += 1
            dist = X.q(got["distance"])
            band = band_of(dt, qs, t, float(dist))
            hp = X.add(oq, X.scale(dq, dist))
            assert point_d2(t.w, hp) <= band * band, (i, "a hit off the triangle")
            nrm = np.array(got["normal"], float)
            assert abs(np.linalg.norm(nrm) - 1) < 1e-5 and nrm @ d[i].astype(float) < 0, (i, "the normal is turned against the ray")
            sides.add(bool(float(den) > 0))
        else:
            miss += 1
            if tq is not None and tq > 0:
                band = band_of(dt, qs, t, float(tq))
                hp = X.add(oq, X.scale(dq, tq))
                inside = closest_q(a, b, c, hp) == hp
                assert not (inside and edge_margin2(t.w, hp) > band * band and tq * X.norm(dq) > band), (i, "a miss of the triangle shrunk by band")
    assert hits >= 250 and miss >= 100 and sides == {True, False}
    # every face of the whole set through the brute force: the closest hit is some triangle's, at an exact hit of it
    got = TC.cast_rays(s, o, d)
    assert (got["collider"] != MISS).sum() >= hits


@pytest.mark.parametrize("dt", DTYPES)
def test_coplanar_and_axis_parallel_rays_miss_and_a_shared_edge_is_never_missed(dt):
    """A flat square of two faces in the plane y = 0.5: rays in that plane and rays parallel above it miss (the denominator is exactly 0); straight-down rays
    through the shared diagonal, through vertices and through the outer edges hit a face -- both faces of the diagonal, the lower index first."""
    v = np.array([[-1, 0.5, -1], [-1, 0.5, 1], [1, 0.5, 1], [1, 0.5, -1]], float)
    tris = [Tri(v[[0, 1, 2]], [0, 0, 0], I, dt), Tri(v[[0, 2, 3]], [0, 0, 0], I, dt)]
    s = snapshot(tris, dt)
    o = np.array([[-2, 0.5, 0.1], [-2, 0.75, 0.1], [0.3, 0.5, -2]], dt); d = np.array([[1, 0, 0], [1, 0, 0.1], [0, 0, 1]], dt)
    assert (TC.cast_rays(s, o, d)["collider"] == MISS).all()
    k = np.linspace(-1, 1, 17)
    o = np.concatenate([np.c_[k, np.full(17, 2.0), k], np.c_[k, np.full(17, 2.0), np.full(17, -1.0)], np.c_[np.full(17, 1.0), np.full(17, 2.0), k]]).astype(dt)
    d = np.tile(np.array([0, -1, 0], dt), (len(o), 1))
    got, (many, cnt) = TC.cast_rays(s, o, d), TC.ray_hits(s, o, d, 2)
    assert (got["collider"] != MISS).all() and (got["distance"] == dt(1.5)).all() and (got["normal"] == [0, 1, 0]).all()
    assert (cnt[:17] == 2).all() and (got["collider"][:17] == 0).all()
    # random directions through random points of the shared diagonal: never missed by both faces
    rng = np.random.default_rng(3)
    w = rng.uniform(0, 1, 400)
    p = (v[0][None, :] * (1 - w)[:, None] + v[2][None, :] * w[:, None]).astype(dt)
    d = rng.normal(size=(400, 3)); d[:, 1] = -np.abs(d[:, 1]) - 0.2
    d = d.astype(dt)
    o = (p.astype(np.float64) - d.astype(np.float64) * rng.uniform(0.5, 2, 400)[:, None]).astype(dt)
    assert (TC.cast_rays(s, o, d)["collider"] != MISS).all()


# ---- projection and the three intersections ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_projection_and_intersections_decided_outside_two_bands(dt):
    rng = np.random.default_rng(21)
    tris = random_tris(rng, 30, dt)
    n = 450
    decided = {k: [0, 0] for k in ("project", BALL, CAP, CUB)}
    for i in range(n):
        t = tris[i % len(tris)]
        p = on_tri(rng, t, i % 3) + rng.normal(size=3) * rng.choice([0.0, 0.02, 0.3, 1.0])
        one = snapshot([t], dt)
        # projection
        pr = TC.project_points(one, np.array([p], dt), np.array([i % 2], np.uint8))[0]
        pq = X.vec(np.array(p, dt))
        d2 = point_d2(t.w, pq)
        band = band_of(dt, SimpleNamespace(pos=pq, size=0.0), t, float(X.sqrt_q(d2)))
        assert pr["collider"] == 0 and abs(X.q(pr["distance"]) - X.sqrt_q(d2)) <= 2 * band, (i, "projection distance")
        assert point_d2(t.w, X.vec(pr["point"])) <= (2 * band) ** 2, (i, "the projected point lies on the triangle")
        if X.sqrt_q(d2) > 2 * band:
            assert pr["is_inside"] == 0, i
            decided["project"][0] += 1
        # intersections
        kind = (BALL, CAP, CUB)[i % 3]
        he = rng.uniform(0.1, 0.5, 3)
        rot = I if i % 4 == 0 else list(random_unit_quats(rng, 1)[0])
        qs = query(kind, he, p, rot, dt)
        band = band_of(dt, qs, t, 0.0)
        got = TC.shape_intersections(one, np.array([kind], np.uint8), np.array([he], dt), np.array([p], dt), np.array([rot], dt), 4)[1][0]
        zero = (Q(0),) * 3
        if touches(qs, t, zero, -2 * band):
            assert got == 1, (i, kind, "an overlap by more than two bands")
            decided[kind][0] += 1
        elif not touches(qs, t, zero, 2 * band):
            assert got == 0, (i, kind, "a gap of more than two bands")
            decided[kind][1] += 1
    assert all(sum(v) >= 100 for k, v in decided.items() if k != "project") and all(min(v) >= 25 for k, v in decided.items() if k != "project"), decided


def test_point_intersection_is_the_exact_identity():
    t = Tri([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [0, 0, 0], I, np.float32)
    s = snapshot([t], np.float32)
    pts = np.array([[0.25, 0.25, 0], [1, 0, 0], [0.5, 0.5, 0], [0.25, 0.25, 1e-6], [0.75, 0.75, 0]], np.float32)
    assert list(TC.point_intersections(s, pts, 2)[1]) == [1, 1, 1, 0, 0]
    pr = TC.project_points(s, pts, np.ones(5, np.uint8))
    assert list(pr["is_inside"]) == [1, 1, 1, 0, 0] and (pr["distance"][:3] == 0).all() and (pr["distance"][3:] > 0).all()


# ---- casts ---------------------------------------------------------------------------------------------------------------------------------------------
ROUNDS_SEEN = {}


@pytest.mark.parametrize("dt", DTYPES)
def test_aimed_casts_bracketed_by_exact_geometry_and_newton_rounds(dt):
    rng = np.random.default_rng(31)
    tris = random_tris(rng, 30, dt)
    n = 360
    TC.reset_rounds()
    hits, grazing, kinds = 0, 0, {BALL: 0, CAP: 0, CUB: 0}
    for i in range(n):
        t = tris[i % len(tris)]
        kind = (BALL, CAP, CUB)[i % 3]
        he = rng.uniform(0.1, 0.5, 3)
        if i % 11 == 0:
            he[1] = 0.0
        rot = I if i % 4 == 0 else list(random_unit_quats(rng, 1)[0])
        tgt = on_tri(rng, t, (i // 3) % 3)
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        pos = tgt - d * rng.uniform(1.0, 4.0) + rng.normal(size=3) * (0.0 if i % 2 else 0.35)     # aimed at the triangle, every other cast off-centre
        d = d * rng.choice([0.5, 1.0, 2.0])
        one = snapshot([t], dt)
        rec = TC.cast_queries(one, np.array([kind], np.uint8), np.array([he], dt), np.array([pos], dt), np.array([rot], dt), np.array([d], dt), ())[0][0]
        qs = query(kind, he, pos, rot, dt)
        dq = X.vec(np.array(d, dt))
        if rec["collider"] == MISS:
            continue                                           # (the off-centre casts that pass the triangle by; the bracketing below is about the hits)
        hits += 1
        kinds[kind] += 1
        dist = X.q(rec["distance"])
        band = band_of(dt, qs, t, float(dist * X.norm(dq)))
        if dist == 0:
            assert touches(qs, t, (Q(0),) * 3, band), (i, kind, "an overlap at the start that is none")
            continue
        step = band / X.norm(dq)                               # band as a parameter step along d
        at = X.scale(dq, dist)
        graze = not touches(qs, t, at, band)
        if graze:
            # a grazing pass (the closest approach within two bands of contact) is only required not to over-estimate
            grazing += 1
            assert touches(qs, t, at, 2 * band), (i, kind, "a hit where the shape grown by two bands does not touch")
        assert not touches(qs, t, X.scale(dq, max(dist - step, Q(0))), -band), (i, kind, "an over-estimate: the shrunk shape already touches a band earlier")
        # witnesses on their shapes, the normal a unit vector pointing from the triangle towards the query
        p1, p2 = X.vec(rec["point1"]), X.vec(rec["point2"])
        assert point_d2(t.w, p1) <= (2 * band) ** 2, (i, kind, "point1 off the triangle")
        moved = SimpleNamespace(**dict(qs.__dict__, pos=X.add(qs.pos, at)))
        if kind == CAP:
            moved.a = X.add(qs.a, at)
        inside_grown = (point_d2((moved.pos,) * 3, p2) <= (moved.he[0] + 2 * band) ** 2 if kind == BALL else
                        seg_seg_d2(moved.a, moved.u, p2, (Q(0),) * 3) <= (moved.he[0] + 2 * band) ** 2 if kind == CAP else
                        box_overlaps((p2, p2, p2), tuple(h + 2 * band for h in moved.he), moved.pos, moved.rot))
        assert inside_grown, (i, kind, "point2 off the query shape")
        nrm = np.array(rec["normal1"], float)
        assert abs(np.linalg.norm(nrm) - 1) < 1e-4 and (nrm == -np.array(rec["normal2"], float)).all(), (i, kind)
    ROUNDS_SEEN[dt] = TC.last_rounds
    print(f"{np.dtype(dt).name}: {hits} hits of {n} casts ({kinds}), {grazing} grazing; most Newton rounds of a pair against a triangle collider: {TC.last_rounds}")
    assert hits >= 200 and min(kinds.values()) >= 50
    assert 1 <= TC.last_rounds < TC.ROUNDS, "a cast of the random set reaches the Newton round cap"


# ---- contacts ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_contacts_are_the_deepest_point_of_the_narrow_phase_manifold(dt):
    rng = np.random.default_rng(41)
    tris = random_tris(rng, 20, dt)
    flags = rng.integers(0, 8, len(tris)).astype(np.uint8)
    s = snapshot(tris, dt, flags)
    n = 240
    kind = np.array([(BALL, CAP, CUB)[i % 3] for i in range(n)], np.uint8)
    he = rng.uniform(0.1, 0.5, (n, 3))
    rot = random_unit_quats(rng, n)
    pos = np.array([on_tri(rng, tris[i % len(tris)], i % 3) + rng.normal(size=3) * 0.25 for i in range(n)])
    pred = np.where(np.arange(n) % 2, 0.2, 0.0)
    lists = TC.contact_lists_of(s, kind, he, pos, rot, pred)
    found = 0
    for i in range(n):
        for r in lists[i]:
            c = int(r["collider"])
            m = T.manifold(int(kind[i]), np.where(kind[i] == BALL, he[i, 0], he[i]).astype(dt) * np.ones(3, dt) if kind[i] == BALL else np.array([he[i, 0], he[i, 1], 0 if kind[i] == CAP else he[i, 2]], dt),
                           np.array(pos[i], dt), np.array(rot[i], dt), TRI, (0, 0, 0), np.array(tris[c].pos_f, dt), np.array(tris[c].rot_f, dt), dt(pred[i]), tris[c].local.astype(dt), flags[c], dt)
            assert m is not None, (i, c)
            normal, pts = m
            k = CR.deepest([p[1] for p in pts], len(pts))
            assert np.array([pts[k][1]], dt).tobytes() == np.array([r["penetration"]], dt).tobytes() and (np.array(normal, dt) == -r["normal"]).all(), (i, c)
            assert (np.array(pts[k][0], dt) == r["anchor1"]).all()
            found += 1
    assert found >= 120


@pytest.mark.parametrize("dt", DTYPES)
def test_a_flat_tessellated_square_gives_every_query_the_face_normal_and_an_isolated_triangle_tilts_it(dt):
    sc = scenes.trimesh_drop(n_boxes=0, n_balls=1, n_capsules=0, nx=4, nz=4, seed=2)
    nf = sc.n_faces
    rng = np.random.default_rng(51)
    tris = [Tri(sc.vertices[f], [0, 0, 0], I, dt) for f in range(nf)]
    n = 150
    kind = np.array([(BALL, CAP, CUB)[i % 3] for i in range(n)], np.uint8)
    he = np.tile([0.25, 0.2, 0.25], (n, 1))
    rot = random_unit_quats(rng, n)
    rot[kind == CUB] = I                                      # (a box lying flat: a tilted box's own edge may carry the contact, with its own normal)
    pos = np.c_[rng.uniform(-1.4, 1.4, n), np.full(n, 0.0), rng.uniform(-1.4, 1.4, n)]
    pos[:, 1] = np.where(kind == BALL, 0.2, np.where(kind == CAP, 0.3, 0.2))      # sunk a little into the ground
    rot[kind == CAP] = I
    for flags, want_tilt in ((sc.edge_flags[:nf], False), (np.full(nf, T.ALL_EDGES, np.uint8), True)):
        s = snapshot(tris, dt, flags)
        lists = TC.contact_lists_of(s, kind, he, pos, rot, 0.05)
        nrm = np.concatenate([l["normal"] for l in lists if len(l)]).astype(float)
        # (the manifold's normal goes through the query's own rotation and back: the face normal up to a few eps of the scalar; a tilted one is off by degrees)
        tilted = np.abs(nrm - [0.0, 1.0, 0.0]).max(1) > 64 * np.finfo(dt).eps
        assert len(nrm) >= n and tilted.any() == want_tilt, (want_tilt, int(tilted.sum()))
        if want_tilt:
            assert tilted.sum() >= 20 and np.median(np.abs(nrm[tilted] - [0.0, 1.0, 0.0]).max(1)) > 1e-2
        for k in (BALL, CAP, CUB):
            assert sum(len(l) for l, kk in zip(lists, kind) if kk == k) >= 40, k


# ---- padding -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_every_triangle_lies_inside_its_leaf_box(dt):
    rng = np.random.default_rng(61)
    tris = random_tris(rng, 200, dt, spread=50.0)
    lo, hi = TC.leaf_boxes(snapshot(tris, dt))
    for i, t in enumerate(tris):
        for v in t.w:
            assert all(X.q(lo[j][i]) <= v[j] <= X.q(hi[j][i]) for j in range(3)), i
