"""The Triangle COLLIDER (parry's Triangle, Avian's Collider::triangle; a static trimesh is one such collider per face): its AABB and its contact
manifolds against a Ball, a Capsule or a Cuboid in either order, DEFINED here operation for operation in scalars of the world's type (numpy
scalars: every operation is rounded once, there is no fused multiply-add) -- so that a device kernel that follows these definitions can be held to
them bit for bit.  parry is not vendored: parity with parry is UNPINNED, as for the capsule collider.  One pair at a time: vectors are tuples of
three scalars, quaternions of four.

The triangle (a, b, c) is two-sided and has zero thickness.  Edge k is (ab, bc, ca)[k]; bit k of the edge flags says that edge k is a real edge
(boundary or convex), a clear bit that it is interior (shared with a coplanar or concave neighbour).  INTERIOR-EDGE RULE: where the feature of the
triangle that gives the contact direction is an edge whose flag is clear, or a vertex both of whose edges have their flags clear, the normal is the
face normal, signed towards the other shape, and depths are measured along it; the acceptance test stays on the true distance.  For the cuboid the
SAT's axis is chosen among the triangle's normal, the edge axes of flagged edges that are the triangle's lowest feature along them, and the box faces whose lowest triangle feature carries the contact
(the whole face; or a real edge or vertex with a vertex over the box face: _face_axis_admissible).  A manifold holds only what lies over its reference
feature, as for two cuboids: a pair within the prediction distance whose clipped polygon has no corner within it has no manifold.
Two triangles have no manifold (not built: it cannot arise for meshes on static bodies).

No backend holds the triangle as a device kind yet.  `TriangleHost` answers the two host-shape callbacks from these functions (the triangles are
AVN_SHAPE_HOST colliders); `MeshHost` does so for a backend that has no capsule kind either (the oracle)."""
from __future__ import annotations

import numpy as np

import spatial_query_reference as R
import spatial_shape_reference as S
from spatial_query_reference import add, qinverse, scale, sub
from spatial_shape_reference import na_cross, na_dot, na_qmul, na_qrot, neg

SHAPE_CUBOID, SHAPE_BALL, SHAPE_HOST, SHAPE_CAPSULE, SHAPE_TRIANGLE = 0, 1, 2, 3, 4
ALL_EDGES = 7
MAX_POINTS = 16   # AVN_MAX_QUERY_POINTS


def fid_vertex(c):
    return (1 << 30) | int(c)


def fid_edge(c):
    return (2 << 30) | int(c)


def fid_face(c):
    return (3 << 30) | int(c)


def tri_fid(region):
    return fid_vertex(region - 4) if region >= 4 else (fid_edge(region - 1) if region >= 1 else fid_face(0))


def tri_interior(flags, region):
    """The interior-edge rule: an edge whose flag is clear, a vertex both of whose edges have theirs clear."""
    if region >= 4:
        k = region - 4
        return not (flags & (1 << k)) and not (flags & (1 << ((k + 2) % 3)))
    if region >= 1:
        return not (flags & (1 << (region - 1)))
    return False


def _norm(v):
    return np.sqrt(na_dot(v, v))


def _div(v, s):
    return (v[0] / s, v[1] / s, v[2] / s)


def unit_normal(a, b, c):
    nrm = na_cross(sub(b, a), sub(c, a))
    return _div(nrm, _norm(nrm))


def closest_point(a, b, c, p, dt):
    """(point, region): Ericson 5.1.5 in its order of tests; region 0 the face, 1 + k edge k, 4 + k vertex k."""
    zero = dt(0)
    ab, ac, ap = sub(b, a), sub(c, a), sub(p, a)
    d1, d2 = na_dot(ab, ap), na_dot(ac, ap)
    if d1 <= zero and d2 <= zero:
        return a, 4
    bp = sub(p, b)
    d3, d4 = na_dot(ab, bp), na_dot(ac, bp)
    if d3 >= zero and d4 <= d3:
        return b, 5
    vc = d1 * d4 - d3 * d2
    if vc <= zero and d1 >= zero and d3 <= zero:
        return add(a, scale(ab, d1 / (d1 - d3))), 1
    cp = sub(p, c)
    d5, d6 = na_dot(ab, cp), na_dot(ac, cp)
    if d6 >= zero and d5 <= d6:
        return c, 6
    vb = d5 * d2 - d1 * d6
    if vb <= zero and d2 >= zero and d6 <= zero:
        return add(a, scale(ac, d2 / (d2 - d6))), 3
    va = d3 * d6 - d5 * d4
    if va <= zero and (d4 - d3) >= zero and (d5 - d6) >= zero:
        return add(b, scale(sub(c, b), (d4 - d3) / ((d4 - d3) + (d5 - d6)))), 2
    nrm = na_cross(ab, ac)
    N = _div(nrm, _norm(nrm))
    return sub(p, scale(N, na_dot(N, ap))), 0


def _clamp01(x, dt):
    return dt(0) if x < dt(0) else (dt(1) if x > dt(1) else x)


def seg_seg(A1, u1, A2, u2, dt):
    """sp_seg_seg's clamped parameters (s, t)."""
    zero, one = dt(0), dt(1)
    w = sub(A1, A2)
    a, e, f, c, b = na_dot(u1, u1), na_dot(u2, u2), na_dot(u2, w), na_dot(u1, w), na_dot(u1, u2)
    s = t = zero
    if a == zero and e == zero:
        pass
    elif a == zero:
        t = _clamp01(f / e, dt)
    elif e == zero:
        s = _clamp01(-c / a, dt)
    else:
        ae = a * e
        den = ae - b * b
        par = not (den > (dt(np.finfo(dt).eps) * dt(64)) * ae)
        s = zero if par else _clamp01((b * f - c * e) / den, dt)
        t = (b * s + f) / e
        if t < zero:
            t = zero; s = _clamp01(-c / a, dt)
        elif t > one:
            t = one; s = _clamp01((b - c) / a, dt)
    return s, t


class _Iso:
    def __init__(self, r, t):
        self.r, self.t = r, t

    def inverse(self, dt):
        ri = qinverse(self.r)
        return _Iso(ri, na_qrot(ri, neg(self.t), dt))

    def point(self, p, dt):
        return add(na_qrot(self.r, p, dt), self.t)

    def inv_vec(self, v, dt):
        return na_qrot(qinverse(self.r), v, dt)

    def inv_point(self, p, dt):
        return na_qrot(qinverse(self.r), sub(p, self.t), dt)


class _Emit:
    """NpEmit + NpArraySink: the world normal and the points as contact_query::contact_manifolds returns them."""

    def __init__(self, rot1, dt):
        self.rot1, self.dt = rot1, dt
        self.normal = None
        self.points = []   # (anchor1, penetration, fid1, fid2)

    def world_normal(self, local_n1):
        dt = self.dt
        ln = _div(local_n1, _norm(local_n1))
        self.normal = R.qrot(self.rot1, ln, dt)
        return bool(abs(R.dot(self.normal, self.normal) - dt(1)) <= dt(2e-4))

    def push(self, local_p1, dist, f1, f2):
        if len(self.points) >= MAX_POINTS:
            return
        dt = self.dt
        point1 = R.qrot(self.rot1, local_p1, dt)
        anchor1 = add(point1, scale(scale(self.normal, dist), dt(0.5)))
        self.points.append((anchor1, -dist, f1, f2))


def _tri_ball(tri, flags, flipped, r, p, pred, em, dt):
    zero = dt(0)
    a, b, c = tri
    q, region = closest_point(a, b, c, p.t, dt)
    d = sub(p.t, q)
    dist = _norm(d)
    if not (dist > zero) or not (dist <= r + pred):
        return False
    n = _div(d, dist)
    sd = dist - r
    if tri_interior(flags, region):
        N = unit_normal(a, b, c)
        n = neg(N) if na_dot(N, d) < zero else N
        sd = na_dot(d, n) - r
    if flipped:
        n_ball = p.inv_vec(neg(n), dt)
        if not em.world_normal(n_ball):
            return False
        em.push(scale(n_ball, r), sd, fid_face(0), tri_fid(region))
    else:
        if not em.world_normal(n):
            return False
        em.push(q, sd, tri_fid(region), fid_face(0))
    return True


def _tri_capsule(tri, flags, flipped, r, h, p, pred, em, dt):
    zero, one = dt(0), dt(1)
    a, b, c = tri
    hv = na_qrot(p.r, (zero, h, zero), dt)
    A, u = sub(p.t, hv), scale(hv, dt(2))
    B = add(A, u)
    N = unit_normal(a, b, c)
    da, db = na_dot(N, sub(A, a)), na_dot(N, sub(B, a))
    if (da > zero and db < zero) or (da < zero and db > zero):
        _, rg = closest_point(a, b, c, add(A, scale(u, da / (da - db))), dt)
        if rg == 0:
            mid = add(A, scale(u, dt(0.5)))
            n = neg(N) if na_dot(N, sub(mid, a)) < zero else N
            pd = B if na_dot(n, u) < zero else A
            dd = na_dot(n, sub(pd, a))
            if flipped:
                if not em.world_normal(p.inv_vec(neg(n), dt)):
                    return False
                em.push(p.inv_point(sub(pd, scale(n, r)), dt), dd - r, fid_face(0), fid_face(0))
            else:
                if not em.world_normal(n):
                    return False
                em.push(sub(pd, scale(n, dd)), dd - r, fid_face(0), fid_face(0))
            return True
    best = [dt(np.inf), A, a, 4]

    def attempt(ps, pt, region):
        d = sub(ps, pt)
        d2 = na_dot(d, d)
        if d2 < best[0]:
            best[:] = [d2, ps, pt, region]
    q0, rg = closest_point(a, b, c, A, dt)
    attempt(A, q0, rg)
    q1, rg = closest_point(a, b, c, B, dt)
    attempt(B, q1, rg)
    for k in range(3):
        vk, vn = tri[k], tri[(k + 1) % 3]
        ek = sub(vn, vk)
        s, t = seg_seg(A, u, vk, ek, dt)
        attempt(add(A, scale(u, s)), add(vk, scale(ek, t)), 4 + k if t == zero else (4 + (k + 1) % 3 if t == one else 1 + k))
    d2, ps, pt, region = best
    dist = np.sqrt(d2)
    if not (dist > zero) or not (dist <= r + pred):
        return False
    d = sub(ps, pt)
    n = _div(d, dist)
    sd = dist - r
    face = region == 0
    if face or tri_interior(flags, region):
        n = neg(N) if na_dot(N, d) < zero else N
        sd = na_dot(d, n) - r
    if not em.world_normal(p.inv_vec(neg(n), dt) if flipped else n):
        return False
    if face and na_dot(u, u) > zero:
        lo, hi = zero, one
        empty = False
        for k in range(3):
            vk, vn = tri[k], tri[(k + 1) % 3]
            m = na_cross(N, sub(vn, vk))
            g0, gu = na_dot(m, sub(A, vk)), na_dot(m, u)
            if gu != zero:
                tk = -g0 / gu
                if gu > zero:
                    if tk > lo:
                        lo = tk
                elif tk < hi:
                    hi = tk
            elif g0 < zero:
                empty = True
        if not empty and lo < hi:
            for k, sk in enumerate((lo, hi)):
                x = add(A, scale(u, sk))
                dcore = na_dot(n, sub(x, a))
                if not (dcore <= r + pred):
                    continue
                if flipped:
                    em.push(p.inv_point(sub(x, scale(n, r)), dt), dcore - r, fid_vertex(k), fid_face(0))
                else:
                    em.push(sub(x, scale(n, dcore)), dcore - r, fid_face(0), fid_vertex(k))
            return True
    if flipped:
        em.push(p.inv_point(sub(ps, scale(n, r)), dt), sd, fid_face(0), tri_fid(region))
    else:
        em.push(pt, sd, tri_fid(region), fid_face(0))
    return True


def _box_axis(he, v, L):
    """(sep, d): the separation along the unit axis L, d = +-L from the box towards the triangle."""
    p0, p1, p2 = na_dot(L, v[0]), na_dot(L, v[1]), na_dot(L, v[2])
    tmin, tmax = (p0, p1) if p0 < p1 else (p1, p0)
    tmin = p2 if p2 < tmin else tmin
    tmax = p2 if p2 > tmax else tmax
    rb = (abs(L[0]) * he[0] + abs(L[1]) * he[1]) + abs(L[2]) * he[2]
    sp, sm = tmin - rb, -tmax - rb
    return (sp, L) if sp >= sm else (sm, neg(L))


def _support_region(v, d):
    p0, p1, p2 = na_dot(d, v[0]), na_dot(d, v[1]), na_dot(d, v[2])
    m = p0 if p0 < p1 else p1
    m = p2 if p2 < m else m
    e0, e1, e2 = p0 == m, p1 == m, p2 == m
    if e0 and e1 and e2:
        return 0
    if e0 and e1:
        return 1
    if e1 and e2:
        return 2
    if e2 and e0:
        return 3
    return 4 if e0 else (5 if e1 else 6)


def _face_axis_admissible(flags, v, d, i, he):
    """Whether box face i may give the manifold's direction: the triangle's lowest feature along d must carry the contact.  The whole face (the three
    projections tie) always does.  An edge or a vertex does if it is real (not interior by the edge flags) AND one of its vertices lies over the box
    face, |x_j| <= he_j on the two other axes: a lowest vertex beside the face touches nothing of it, however small the overlap along the axis is --
    that is the ghost normal of a box side against a face it merely overlaps."""
    region = _support_region(v, d)
    if region == 0:
        return True
    if tri_interior(flags, region):
        return False
    low = (region - 1, region % 3) if region < 4 else (region - 4,)
    return any(all(abs(v[k][j]) <= he[j] for j in range(3) if j != i) for k in low)


def _clip(poly, m, c, plane, dt):
    """Sutherland - Hodgman, one plane: keeps dot(m, x) + c >= 0.  poly: list of (point, raw id, tag of the edge that leaves it)."""
    zero = dt(0)
    out = []
    n = len(poly)
    for i in range(n):
        P, pid, tag = poly[i]
        Q = poly[(i + 1) % n][0]
        gp, gq = na_dot(m, P) + c, na_dot(m, Q) + c
        pin, qin = gp >= zero, gq >= zero
        if pin and len(out) < 8:
            out.append((P, pid, tag))
        if pin != qin and len(out) < 8:
            X = add(P, scale(sub(Q, P), gp / (gp - gq)))
            out.append((X, ((1 << 8) | (tag << 4) | plane) if tag < 4 else ((2 << 8) | ((tag - 4) << 4) | plane), 4 + plane if pin else tag))
    return out


def cuboid_support_face(he, d, dt):
    """avn_narrow.h cuboid_support_face: (corners, vertex ids, edge ids, face id)."""
    zero, one = dt(0), dt(1)
    ax, ay, az = abs(d[0]), abs(d[1]), abs(d[2])
    iamax, mx = 0, ax
    if ay > mx:
        mx, iamax = ay, 1
    if az > mx:
        mx, iamax = az, 2
    sign = np.copysign(one, d[iamax])
    hx, hy, hz = he
    if iamax == 0:
        v = [(hx * sign, hy, hz), (hx * sign, -hy, hz), (hx * sign, -hy, -hz), (hx * sign, hy, -hz)]
    elif iamax == 1:
        v = [(hx, hy * sign, hz), (-hx, hy * sign, hz), (-hx, hy * sign, -hz), (hx, hy * sign, -hz)]
    else:
        v = [(hx, hy, hz * sign), (hx, -hy, hz * sign), (-hx, -hy, hz * sign), (-hx, hy, hz * sign)]
    code = [(1 if p[0] < zero else 0) | (2 if p[1] < zero else 0) | (4 if p[2] < zero else 0) for p in v]
    vid = [fid_vertex(k) for k in code]
    eid = []
    for k in range(4):
        a, b = code[k], code[(k + 1) & 3]
        eid.append(fid_edge((max(a, b) << 3) | min(a, b) | 0xC0))
    return v, vid, eid, fid_face(iamax + (3 if sign > zero else 0) + 10)


def _tri_cuboid(tri, flags, flipped, he, q, pred, em, dt):
    zero, one = dt(0), dt(1)
    eps = dt(np.finfo(dt).eps)
    v = [q.point(x, dt) for x in tri]
    N = unit_normal(v[0], v[1], v[2])
    best, bd, kind = -dt(np.finfo(dt).max), (zero, zero, zero), 3
    for i in range(3):
        sep, d = _box_axis(he, v, tuple(one if j == i else zero for j in range(3)))
        if sep > pred:
            return False
        if _face_axis_admissible(flags, v, d, i, he) and sep > best:
            best, bd, kind = sep, d, i
    sep, d = _box_axis(he, v, N)
    if sep > pred:
        return False
    if sep > best:
        best, bd, kind = sep, d, 3
    for k in range(3):
        ek = sub(v[(k + 1) % 3], v[k])
        el = _norm(ek)
        for i in range(3):
            cx = (zero, -ek[2], ek[1]) if i == 0 else ((ek[2], zero, -ek[0]) if i == 1 else (-ek[1], ek[0], zero))
            nl = _norm(cx)
            if not (nl > eps * el):
                continue
            sep, d = _box_axis(he, v, _div(cx, nl))
            if sep > pred:
                return False
            # (a flagged edge gives the direction only where the edge itself is the triangle's lowest feature along it: where the opposite vertex lies
            #  strictly lower the axis would speak for an edge that touches nothing)
            if (flags & (1 << k)) and not (na_dot(d, v[(k + 2) % 3]) < na_dot(d, v[k])) and sep > best:
                best, bd, kind = sep, d, 4 + 3 * k + i
    if not em.world_normal(bd if flipped else q.inv_vec(neg(bd), dt)):
        return False
    if kind >= 4:
        k, i = (kind - 4) // 3, (kind - 4) % 3
        vk = v[k]
        ek = sub(v[(k + 1) % 3], vk)
        sp = tuple(np.copysign(hh, x) for hh, x in zip(he, bd))
        hi_ = he[i]
        A1 = tuple(-hi_ if j == i else sp[j] for j in range(3))
        u1 = tuple(hi_ * dt(2) if j == i else zero for j in range(3))
        s, t = seg_seg(A1, u1, vk, ek, dt)
        pb, pt = add(A1, scale(u1, s)), add(vk, scale(ek, t))
        dist = na_dot(sub(pt, pb), bd)
        fidt = fid_edge(k)
        lo = sum((1 << j) for j in range(3) if j != i and sp[j] < zero)
        fidb = fid_edge(((lo | (1 << i)) << 3) | lo | 0xC0)
        if flipped:
            em.push(pb, dist, fidb, fidt)
        else:
            em.push(q.inv_point(pt, dt), dist, fidt, fidb)
        return True
    if kind < 3:
        i = kind
        sg = one if bd[i] > zero else -one
        poly = [(v[m], m, m) for m in range(3)]
        plane = 0
        for j in range(3):
            if j == i:
                continue
            poly = _clip(poly, tuple(-one if jj == j else zero for jj in range(3)), he[j], plane, dt); plane += 1
            poly = _clip(poly, tuple(one if jj == j else zero for jj in range(3)), he[j], plane, dt); plane += 1
        hf = he[i]
        fidb = fid_face(i + (3 if sg > zero else 0) + 10)
        for x, pid, _ in poly:
            dist = sg * x[i] - hf
            if not (dist <= pred):
                continue
            ka, kb = (pid >> 4) & 15, pid & 15
            fidt = fid_vertex(kb) if (pid >> 8) == 0 else (fid_edge(ka | ((kb + 1) << 2)) if (pid >> 8) == 1 else fid_face(16 + ka * 4 + kb))
            if flipped:
                em.push(tuple(sg * hf if j == i else x[j] for j in range(3)), dist, fidb, fidt)
            else:
                em.push(q.inv_point(x, dt), dist, fidt, fidb)
        return True
    fv, vid, eid, ffid = cuboid_support_face(he, bd, dt)
    poly = [(fv[m], m, m) for m in range(4)]
    for k in range(3):
        vk, vn = v[k], v[(k + 1) % 3]
        m = na_cross(N, sub(vn, vk))
        poly = _clip(poly, m, -na_dot(m, vk), k, dt)
    for x, pid, _ in poly:
        dist = na_dot(bd, sub(v[0], x))
        if not (dist <= pred):
            continue
        ka, kb = (pid >> 4) & 15, pid & 15
        fidb = vid[kb & 3] if (pid >> 8) == 0 else ((eid[ka & 3] | ((kb + 1) << 8)) if (pid >> 8) == 1 else (ffid | ((1 + ka * 3 + kb) << 8)))
        if flipped:
            em.push(x, dist, fidb, fid_face(0))
        else:
            em.push(q.inv_point(add(x, scale(bd, dist)), dt), dist, fid_face(0), fidb)
    return True


def manifold(shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, pred, tri, flags, dt):
    """One pair that holds a triangle (`tri`: its three vertices, of shape 1 if that is a triangle, else of shape 2): (normal, points) or None.
    points: [(anchor1, penetration, fid1, fid2)]."""
    S_ = lambda a: tuple(dt(x) for x in a)
    he1, pos1, rot1, he2, pos2, rot2, pred = S_(he1), S_(pos1), S_(rot1), S_(he2), S_(pos2), S_(rot2), dt(pred)
    tri = tuple(S_(x) for x in np.asarray(tri).reshape(3, 3))
    flags = int(flags)
    tri1, tri2 = shape1 == SHAPE_TRIANGLE, shape2 == SHAPE_TRIANGLE
    if tri1 and tri2:
        return None   # (not built)
    with np.errstate(all="ignore"):
        r1m, r2m = S.make_isometry_rotation(rot1, dt), S.make_isometry_rotation(rot2, dt)
        ri = qinverse(r1m)
        pos12 = _Iso(na_qmul(ri, r2m), na_qrot(ri, sub(pos2, pos1), dt))
        em = _Emit(rot1, dt)
        flipped = not tri1
        other = shape1 if flipped else shape2
        heo = he1 if flipped else he2
        if other == SHAPE_CUBOID:
            ok = _tri_cuboid(tri, flags, flipped, heo, pos12 if flipped else pos12.inverse(dt), pred, em, dt)
        else:
            p = pos12.inverse(dt) if flipped else pos12
            if other == SHAPE_BALL:
                ok = _tri_ball(tri, flags, flipped, heo[0], p, pred, em, dt)
            elif other == SHAPE_CAPSULE:
                ok = _tri_capsule(tri, flags, flipped, heo[0], heo[1], p, pred, em, dt)
            else:
                ok = False
    if not ok or not em.points:
        return None
    return em.normal, em.points


def manifolds(shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction, vertices1, vertices2, flags1, flags2, dt):
    """The manifolds of the rows that hold a triangle (the other rows come back empty), in the layout of World.contact_manifolds (plus the triangles' vertices and edge flags per row)."""
    n = len(shape1)
    A = lambda a, k: np.asarray(a, dt).reshape(n, k)
    he1, pos1, rot1, he2, pos2, rot2 = A(he1, 3), A(pos1, 3), A(rot1, 4), A(he2, 3), A(pos2, 3), A(rot2, 4)
    pred = np.broadcast_to(np.asarray(prediction, dt), (n,))
    v1 = None if vertices1 is None else A(vertices1, 9)
    v2 = None if vertices2 is None else A(vertices2, 9)
    f1 = np.full(n, ALL_EDGES, np.uint8) if flags1 is None else np.asarray(flags1, np.uint8)
    f2 = np.full(n, ALL_EDGES, np.uint8) if flags2 is None else np.asarray(flags2, np.uint8)
    out = dict(point_count=np.zeros(n, np.uint8), normal=np.zeros((n, 3), dt), anchor1=np.zeros((n, MAX_POINTS, 3), dt), anchor2=np.zeros((n, MAX_POINTS, 3), dt),
               point=np.zeros((n, MAX_POINTS, 3), dt), penetration=np.zeros((n, MAX_POINTS), dt), feature_id1=np.zeros((n, MAX_POINTS), np.uint32),
               feature_id2=np.zeros((n, MAX_POINTS), np.uint32))
    for i in range(n):
        t1, t2 = shape1[i] == SHAPE_TRIANGLE, shape2[i] == SHAPE_TRIANGLE
        if not (t1 or t2):
            continue
        m = manifold(int(shape1[i]), he1[i], pos1[i], rot1[i], int(shape2[i]), he2[i], pos2[i], rot2[i], pred[i], v1[i] if t1 else v2[i], f1[i] if t1 else f2[i], dt)
        if m is None:
            continue
        normal, pts = m
        d12 = sub(tuple(dt(x) for x in pos1[i]), tuple(dt(x) for x in pos2[i]))
        out["point_count"][i] = len(pts)
        out["normal"][i] = normal
        for j, (a1, pen, g1, g2) in enumerate(pts):
            out["anchor1"][i, j] = a1
            out["anchor2"][i, j] = add(a1, d12)
            out["point"][i, j] = add(tuple(dt(x) for x in pos1[i]), a1)
            out["penetration"][i, j] = pen
            out["feature_id1"][i, j] = g1; out["feature_id2"][i, j] = g2
    return out


def aabb(vertices, pos, rot, dt):
    """The component-wise min / max of position + qrot(rotation, v) over the three vertices (one triangle; scalars)."""
    pos, rot = tuple(dt(x) for x in pos), tuple(dt(x) for x in rot)
    pts = [add(pos, R.qrot(rot, tuple(dt(x) for x in v), dt)) for v in np.asarray(vertices).reshape(3, 3)]
    mn = tuple(min(p[k] for p in pts) for k in range(3))
    mx = tuple(max(p[k] for p in pts) for k in range(3))
    return mn, mx


class TriangleHost:
    """AnyCollider::aabb_with_context / contact_manifolds_with_context of triangles held as AVN_SHAPE_HOST, answered from the definitions above.
    `shape` / `half_extents` / `vertices` / `edge_flags` by collider entity: the REAL kinds (triangles are SHAPE_TRIANGLE here whatever the world
    was told)."""

    def __init__(self, entity_index, shape, half_extents, vertices, edge_flags=None):
        n = len(entity_index)
        flags = np.full(n, ALL_EDGES, np.uint8) if edge_flags is None else np.asarray(edge_flags, np.uint8)
        self.shape = {int(e): int(s) for e, s in zip(entity_index, shape)}
        self.he = {int(e): np.asarray(x, np.float64) for e, x in zip(entity_index, half_extents)}
        self.tri = {int(e): np.asarray(x, np.float64).reshape(9) for e, x in zip(entity_index, np.asarray(vertices).reshape(n, 9))}
        self.flags = {int(e): int(f) for e, f in zip(entity_index, flags)}
        self.manifold_queries = 0
        self.kinds = {}    # (kind pair, point count) -> queries: the coverage the closed-loop tests assert

    def aabb(self, q, out):
        dt = q["start_position"].dtype.type
        for i in range(len(q)):
            tri = self.tri[int(q["collider"][i])].astype(dt)
            mn, mx = aabb(tri, q["start_position"][i], q["start_rotation"][i], dt)
            if q["swept"][i]:   # swept_aabb_with_context's default: aabb(start).merged(aabb(end))
                mn1, mx1 = aabb(tri, q["end_position"][i], q["end_rotation"][i], dt)
                mn, mx = tuple(min(a, b) for a, b in zip(mn, mn1)), tuple(max(a, b) for a, b in zip(mx, mx1))
            out["min"][i] = mn; out["max"][i] = mx

    def manifolds(self, q, out):
        dt = q["position1"].dtype.type
        n = len(q)
        self.manifold_queries += n
        for i in range(n):
            e1, e2 = int(q["collider1"][i]), int(q["collider2"][i])
            s1, s2 = self.shape[e1], self.shape[e2]
            assert s1 == SHAPE_TRIANGLE or s2 == SHAPE_TRIANGLE
            et = e1 if s1 == SHAPE_TRIANGLE else e2
            m = manifold(s1, self.he[e1], q["position1"][i], q["rotation1"][i], s2, self.he[e2], q["position2"][i], q["rotation2"][i], q["max_contact_distance"][i],
                         self.tri[et].astype(dt), self.flags[et], dt)
            out["point_count"][i] = 0
            count = 0
            if m is not None:
                normal, pts = m
                count = len(pts)
                out["point_count"][i] = count
                out["normal"][i] = normal
                for j, (a1, pen, g1, g2) in enumerate(pts):
                    out["anchor1"][i, j] = a1; out["penetration"][i, j] = pen
                    out["feature_id1"][i, j] = g1; out["feature_id2"][i, j] = g2
            key = (tuple(sorted((s1, s2))), count)
            self.kinds[key] = self.kinds.get(key, 0) + 1


class MeshHost:
    """The host of a mesh scene on a backend WITHOUT the triangle and the capsule kind (the oracle): triangles and capsules are both AVN_SHAPE_HOST there.
    A pair that holds a triangle is answered by TriangleHost, a capsule pair without one by the capsule collider's reference (CapsuleHost); boxes likewise."""

    def __init__(self, entity_index, shape, half_extents, vertices, edge_flags=None):
        import capsule_collider_reference as CC
        self.triangles = TriangleHost(entity_index, shape, half_extents, vertices, edge_flags)
        self.capsules = CC.CapsuleHost(entity_index, shape, half_extents)
        self.shape = self.triangles.shape

    @property
    def kinds(self):
        return self.triangles.kinds

    @property
    def manifold_queries(self):
        return self.triangles.manifold_queries

    def aabb(self, q, out):
        tri = np.array([self.shape[int(e)] == SHAPE_TRIANGLE for e in q["collider"]], bool)
        for rows, host in ((tri, self.triangles), (~tri, self.capsules)):
            if rows.any():
                sub = out[rows].copy()
                host.aabb(q[rows], sub)
                out[rows] = sub

    def manifolds(self, q, out):
        tri = np.array([self.shape[int(a)] == SHAPE_TRIANGLE or self.shape[int(b)] == SHAPE_TRIANGLE for a, b in zip(q["collider1"], q["collider2"])], bool)
        for rows, host in ((tri, self.triangles), (~tri, self.capsules)):
            if rows.any():
                sub = out[rows].copy()
                host.manifolds(q[rows], sub)
                out[rows] = sub
