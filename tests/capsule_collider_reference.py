"""numpy restatement of the Capsule COLLIDER of include/avian_mi355x.h ("capsule colliders"): its AABB and its contact manifolds against a Ball, a
Cuboid or another Capsule in either order, written from the header's text in scalars of the world's type with no fused multiply-adds, in the
header's operation order -- so a device that follows the header agrees bit for bit.  The core geometry (P, X) is the capsule query shape's
restatement (spatial_capsule_reference.py), as the header shares it.  Everything broadcasts over the pairs of a batch: vectors are tuples of
three arrays, quaternions of four.

`CapsuleHost` answers the two host-shape callbacks from these functions: a world that holds its capsules as AVN_SHAPE_HOST and asks this class
must equal the world that holds them as AVN_SHAPE_CAPSULE."""
from __future__ import annotations

import numpy as np

import spatial_capsule_reference as C
import spatial_query_reference as R
import spatial_shape_reference as S
from spatial_query_reference import add, qinverse, scale, sub
from spatial_shape_reference import na_dot, na_qmul, na_qrot, neg

SHAPE_CUBOID, SHAPE_BALL, SHAPE_HOST, SHAPE_CAPSULE = 0, 1, 2, 3
MAX_POINTS = 16   # AVN_MAX_QUERY_POINTS
_w = np.where


def fid_vertex(c):
    return np.uint32((1 << 30) | c)


def fid_face(c):
    return np.uint32((3 << 30) | c)


def parallel_threshold(dt):
    """sin^2 of the angle under which two capsule axes count as parallel: 64 eps."""
    return dt(np.finfo(dt).eps) * dt(64)


def _clamp01(x, dt):
    return _w(x < dt(0), dt(0), _w(x > dt(1), dt(1), x))


def _norm(v):
    return np.sqrt(na_dot(v, v))


def _vget(v, i):
    return _w(i == 0, v[0], _w(i == 1, v[1], v[2]))


def aabb(he, pos, rot, dt):
    """position -+ (|qrot(rotation, (0, h, 0))| + (r, r, r)): the capsule query shape's box (one definition for both)."""
    return C.capsule_aabb(he, pos, rot, dt)


class _Points:
    """Up to two candidate points per row in emission order: (valid, local_p1, signed distance, fid1, fid2)."""

    def __init__(self, n, dt):
        self.n, self.dt = n, dt
        self.valid = [np.zeros(n, bool), np.zeros(n, bool)]
        self.p = [tuple(np.zeros(n, dt) for _ in range(3)) for _ in range(2)]
        self.dist = [np.zeros(n, dt), np.zeros(n, dt)]
        self.f1 = [np.zeros(n, np.uint32), np.zeros(n, np.uint32)]
        self.f2 = [np.zeros(n, np.uint32), np.zeros(n, np.uint32)]

    def put(self, k, rows, valid, p, dist, f1, f2):
        v = rows & valid
        self.valid[k] = _w(rows, v, self.valid[k])
        self.p[k] = tuple(_w(rows, a, b) for a, b in zip(p, self.p[k]))
        self.dist[k] = _w(rows, dist, self.dist[k])
        self.f1[k] = _w(rows, f1, self.f1[k]).astype(np.uint32)
        self.f2[k] = _w(rows, f2, self.f2[k]).astype(np.uint32)


def _capsule_capsule(he1, he2, q12r, q12t, pred, dt, pts, rows):
    """(manifold, local_n1) of the rows; the points go to pts."""
    zero, one, two_ = dt(0), dt(1), dt(2)
    n = len(pred)
    z = np.zeros(n, dt)
    r1, r2 = he1[0], he2[0]
    A1, u1 = (z, -he1[1], z), (z, he1[1] * two_, z)
    A2, u2 = C.capsule_core(q12r, q12t, he2[1], dt)
    w = sub(A1, A2)
    a, e, f, c, b = na_dot(u1, u1), na_dot(u2, u2), na_dot(u2, w), na_dot(u1, w), na_dot(u1, u2)
    ae = a * e
    den = ae - b * b
    par_g = ~(den > parallel_threshold(dt) * ae)
    s_g = _w(par_g, zero, _clamp01((b * f - c * e) / den, dt))
    t_g = (b * s_g + f) / e
    lt = t_g < zero
    gt = ~lt & (t_g > one)
    s_g = _w(lt, _clamp01(-c / a, dt), _w(gt, _clamp01((b - c) / a, dt), s_g))
    t_g = _w(lt, zero, _w(gt, one, t_g))
    case0 = (a == zero) & (e == zero)
    case1 = ~case0 & (a == zero)
    case2 = ~case0 & ~case1 & (e == zero)
    gen = ~case0 & ~case1 & ~case2
    s = _w(case0 | case1, zero, _w(case2, _clamp01(-c / a, dt), s_g))
    t = _w(case0 | case2, zero, _w(case1, _clamp01(f / e, dt), t_g))
    par = gen & par_g
    # parallel axes with overlapping projections: two points
    sa, sb = -c / a, (b - c) / a
    lo, hi = _w(sa < sb, sa, sb), _w(sa < sb, sb, sa)
    lo = _w(lo < zero, zero, lo)
    hi = _w(hi > one, one, hi)
    two = par & (lo < hi)
    sm = (lo + hi) * dt(0.5)
    tm = _clamp01((b * sm + f) / e, dt)
    dm = sub(add(A2, scale(u2, tm)), add(A1, scale(u1, sm)))
    dp = sub(dm, scale(u1, na_dot(dm, u1) / a))
    ln = _norm(dp)
    n2 = tuple(x / ln for x in dp)
    ok2 = ln > zero
    for k, sk in enumerate((lo, hi)):
        tk = _clamp01((b * sk + f) / e, dt)
        p1 = add(A1, scale(u1, sk))
        dk = na_dot(sub(add(A2, scale(u2, tk)), p1), n2)
        pts.put(k, rows & two, dk <= (r1 + r2) + pred, add(p1, scale(n2, r1)), (dk - r1) - r2, fid_vertex(k), fid_vertex(k))
    # the closest points of the two segments: one point
    p1 = add(A1, scale(u1, s))
    d = sub(add(A2, scale(u2, t)), p1)
    dist = _norm(d)
    ok1 = (dist > zero) & (dist <= (r1 + r2) + pred)
    n1 = tuple(x / dist for x in d)
    pts.put(0, rows & ~two, ok1, add(p1, scale(n1, r1)), (dist - r1) - r2, fid_face(0), fid_face(0))
    return _w(two, ok2, ok1), tuple(_w(two, x, y) for x, y in zip(n2, n1))


def _capsule_ball(flipped, r, h, rb, q12r, q12t, q21r, q21t, pred, dt, pts, rows):
    zero = dt(0)
    n = len(pred)
    z = np.zeros(n, dt)
    pr = tuple(_w(flipped, x, y) for x, y in zip(q21r, q12r))   # the ball in the capsule's frame
    pt = tuple(_w(flipped, x, y) for x, y in zip(q21t, q12t))
    A, u = (z, -h, z), (z, h * dt(2), z)
    d2, s = C.seg_point(A, u, pt, dt)
    dist = np.sqrt(d2)
    ok = (dist > zero) & (dist <= (r + rb) + pred)
    ps = add(A, scale(u, s))
    n_cap = tuple(x / dist for x in sub(pt, ps))
    sd = (dist - r) - rb
    n_ball = na_qrot(qinverse(pr), neg(n_cap), dt)
    local_n1 = tuple(_w(flipped, x, y) for x, y in zip(n_ball, n_cap))
    local_p1 = tuple(_w(flipped, x, y) for x, y in zip(scale(n_ball, rb), add(ps, scale(n_cap, r))))
    pts.put(0, rows, ok, local_p1, sd, fid_face(0), fid_face(0))
    return ok, local_n1


def seg_box_axis(A, u, he, dt):
    """The six-axis smallest-overlap rule of a segment that touches or crosses the box: (n towards the segment's midpoint, overlap, the box's radius along n)."""
    zero, inf = dt(0), dt(np.inf)
    eps = dt(np.finfo(dt).eps)
    shp = np.broadcast(A[0], u[0], he[0]).shape
    zv = tuple(np.zeros(shp, dt) for _ in range(3))
    one = np.ones(shp, dt)
    hv = scale(u, dt(0.5))
    m = add(A, hv)
    eps2 = eps * eps * na_dot(u, u)
    best = np.full(shp, inf, dt); brb = np.zeros(shp, dt)
    n = zv
    for k in range(6):
        if k < 3:
            ax = tuple(one if j == k else zv[0] for j in range(3))
            live = np.ones(shp, bool)
        else:
            cx = (zv[0], u[2], -u[1]) if k == 3 else ((-u[2], zv[0], u[0]) if k == 4 else (u[1], -u[0], zv[0]))
            l2 = na_dot(cx, cx)
            live = l2 > eps2
            nrm = np.sqrt(l2)
            ax = tuple(x / nrm for x in cx)
        rb = np.abs(ax[0]) * he[0] + np.abs(ax[1]) * he[1] + np.abs(ax[2]) * he[2]
        rs = np.abs(na_dot(ax, hv))
        c = na_dot(ax, m)
        ov = (rb + rs) - np.abs(c)
        upd = live & (ov < best)
        best = _w(upd, ov, best); brb = _w(upd, rb, brb)
        n = tuple(_w(upd, _w(c < zero, -a, a), b) for a, b in zip(ax, n))
    return n, best, brb


def _capsule_cuboid(flipped, r, h, heo, q12r, q12t, q21r, q21t, pred, dt, pts, rows):
    zero, one = dt(0), dt(1)
    n_rows = len(pred)
    qr = tuple(_w(flipped, x, y) for x, y in zip(q12r, q21r))   # the capsule in the cuboid's frame
    qt = tuple(_w(flipped, x, y) for x, y in zip(q12t, q21t))
    A, u = C.capsule_core(qr, qt, h, dt)
    f, _, ps, pb = C.seg_box(A, u, heo, dt)
    dist = np.sqrt(f)
    apart = dist > zero
    n_a = tuple((a - b) / dist for a, b in zip(ps, pb))
    n_z, best, brb = seg_box_axis(A, u, heo, dt)
    n = tuple(_w(apart, a, b) for a, b in zip(n_a, n_z))
    qri = qinverse(qr)
    local_n1 = tuple(_w(flipped, a, b) for a, b in zip(n, na_qrot(qri, neg(n), dt)))
    to_capsule = lambda p: na_qrot(qri, sub(p, qt), dt)   # iso_inv_point(q, p)
    fa = _w((n[1] == zero) & (n[2] == zero), 0, _w((n[0] == zero) & (n[2] == zero), 1, _w((n[0] == zero) & (n[1] == zero), 2, -1)))
    sg = _w((fa >= 0) & (_vget(n, fa) > zero), one, -one)
    fidb = _w(fa >= 0, (np.uint32(3 << 30) | (fa.astype(np.int64) + _w(sg > zero, 3, 0) + 10).astype(np.uint32)), np.uint32(0)).astype(np.uint32)
    lo, hi = np.zeros(n_rows, dt), np.ones(n_rows, dt)
    empty = np.zeros(n_rows, bool)
    for j in range(3):
        act = fa != j
        aj, uj, hj = A[j], u[j], heo[j]
        nz = uj != zero
        t1, t2 = (-hj - aj) / uj, (hj - aj) / uj
        t1, t2 = _w(uj < zero, t2, t1), _w(uj < zero, t1, t2)
        lo = _w(act & nz & (t1 > lo), t1, lo)
        hi = _w(act & nz & (t2 < hi), t2, hi)
        empty = empty | (act & ~nz & ((aj < -hj) | (aj > hj)))
    two = (fa >= 0) & (na_dot(u, u) > zero) & ~empty & (lo < hi)
    hf = _vget(heo, fa)
    for k, sk in enumerate((lo, hi)):
        x = add(A, scale(u, sk))
        dcore = sg * _vget(x, fa) - hf
        on_box = tuple(_w(fa == i, sg * hf, x[i]) for i in range(3))
        on_cap = to_capsule(sub(x, scale(n, r)))
        pts.put(k, rows & two, dcore <= r + pred, tuple(_w(flipped, a, b) for a, b in zip(on_box, on_cap)), dcore - r,
                _w(flipped, fidb, fid_vertex(k)), _w(flipped, fid_vertex(k), fidb))
    # one point: the closest pair of X ...
    one_a = rows & ~two & apart
    on_cap = to_capsule(sub(ps, scale(n, r)))
    pts.put(0, one_a, dist <= r + pred, tuple(_w(flipped, a, b) for a, b in zip(pb, on_cap)), dist - r, _w(flipped, fidb, fid_face(0)), _w(flipped, fid_face(0), fidb))
    # ... or, the segment touching / crossing the box, its end deepest along -n against the box's supporting plane
    one_z = rows & ~two & ~apart
    pd = tuple(_w(na_dot(n, u) < zero, a, b) for a, b in zip(add(A, u), A))
    on_box = add(pd, scale(n, brb - na_dot(n, pd)))
    on_cap = to_capsule(sub(pd, scale(n, r)))
    pts.put(0, one_z, np.ones(n_rows, bool), tuple(_w(flipped, a, b) for a, b in zip(on_box, on_cap)), -(best + r), _w(flipped, fidb, fid_face(0)), _w(flipped, fid_face(0), fidb))
    return np.ones(n_rows, bool), local_n1


def manifolds(shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction, dt):
    """The manifolds of the rows that hold a capsule (the other rows come back empty), in the layout of World.contact_manifolds.  Every row is
    computed on its own: a batch is answered kind by kind (capsule-capsule, capsule-ball, capsule-cuboid) only to spare the other kinds' arithmetic."""
    shape1, shape2 = np.asarray(shape1).astype(np.int64), np.asarray(shape2).astype(np.int64)
    n = len(shape1)
    cap1, cap2 = shape1 == SHAPE_CAPSULE, shape2 == SHAPE_CAPSULE
    other = np.where(cap1, shape2, shape1)
    groups = [g for g in (cap1 & cap2, (cap1 ^ cap2) & (other == SHAPE_BALL), (cap1 ^ cap2) & (other != SHAPE_BALL)) if g.any()]
    if len(groups) > 1:
        A = lambda a, k: np.asarray(a, dt).reshape(n, k)
        pred = np.broadcast_to(np.asarray(prediction, dt), (n,))
        out = None
        for g in groups:
            m = _manifolds(shape1[g], A(he1, 3)[g], A(pos1, 3)[g], A(rot1, 4)[g], shape2[g], A(he2, 3)[g], A(pos2, 3)[g], A(rot2, 4)[g], pred[g], dt)
            if out is None:
                out = {k: np.zeros((n,) + v.shape[1:], v.dtype) for k, v in m.items()}
            for k, v in m.items():
                out[k][g] = v
        return out
    return _manifolds(shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction, dt)


def _manifolds(shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction, dt):
    n = len(shape1)
    col = lambda a, k: tuple(np.ascontiguousarray(np.asarray(a, dt).reshape(n, k)[:, i]) for i in range(k))
    he1, pos1, rot1, he2, pos2, rot2 = col(he1, 3), col(pos1, 3), col(rot1, 4), col(he2, 3), col(pos2, 3), col(rot2, 4)
    pred = np.ascontiguousarray(np.broadcast_to(np.asarray(prediction, dt), (n,)))
    out = dict(point_count=np.zeros(n, np.uint8), normal=np.zeros((n, 3), dt), anchor1=np.zeros((n, MAX_POINTS, 3), dt), anchor2=np.zeros((n, MAX_POINTS, 3), dt),
               point=np.zeros((n, MAX_POINTS, 3), dt), penetration=np.zeros((n, MAX_POINTS), dt), feature_id1=np.zeros((n, MAX_POINTS), np.uint32),
               feature_id2=np.zeros((n, MAX_POINTS), np.uint32))
    cap1, cap2 = shape1 == SHAPE_CAPSULE, shape2 == SHAPE_CAPSULE
    rows = cap1 | cap2
    if not n or not rows.any():
        return out
    with np.errstate(all="ignore"):
        iso = lambda rot: tuple(np.array(c, dt) for c in zip(*[S.make_isometry_rotation([rot[0][i], rot[1][i], rot[2][i], rot[3][i]], dt) for i in range(n)]))
        r1m, r2m = iso(rot1), iso(rot2)
        ri = qinverse(r1m)
        q12r, q12t = na_qmul(ri, r2m), na_qrot(ri, sub(pos2, pos1), dt)   # pos12 = iso_inv_mul(isometry1, isometry2)
        q21r = qinverse(q12r)                                            # iso_inverse(pos12)
        q21t = na_qrot(q21r, neg(q12t), dt)
        flipped = ~cap1
        other = _w(flipped, shape1, shape2)
        heo = tuple(_w(flipped, a, b) for a, b in zip(he1, he2))
        r, h = _w(flipped, he2[0], he1[0]), _w(flipped, he2[1], he1[1])
        pts = _Points(n, dt)
        both = cap1 & cap2
        ball = rows & ~both & (other == SHAPE_BALL)
        box = rows & ~both & ~ball
        none = (np.zeros(n, bool), tuple(np.zeros(n, dt) for _ in range(3)))
        ok_c, n_c = _capsule_capsule(he1, he2, q12r, q12t, pred, dt, pts, both) if both.any() else none
        ok_b, n_b = _capsule_ball(flipped, r, h, heo[0], q12r, q12t, q21r, q21t, pred, dt, pts, ball) if ball.any() else none
        ok_x, n_x = _capsule_cuboid(flipped, r, h, heo, q12r, q12t, q21r, q21t, pred, dt, pts, box) if box.any() else none
        ok = _w(both, ok_c, _w(ball, ok_b, ok_x)) & rows
        local_n1 = tuple(_w(both, a, _w(ball, b, c)) for a, b, c in zip(n_c, n_b, n_x))
        # np_world_normal: normalise, rotate by the collider's own rotation, is_normalized
        ln = _norm(local_n1)
        normal = R.qrot(rot1, tuple(x / ln for x in local_n1), dt)
        ok = ok & (np.abs(R.dot(normal, normal) - dt(1)) <= dt(2e-4))
        d12 = sub(pos1, pos2)
        count = np.zeros(n, np.int64)
        for k in range(2):
            v = ok & pts.valid[k]
            point1 = R.qrot(rot1, pts.p[k], dt)
            anchor1 = add(point1, scale(scale(normal, pts.dist[k]), dt(0.5)))
            anchor2 = add(anchor1, d12)
            point = add(pos1, anchor1)
            for i in np.nonzero(v)[0]:
                j = count[i]
                out["anchor1"][i, j] = [x[i] for x in anchor1]; out["anchor2"][i, j] = [x[i] for x in anchor2]; out["point"][i, j] = [x[i] for x in point]
                out["penetration"][i, j] = -pts.dist[k][i]
                out["feature_id1"][i, j] = pts.f1[k][i]; out["feature_id2"][i, j] = pts.f2[k][i]
            count += v
        has = count > 0
        out["point_count"][:] = count
        out["normal"][:] = np.stack([_w(has, x, dt(0)) for x in normal], axis=1)
    return out


class CapsuleHost:
    """AnyCollider::aabb_with_context / contact_manifolds_with_context of capsules held as AVN_SHAPE_HOST, answered from the definitions above.
    `shape` / `half_extents` by collider entity: the REAL kinds (capsules are SHAPE_CAPSULE here whatever the world was told)."""

    def __init__(self, entity_index, shape, half_extents):
        self.shape = {int(e): int(s) for e, s in zip(entity_index, shape)}
        self.he = {int(e): np.asarray(x, np.float64) for e, x in zip(entity_index, half_extents)}
        self.manifold_queries = 0
        self.kinds = {}    # (kind pair, point count) -> queries: the coverage the closed-loop tests assert

    def aabb(self, q, out):
        dt = q["start_position"].dtype.type
        n = len(q)
        he = np.array([self.he[int(e)] for e in q["collider"]], dt).reshape(n, 3)
        cols = lambda a, k: tuple(np.asarray(a, dt).reshape(n, k)[:, i] for i in range(k))
        mn, mx = aabb(cols(he, 3), cols(q["start_position"], 3), cols(q["start_rotation"], 4), dt)
        mn1, mx1 = aabb(cols(he, 3), cols(q["end_position"], 3), cols(q["end_rotation"], 4), dt)
        sw = q["swept"] != 0
        for i in range(3):   # swept_aabb_with_context's default: aabb(start).merged(aabb(end))
            out["min"][:, i] = np.where(sw, np.minimum(mn[i], mn1[i]), mn[i]); out["max"][:, i] = np.where(sw, np.maximum(mx[i], mx1[i]), mx[i])

    def manifolds(self, q, out):
        dt = q["position1"].dtype.type
        n = len(q)
        self.manifold_queries += n
        s1 = np.array([self.shape[int(e)] for e in q["collider1"]]); s2 = np.array([self.shape[int(e)] for e in q["collider2"]])
        assert ((s1 == SHAPE_CAPSULE) | (s2 == SHAPE_CAPSULE)).all()
        m = manifolds(s1, np.array([self.he[int(e)] for e in q["collider1"]]), q["position1"], q["rotation1"],
                      s2, np.array([self.he[int(e)] for e in q["collider2"]]), q["position2"], q["rotation2"], q["max_contact_distance"], dt)
        out["point_count"][:] = m["point_count"]
        out["normal"][:] = m["normal"]
        out["anchor1"][:] = m["anchor1"]; out["penetration"][:] = m["penetration"]
        out["feature_id1"][:] = m["feature_id1"]; out["feature_id2"][:] = m["feature_id2"]
        for a, b, c in zip(s1, s2, m["point_count"]):
            key = (tuple(sorted((int(a), int(b)))), int(c))
            self.kinds[key] = self.kinds.get(key, 0) + 1
