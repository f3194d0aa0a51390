"""numpy restatement of the point-projection and shape-intersection tests of include/avian_mi355x_spatial.h, in the device's operation order
(k_spatial.hip: sp_project_exact, sp_shape_exact, sp_point_box_distance; avn_narrow.h: nalgebra arithmetic, make_isometry and the SAT
functions), and brute-force versions of avn_spatial_project_points / avn_spatial_shape_intersections with the same filter, tie and cap rules.

Built on spatial_query_reference (vectors are tuples of three arrays, quaternions of four; everything in the world's dtype, no fused
multiply-adds).  make_isometry runs once per query shape and is written with scalars; the pair tests broadcast over (query, collider)."""
from __future__ import annotations

import numpy as np

import spatial_query_reference as R
from spatial_query_reference import MISS, SHAPE_BALL, SHAPE_CUBOID, SHAPE_HOST, add, dot, qinverse, qrot, scale, sub


# ---- avn_narrow.h: nalgebra arithmetic -----------------------------------------------------------------------------------------------------
def na_cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def na_dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def neg(a):
    return tuple(-x for x in a)


def na_qrot(q, v, dt):
    qv = (q[0], q[1], q[2])
    t = scale(na_cross(qv, v), dt(2))
    c = na_cross(qv, t)
    return add(add(scale(t, q[3]), c), v)


def na_qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)


def support(he, d):
    return tuple(np.copysign(h, x) for h, x in zip(he, d))


# ---- avn_narrow.h / avn_math.h: the build's libm, scalars ----------------------------------------------------------------------------------
def atan_pos(x, dt):
    if x < dt(0.4375):
        i = -1
    elif x < dt(0.6875):
        i = 0; x = (dt(2) * x - dt(1)) / (dt(2) + x)
    elif x < dt(1.1875):
        i = 1; x = (x - dt(1)) / (x + dt(1))
    elif x < dt(2.4375):
        i = 2; x = (x - dt(1.5)) / (dt(1) + dt(1.5) * x)
    else:
        i = 3; x = dt(-1) / x
    z = x * x
    w = z * z
    s1 = z * (dt(3.33333333333329318027e-01) + w * (dt(1.42857142725034663711e-01) + w * (dt(9.09088713343650656196e-02) +
         w * (dt(6.66107313738753120669e-02) + w * (dt(4.97687799461593236017e-02) + w * dt(1.62858201153657823623e-02))))))
    s2 = w * (dt(-1.99999999998764832476e-01) + w * (dt(-1.11111104054623557880e-01) + w * (dt(-7.69187620504482999495e-02) +
         w * (dt(-5.83357013379057348645e-02) + w * dt(-3.65315727442169155270e-02)))))
    if i < 0:
        return x - x * (s1 + s2)
    hi = (dt(4.63647609000806093515e-01), dt(7.85398163397448278999e-01), dt(9.82793723247329054082e-01), dt(1.57079632679489655800e+00))[i]
    return hi - (x * (s1 + s2) - x)


def atan2_ypos(y, x, dt):
    if x == dt(0):
        return dt(1.57079632679489661923)
    a = atan_pos(y / abs(x), dt)
    return a if x > dt(0) else dt(3.14159265358979323846) - a


def sin_cos(a, dt):
    if dt == np.float32:
        f = np.float32
        kf = np.rint(a * f(0.63661977236758134308))
        r = ((a - kf * f(1.5703125)) - kf * f(4.837512969970703125e-4)) - kf * f(7.54978995489188216e-8)
        z = r * r
        sp = ((f(-1.9515295891e-4) * z + f(8.3321608736e-3)) * z - f(1.6666654611e-1)) * z * r + r
        cp = ((f(2.443315711809948e-5) * z - f(1.388731625493765e-3)) * z + f(4.166664568298827e-2)) * z * z - f(0.5) * z + f(1.0)
        qf = kf - f(4.0) * np.floor(kf * f(0.25))
    else:
        f = np.float64
        kf = np.rint(a * f(6.36619772367581382433e-01))
        r = ((a - kf * f(1.57079632673412561417e+00)) - kf * f(6.07710050630396597660e-11)) - kf * f(2.02226624871116645580e-21)
        z = r * r
        sp = (((((f(1.58962301576546568060e-10) * z - f(2.50507477628578072866e-8)) * z + f(2.75573136213857245213e-6)) * z
                - f(1.98412698295895385996e-4)) * z + f(8.33333333332211858878e-3)) * z - f(1.66666666666666307295e-1)) * z * r + r
        cp = (((((f(-1.13585365213876817300e-11) * z + f(2.08757008419747316778e-9)) * z - f(2.75573141792967388112e-7)) * z
                + f(2.48015872888517045348e-5)) * z - f(1.38888888888730564116e-3)) * z + f(4.16666666666665929218e-2)) * z * z - f(0.5) * z + f(1.0)
        qf = kf - f(4.0) * np.floor(kf * f(0.25))
    q = 1 if qf == 1 else 2 if qf == 2 else 3 if qf == 3 else 0
    return ((sp, cp), (cp, -sp), (-sp, -cp), (-cp, sp))[q]


def make_isometry_rotation(rot, dt):
    """The rotation of avn_narrow.h's make_isometry for one quaternion xyzw (scalars of dtype dt): Quat::to_scaled_axis ->
    UnitQuaternion::from_scaled_axis.  The translation is the position unchanged."""
    x, y, z, w = (dt(v) for v in rot)
    ln = np.sqrt(x * x + y * y + z * z)
    scaled = (dt(0), dt(0), dt(0))
    if ln >= dt(1.0e-8):
        angle = dt(2) * atan2_ypos(ln, w, dt)
        scaled = ((x / ln) * angle, (y / ln) * angle, (z / ln) * angle)
    angle = np.sqrt(scaled[0] * scaled[0] + scaled[1] * scaled[1] + scaled[2] * scaled[2])
    if angle != dt(0):
        s, c = sin_cos(angle * dt(0.5), dt)
        return ((scaled[0] / angle) * s, (scaled[1] / angle) * s, (scaled[2] / angle) * s, c)
    return (dt(0), dt(0), dt(0), dt(1))


# ---- avn_narrow.h: the SAT of two cuboids, broadcasting ------------------------------------------------------------------------------------
def sat_normal_oneway(he1, he2, r, t, dt):
    best = None
    ri = qinverse(r)
    for i in range(3):
        sign = np.copysign(dt(1), t[i])
        zero = np.zeros_like(sign)
        axis1 = tuple(sign if k == i else zero for k in range(3))
        axis2 = na_qrot(ri, neg(axis1), dt)
        pt2 = add(na_qrot(r, support(he2, axis2), dt), t)
        sep = pt2[i] * sign - he1[i]
        best = np.where(sep > -dt(np.finfo(dt).max), sep, -dt(np.finfo(dt).max)) if best is None else np.where(sep > best, sep, best)
    return best


def sat_line_separation(he1, he2, r, t, axis1, dt):
    axis1_2 = na_qrot(qinverse(r), axis1, dt)
    pa = support(he1, axis1)
    pb = add(na_qrot(r, support(he2, neg(axis1_2)), dt), t)
    sep1 = na_dot(sub(pb, pa), axis1)
    pc = support(he1, neg(axis1))
    pd = add(na_qrot(r, support(he2, axis1_2), dt), t)
    sep2 = na_dot(sub(pd, pc), neg(axis1))
    return np.where(sep1 > sep2, sep1, sep2)


def sat_edge_twoway(he1, he2, r, t, dt, skipped=None):
    """`skipped`, when a list, receives per edge axis the mask of pairs whose axis was skipped (norm <= eps)."""
    one, zero = dt(1), dt(0)
    shp = np.broadcast(r[0], t[0], he1[0], he2[0]).shape
    z = np.zeros(shp, dt)
    units = ((z + one, z, z), (z, z + one, z), (z, z, z + one))
    e2 = [na_qrot(r, u, dt) for u in units]
    best = np.full(shp, -dt(np.finfo(dt).max), dt)
    eps = dt(np.finfo(dt).eps)
    for b in range(3):
        for a in range(3):
            u = e2[b]
            axis = (z, -u[2], u[1]) if a == 0 else ((u[2], z, -u[0]) if a == 1 else (-u[1], u[0], z))
            norm1 = np.sqrt(na_dot(axis, axis))
            ok = norm1 > eps
            if skipped is not None:
                skipped.append(~ok)
            with np.errstate(all="ignore"):
                sep = sat_line_separation(he1, he2, r, t, tuple(x / norm1 for x in axis), dt)
            best = np.where(ok & (sep > best), sep, best)
    return best


# ---- exact per-collider tests ---------------------------------------------------------------------------------------------------------------
def _clamp(c, he):
    return tuple(np.where(x < -h, -h, np.where(x > h, h, x)) for x, h in zip(c, he))


def project_exact(shape, he, pos, rot, p, solid, dt):
    """sp_project_exact, broadcasting: (ok, distance, world point xyz, is_inside); ok = the distance is finite."""
    pl = qrot(qinverse(rot), sub(p, pos), dt)
    zero = dt(0)
    with np.errstate(all="ignore"):
        r = he[0]
        d2 = dot(pl, pl)
        b_in = d2 <= r * r
        k = r / np.sqrt(d2)
        centre = d2 == zero
        bproj = (np.where(centre, zero, pl[0] * k), np.where(centre, r, pl[1] * k), np.where(centre, zero, pl[2] * k))
        c_in = (np.abs(pl[0]) <= he[0]) & (np.abs(pl[1]) <= he[1]) & (np.abs(pl[2]) <= he[2])
        clamped = _clamp(pl, he)
        m = he[0] - np.abs(pl[0])
        axis = np.zeros(np.shape(m), np.int32)
        for i in (1, 2):
            mi = he[i] - np.abs(pl[i])
            upd = mi < m
            m = np.where(upd, mi, m); axis = np.where(upd, i, axis)
        face = tuple(np.where(axis == i, np.copysign(he[i], pl[i]), pl[i]) for i in range(3))
        cproj = tuple(np.where(c_in, f, c) for f, c in zip(face, clamped))
        ball = shape == SHAPE_BALL
        inside = np.where(ball, b_in, c_in)
        proj = tuple(np.where(ball, b, c) for b, c in zip(bproj, cproj))
        diff = sub(pl, proj)
        dist = np.sqrt(dot(diff, diff))
        world = add(qrot(rot, proj, dt), pos)
        keep = inside & solid
        dist = np.where(keep, zero, dist)
        world = tuple(np.where(keep, q, x) for q, x in zip(p, world))
    return np.isfinite(dist) & (shape != SHAPE_HOST), dist, world, inside


def shape_exact(shape1, he1, r1, pos1, shape2, he2, pos2, rot2, dt):
    """sp_shape_exact, broadcasting over (query, collider): r1 is make_isometry's rotation of the query, pos1 its position."""
    ri = qinverse(r1)
    r12 = na_qmul(ri, rot2)
    t12 = na_qrot(ri, sub(pos2, pos1), dt)
    b1, b2 = shape1 == SHAPE_BALL, shape2 == SHAPE_BALL
    with np.errstate(all="ignore"):
        rr = he1[0] + he2[0]
        ball_ball = na_dot(t12, t12) <= rr * rr
        zero = np.zeros_like(t12[0])
        c_in2 = na_qrot(qinverse(r12), sub((zero, zero, zero), t12), dt)    # iso_inv_point(pos12, 0): a ball query in the cuboid collider's frame
        c = tuple(np.where(b1, x, y) for x, y in zip(c_in2, t12))
        he = tuple(np.where(b1, x, y) for x, y in zip(he2, he1))
        r = np.where(b1, he1[0], he2[0])
        inside = (np.abs(c[0]) <= he[0]) & (np.abs(c[1]) <= he[1]) & (np.abs(c[2]) <= he[2])
        d = sub(c, _clamp(c, he))
        ball_cub = inside | (na_dot(d, d) <= r * r)
        s1 = sat_normal_oneway(he1, he2, r12, t12, dt)
        r21 = qinverse(r12)
        t21 = na_qrot(r21, neg(t12), dt)
        s2 = sat_normal_oneway(he2, he1, r21, t21, dt)
        s3 = sat_edge_twoway(he1, he2, r12, t12, dt)
        cub_cub = ~(s1 > dt(0)) & ~(s2 > dt(0)) & ~(s3 > dt(0))
    return np.where(b1 & b2, ball_ball, np.where(b1 | b2, ball_cub, cub_cub)) & (shape2 != SHAPE_HOST)


# ---- the tree's node tests -------------------------------------------------------------------------------------------------------------------
def point_box_distance(p, lo, hi, dt):
    """sp_point_box_distance with the query's tolerance 64 eps * max |p|: the lower bound of the projection distance of anything inside the
    box (broadcasting); -1 for an empty box."""
    eps = dt(np.finfo(dt).eps)
    with np.errstate(all="ignore"):
        tol = dt(64) * eps * np.maximum(np.maximum(np.abs(p[0]), np.abs(p[1])), np.abs(p[2]))
        m = np.maximum.reduce([np.abs(x) for x in lo + hi])
        g = tol + dt(64) * eps * m
        d = tuple(np.maximum(np.maximum((lo[i] - g) - p[i], p[i] - (hi[i] + g)), dt(0)) for i in range(3))
        b = np.sqrt(dot(d, d)) * (dt(1) - dt(8) * eps)
    return np.where(lo[0] <= hi[0], b, dt(-1))


def shape_valid(shape, he, pos, rot, dt):
    """k_sp_shapes' per-query guard and the half extents it uses (a ball: its radius on every axis)."""
    shape = np.asarray(shape); he = np.asarray(he, dt).reshape(-1, 3).copy()
    ball = shape == SHAPE_BALL
    he[ball] = he[ball, :1]
    pos = np.asarray(pos, dt).reshape(-1, 3); rot = np.asarray(rot, dt).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ok = (shape <= SHAPE_BALL) & np.isfinite(pos).all(1) & np.isfinite(rot).all(1) & np.isfinite(he).all(1) & (he >= 0).all(1)
        lo, hi = query_shape_aabb(shape, he, pos, rot, dt)
        ok &= np.logical_and.reduce([np.isfinite(x) for x in lo + hi])
    return ok, he, pos, rot


def query_shape_aabb(shape, he, pos, rot, dt):
    """The box k_sp_shapes tests node boxes against: shape_aabb at the query's pose grown by 64 eps * its largest coordinate."""
    cols = lambda a, k: tuple(np.asarray(a, dt).reshape(-1, k)[:, i] for i in range(k))
    with np.errstate(all="ignore"):
        mn, mx = R.shape_aabb(np.asarray(shape), cols(he, 3), cols(pos, 3), cols(rot, 4), dt)
        pad = dt(64) * dt(np.finfo(dt).eps) * np.maximum.reduce([np.abs(x) for x in mn + mx])
        return tuple(x - pad for x in mn), tuple(x + pad for x in mx)


# ---- brute-force queries -------------------------------------------------------------------------------------------------------------------
def _bits(dt):
    return 32 if dt == np.float32 else 64


def project_all(s: R.Snapshot, points, solid=None, chunk=64):
    """Per (point, collider): (ok, distance, point xyz, inside) of project_exact, no filter."""
    dt = s.dt
    points = np.asarray(points, dt).reshape(-1, 3)
    n = len(points)
    solid = np.ones(n, bool) if solid is None else np.asarray(solid) != 0
    col = lambda t: tuple(x[None, :] for x in t)
    outs = []
    for a in range(0, n, chunk):
        p = tuple(points[a:a + chunk, i][:, None] for i in range(3))
        outs.append(project_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), p, solid[a:a + chunk, None], dt))
    if not outs:
        z = np.zeros((0, s.n))
        return z.astype(bool), z.astype(dt), (z.astype(dt),) * 3, z.astype(bool)
    cat = lambda xs: np.concatenate([np.broadcast_to(x, (x.shape[0], s.n)) for x in xs])
    return cat([o[0] for o in outs]), cat([o[1] for o in outs]), tuple(cat([o[2][i] for o in outs]) for i in range(3)), cat([o[3] for o in outs])


def project_points(s: R.Snapshot, points, solid=None, mask=None, excluded=()):
    """avn_spatial_project_points by brute force: the smallest (distance, collider index) over every candidate."""
    from avian_amd.spatial_query import projection_dtype
    dt = s.dt
    points = np.asarray(points, dt).reshape(-1, 3)
    n = len(points)
    out = np.zeros(n, projection_dtype(_bits(dt)))
    out["collider"] = MISS; out["entity"] = MISS
    cand = R._masks(s, n, mask, excluded, R._finite_rows(points))
    ok, dist, pt, inside = project_all(s, points, solid)
    key = np.where(ok & cand, dist, np.inf)
    for r in range(n):
        c = int(np.argmin(key[r])) if s.n else 0       # the first minimum: the lowest collider index
        if s.n and np.isfinite(key[r, c]):
            out[r] = (c, s.entity[c], int(inside[r, c]), (pt[0][r, c], pt[1][r, c], pt[2][r, c]), dist[r, c])
    return out


def shape_pairs(s: R.Snapshot, shape, half_extents, position, rotation):
    """Per (query shape, collider): shape_exact, no filter; rows of invalid query shapes are all False.  Also returns the validity."""
    dt = s.dt
    ok, he, pos, rot = shape_valid(shape, half_extents, position, rotation, dt)
    shape = np.asarray(shape)
    n = len(shape)
    hits = np.zeros((n, s.n), bool)
    idx = np.nonzero(ok)[0]
    if len(idx) and s.n:
        r1 = np.array([make_isometry_rotation(rot[i], dt) for i in idx], dt).reshape(-1, 4)
        q = lambda a, k: tuple(a[:, i][:, None] for i in range(k))
        col = lambda t: tuple(x[None, :] for x in t)
        hits[idx] = shape_exact(shape[idx][:, None], q(he[idx], 3), q(r1, 4), q(pos[idx], 3), s.shape[None, :], col(s.he), col(s.pos), col(s.rot), dt)
    return hits, ok


def shape_intersections(s: R.Snapshot, shape, half_extents, position, rotation, cap, mask=None, excluded=()):
    """avn_spatial_shape_intersections by brute force: ascending collider index, the first `cap`, MISS padding, true counts."""
    hits, ok = shape_pairs(s, shape, half_extents, position, rotation)
    cand = R._masks(s, len(ok), mask, excluded, ok)
    return R._ids(hits & cand, cap)
