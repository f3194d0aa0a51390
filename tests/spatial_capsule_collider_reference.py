"""numpy restatement of the spatial queries against Capsule COLLIDERS of include/avian_mi355x_spatial.h ("queries against capsule colliders"), in
the device's operation order (avn_spatial_pair.h: sp_seg_seg, sp_newton_cast, sp_capsule_ray_exit, sp_capcol_ray / _point / _project /
_intersects / _cast_exact; k_spatial.hip: the CCAP branches of the leaf tests), and brute-force versions of every entry point for snapshots that
hold capsule colliders next to balls and cuboids.

Built on the existing references: vectors are tuples of three arrays, quaternions of four, everything in the world's dtype with no fused
multiply-adds; the pair tests broadcast over (query, collider).  The rows of Ball / Cuboid colliders are answered by the existing references
unchanged, capsule QUERY shapes against them by spatial_capsule_reference, and the contacts against a capsule collider are the deepest point of
capsule_collider_reference's manifold (the narrow phase's).  The filter, snapshot, padding, nearest-k, depenetration, velocity-projection and
slide-loop code is the existing references' too: `patched()` lends them this module's pair functions for the length of one call and puts
theirs back."""
from __future__ import annotations

import contextlib

import numpy as np

import capsule_collider_reference as K
import spatial_capsule_reference as C
import spatial_cast_reference as CA
import spatial_caster_reference as CS
import spatial_contact_reference as CR
import spatial_move_reference as M
import spatial_query_reference as R
import spatial_shape_reference as S
from spatial_query_reference import add, dot, qinverse, qrot, scale, sub
from spatial_shape_reference import na_dot, na_qmul, na_qrot, neg

SHAPE_CAPSULE = 3
ROUNDS = C.ROUNDS
_w = np.where
_sel = C._sel

# the originals this module wraps (captured once: patched() may nest)
_o = dict(shape_aabb=R.shape_aabb, ray_exact=R.ray_exact, point_exact=R.point_exact, project_exact=S.project_exact, shape_exact=S.shape_exact,
          cast_exact=CA.cast_exact, capsule_intersects=C.capsule_intersects, capsule_cast_exact=C.capsule_cast_exact, capsule_contacts=C._capsule_contacts)

last_rounds = 0   # the most Newton rounds of a pair against a capsule collider since reset_rounds(): the tests' cap check reads it


def reset_rounds():
    global last_rounds
    last_rounds = 0


def _note_rounds(rounds, rows):
    global last_rounds
    if np.size(rounds) and np.any(rows):
        last_rounds = max(last_rounds, int(np.max(_w(rows, rounds, 0))))


# ---- the primitives ----------------------------------------------------------------------------------------------------------------------
def capcol_core(h, dt):
    """sp_capcol_core: the collider's core A + s u in its own frame."""
    z = np.zeros(np.shape(h), dt)
    return (z, -h, z), (z, h * dt(2), z)


def _clamp01(x, dt):
    return _w(x < dt(0), dt(0), _w(x > dt(1), dt(1), x))


def seg_seg(A1, u1, A2, u2, dt):
    """sp_seg_seg: the clamped closest parameters (s, t) of A1 + s u1 and A2 + t u2."""
    zero, one = dt(0), dt(1)
    w = sub(A1, A2)
    a, e, f, c, b = na_dot(u1, u1), na_dot(u2, u2), na_dot(u2, w), na_dot(u1, w), na_dot(u1, u2)
    ae = a * e
    den = ae - b * b
    par = ~(den > K.parallel_threshold(dt) * ae)
    s_g = _w(par, zero, _clamp01((b * f - c * e) / den, dt))
    t_g = (b * s_g + f) / e
    lt = t_g < zero
    gt = ~lt & (t_g > one)
    s_g = _w(lt, _clamp01(-c / a, dt), _w(gt, _clamp01((b - c) / a, dt), s_g))
    t_g = _w(lt, zero, _w(gt, one, t_g))
    case0 = (a == zero) & (e == zero)
    case1 = ~case0 & (a == zero)
    case2 = ~case0 & ~case1 & (e == zero)
    s = _w(case0 | case1, zero, _w(case2, _clamp01(-c / a, dt), s_g))
    t = _w(case0 | case2, zero, _w(case1, _clamp01(f / e, dt), t_g))
    return s, t


def seg_seg_d2(A1, u1, A2, u2, dt):
    """sp_seg_seg_d2: (d2, p1, p2) -- the first smallest of six candidate pairs evaluated in full: sp_seg_seg's, the interior point in its
    well-conditioned (perpendicular) form, and the four ends against the other segment.  A NaN candidate never wins."""
    w = sub(A1, A2)
    a, e, f, c, b = na_dot(u1, u1), na_dot(u2, u2), na_dot(u2, w), na_dot(u1, w), na_dot(u1, u2)
    s0, t0 = seg_seg(A1, u1, A2, u2, dt)
    shp = np.broadcast(s0, t0, A1[0], A2[0]).shape
    best = np.full(shp, np.inf, dt)
    p1 = tuple(np.broadcast_to(x, shp) for x in add(A1, scale(u1, s0)))
    p2 = tuple(np.broadcast_to(x, shp) for x in add(A2, scale(u2, t0)))

    def attempt(s, t):
        nonlocal best, p1, p2
        q1, q2 = add(A1, scale(u1, s)), add(A2, scale(u2, t))
        d = sub(q2, q1)
        d2 = na_dot(d, d)
        upd = d2 < best
        best = _w(upd, d2, best); p1 = _sel(upd, q1, p1); p2 = _sel(upd, q2, p2)

    attempt(s0, t0)
    u2p, wp = sub(u2, scale(u1, b / a)), sub(w, scale(u1, c / a))
    t = _clamp01(na_dot(wp, u2p) / na_dot(u2p, u2p), dt)
    s = _clamp01((b * t - c) / a, dt)
    t = _clamp01((b * s + f) / e, dt)
    attempt(s, t)
    zero, one = np.zeros(shp, dt), np.ones(shp, dt)
    attempt(zero, _clamp01(f / e, dt))
    attempt(one, _clamp01((b + f) / e, dt))
    attempt(_clamp01(-c / a, dt), zero)
    attempt(_clamp01((b - c) / a, dt), one)
    d = sub(p2, p1)
    return na_dot(d, d), p1, p2


def newton_cast(closest, dl, R_, max_distance, shp, dt):
    """sp_newton_cast, broadcasting: closest(t) answers (d2, the moving core's point, the fixed core's point).
    Returns (hit, t, n, p_moving, p_fixed, pen, rounds)."""
    zero = dt(0)
    zv = tuple(np.zeros(shp, dt) for _ in range(3))
    t = np.zeros(shp, dt)
    status = np.zeros(shp, np.int8)     # 0 running, 1 a hit, 2 a miss
    pen = np.zeros(shp, bool)
    rounds = np.zeros(shp, np.int32)
    n, pm, pf = zv, zv, zv
    for k in range(ROUNDS):
        run = status == 0
        if not run.any():
            break
        rounds = rounds + run
        f, a, b = closest(t)
        dist = np.sqrt(f)
        s_n = tuple(_w(dist > zero, (x - y) / dist, m) for x, y, m in zip(a, b, n))
        n, pm, pf = _sel(run, s_n, n), _sel(run, a, pm), _sel(run, b, pf)
        touch = run & (dist <= R_)
        status = _w(touch, 1, status)
        if k == 0:
            pen = touch
        run = run & ~touch
        v = -na_dot(s_n, dl)
        away = run & ~(v > zero)
        status = _w(away, 2, status)
        run = run & ~away
        tn = t + (dist - R_) / v
        far = run & (tn > max_distance)
        status = _w(far, 2, status)
        run = run & ~far
        stop = run & (~(tn > t) | (k == ROUNDS - 1))
        status = _w(stop, 1, status)
        run = run & ~stop
        t = _w(run, tn, t)
    return status == 1, t, n, pm, pf, pen, rounds


def capsule_ray_exit(o, d, h, R_, dt):
    """sp_capsule_ray_exit: (ok, t, outward normal) of a ray whose origin is inside the capsule (R_, h), in the capsule's frame."""
    zero, inf = dt(0), dt(np.inf)
    shp = np.broadcast(o[0], d[0], h, R_).shape
    a = d[0] * d[0] + d[2] * d[2]
    b = o[0] * d[0] + o[2] * d[2]
    q = b / a
    fa, fb = o[0] - d[0] * q, o[2] - d[2] * q
    delta = a * (R_ * R_ - (fa * fa + fb * fb))
    t = (-b + np.sqrt(delta)) / a
    y = o[1] + d[1] * t
    cyl = ((a > zero) & ~(delta < zero) & (np.abs(y) <= h)) | np.zeros(shp, bool)
    pa, pb = o[0] + d[0] * t, o[2] + d[2] * t
    l = np.sqrt(pa * pa + pb * pb)
    best = _w(cyl, t, -inf) + np.zeros(shp, dt)
    on = cyl & (l > zero)
    bn = (_w(on, pa / l, zero) + np.zeros(shp, dt), np.zeros(shp, dt), _w(on, pb / l, zero) + np.zeros(shp, dt))
    for e in range(2):
        oc = (o[0], o[1] + h if e == 0 else o[1] - h, o[2])
        a, b = dot(d, d), dot(oc, d)
        f = sub(oc, scale(d, b / a))
        delta = a * (R_ * R_ - dot(f, f))
        t = (-b + np.sqrt(delta)) / a
        upd = ~(delta < zero) & (t > best)
        p = add(oc, scale(d, t))
        l = np.sqrt(dot(p, p))
        best = _w(upd, t, best)
        bn = tuple(_w(upd, _w(l > zero, p[j] / l, zero), bn[j]) for j in range(3))
    return best > -inf, best, bn


def capcol_ray(he, ol, dl, solid, dt):
    """sp_capcol_ray: (ok, t, local normal) of the local ray against the capsule collider he = (r_c, h_c, .)."""
    ok, t, n, pen = C.capsule_ray(ol, dl, he[1], he[0], dt)
    x_ok, x_t, x_n = capsule_ray_exit(ol, dl, he[1], he[0], dt)
    out = ok & pen & ~solid
    return ok & (~out | x_ok), _w(out, x_t, t), _sel(out, x_n, n)


# ---- the exact tests of k_spatial.hip with their CCAP branches -----------------------------------------------------------------------------------
def shape_aabb(shape, h, pos, q, dt):
    """shape_aabb<T, true>: the capsule box for a capsule, the usual one otherwise."""
    mn, mx = _o["shape_aabb"](shape, h, pos, q, dt)
    cap = np.asarray(shape) == SHAPE_CAPSULE
    if not np.any(cap):
        return mn, mx
    a, b = C.capsule_aabb(h, pos, q, dt)
    return _sel(cap, a, mn), _sel(cap, b, mx)


def ray_exact(shape, he, pos, rot, o, d, max_distance, solid, dt):
    hit, toi, nw = _o["ray_exact"](shape, he, pos, rot, o, d, max_distance, solid, dt)
    cap = np.asarray(shape) == SHAPE_CAPSULE
    if not np.any(cap):
        return hit, toi, nw
    zero = dt(0)
    with np.errstate(all="ignore"):
        ci = qinverse(rot)
        ol = qrot(ci, sub(o, pos), dt)
        dl = qrot(ci, d, dt)
        ok, t, nl = capcol_ray(tuple(np.asarray(x, dt) for x in he), ol, dl, np.asarray(solid, bool), dt)
        c_hit = ok & (t <= max_distance) & np.isfinite(t)
        zn = (nl[0] == zero) & (nl[1] == zero) & (nl[2] == zero)
        cn = qrot(rot, nl, dt)
        cn = tuple(_w(zn | ~c_hit, zero, x) for x in cn)
    return _w(cap, c_hit, hit), _w(cap, _w(c_hit, t, zero), toi), _sel(cap, cn, nw)


def point_exact(shape, he, pos, rot, p, dt):
    hit = _o["point_exact"](shape, he, pos, rot, p, dt)
    cap = np.asarray(shape) == SHAPE_CAPSULE
    if not np.any(cap):
        return hit
    with np.errstate(all="ignore"):
        pl = qrot(qinverse(rot), sub(p, pos), dt)
        A, u = capcol_core(he[1], dt)
        d2, _ = C.seg_point(A, u, pl, dt)
        return _w(cap, d2 <= he[0] * he[0], hit)


def project_exact(shape, he, pos, rot, p, solid, dt):
    ok, dist, world, inside = _o["project_exact"](shape, he, pos, rot, p, solid, dt)
    cap = np.asarray(shape) == SHAPE_CAPSULE
    if not np.any(cap):
        return ok, dist, world, inside
    zero = dt(0)
    with np.errstate(all="ignore"):
        pl = qrot(qinverse(rot), sub(p, pos), dt)
        A, u = capcol_core(he[1], dt)
        r = he[0]
        d2, s = C.seg_point(A, u, pl, dt)
        pc = add(A, scale(u, s))
        c_in = d2 <= r * r
        z = np.zeros_like(r)
        proj = _sel(d2 == zero, add(pc, (z, r, z)), add(pc, scale(sub(pl, pc), r / np.sqrt(d2))))
        diff = sub(pl, proj)
        c_dist = np.sqrt(dot(diff, diff))
        c_world = add(qrot(rot, proj, dt), pos)
        keep = c_in & solid
        c_dist = _w(keep, zero, c_dist)
        c_world = tuple(_w(keep, q, x) for q, x in zip(p, c_world))
    return _w(cap, np.isfinite(c_dist), ok), _w(cap, c_dist, dist), _sel(cap, c_world, world), _w(cap, c_in, inside)


def shape_exact(shape1, he1, r1, pos1, shape2, he2, pos2, rot2, dt):
    """S.shape_exact (a ball or a cuboid query, shape 1) with capsule colliders: sp_capsule_intersects, the roles exchanged."""
    hit = _o["shape_exact"](shape1, he1, r1, pos1, shape2, he2, pos2, rot2, dt)
    cap = np.asarray(shape2) == SHAPE_CAPSULE
    if not np.any(cap):
        return hit
    c_hit = _o["capsule_intersects"](he2[0], he2[1], rot2, pos2, shape1, he1, pos1, r1, dt)
    return _w(cap, c_hit, hit)


def capsule_intersects(r, h, r2, pos2, shape1, he1, pos1, rot1, dt):
    """C.capsule_intersects (a capsule query) with capsule colliders: the two cores by seg_seg, the collider's as segment 1."""
    hit = _o["capsule_intersects"](r, h, r2, pos2, shape1, he1, pos1, rot1, dt)
    cap = np.asarray(shape1) == SHAPE_CAPSULE
    if not np.any(cap):
        return hit
    with np.errstate(all="ignore"):
        _, qr, qt = C._relative(r2, pos2, pos1, rot1, dt)
        A2, u2 = C.capsule_core(qr, qt, h, dt)
        A1, u1 = capcol_core(he1[1], dt)
        d2, _, _ = seg_seg_d2(A1, u1, A2, u2, dt)
        rr = r + he1[0]
        return _w(cap, d2 <= rr * rr, hit)


def _bc(shp):
    return lambda t: tuple(np.broadcast_to(x, shp) for x in t)


def capcol_cast_exact(shape2, he2, r2, pos2, d, max_distance, he1, pos1, rot1, dt):
    """sp_capcol_cast_exact<T, false>, broadcasting: a ball or a cuboid query (shape 2; r2 = make_isometry's rotation) against the capsule collider
    he1 = (r_c, h_c, .).  Returns (hit, toi, point1, point2, normal1, Newton rounds of the cuboid queries)."""
    zero = dt(0)
    with np.errstate(all="ignore"):
        shp = np.broadcast(np.asarray(shape2), he2[0], r2[0], pos2[0], d[0], max_distance, he1[0], pos1[0], rot1[0]).shape
        bc = _bc(shp)
        he2, r2, pos2, d, he1, pos1, rot1 = bc(he2), bc(r2), bc(pos2), bc(d), bc(he1), bc(pos1), bc(rot1)
        max_distance = np.broadcast_to(max_distance, shp)
        ball2 = np.broadcast_to(np.asarray(shape2) == R.SHAPE_BALL, shp)
        rc, hc = he1[0], he1[1]
        zv = tuple(np.zeros(shp, dt) for _ in range(3))
        # a ball: its centre as a ray against the capsule grown by its radius, in the collider's frame
        ri = qinverse(rot1)
        qt = na_qrot(ri, sub(pos2, pos1), dt)
        dl = na_qrot(ri, d, dt)
        b_ok, b_t, b_n, b_pen = C.capsule_ray(qt, dl, hc, rc + he2[0], dt)
        b_hit = b_ok & (b_t <= max_distance) & np.isfinite(b_t)
        c2 = add(pos2, scale(d, b_t))
        pb = add(qt, scale(dl, b_t))
        ys = _w(pb[1] < -hc, -hc, _w(pb[1] > hc, hc, pb[1]))
        pk = add((zv[0], ys, zv[2]), scale(b_n, rc))
        b_n1 = na_qrot(rot1, b_n, dt)
        b_p1 = add(na_qrot(rot1, pk, dt), pos1)
        b_p2 = add(c2, scale(neg(b_n1), he2[0]))
        # a cuboid: Newton in the query's frame, the collider's core moving by -d
        r2i = qinverse(r2)
        qcr = na_qmul(r2i, rot1)
        qct = na_qrot(r2i, sub(pos1, pos2), dt)
        dm = neg(na_qrot(r2i, d, dt))
        A, u = C.capsule_core(qcr, qct, hc, dt)

        def closest(t):
            f, _, ps, pbx = C.seg_box(add(A, scale(dm, t)), u, he2, dt)
            return f, ps, pbx

        c_ok, c_t, n, ps, pbx, c_pen, rounds = newton_cast(closest, dm, rc, max_distance, shp, dt)
        c_hit = c_ok & (c_t <= max_distance) & np.isfinite(c_t)
        c2 = add(pos2, scale(d, c_t))
        c_n1 = neg(na_qrot(r2, n, dt))
        c_p1 = add(na_qrot(r2, sub(ps, scale(n, rc)), dt), c2)
        c_p2 = add(na_qrot(r2, pbx, dt), c2)
        k_hit = _w(ball2, b_hit, c_hit)
        k_t = _w(ball2, b_t, c_t)
        keep = k_hit & ~_w(ball2, b_pen, c_pen)
        k_n1 = _sel(keep, _sel(ball2, b_n1, c_n1), zv)
        k_p1 = _sel(keep, _sel(ball2, b_p1, c_p1), zv)
        k_p2 = _sel(keep, _sel(ball2, b_p2, c_p2), zv)
    return k_hit, _w(k_hit, k_t, zero), k_p1, k_p2, k_n1, _w(ball2, 0, rounds)


def cast_exact(shape2, he2, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt):
    """CA.cast_exact (a ball or a cuboid query, shape 2) with capsule colliders."""
    hit, toi, p1, p2, n1 = _o["cast_exact"](shape2, he2, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt)
    cap = np.asarray(shape1) == SHAPE_CAPSULE
    if not np.any(cap):
        return hit, toi, p1, p2, n1
    k_hit, k_toi, k_p1, k_p2, k_n1, rounds = capcol_cast_exact(shape2, he2, r2, pos2, d, max_distance, he1, pos1, rot1, dt)
    _note_rounds(rounds, np.broadcast_to(cap, rounds.shape))
    return _w(cap, k_hit, hit), _w(cap, k_toi, toi), _sel(cap, k_p1, p1), _sel(cap, k_p2, p2), _sel(cap, k_n1, n1)


def capcol_capsule_cast_exact(r, h, r2, pos2, d, max_distance, he1, pos1, rot1, dt):
    """sp_capcol_cast_exact<T, true>, broadcasting: the capsule query (r, h) against the capsule collider he1, Newton on the two cores.
    Returns (hit, toi, point1, point2, normal1, Newton rounds)."""
    zero = dt(0)
    with np.errstate(all="ignore"):
        shp = np.broadcast(r, h, r2[0], pos2[0], d[0], max_distance, he1[0], pos1[0], rot1[0]).shape
        bc = _bc(shp)
        r2, pos2, d, he1, pos1, rot1 = bc(r2), bc(pos2), bc(d), bc(he1), bc(pos1), bc(rot1)
        r, h, max_distance = (np.broadcast_to(x, shp) for x in (r, h, max_distance))
        rc = he1[0]
        zv = tuple(np.zeros(shp, dt) for _ in range(3))
        ri, qr, qt = C._relative(r2, pos2, pos1, rot1, dt)
        dl = na_qrot(ri, d, dt)
        A1, u1 = capcol_core(he1[1], dt)
        A2, u2 = C.capsule_core(qr, qt, h, dt)

        def closest(t):
            f, p1_, p2_ = seg_seg_d2(A1, u1, add(A2, scale(dl, t)), u2, dt)
            return f, p2_, p1_

        ok, t, n, pq, pc, pen, k_rounds = newton_cast(closest, dl, r + rc, max_distance, shp, dt)
        k_hit = ok & (t <= max_distance) & np.isfinite(t)
        keep = k_hit & ~pen
        k_n1 = _sel(keep, na_qrot(rot1, n, dt), zv)
        k_p1 = _sel(keep, add(na_qrot(rot1, add(pc, scale(n, rc)), dt), pos1), zv)
        k_p2 = _sel(keep, add(na_qrot(rot1, sub(pq, scale(n, r)), dt), pos1), zv)
    return k_hit, _w(k_hit, t, zero), k_p1, k_p2, k_n1, k_rounds


def capsule_cast_exact(r, h, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt):
    """C.capsule_cast_exact (a capsule query) with capsule colliders."""
    hit, toi, p1, p2, n1, rounds = _o["capsule_cast_exact"](r, h, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt)
    cap = np.asarray(shape1) == SHAPE_CAPSULE
    if not np.any(cap):
        return hit, toi, p1, p2, n1, rounds
    k_hit, k_toi, k_p1, k_p2, k_n1, k_rounds = capcol_capsule_cast_exact(r, h, r2, pos2, d, max_distance, he1, pos1, rot1, dt)
    cap = np.broadcast_to(cap, k_rounds.shape)
    _note_rounds(k_rounds, cap)
    return _w(cap, k_hit, hit), _w(cap, k_toi, toi), _sel(cap, k_p1, p1), _sel(cap, k_p2, p2), _sel(cap, k_n1, n1), _w(cap, k_rounds, rounds)


# ---- contacts: the narrow phase's capsule manifolds, the deepest point ------------------------------------------------------------------------------
class _Manifolds:
    """contact_manifolds for a batch of (query shape, collider) pairs: the rows whose collider is a capsule come from capsule_collider_reference
    (the query as shape 1, whatever its kind), the others from spatial_capsule_reference's (the oracle, or the capsule query's own contact)."""

    def __init__(self, bits):
        self.bits = bits

    def contact_manifolds(self, shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction):
        dt = np.float32 if self.bits == 32 else np.float64
        shape1, shape2 = np.asarray(shape1), np.asarray(shape2)
        k = len(shape1)
        A = lambda a, n: np.asarray(a, dt).reshape(k, n)
        he1, pos1, rot1, he2, pos2, rot2 = A(he1, 3), A(pos1, 3), A(rot1, 4), A(he2, 3), A(pos2, 3), A(rot2, 4)
        prediction = np.broadcast_to(np.asarray(prediction, dt), (k,))
        cap = shape2 == SHAPE_CAPSULE
        m = {"point_count": np.zeros(k, np.uint32), "penetration": np.zeros((k, 16), dt), "normal": np.zeros((k, 3), dt),
             "point": np.zeros((k, 16, 3), dt), "anchor1": np.zeros((k, 16, 3), dt), "anchor2": np.zeros((k, 16, 3), dt)}
        for rows, fn in ((~cap, lambda *a: C._Manifolds(self.bits).contact_manifolds(*a)), (cap, lambda *a: K.manifolds(*a, dt))):
            i = np.nonzero(rows)[0]
            if not len(i):
                continue
            o = fn(shape1[i], he1[i], pos1[i], rot1[i], shape2[i], he2[i], pos2[i], rot2[i], prediction[i])
            for key in m:
                m[key][i] = o[key]
        return m


def _capsule_contacts(s, shape, he, pos, rot, pred):
    """C._capsule_contacts (the capsule rows of a contact query) with capsule colliders: those pairs take the capsule-capsule manifold."""
    dt = s.dt
    ok, out = _o["capsule_contacts"](s, shape, he, pos, rot, pred)
    ccol = np.nonzero(s.shape == SHAPE_CAPSULE)[0]
    shape = np.asarray(shape)
    _, he_v, pos_v, rot_v = C.shape_valid(shape, he, pos, rot, dt)
    idx = np.nonzero(ok & (shape == SHAPE_CAPSULE))[0]
    if not len(ccol) or not len(idx):
        return ok, out
    out = [e for e in out if s.shape[e[1]] != SHAPE_CAPSULE]
    with np.errstate(all="ignore"):
        a, b = C.capsule_aabb(C._cols(he_v[idx], 3), C._cols(pos_v[idx], 3), C._cols(rot_v[idx], 4), dt)
        mn, mx = shape_aabb(s.shape[ccol], tuple(x[ccol] for x in s.he), tuple(x[ccol] for x in s.pos), tuple(x[ccol] for x in s.rot), dt)
        pre = np.ones((len(idx), len(ccol)), bool)
        for i in range(3):
            pre &= (mn[i][None, :] <= (b[i] + pred[idx])[:, None]) & (mx[i][None, :] >= (a[i] - pred[idx])[:, None])
        qi, ci = np.nonzero(pre)
        if len(qi):
            q, c = idx[qi], ccol[ci]
            cpos, crot, che = np.stack(s.pos, 1), np.stack(s.rot, 1), np.stack(s.he, 1)
            m = K.manifolds(shape[q], he_v[q], pos_v[q], rot_v[q], s.shape[c], che[c], cpos[c], crot[c], pred[q], dt)
            for j in range(len(q)):
                cnt = int(m["point_count"][j])
                if cnt:
                    k = CR.deepest(m["penetration"][j], cnt)
                    out.append((q[j], c[j], m["penetration"][j, k], list(-m["normal"][j]), list(m["anchor1"][j, k]), list(m["anchor2"][j, k])))
    out.sort(key=lambda e: (e[0], e[1]))
    return ok, out


@contextlib.contextmanager
def patched():
    """Lends this module's pair functions (and spatial_capsule_reference's, for capsule query shapes) to the existing references for one call."""
    with C.patched():
        saved = (R.shape_aabb, R.ray_exact, R.point_exact, S.project_exact, S.shape_exact, CA.cast_exact, C.capsule_intersects, C.capsule_cast_exact,
                 C._capsule_contacts, CR.oracle_world)
        (R.shape_aabb, R.ray_exact, R.point_exact, S.project_exact, S.shape_exact, CA.cast_exact, C.capsule_intersects, C.capsule_cast_exact,
         C._capsule_contacts, CR.oracle_world) = (shape_aabb, ray_exact, point_exact, project_exact, shape_exact, cast_exact, capsule_intersects,
                                                  capsule_cast_exact, _capsule_contacts, _Manifolds)
        try:
            yield
        finally:
            (R.shape_aabb, R.ray_exact, R.point_exact, S.project_exact, S.shape_exact, CA.cast_exact, C.capsule_intersects, C.capsule_cast_exact,
             C._capsule_contacts, CR.oracle_world) = saved


def _lend(fn):
    def call(*a, **kw):
        with patched(), np.errstate(all="ignore"):
            return fn(*a, **kw)
    call.__doc__ = fn.__doc__
    return call


# ---- brute force: every entry point, for a snapshot whose capsule colliders are candidates ---------------------------------------------------------
ray_queries = _lend(R.ray_queries)
cast_rays = _lend(R.cast_rays)
ray_hits = _lend(R.ray_hits)
point_intersections = _lend(R.point_intersections)
aabb_intersections = _lend(R.aabb_intersections)
project_points = _lend(S.project_points)
shape_intersections = _lend(C.shape_intersections)
cast_queries = _lend(CA.cast_queries)
contact_lists = _lend(C.contact_lists)
shape_contacts = _lend(C.shape_contacts)
cast_moves = _lend(M.cast_moves)          # (not spatial_capsule_reference's wrappers: their patched() would put its own manifolds back)
move_and_slide = _lend(M.move_and_slide)
ray_casters = _lend(CS.ray_casters)
shape_casters = _lend(CS.shape_casters)
leaf_boxes = _lend(R.leaf_boxes)


def without_capsules(s: R.Snapshot):
    """The snapshot as the queries see it with the switch off: its capsule colliders are host shapes."""
    import copy
    o = copy.copy(s)
    o.shape = np.where(s.shape == SHAPE_CAPSULE, R.SHAPE_HOST, s.shape).astype(np.uint32)
    return o
