"""numpy restatement of the capsule query shape of include/avian_mi355x_spatial.h ("capsule query shapes"), in the device's operation order
(avn_spatial_pair.h: sp_capsule_core, sp_seg_point, sp_seg_box, sp_capsule_intersects, sp_capsule_ray, sp_capsule_cast_exact,
sp_capsule_contact; k_spatial.hip: sp_load_shape<CAPSULE>), and brute-force versions of every entry point that takes a query shape, for calls
that mix capsules with balls and cuboids.

Built on the existing references: vectors are tuples of three arrays, quaternions of four, everything in the world's dtype with no fused
multiply-adds; the pair tests broadcast over (query, collider).  The Ball / Cuboid rows of a call are answered by the existing references
unchanged.  The filter, snapshot, padding, depenetration, velocity-projection and slide-loop code is theirs too: `patched()` lends them this
module's pair functions for the length of one call and puts theirs back."""
from __future__ import annotations

import contextlib

import numpy as np

import spatial_cast_reference as CA
import spatial_contact_reference as CR
import spatial_move_reference as M
import spatial_query_reference as R
import spatial_shape_reference as S
from spatial_query_reference import MISS, SHAPE_BALL, SHAPE_HOST, add, dot, qinverse, scale, sub
from spatial_shape_reference import na_dot, na_qmul, na_qrot, neg

SHAPE_CAPSULE = 3
ROUNDS = 32          # SP_CAPSULE_ROUNDS
_INVALID_KIND = 2    # what a capsule row is handed to the Ball / Cuboid references as: they answer it a miss / count 0

_w = np.where


def _sel(c, a, b):
    return tuple(np.where(c, x, y) for x, y in zip(a, b))


def _clamp(p, he):
    return tuple(_w(x < -h, -h, _w(x > h, h, x)) for x, h in zip(p, he))


# ---- the primitives ----------------------------------------------------------------------------------------------------------------------
def capsule_core(qr, qt, h, dt):
    """sp_capsule_core: (A, u) of the segment A + s u in the collider's frame."""
    z = np.zeros(np.shape(h), dt)
    hv = na_qrot(qr, (z, h, z), dt)
    return sub(qt, hv), scale(hv, dt(2))


def seg_point(A, u, c, dt):
    """sp_seg_point: (d2, s)."""
    zero, one = dt(0), dt(1)
    uu = na_dot(u, u)
    s = na_dot(sub(c, A), u) / uu
    s = _w(s < zero, zero, _w(s > one, one, s))
    s = _w(uu == zero, zero, s)
    e = sub(c, add(A, scale(u, s)))
    return na_dot(e, e), s


def _seg_f(A, u, he, s):
    p = add(A, scale(u, s))
    e = sub(p, _clamp(p, he))
    return na_dot(e, e)


def seg_box(A, u, he, dt):
    """sp_seg_box: (f, s, p_seg, p_box)."""
    zero, one, half = dt(0), dt(1), dt(0.5)
    shp = np.broadcast(A[0], u[0], he[0]).shape

    def brk(a, uu, h):
        s = (h - a) / uu
        return _w((uu != zero) & (s > zero) & (s < one), s, one) + np.zeros(shp, dt)

    b = [brk(A[0], u[0], -he[0]), brk(A[0], u[0], he[0]), brk(A[1], u[1], -he[1]), brk(A[1], u[1], he[1]), brk(A[2], u[2], -he[2]), brk(A[2], u[2], he[2])]
    for i, j in ((0, 5), (1, 3), (2, 4), (1, 2), (3, 4), (0, 3), (2, 5), (0, 1), (2, 3), (4, 5), (1, 2), (3, 4)):
        sw = b[j] < b[i]
        b[i], b[j] = _w(sw, b[j], b[i]), _w(sw, b[i], b[j])
    bf = np.full(shp, np.inf, dt)
    bs = np.zeros(shp, dt)

    def attempt(s):
        nonlocal bf, bs
        f = _seg_f(A, u, he, s)
        upd = f < bf
        bf = _w(upd, f, bf); bs = _w(upd, s, bs)

    z0, z1 = np.zeros(shp, dt), np.ones(shp, dt)
    for s in [z0, z1] + b:
        attempt(s)
    ends = [z0] + b + [z1]
    for lo, hi in zip(ends[:-1], ends[1:]):
        mid = (lo + hi) * half
        m = add(A, scale(u, mid))
        sg = tuple(_w(m[i] > he[i], one, _w(m[i] < -he[i], -one, zero)) for i in range(3))
        act = tuple(x != zero for x in sg)
        den = (_w(act[0], u[0] * u[0], zero) + _w(act[1], u[1] * u[1], zero)) + _w(act[2], u[2] * u[2], zero)
        num = (_w(act[0], u[0] * (A[0] - sg[0] * he[0]), zero) + _w(act[1], u[1] * (A[1] - sg[1] * he[1]), zero)) + _w(act[2], u[2] * (A[2] - sg[2] * he[2]), zero)
        s = -num / den
        s = _w(s < lo, lo, _w(s > hi, hi, s))
        none = ~act[0] & ~act[1] & ~act[2]
        attempt(_w(none, mid, _w(den > zero, s, lo)))
    ps = add(A, scale(u, bs))
    return bf, bs, ps, _clamp(ps, he)


def capsule_ray(o, d, h, R_, dt):
    """sp_capsule_ray: (ok, t, normal xyz, pen) of a ball centre's ray against the capsule (R_, h) in the capsule's frame."""
    zero, inf = dt(0), dt(np.inf)
    shp = np.broadcast(o[0], d[0], h, R_).shape
    a = d[0] * d[0] + d[2] * d[2]
    b, c = o[0] * d[0] + o[2] * d[2], (o[0] * o[0] + o[2] * o[2]) - R_ * R_
    q = b / a
    fa, fb = o[0] - d[0] * q, o[2] - d[2] * q
    delta = a * (R_ * R_ - (fa * fa + fb * fb))
    t = (-b - np.sqrt(delta)) / a
    inside = t <= zero
    t = _w(inside, zero, t)
    y = o[1] + d[1] * t
    cyl = (a > zero) & ~((c > zero) & (b > zero)) & ~(delta < zero) & (np.abs(y) <= h)
    pa, pb = o[0] + d[0] * t, o[2] + d[2] * t
    l = np.sqrt(pa * pa + pb * pb)
    zn = inside | ~(l > zero)
    best = _w(cyl, t, inf) + np.zeros(shp, dt)
    found = cyl | np.zeros(shp, bool)
    bpen = cyl & inside
    bn = (_w(cyl & ~zn, pa / l, zero) + np.zeros(shp, dt), np.zeros(shp, dt), _w(cyl & ~zn, pb / l, zero) + np.zeros(shp, dt))
    for e in range(2):
        oc = (o[0], o[1] + h if e == 0 else o[1] - h, o[2])
        ok, t, inside = CA.ball_ray(oc, d, R_, dt)
        upd = ok & (t < best)
        p = add(oc, scale(d, t))
        l = np.sqrt(dot(p, p))
        zn = inside | ~(l > zero)
        best = _w(upd, t, best); found = found | upd; bpen = _w(upd, inside, bpen)
        bn = tuple(_w(upd, _w(zn, zero, p[j] / l), bn[j]) for j in range(3))
    return found, best, bn, bpen


def _relative(r2, pos2, pos1, rot1, dt):
    ri = qinverse(rot1)
    return ri, na_qmul(ri, r2), na_qrot(ri, sub(pos2, pos1), dt)


# ---- the pair tests -----------------------------------------------------------------------------------------------------------------------
def capsule_intersects(r, h, r2, pos2, shape1, he1, pos1, rot1, dt):
    """sp_capsule_intersects, broadcasting over (query, collider)."""
    with np.errstate(all="ignore"):
        _, qr, qt = _relative(r2, pos2, pos1, rot1, dt)
        A, u = capsule_core(qr, qt, h, dt)
        z = np.zeros_like(A[0])
        d2, _ = seg_point(A, u, (z, z, z), dt)
        rr = r + he1[0]
        f = seg_box(A, u, he1, dt)[0]
        return _w(shape1 == SHAPE_BALL, d2 <= rr * rr, f <= r * r) & (shape1 != SHAPE_HOST)


def capsule_cast_exact(r, h, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt):
    """sp_capsule_cast_exact, broadcasting: (hit, toi, point1, point2, normal1, Newton rounds of the capsule-cuboid pairs)."""
    zero = dt(0)
    with np.errstate(all="ignore"):
        ri, qr, qt = _relative(r2, pos2, pos1, rot1, dt)
        dl = na_qrot(ri, d, dt)
        shp = np.broadcast(qr[0], qt[0], dl[0], he1[0], max_distance, r, h).shape
        bc = lambda t: tuple(np.broadcast_to(x, shp) for x in t)
        qr, qt, dl, he1, d, pos1, pos2, rot1, r2 = bc(qr), bc(qt), bc(dl), bc(he1), bc(d), bc(pos1), bc(pos2), bc(rot1), bc(r2)
        r, h, max_distance = (np.broadcast_to(x, shp) for x in (r, h, max_distance))
        zv = tuple(np.zeros(shp, dt) for _ in range(3))
        ball1 = np.broadcast_to(shape1 == SHAPE_BALL, shp)
        # a ball collider: its centre's ray in the capsule's frame, reversed
        qri = qinverse(qr)
        o = na_qrot(qri, sub(zv, qt), dt)
        dd = neg(na_qrot(qri, dl, dt))
        b_ok, b_t, b_n, b_pen = capsule_ray(o, dd, h, r + he1[0], dt)
        b_hit = b_ok & (b_t <= max_distance) & np.isfinite(b_t)
        c2 = add(pos2, scale(d, b_t))
        pc = add(o, scale(dd, b_t))
        ys = _w(pc[1] < -h, -h, _w(pc[1] > h, h, pc[1]))
        pk = add((zv[0], ys, zv[2]), scale(b_n, r))
        b_n1 = neg(na_qrot(r2, b_n, dt))
        b_p2 = add(na_qrot(r2, pk, dt), c2)
        b_p1 = add(pos1, scale(b_n1, he1[0]))
        # a cuboid collider: Newton from t = 0
        A, u = capsule_core(qr, qt, h, dt)
        t = np.zeros(shp, dt)
        status = np.zeros(shp, np.int8)     # 0 running, 1 a hit, 2 a miss
        c_pen = np.zeros(shp, bool)
        rounds = np.zeros(shp, np.int32)
        n, ps, pb = zv, zv, zv
        for k in range(ROUNDS):
            run = status == 0
            if not run.any():
                break
            rounds = rounds + run
            f, _, s_ps, s_pb = seg_box(add(A, scale(dl, t)), u, he1, dt)
            dist = np.sqrt(f)
            s_n = tuple(_w(dist > zero, (a - b) / dist, m) for a, b, m in zip(s_ps, s_pb, n))      # dist == 0: the round before's direction stands
            n, ps, pb = _sel(run, s_n, n), _sel(run, s_ps, ps), _sel(run, s_pb, pb)
            touch = run & (dist <= r)
            status = _w(touch, 1, status)
            if k == 0:
                c_pen = touch
            run = run & ~touch
            v = -na_dot(s_n, dl)
            away = run & ~(v > zero)
            status = _w(away, 2, status)
            run = run & ~away
            tn = t + (dist - r) / v
            far = run & (tn > max_distance)
            status = _w(far, 2, status)
            run = run & ~far
            stop = run & (~(tn > t) | (k == ROUNDS - 1))
            status = _w(stop, 1, status)
            run = run & ~stop
            t = _w(run, tn, t)
        c_hit = (status == 1) & (t <= max_distance) & np.isfinite(t)
        c_n1 = na_qrot(rot1, n, dt)
        c_p1 = add(na_qrot(rot1, pb, dt), pos1)
        c_p2 = add(na_qrot(rot1, sub(ps, scale(n, r)), dt), pos1)
        hit = _w(ball1, b_hit, c_hit) & np.broadcast_to(shape1 != SHAPE_HOST, shp)
        toi = _w(ball1, b_t, t)
        keep = hit & ~_w(ball1, b_pen, c_pen)
        n1 = _sel(keep, _sel(ball1, b_n1, c_n1), zv)
        p1 = _sel(keep, _sel(ball1, b_p1, c_p1), zv)
        p2 = _sel(keep, _sel(ball1, b_p2, c_p2), zv)
    return hit, _w(hit, toi, zero), p1, p2, n1, _w(ball1, 0, rounds)


def capsule_contact(r, h, r2, pos2, shape1, he1, pos1, rot1, prediction, dt):
    """sp_capsule_contact, broadcasting: (contact, penetration, normal, anchor1, anchor2), the normal from the collider towards the capsule."""
    zero, inf = dt(0), dt(np.inf)
    eps = dt(np.finfo(dt).eps)
    with np.errstate(all="ignore"):
        _, qr, qt = _relative(r2, pos2, pos1, rot1, dt)
        shp = np.broadcast(qr[0], qt[0], he1[0], prediction, r, h).shape
        bc = lambda t: tuple(np.broadcast_to(x, shp) for x in t)
        qr, qt, he1, rot1 = bc(qr), bc(qt), bc(he1), bc(rot1)
        r, h, prediction = (np.broadcast_to(x, shp) for x in (r, h, prediction))
        ball1 = np.broadcast_to(shape1 == SHAPE_BALL, shp)
        A, u = capsule_core(qr, qt, h, dt)
        zv = tuple(np.zeros(shp, dt) for _ in range(3))
        rc = _w(ball1, he1[0], zero)
        b_d2, b_s = seg_point(A, u, zv, dt)
        b_ps = add(A, scale(u, b_s))
        c_f, _, c_ps, c_pb = seg_box(A, u, he1, dt)
        d2 = _w(ball1, b_d2, c_f)
        ps, pc = _sel(ball1, b_ps, c_ps), _sel(ball1, zv, c_pb)
        dist = np.sqrt(d2)
        apart = dist > zero
        gap = (dist - r) - rc
        a_n = tuple((a - b) / dist for a, b in zip(ps, pc))
        a_l1 = sub(ps, scale(a_n, r))
        a_l2 = add(pc, scale(a_n, rc))
        # the segment touches or crosses the box: the six axes of the Minkowski difference
        hv = scale(u, dt(0.5))
        m = add(A, hv)
        eps2 = eps * eps * na_dot(u, u)
        best = np.full(shp, inf, dt); brb = np.zeros(shp, dt)
        n = zv
        one = np.ones(shp, dt)
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
            rb = np.abs(ax[0]) * he1[0] + np.abs(ax[1]) * he1[1] + np.abs(ax[2]) * he1[2]
            rs = np.abs(na_dot(ax, hv))
            c = na_dot(ax, m)
            ov = (rb + rs) - np.abs(c)
            upd = live & (ov < best)
            best = _w(upd, ov, best); brb = _w(upd, rb, brb)
            n = _sel(upd, _sel(c < zero, neg(ax), ax), n)
        pd = _sel(na_dot(n, u) < zero, add(A, u), A)
        z_l1 = sub(pd, scale(n, r))
        z_l2 = add(pd, scale(n, brb - na_dot(n, pd)))
        contact = _w(apart, ~(gap > prediction), ~ball1) & np.broadcast_to(shape1 != SHAPE_HOST, shp)
        pen = _w(apart, -gap, best + r)
        nl, l1, l2 = _sel(apart, a_n, n), _sel(apart, a_l1, z_l1), _sel(apart, a_l2, z_l2)
        normal = na_qrot(rot1, nl, dt)
        anchor1 = na_qrot(rot1, sub(l1, qt), dt)
        anchor2 = na_qrot(rot1, l2, dt)
    return contact, pen, normal, anchor1, anchor2


# ---- the query shape: validity and boxes ----------------------------------------------------------------------------------------------------
def capsule_aabb(he, pos, rot, dt):
    """sp_load_shape<CAPSULE>'s [a, b]: pos -+ (|qrot(rot, (0, h, 0))| + (r, r, r)); he / pos / rot are tuples of columns."""
    z = np.zeros_like(he[1])
    hv = R.qrot(rot, (z, he[1], z), dt)
    ext = tuple(np.abs(x) + he[0] for x in hv)
    return sub(pos, ext), add(pos, ext)


_cols = lambda a, k: tuple(a[:, i] for i in range(k))
_orig_shape_valid, _orig_cast_pairs, _orig_contact_lists, _orig_oracle_world = S.shape_valid, CA.cast_pairs, CR.contact_lists, CR.oracle_world
_orig_query_shape_aabb = S.query_shape_aabb


def shape_valid(shape, he, pos, rot, dt):
    """S.shape_valid with the capsule rule: finite r, h >= 0 (z is not read and comes back 0), a finite pose and a finite AABB."""
    shape = np.asarray(shape)
    cap = shape == SHAPE_CAPSULE
    ok, he_o, pos, rot = _orig_shape_valid(np.where(cap, _INVALID_KIND, shape), he, pos, rot, dt)
    he_o = he_o.copy()
    he_o[cap, 2] = 0
    with np.errstate(all="ignore"):
        c_ok = cap & np.isfinite(pos).all(1) & np.isfinite(rot).all(1) & np.isfinite(he_o).all(1) & (he_o >= 0).all(1)
        a, b = capsule_aabb(_cols(he_o, 3), _cols(pos, 3), _cols(rot, 4), dt)
        c_ok &= np.logical_and.reduce([np.isfinite(x) for x in a + b])
    return ok | c_ok, he_o, pos, rot


def query_shape_aabb(shape, he, pos, rot, dt):
    """S.query_shape_aabb for a mixed batch: the capsule's exact box padded as every query box is."""
    shape = np.asarray(shape)
    cap = shape == SHAPE_CAPSULE
    lo, hi = _orig_query_shape_aabb(np.where(cap, 0, shape), he, pos, rot, dt)
    cols = lambda a, k: tuple(np.asarray(a, dt).reshape(-1, k)[:, i] for i in range(k))
    with np.errstate(all="ignore"):
        mn, mx = capsule_aabb(cols(he, 3), cols(pos, 3), cols(rot, 4), dt)
        pad = dt(64) * dt(np.finfo(dt).eps) * np.maximum.reduce([np.abs(x) for x in mn + mx])
        return tuple(_w(cap, c - pad, x) for c, x in zip(mn, lo)), tuple(_w(cap, c + pad, x) for c, x in zip(mx, hi))


def _capsule_rows(s, shape, he, pos, rot):
    """(indices of the valid capsule rows, their (r, h) / make_isometry rotation / position as [k, 1] columns, the snapshot as [1, C] rows)."""
    dt = s.dt
    ok, he, pos, rot = shape_valid(shape, he, pos, rot, dt)
    idx = np.nonzero(ok & (np.asarray(shape) == SHAPE_CAPSULE))[0]
    r2 = np.array([S.make_isometry_rotation(rot[i], dt) for i in idx], dt).reshape(-1, 4)
    q = lambda a, k: tuple(a[:, i][:, None] for i in range(k))
    col = lambda t: tuple(x[None, :] for x in t)
    return ok, idx, he[idx, 0][:, None], he[idx, 1][:, None], q(r2, 4), q(pos[idx], 3), (s.shape[None, :], col(s.he), col(s.pos), col(s.rot))


# ---- brute force ----------------------------------------------------------------------------------------------------------------------------
def shape_intersections(s: R.Snapshot, shape, half_extents, position, rotation, cap, mask=None, excluded=()):
    """avn_spatial_shape_intersections for a mixed batch."""
    shape = np.asarray(shape)
    hits, _ = S.shape_pairs(s, np.where(shape == SHAPE_CAPSULE, _INVALID_KIND, shape), half_extents, position, rotation)
    ok, idx, r, h, r2, p2, (cs, che, cpos, crot) = _capsule_rows(s, shape, half_extents, position, rotation)
    if len(idx) and s.n:
        hits[idx] = capsule_intersects(r, h, r2, p2, cs, che, cpos, crot, s.dt)
    return R._ids(hits & R._masks(s, len(ok), mask, excluded, ok), cap)


last_rounds = None   # the Newton rounds [capsule rows, C] of the last cast_pairs call (0 for ball colliders): the tests' cap check reads it


def cast_pairs(s: R.Snapshot, shape, half_extents, position, rotation, direction, max_distance=None):
    """CA.cast_pairs for a mixed batch: (hit, toi, p1, p2, n1, valid) per (cast, collider), no filter."""
    global last_rounds
    dt = s.dt
    shape = np.asarray(shape)
    n = len(shape)
    max_distance = np.full(n, np.inf, dt) if max_distance is None else np.asarray(max_distance, dt).reshape(-1)
    direction = np.asarray(direction, dt).reshape(-1, 3)
    hit, toi, p1, p2, n1, okb = _orig_cast_pairs(s, np.where(shape == SHAPE_CAPSULE, _INVALID_KIND, shape), half_extents, position, rotation, direction, max_distance)
    ok, idx, r, h, r2, pp, (cs, che, cpos, crot) = _capsule_rows(s, shape, half_extents, position, rotation)
    with np.errstate(all="ignore"):
        good = np.isfinite(direction[idx]).all(1) & ~np.isnan(max_distance[idx])
    idx, r, h, r2, pp = idx[good], r[good], h[good], tuple(x[good] for x in r2), tuple(x[good] for x in pp)
    valid = okb.copy()
    valid[idx] = True
    last_rounds = np.zeros((0, s.n), np.int32)
    if len(idx) and s.n:
        d = tuple(direction[idx, i][:, None] for i in range(3))
        c_hit, c_toi, a, b, c, last_rounds = capsule_cast_exact(r, h, r2, pp, d, max_distance[idx][:, None], cs, che, cpos, crot, dt)
        hit[idx] = c_hit; toi[idx] = c_toi
        for j in range(3):
            p1[j][idx] = a[j]; p2[j][idx] = b[j]; n1[j][idx] = c[j]
    return hit, toi, p1, p2, n1, valid


def _capsule_contacts(s, shape, he, pos, rot, pred):
    """(query index, collider index, record fields) of every capsule pair whose AABB precondition and contact hold; no filter."""
    dt = s.dt
    ok, idx, r, h, r2, pp, (cs, che, cpos, crot) = _capsule_rows(s, shape, he, pos, rot)
    if not len(idx) or not s.n:
        return ok, []
    _, he_v, pos_v, rot_v = shape_valid(shape, he, pos, rot, dt)
    p = pred[idx][:, None]
    with np.errstate(all="ignore"):
        a, b = capsule_aabb(_cols(he_v[idx], 3), _cols(pos_v[idx], 3), _cols(rot_v[idx], 4), dt)
        mn, mx = R.shape_aabb(s.shape, s.he, s.pos, s.rot, dt)
        pre = np.ones((len(idx), s.n), bool)
        for i in range(3):
            pre &= (mn[i][None, :] <= (b[i] + pred[idx])[:, None]) & (mx[i][None, :] >= (a[i] - pred[idx])[:, None])
        con, pen, nrm, a1, a2 = capsule_contact(r, h, r2, pp, cs, che, cpos, crot, p, dt)
    out = []
    for k, c in zip(*np.nonzero(con & pre)):
        out.append((idx[k], c, pen[k, c], [x[k, c] for x in nrm], [x[k, c] for x in a1], [x[k, c] for x in a2]))
    return ok, out


def contact_lists(s: R.Snapshot, shape, half_extents, position, rotation, prediction, mask=None, excluded=(), sensor=None, skip_sensors=False):
    """CR.contact_lists for a mixed batch."""
    from avian_amd.spatial_query import shape_contact_dtype
    dt = s.dt
    shape = np.asarray(shape)
    n = len(shape)
    cap = shape == SHAPE_CAPSULE
    pred = np.broadcast_to(np.asarray(prediction, dt), (n,)).copy()
    if (~cap).any():
        out = _orig_contact_lists(s, np.where(cap, _INVALID_KIND, shape), half_extents, position, rotation, pred, mask, excluded, sensor, skip_sensors)
    else:
        out = [np.zeros(0, shape_contact_dtype(CR._bits(dt))) for _ in range(n)]
    if not cap.any():
        return out
    ok, pairs = _capsule_contacts(s, shape, half_extents, position, rotation, pred)
    with np.errstate(all="ignore"):
        ok = ok & np.isfinite(pred) & (pred >= 0)
    cand = R._masks(s, n, mask, excluded, ok)
    if skip_sensors and sensor is not None:
        cand = cand & ~(np.asarray(sensor) != 0)[None, :]
    pos = np.asarray(position, dt).reshape(-1, 3)
    rows = {}
    for q, c, pen, nrm, a1, a2 in pairs:
        if not cand[q, c]:
            continue
        rec = np.zeros((), shape_contact_dtype(CR._bits(dt)))
        rec["collider"] = c; rec["entity"] = s.entity[c]; rec["penetration"] = pen
        rec["normal"] = nrm; rec["anchor1"] = a1; rec["anchor2"] = a2
        with np.errstate(all="ignore"):
            rec["point"] = [pos[q, i] + a1[i] for i in range(3)]
        rows.setdefault(q, []).append(rec)
    for q, l in rows.items():
        out[q] = np.array(l, shape_contact_dtype(CR._bits(dt)))
    return out


class _Manifolds:
    """contact_manifolds of the oracle world for a batch of pairs that may hold capsule queries: those rows come from capsule_contact (one
    point; the manifold normal is the oracle's, from the query towards the collider), the others from the oracle."""

    def __init__(self, bits):
        self.bits = bits

    def contact_manifolds(self, shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction):
        dt = np.float32 if self.bits == 32 else np.float64
        shape1 = np.asarray(shape1)
        cap = shape1 == SHAPE_CAPSULE
        k = len(shape1)
        m = {"point_count": np.zeros(k, np.uint32), "penetration": np.zeros((k, 16), dt), "normal": np.zeros((k, 3), dt),
             "point": np.zeros((k, 16, 3), dt), "anchor1": np.zeros((k, 16, 3), dt), "anchor2": np.zeros((k, 16, 3), dt)}
        if (~cap).any():
            i = np.nonzero(~cap)[0]
            o = _orig_oracle_world(self.bits).contact_manifolds(shape1[i], he1[i], pos1[i], rot1[i], shape2[i], he2[i], pos2[i], rot2[i], np.asarray(prediction, dt)[i])
            for key in m:
                m[key][i] = o[key]
        for j in np.nonzero(cap)[0]:
            r2 = S.make_isometry_rotation(rot1[j], dt)
            col = lambda a, n: tuple(np.asarray(a[j], dt)[i].reshape(1) for i in range(n))
            con, pen, nrm, a1, a2 = capsule_contact(dt(he1[j][0]), dt(he1[j][1]), tuple(np.array([x], dt) for x in r2), col(pos1, 3), np.asarray(shape2)[j:j + 1].astype(np.uint32),
                                                    col(he2, 3), col(pos2, 3), col(rot2, 4), np.asarray(prediction, dt)[j], dt)
            if con[0]:
                m["point_count"][j] = 1
                m["penetration"][j, 0] = pen[0]
                m["normal"][j] = [-x[0] for x in nrm]
                m["anchor1"][j, 0] = [x[0] for x in a1]; m["anchor2"][j, 0] = [x[0] for x in a2]
                with np.errstate(all="ignore"):
                    m["point"][j, 0] = [np.asarray(pos1[j], dt)[i] + a1[i][0] for i in range(3)]
        return m


@contextlib.contextmanager
def patched():
    """Lends this module's validity rule and pair functions to the existing references for one call and puts theirs back."""
    saved = (S.shape_valid, S.query_shape_aabb, CA.cast_pairs, CR.contact_lists, CR.oracle_world)
    S.shape_valid, S.query_shape_aabb, CA.cast_pairs, CR.contact_lists, CR.oracle_world = shape_valid, query_shape_aabb, cast_pairs, contact_lists, _Manifolds
    try:
        yield
    finally:
        S.shape_valid, S.query_shape_aabb, CA.cast_pairs, CR.contact_lists, CR.oracle_world = saved


def cast_queries(s, shape, half_extents, position, rotation, direction, ks=(), max_distance=None, mask=None, excluded=()):
    """avn_spatial_cast_shapes and avn_spatial_shape_hits for every k in ks from one brute-force pass."""
    with patched():
        return CA.cast_queries(s, shape, half_extents, position, rotation, direction, ks, max_distance, mask, excluded)


def shape_contacts(s, shape, half_extents, position, rotation, prediction, cap, **kw):
    return CR.pad(contact_lists(s, shape, half_extents, position, rotation, prediction, **kw), cap, CR._bits(s.dt))


def cast_moves(s, *a, **kw):
    with patched():
        return M.cast_moves(s, *a, **kw)


def move_and_slide(s, *a, **kw):
    with patched():
        return M.move_and_slide(s, *a, **kw)
