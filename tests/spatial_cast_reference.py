"""numpy restatement of the shape-cast tests of include/avian_mi355x_spatial.h, in the device's operation order (k_spatial.hip: sp_ball_ray,
sp_slab_ray, sp_round_box_ray, sp_sat_cast, sp_sat_witness, sp_cast_exact and k_sp_cast's node test), and brute-force versions of
avn_spatial_cast_shapes / avn_spatial_shape_hits with the same filter, tie and validity rules.

Built on spatial_query_reference and spatial_shape_reference: vectors are tuples of three arrays, quaternions of four, everything in the
world's dtype with no fused multiply-adds.  The pair tests broadcast over (query, collider); all three pair kinds are evaluated for every
pair and the one that applies is selected, which is what lets one pass serve a mixed scene."""
from __future__ import annotations

import numpy as np

import spatial_query_reference as R
import spatial_shape_reference as S
from spatial_query_reference import MISS, SHAPE_BALL, SHAPE_HOST, add, dot, qinverse, scale, sub
from spatial_shape_reference import na_dot, na_qmul, na_qrot, neg, support


def _w(c, a, b):
    return np.where(c, a, b)


def _sel(c, a, b):
    return tuple(np.where(c, x, y) for x, y in zip(a, b))


# ---- the primitives -------------------------------------------------------------------------------------------------------------------------
def ball_ray(o, d, r, dt):
    """sp_ball_ray: (ok, t, inside)."""
    zero = dt(0)
    a, b, c = dot(d, d), dot(o, d), dot(o, o) - r * r
    miss = (c > zero) & (b > zero)
    f = sub(o, scale(d, b / a))
    delta = a * (r * r - dot(f, f))
    miss = miss | (delta < zero)
    t = (-b - np.sqrt(delta)) / a
    inside = t <= zero
    return ~miss, _w(inside, zero, t), inside


def slab_ray(o, d, h, dt):
    """sp_slab_ray: (ok, t, axis, sg); axis = -1 when the origin is inside."""
    zero, one, inf = dt(0), dt(1), dt(np.inf)
    shp = np.broadcast(o[0], d[0], h[0]).shape
    tmin = np.full(shp, -inf, dt); tmax = np.full(shp, inf, dt)
    na = np.full(shp, -1, np.int32); nsg = np.zeros(shp, dt)
    ok = np.ones(shp, bool)
    for i in range(3):
        oi, di, hi = o[i], d[i], h[i]
        nz = di != zero
        inv = one / di
        t1, t2 = (-hi - oi) * inv, (hi - oi) * inv
        ng = inv < zero
        t1, t2 = _w(ng, t2, t1), _w(ng, t1, t2)
        sn = _w(ng, one, -one)
        un = nz & (t1 > tmin)
        uf = nz & (t2 < tmax)
        tmin = _w(un, t1, tmin); na = _w(un, i, na); nsg = _w(un, sn, nsg)
        tmax = _w(uf, t2, tmax)
        ok = ok & (nz | ~((oi < -hi) | (oi > hi)))
    ok = ok & (tmin <= tmax) & ~(tmax < zero)
    inside = tmin < zero
    return ok, _w(inside, zero, tmin), _w(inside, -1, na), _w(inside, zero, nsg)


def round_box_ray(o, d, he, r, dt):
    """sp_round_box_ray: (ok, t, normal xyz, pen) of a ball centre's ray against the cuboid rounded by r, in the cuboid's frame."""
    zero, one, inf = dt(0), dt(1), dt(np.inf)
    shp = np.broadcast(o[0], d[0], he[0], r).shape
    best = np.full(shp, inf, dt)
    found = np.zeros(shp, bool); bpen = np.zeros(shp, bool)
    bn = tuple(np.zeros(shp, dt) for _ in range(3))
    for i in range(3):
        h = tuple(he[j] + (r if j == i else zero) for j in range(3))
        ok, t, axis, sg = slab_ray(o, d, h, dt)
        upd = ok & (t < best)
        best = _w(upd, t, best); found = found | upd; bpen = _w(upd, axis < 0, bpen)
        bn = tuple(_w(upd, _w(axis == j, sg, zero), bn[j]) for j in range(3))
    rpos = r > zero
    for e in range(12):
        k = e >> 2
        ia, ib = (k + 1) % 3, (k + 2) % 3
        sa = one if e & 1 else -one
        sb = one if e & 2 else -one
        oa, ob = o[ia] - sa * he[ia], o[ib] - sb * he[ib]
        da, db, okk, dk, hk = d[ia], d[ib], o[k], d[k], he[k]
        a = da * da + db * db
        live = rpos & (a > zero)
        b, c = oa * da + ob * db, (oa * oa + ob * ob) - r * r
        live = live & ~((c > zero) & (b > zero))
        q = b / a
        fa, fb = oa - da * q, ob - db * q
        delta = a * (r * r - (fa * fa + fb * fb))
        live = live & ~(delta < zero)
        t = (-b - np.sqrt(delta)) / a
        inside = t <= zero
        t = _w(inside, zero, t)
        z = okk + dk * t
        live = live & (np.abs(z) <= hk)
        upd = live & (t < best)
        pa, pb = oa + da * t, ob + db * t
        l = np.sqrt(pa * pa + pb * pb)
        zn = inside | ~(l > zero)
        comp = {ia: _w(zn, zero, pa / l), ib: _w(zn, zero, pb / l), k: np.zeros(shp, dt)}
        best = _w(upd, t, best); found = found | upd; bpen = _w(upd, inside, bpen)
        bn = tuple(_w(upd, comp[j], bn[j]) for j in range(3))
    for s in range(8):
        cen = tuple(he[j] if s & (1 << j) else -he[j] for j in range(3))
        oc = sub(o, cen)
        ok, t, inside = ball_ray(oc, d, r, dt)
        upd = rpos & ok & (t < best)
        p = add(oc, scale(d, t))
        l = np.sqrt(dot(p, p))
        zn = inside | ~(l > zero)
        best = _w(upd, t, best); found = found | upd; bpen = _w(upd, inside, bpen)
        bn = tuple(_w(upd, _w(zn, zero, p[j] / l), bn[j]) for j in range(3))
    return found, best, bn, bpen


def _units(shp, dt):
    z = np.zeros(shp, dt)
    return ((z + dt(1), z, z), (z, z + dt(1), z), (z, z, z + dt(1)))


def sat_cast(he1, he2, qr, qt, dl, dt):
    """sp_sat_cast: (ok, t, kin, n xyz, pen)."""
    zero, one, inf = dt(0), dt(1), dt(np.inf)
    eps = dt(np.finfo(dt).eps)
    shp = np.broadcast(he1[0], he2[0], qr[0], qt[0], dl[0]).shape
    e = _units(shp, dt)
    u = [na_qrot(qr, x, dt) for x in e]
    tin = np.full(shp, -inf, dt); tout = np.full(shp, inf, dt)
    kin = np.full(shp, -1, np.int32)
    nin = tuple(np.zeros(shp, dt) for _ in range(3))
    miss = np.zeros(shp, bool)
    z = np.zeros(shp, dt)
    for k in range(15):
        live = np.ones(shp, bool)
        if k < 3:
            ax = e[k]
        elif k < 6:
            ax = u[k - 3]
        else:
            b, a = (k - 6) // 3, (k - 6) % 3
            ub = u[b]
            axis = (z, -ub[2], ub[1]) if a == 0 else ((ub[2], z, -ub[0]) if a == 1 else (-ub[1], ub[0], z))
            norm1 = np.sqrt(na_dot(axis, axis))
            live = norm1 > eps
            ax = tuple(x / norm1 for x in axis)
        s0, v = na_dot(ax, qt), na_dot(ax, dl)
        r1 = np.abs(ax[0]) * he1[0] + np.abs(ax[1]) * he1[1] + np.abs(ax[2]) * he1[2]
        r2 = np.abs(na_dot(ax, u[0])) * he2[0] + np.abs(na_dot(ax, u[1])) * he2[1] + np.abs(na_dot(ax, u[2])) * he2[2]
        rr = r1 + r2
        nz = v != zero
        inv = one / v
        t1, t2 = (-rr - s0) * inv, (rr - s0) * inv
        ng = inv < zero
        t1, t2 = _w(ng, t2, t1), _w(ng, t1, t2)
        sg = _w(ng, one, -one)
        un = live & nz & (t1 > tin)
        uf = live & nz & (t2 < tout)
        tin = _w(un, t1, tin); kin = _w(un, k, kin)
        nin = tuple(_w(un, ax[j] * sg, nin[j]) for j in range(3))
        tout = _w(uf, t2, tout)
        miss = miss | (live & ~nz & ((s0 < -rr) | (s0 > rr)))
    ok = ~miss & (tin <= tout) & ~(tout < zero)
    pen = tin < zero
    return ok, _w(pen, zero, tin), kin, nin, pen


def _clamp3(p, h):
    return tuple(_w(x < -hh, -hh, _w(x > hh, hh, x)) for x, hh in zip(p, h))


def sat_witness(he1, he2, qr, tp, kin, n, dt):
    """sp_sat_witness: (p1, p2) in the collider's frame."""
    shp = np.broadcast(he1[0], he2[0], qr[0], tp[0], kin, n[0]).shape
    eps = dt(np.finfo(dt).eps)
    qri = qinverse(qr)
    s1 = support(he1, n)
    s2 = add(na_qrot(qr, support(he2, na_qrot(qri, neg(n), dt)), dt), tp)
    # a face of the collider
    f1 = tuple(_w(kin == j, n[j] * he1[j], s2[j]) for j in range(3))
    f2 = s2
    f_in = np.logical_and.reduce([(kin == j) | (np.abs(s2[j]) <= he1[j]) for j in range(3)])
    # a face of the query
    h = _w(kin == 3, he2[0], _w(kin == 4, he2[1], he2[2]))
    g1 = s1
    g2 = sub(s1, scale(n, na_dot(sub(s1, tp), n) + h))
    x = na_qrot(qri, sub(s1, tp), dt)
    g_in = np.logical_and.reduce([(kin == 3 + j) | (np.abs(x[j]) <= he2[j]) for j in range(3)])
    xl = na_qrot(qri, neg(n), dt)
    xc = _clamp3(x, he2)
    xf = tuple(_w(kin == 3 + j, np.copysign(he2[j], xl[j]), xc[j]) for j in range(3))
    go = add(na_qrot(qr, xf, dt), tp)
    # an edge pair
    ke = np.where(kin >= 6, kin - 6, 0)
    b, a = ke // 3, ke % 3
    ea = tuple(_w(a == j, dt(1), dt(0)) + np.zeros(shp, dt) for j in range(3))
    eb = tuple(_w(b == j, dt(1), dt(0)) + np.zeros(shp, dt) for j in range(3))
    ub = na_qrot(qr, eb, dt)
    w = sub(s1, s2)
    bc, cc, dd, ee = na_dot(ea, ub), na_dot(ub, ub), na_dot(ea, w), na_dot(ub, w)
    den = cc - bc * bc
    cross = den > eps
    lam, mu = (bc * ee - cc * dd) / den, (ee - bc * dd) / den
    h1 = _sel(cross, add(s1, scale(ea, lam)), sub(s1, scale(ea, na_dot(ea, s1))))
    h2 = add(s2, scale(ub, mu))
    xe = na_qrot(qri, sub(h2, tp), dt)
    hea = _w(a == 0, he1[0], _w(a == 1, he1[1], he1[2]))
    heb = _w(b == 0, he2[0], _w(b == 1, he2[1], he2[2]))
    xeb = _w(b == 0, xe[0], _w(b == 1, xe[1], xe[2]))
    h_in = cross & (np.abs(na_dot(ea, h1)) <= hea) & (np.abs(xeb) <= heb)
    face1, face2 = kin < 3, kin < 6
    p1 = _sel(face1, f1, _sel(face2, g1, h1))
    p2 = _sel(face1, f2, _sel(face2, g2, h2))
    inside = _w(face1, f_in, _w(face2, g_in, h_in))
    # the common way out: onto the collider, onto the query, and once more
    cq = lambda p: add(na_qrot(qr, _clamp3(na_qrot(qri, sub(p, tp), dt), he2), dt), tp)
    start = _sel(face2 & ~face1, go, p1)
    c1 = _clamp3(cq(_clamp3(start, he1)), he1)
    return _sel(inside, p1, c1), _sel(inside, p2, cq(c1))


def cast_exact(shape2, he2, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt):
    """sp_cast_exact, broadcasting over (query, collider): r2 is make_isometry's rotation of the query shape, pos2 its position.
    Returns (hit, toi, point1, point2, normal1), everything 0 where there is no hit."""
    zero = dt(0)
    with np.errstate(all="ignore"):
        ri = qinverse(rot1)
        qr = na_qmul(ri, r2)
        qt = na_qrot(ri, sub(pos2, pos1), dt)
        dl = na_qrot(ri, d, dt)
        shp = np.broadcast(qr[0], qt[0], dl[0], he1[0], he2[0], max_distance).shape
        bc = lambda t: tuple(np.broadcast_to(x, shp) for x in t)
        qr, qt, dl, he1, he2, d, pos1, pos2, rot1, r2 = bc(qr), bc(qt), bc(dl), bc(he1), bc(he2), bc(d), bc(pos1), bc(pos2), bc(rot1), bc(r2)
        ball1 = np.broadcast_to(shape1 == SHAPE_BALL, shp); ball2 = np.broadcast_to(shape2 == SHAPE_BALL, shp)
        zv = tuple(np.zeros(shp, dt) for _ in range(3))
        # ball / ball
        bb_ok, bb_t, bb_pen = ball_ray(qt, dl, he1[0] + he2[0], dt)
        # ball and cuboid: the ball's centre in the cuboid's frame
        qri = qinverse(qr)
        o_b = na_qrot(qri, sub(zv, qt), dt)
        d_b = neg(na_qrot(qri, dl, dt))
        o = _sel(ball2, qt, o_b); dd = _sel(ball2, dl, d_b)
        hek = _sel(ball2, he1, he2); rk = _w(ball2, he2[0], he1[0])
        rb_ok, rb_t, rb_n, rb_pen = round_box_ray(o, dd, hek, rk, dt)
        # cuboid / cuboid
        st_ok, st_t, kin, st_n, st_pen = sat_cast(he1, he2, qr, qt, dl, dt)
        both, one = ball1 & ball2, ball1 | ball2
        ok = _w(both, bb_ok, _w(one, rb_ok, st_ok))
        t = _w(both, bb_t, _w(one, rb_t, st_t))
        pen = _w(both, bb_pen, _w(one, rb_pen, st_pen))
        hit = ok & (t <= max_distance) & np.isfinite(t) & np.broadcast_to(shape1 != SHAPE_HOST, shp)
        c2 = add(pos2, scale(d, t))
        # ball / ball witnesses
        p = add(qt, scale(dl, t))
        l = np.sqrt(dot(p, p))
        nbb = tuple(_w(l > zero, x / l, zero) for x in p)
        bb_n1 = na_qrot(rot1, nbb, dt)
        bb_p1 = add(na_qrot(rot1, scale(nbb, he1[0]), dt), pos1)
        bb_p2 = add(c2, scale(neg(bb_n1), he2[0]))
        # ball query on a cuboid collider
        pk = sub(add(qt, scale(dl, t)), scale(rb_n, he2[0]))
        a_n1 = na_qrot(rot1, rb_n, dt)
        a_p1 = add(na_qrot(rot1, pk, dt), pos1)
        a_p2 = add(c2, scale(neg(a_n1), he2[0]))
        # cuboid query on a ball collider
        pk = sub(add(o_b, scale(d_b, t)), scale(rb_n, he1[0]))
        b_n1 = neg(na_qrot(r2, rb_n, dt))
        b_p2 = add(na_qrot(r2, pk, dt), c2)
        b_p1 = add(pos1, scale(b_n1, he1[0]))
        # cuboid / cuboid
        w1, w2 = sat_witness(he1, he2, qr, add(qt, scale(dl, t)), kin, st_n, dt)
        c_n1 = na_qrot(rot1, st_n, dt)
        c_p1 = add(na_qrot(rot1, w1, dt), pos1)
        c_p2 = add(na_qrot(rot1, w2, dt), pos1)
        pick = lambda bb, a, b, c: _sel(both, bb, _sel(ball2, a, _sel(ball1, b, c)))
        keep = hit & ~pen
        n1 = _sel(keep, pick(bb_n1, a_n1, b_n1, c_n1), zv)
        p1 = _sel(keep, pick(bb_p1, a_p1, b_p1, c_p1), zv)
        p2 = _sel(keep, pick(bb_p2, a_p2, b_p2, c_p2), zv)
    return hit, _w(hit, t, zero), p1, p2, n1


# ---- the query's validity, box and node test --------------------------------------------------------------------------------------------------
def cast_valid(shape, he, pos, rot, direction, max_distance, dt):
    """k_sp_cast's per-query guard: k_sp_shapes' rule plus a finite direction and a max_distance that is not NaN."""
    ok, he, pos, rot = S.shape_valid(shape, he, pos, rot, dt)
    direction = np.asarray(direction, dt).reshape(-1, 3)
    max_distance = np.asarray(max_distance, dt).reshape(-1)
    return ok & np.isfinite(direction).all(1) & ~np.isnan(max_distance), he, pos, rot, direction, max_distance


def cast_box(shape, he, pos, rot, dt):
    """The origin of the cast ray and the half widths the node boxes grow by: centre and half widths of the query shape's padded AABB."""
    lo, hi = S.query_shape_aabb(shape, he, pos, rot, dt)
    with np.errstate(all="ignore"):
        return tuple((a + b) * dt(0.5) for a, b in zip(lo, hi)), tuple((b - a) * dt(0.5) for a, b in zip(lo, hi))


def node_entry(centre, hw, d, lo, hi, limit, dt):
    """k_sp_cast's node test: sp_ray_box of the cast ray against the node box grown by the half widths (+inf = culled)."""
    with np.errstate(all="ignore"):
        return R.ray_box(centre, d, tuple(l - h for l, h in zip(lo, hw)), tuple(x + h for x, h in zip(hi, hw)), limit, dt)


# ---- brute-force queries -----------------------------------------------------------------------------------------------------------------------
def _bits(dt):
    return 32 if dt == np.float32 else 64


def cast_pairs(s: R.Snapshot, shape, half_extents, position, rotation, direction, max_distance=None):
    """Per (cast, collider): cast_exact, no filter; rows of invalid casts are all misses.  Returns (hit, toi, p1, p2, n1, valid)."""
    dt = s.dt
    shape = np.asarray(shape)
    n = len(shape)
    max_distance = np.full(n, np.inf, dt) if max_distance is None else max_distance
    ok, he, pos, rot, direction, max_distance = cast_valid(shape, half_extents, position, rotation, direction, max_distance, dt)
    z = lambda: np.zeros((n, s.n), dt)
    hit = np.zeros((n, s.n), bool); toi = z()
    p1, p2, n1 = tuple(z() for _ in range(3)), tuple(z() for _ in range(3)), tuple(z() for _ in range(3))
    idx = np.nonzero(ok)[0]
    if len(idx) and s.n:
        r2 = np.array([S.make_isometry_rotation(rot[i], dt) for i in idx], dt).reshape(-1, 4)
        q = lambda a, k: tuple(a[:, i][:, None] for i in range(k))
        col = lambda t: tuple(x[None, :] for x in t)
        h, t, a, b, c = cast_exact(shape[idx][:, None], q(he[idx], 3), q(r2, 4), q(pos[idx], 3), q(direction[idx], 3), max_distance[idx][:, None],
                                   s.shape[None, :], col(s.he), col(s.pos), col(s.rot), dt)
        hit[idx] = h; toi[idx] = t
        for j in range(3):
            p1[j][idx] = a[j]; p2[j][idx] = b[j]; n1[j][idx] = c[j]
    return hit, toi, p1, p2, n1, ok


def cast_queries(s: R.Snapshot, shape, half_extents, position, rotation, direction, ks=(), max_distance=None, mask=None, excluded=()):
    """avn_spatial_cast_shapes and avn_spatial_shape_hits for every k in ks from ONE brute-force pass: (closest, {k: (records, counts)})."""
    from avian_amd.spatial_query import shape_hit_dtype
    hd = shape_hit_dtype(_bits(s.dt))
    hit, toi, p1, p2, n1, ok = cast_pairs(s, shape, half_extents, position, rotation, direction, max_distance)
    n = len(ok)
    hit = hit & R._masks(s, n, mask, excluded, ok)
    blank = lambda shp: _miss(np.zeros(shp, hd))
    closest = blank(n)
    many = {k: (blank((n, k)), np.zeros(n, np.uint32)) for k in ks}
    kmax = max(ks) if ks else 1
    for r in range(n):
        idx = np.nonzero(hit[r])[0]
        if not len(idx):
            continue
        order = idx[np.lexsort((idx, toi[r, idx]))][:kmax]
        recs = []
        for c in order:
            nn = np.array([n1[j][r, c] for j in range(3)], s.dt)
            n2 = np.where(nn == 0, s.dt(0), -nn)
            recs.append((c, s.entity[c], toi[r, c], tuple(p1[j][r, c] for j in range(3)), tuple(p2[j][r, c] for j in range(3)), tuple(nn), tuple(n2)))
        closest[r] = recs[0]
        for k, (h, cnt) in many.items():
            cnt[r] = len(idx)
            for j, rec in enumerate(recs[:k]):
                h[r, j] = rec
    return closest, many


def _miss(a):
    a["collider"] = MISS; a["entity"] = MISS
    return a


def cast_shapes(s, shape, half_extents, position, rotation, direction, max_distance=None, mask=None, excluded=()):
    return cast_queries(s, shape, half_extents, position, rotation, direction, (), max_distance, mask, excluded)[0]


def shape_hits(s, shape, half_extents, position, rotation, direction, max_hits, max_distance=None, mask=None, excluded=()):
    return cast_queries(s, shape, half_extents, position, rotation, direction, (max_hits,), max_distance, mask, excluded)[1][max_hits]
