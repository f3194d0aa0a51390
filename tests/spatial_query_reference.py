"""numpy restatement of the spatial queries' exact per-collider tests (include/avian_mi355x_spatial.h) and brute-force versions of the four
queries with the same tie rules and filters.

Every function computes in the world's dtype, in the device's operation order (the library is compiled with -ffp-contract=off: no fused
multiply-adds), vectorised over colliders and queries by broadcasting.  Vectors are tuples of three arrays (x, y, z), quaternions of four."""
from __future__ import annotations

import numpy as np

MISS = 0xFFFFFFFF
SHAPE_CUBOID, SHAPE_BALL, SHAPE_HOST = 0, 1, 2


# ---- avn_math.h ------------------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def qrot(q, v, dt):
    w = q[3]
    b = (q[0], q[1], q[2])
    b2 = dot(b, b)
    return add(add(scale(v, w * w - b2), scale(b, dot(v, b) * dt(2))), scale(cross(b, v), w * dt(2)))


def qinverse(q):
    return (-q[0], -q[1], -q[2], q[3])


def qmul(l, r, dt):
    lx, ly, lz, lw = l
    rx, ry, rz, rw = r
    if dt == np.float32:   # glam's SSE2 association
        return ((lw * rx + lx * rw) + (ly * rz + -(lz * ry)),
                (lw * ry + -(lx * rz)) + (ly * rw + lz * rx),
                (lw * rz + lx * ry) + (-(ly * rx) + lz * rw),
                (lw * rw + -(lx * rx)) + (-(ly * ry) + -(lz * rz)))
    return (lw * rx + lx * rw + ly * rz - lz * ry, lw * ry - lx * rz + ly * rw + lz * rx, lw * rz + lx * ry - ly * rx + lz * rw, lw * rw - lx * rx - ly * ry - lz * rz)


def qnormalize(q, dt):
    if dt == np.float32:
        l = np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
        return (q[0] / l, q[1] / l, q[2] / l, q[3] / l)
    r = dt(1) / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return (q[0] * r, q[1] * r, q[2] * r, q[3] * r)


def _cols(a, dt, k):
    a = np.asarray(a, dt).reshape(-1, k)
    return tuple(a[:, i] for i in range(k))


# ---- snapshot ---------------------------------------------------------------------------------------------------------------------------
class Snapshot:
    """What avn_spatial_update records per collider: pose (collider_pose), half extents, shape, entity, memberships."""

    def __init__(self, bodies, colliders, transforms=None, dtype=np.float32):
        dt = self.dt = dtype
        body = np.asarray(colliders["body"], np.int64)
        bp = _cols(np.asarray(bodies["position"], dt)[body], dt, 3)
        br = _cols(np.asarray(bodies["rotation"], dt)[body], dt, 4)
        pos, rot = bp, br
        if transforms is not None and transforms.get("is_child") is not None and np.any(np.asarray(transforms["is_child"]) != 0):
            child = np.asarray(transforms["is_child"]) != 0
            lp = _cols(transforms["translation"], dt, 3)
            lr = _cols(transforms["rotation"], dt, 4)
            cpos = add(bp, qrot(br, lp, dt))
            crot = qnormalize(qmul(br, lr, dt), dt)
            pos = tuple(np.where(child, c, b) for c, b in zip(cpos, bp))
            rot = tuple(np.where(child, c, b) for c, b in zip(crot, br))
        self.pos, self.rot = pos, rot
        self.he = _cols(colliders["half_extents"], dt, 3)
        self.shape = np.asarray(colliders["shape"], np.uint32)
        self.entity = np.asarray(colliders["entity_index"], np.uint32)
        m = colliders.get("memberships")
        self.memberships = np.ones(len(self.shape), np.uint32) if m is None else np.asarray(m, np.uint32)
        self.n = len(self.shape)

    def finite(self):
        """k_sp_snapshot's candidate flag: a finite position, rotation and shape AABB (the header's non-finite contract)."""
        with np.errstate(all="ignore"):
            mn, mx = shape_aabb(self.shape, self.he, self.pos, self.rot, self.dt)
        return np.logical_and.reduce([np.isfinite(x) for x in self.pos + self.rot + mn + mx])

    def candidates(self, mask=0xFFFFFFFF, excluded=()):
        ok = (self.shape != SHAPE_HOST) & self.finite() & ((self.memberships & np.uint32(mask)) != 0)
        if len(excluded):
            ok &= ~np.isin(self.entity, np.asarray(excluded, np.uint32))
        return ok


# ---- exact tests (k_spatial.hip: sp_ray_exact, sp_point_exact, sp_aabb_exact; avn_kernels.h: shape_aabb) ------------------------------------
def shape_aabb(shape, h, pos, q, dt):
    i, j, k, w = q
    two = dt(2)
    ww, ii, jj, kk = w * w, i * i, j * j, k * k
    ij, wk, wj, ik, jk, wi = i * j * two, w * k * two, w * j * two, i * k * two, j * k * two, w * i * two
    m00, m01, m02 = np.abs(((ww + ii) - jj) - kk), np.abs(ij - wk), np.abs(wj + ik)
    m10, m11, m12 = np.abs(wk + ij), np.abs(((ww - ii) + jj) - kk), np.abs(jk - wi)
    m20, m21, m22 = np.abs(ik - wj), np.abs(wi + jk), np.abs(((ww - ii) - jj) + kk)
    cub = ((m00 * h[0] + m01 * h[1]) + m02 * h[2], (m10 * h[0] + m11 * h[1]) + m12 * h[2], (m20 * h[0] + m21 * h[1]) + m22 * h[2])
    ball = shape == SHAPE_BALL
    he = tuple(np.where(ball, h[0], c) for c in cub)
    return sub(pos, he), add(pos, he)


def ray_exact(shape, he, pos, rot, o, d, max_distance, solid, dt):
    """Broadcast over colliders / rays: (hit, toi, normal xyz) with the header's tie rules; toi / normal are 0 where there is no hit."""
    ci = qinverse(rot)
    ol = qrot(ci, sub(o, pos), dt)
    dl = qrot(ci, d, dt)
    zero, one, inf = dt(0), dt(1), dt(np.inf)
    shp = np.broadcast(shape, ol[0], dl[0], max_distance, solid).shape
    shape = np.broadcast_to(shape, shp); solid = np.broadcast_to(solid, shp)
    ol = tuple(np.broadcast_to(x, shp) for x in ol); dl = tuple(np.broadcast_to(x, shp) for x in dl)
    he = tuple(np.broadcast_to(np.asarray(x, dt), shp) for x in he)
    with np.errstate(all="ignore"):
        # ball (parry ray_toi_with_ball)
        r = he[0]
        a, b, c = dot(dl, dl), dot(ol, dl), dot(ol, ol) - r * r
        f = sub(ol, scale(dl, b / a))          # b^2 - a c in its well-conditioned form
        delta = a * (r * r - dot(f, f))
        b_ok = ~((c > zero) & (b > zero)) & ~(delta < zero)
        sq = np.sqrt(delta)
        tb = (-b - sq) / a
        b_inside = tb <= zero
        b_zero = b_inside & solid
        tb = np.where(b_inside, np.where(solid, zero, (-b + sq) / a), tb)
        p = add(ol, scale(dl, tb))
        lp = np.sqrt(dot(p, p))
        b_zero = b_zero | ~(lp > zero)
        nb = tuple(np.where(b_zero, zero, x / lp) for x in p)
        # cuboid (slab clip)
        tmin = np.full(shp, -inf, dt); tmax = np.full(shp, inf, dt)
        na = np.full(shp, -1, np.int32); fa = np.full(shp, -1, np.int32)
        nsg = np.zeros(shp, dt); fsg = np.zeros(shp, dt)
        c_ok = np.ones(shp, bool)
        for i in range(3):
            oi, di, hi = ol[i], dl[i], he[i]
            nz = di != zero
            inv = one / di
            t1, t2 = (-hi - oi) * inv, (hi - oi) * inv
            neg = inv < zero
            t1, t2 = np.where(neg, t2, t1), np.where(neg, t1, t2)
            sn, sf = np.where(neg, one, -one), np.where(neg, -one, one)
            upd_n = nz & (t1 > tmin)
            upd_f = nz & (t2 < tmax)
            tmin = np.where(upd_n, t1, tmin); na = np.where(upd_n, i, na); nsg = np.where(upd_n, sn, nsg)
            tmax = np.where(upd_f, t2, tmax); fa = np.where(upd_f, i, fa); fsg = np.where(upd_f, sf, fsg)
            c_ok &= nz | ~((oi < -hi) | (oi > hi))
        c_ok &= (tmin <= tmax) & ~(tmax < zero)
        inside = tmin < zero
        tc = np.where(inside, np.where(solid, zero, tmax), tmin)
        axis = np.where(inside, np.where(solid, -1, fa), na)
        sg = np.where(inside, fsg, nsg)
        nl = tuple(np.where(axis == i, sg, zero) for i in range(3))
        c_zero = axis < 0
        is_ball = shape == SHAPE_BALL
        toi = np.where(is_ball, tb, tc)
        hit = np.where(is_ball, b_ok, c_ok) & (toi <= max_distance) & np.isfinite(toi) & (shape != SHAPE_HOST)
        nloc = tuple(np.where(is_ball, x, y) for x, y in zip(nb, nl))
        zn = np.where(is_ball, b_zero, c_zero)
        nw = qrot(rot, nloc, dt)
        nw = tuple(np.where(zn | ~hit, zero, np.broadcast_to(x, shp)) for x in nw)
    return hit, np.where(hit, toi, zero), nw


def point_exact(shape, he, pos, rot, p, dt):
    pl = qrot(qinverse(rot), sub(p, pos), dt)
    ball = dot(pl, pl) <= he[0] * he[0]
    cub = (np.abs(pl[0]) <= he[0]) & (np.abs(pl[1]) <= he[1]) & (np.abs(pl[2]) <= he[2])
    return np.where(shape == SHAPE_BALL, ball, cub) & (shape != SHAPE_HOST)


def aabb_exact(shape, he, pos, rot, qmin, qmax, dt):
    mn, mx = shape_aabb(shape, he, pos, rot, dt)
    ok = np.ones(np.broadcast(mn[0], qmin[0]).shape, bool)
    for i in range(3):
        ok &= (mn[i] <= qmax[i]) & (mx[i] >= qmin[i])
    return ok & (shape != SHAPE_HOST)


# ---- brute-force queries ----------------------------------------------------------------------------------------------------------------
def _masks(s: Snapshot, n, mask, excluded, finite_query):
    """Candidates per (query, collider); a query whose inputs are not all finite has none (k_sp_query's guard)."""
    base = s.candidates(0xFFFFFFFF, excluded)[None, :] & np.asarray(finite_query, bool).reshape(n, 1)
    if mask is None:
        return base
    return base & ((s.memberships[None, :] & np.asarray(mask, np.uint32)[:, None]) != 0)


def _finite_rows(*arrays):
    return np.logical_and.reduce([np.isfinite(a).all(axis=1) for a in arrays])


def _ray_all(s: Snapshot, origin, direction, max_distance, solid, mask, excluded, chunk):
    dt = s.dt
    origin = np.asarray(origin, dt).reshape(-1, 3); direction = np.asarray(direction, dt).reshape(-1, 3)
    n = len(origin)
    max_distance = np.full(n, np.inf, dt) if max_distance is None else np.asarray(max_distance, dt)
    solid = np.ones(n, bool) if solid is None else np.asarray(solid) != 0
    cand = _masks(s, n, mask, excluded, _finite_rows(origin, direction))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        o = tuple(origin[a:b, i][:, None] for i in range(3)); d = tuple(direction[a:b, i][:, None] for i in range(3))
        hit, toi, nrm = ray_exact(s.shape[None, :], tuple(x[None, :] for x in s.he), tuple(x[None, :] for x in s.pos), tuple(x[None, :] for x in s.rot),
                                  o, d, max_distance[a:b, None], solid[a:b, None], dt)
        yield a, b, hit & cand[a:b], toi, nrm


def cast_rays(s: Snapshot, origin, direction, max_distance=None, solid=None, mask=None, excluded=(), chunk=16):
    """Closest hit per ray by (distance, collider index): a structured array like avn_spatial_hit_fNN."""
    from avian_amd.spatial_query import hit_dtype
    n = len(np.asarray(origin).reshape(-1, 3))
    out = np.zeros(n, hit_dtype(32 if s.dt == np.float32 else 64))
    out["collider"] = MISS; out["entity"] = MISS
    for a, b, hit, toi, nrm in _ray_all(s, origin, direction, max_distance, solid, mask, excluded, chunk):
        key = np.where(hit, toi, np.inf)
        for r in range(b - a):
            if not hit[r].any():
                continue
            c = int(np.lexsort((np.arange(s.n), key[r]))[0])   # smallest distance, then smallest index
            out[a + r] = (c, s.entity[c], toi[r, c], (nrm[0][r, c], nrm[1][r, c], nrm[2][r, c]))
    return out


def ray_hits(s: Snapshot, origin, direction, max_hits, max_distance=None, solid=None, mask=None, excluded=(), chunk=16):
    """The max_hits nearest hits per ray by (distance, collider index), MISS-padded, and the true counts."""
    from avian_amd.spatial_query import hit_dtype
    n = len(np.asarray(origin).reshape(-1, 3))
    out = np.zeros((n, max_hits), hit_dtype(32 if s.dt == np.float32 else 64))
    out["collider"] = MISS; out["entity"] = MISS
    count = np.zeros(n, np.uint32)
    for a, b, hit, toi, nrm in _ray_all(s, origin, direction, max_distance, solid, mask, excluded, chunk):
        for r in range(b - a):
            idx = np.nonzero(hit[r])[0]
            count[a + r] = len(idx)
            order = idx[np.lexsort((idx, toi[r, idx]))][:max_hits]
            for k, c in enumerate(order):
                out[a + r, k] = (c, s.entity[c], toi[r, c], (nrm[0][r, c], nrm[1][r, c], nrm[2][r, c]))
    return out, count


def _ids(hits_rows, cap):
    n = len(hits_rows)
    ids = np.full((n, cap), MISS, np.uint32)
    count = np.zeros(n, np.uint32)
    for r, row in enumerate(hits_rows):
        idx = np.nonzero(row)[0]
        count[r] = len(idx)
        ids[r, :min(cap, len(idx))] = idx[:cap]
    return ids, count


def point_intersections(s: Snapshot, points, cap, mask=None, excluded=(), chunk=64):
    dt = s.dt
    points = np.asarray(points, dt).reshape(-1, 3)
    cand = _masks(s, len(points), mask, excluded, _finite_rows(points))
    rows = []
    for a in range(0, len(points), chunk):
        p = tuple(points[a:a + chunk, i][:, None] for i in range(3))
        rows.append(point_exact(s.shape[None, :], tuple(x[None, :] for x in s.he), tuple(x[None, :] for x in s.pos), tuple(x[None, :] for x in s.rot), p, dt) & cand[a:a + chunk])
    return _ids(np.concatenate(rows) if rows else np.zeros((0, s.n), bool), cap)


def aabb_intersections(s: Snapshot, qmin, qmax, cap, mask=None, excluded=()):
    dt = s.dt
    qmin = np.asarray(qmin, dt).reshape(-1, 3); qmax = np.asarray(qmax, dt).reshape(-1, 3)
    mn, mx = shape_aabb(s.shape, s.he, s.pos, s.rot, dt)
    cand = _masks(s, len(qmin), mask, excluded, _finite_rows(qmin, qmax))
    ok = np.ones((len(qmin), s.n), bool)
    for i in range(3):
        ok &= (mn[i][None, :] <= qmax[:, i][:, None]) & (mx[i][None, :] >= qmin[:, i][:, None])
    return _ids(ok & (s.shape != SHAPE_HOST)[None, :] & cand, cap)


def ray_queries(s: Snapshot, origin, direction, ks=(), max_distance=None, solid=None, mask=None, excluded=(), chunk=16):
    """cast_rays and ray_hits for every k in ks from ONE brute-force pass: (closest, {k: (records, counts)})."""
    from avian_amd.spatial_query import hit_dtype
    hd = hit_dtype(32 if s.dt == np.float32 else 64)
    n = len(np.asarray(origin).reshape(-1, 3))
    closest = np.zeros(n, hd); closest["collider"] = MISS; closest["entity"] = MISS
    many = {}
    for k in ks:
        h = np.zeros((n, k), hd); h["collider"] = MISS; h["entity"] = MISS
        many[k] = (h, np.zeros(n, np.uint32))
    kmax = max(ks) if ks else 1
    for a, b, hit, toi, nrm in _ray_all(s, origin, direction, max_distance, solid, mask, excluded, chunk):
        for r in range(b - a):
            idx = np.nonzero(hit[r])[0]
            if not len(idx):
                continue
            order = idx[np.lexsort((idx, toi[r, idx]))][:kmax]
            recs = [(c, s.entity[c], toi[r, c], (nrm[0][r, c], nrm[1][r, c], nrm[2][r, c])) for c in order]
            closest[a + r] = recs[0]
            for k, (h, cnt) in many.items():
                cnt[a + r] = len(idx)
                for j, rec in enumerate(recs[:k]):
                    h[a + r, j] = rec
    return closest, many


# ---- the tree's node tests (k_spatial.hip: k_sp_snapshot's padded leaf box, sp_ray_box, sp_point_box) -------------------------------------
def leaf_boxes(s: Snapshot):
    """The leaf box of every collider: the shape AABB grown by 64 eps * its largest coordinate; empty (+inf / -inf) for non-candidates."""
    dt = s.dt
    with np.errstate(all="ignore"):
        mn, mx = shape_aabb(s.shape, s.he, s.pos, s.rot, dt)
        m = np.maximum.reduce([np.abs(x) for x in mn + mx])
        pad = dt(64) * dt(np.finfo(dt).eps) * m
        ok = (s.shape != SHAPE_HOST) & s.finite()
        lo = tuple(np.where(ok, x - pad, dt(np.inf)) for x in mn)
        hi = tuple(np.where(ok, x + pad, dt(-np.inf)) for x in mx)
    return lo, hi


def ray_box(o, d, lo, hi, limit, dt):
    """sp_ray_box with the query's tolerance 64 eps * max |o|: the entry distance into the grown box, +inf for a miss (broadcasting)."""
    with np.errstate(all="ignore"):
        tol = dt(64) * dt(np.finfo(dt).eps) * np.maximum(np.maximum(np.abs(o[0]), np.abs(o[1])), np.abs(o[2]))
        tmin, tmax = dt(-np.inf), dt(np.inf)
        miss = np.zeros(np.broadcast(o[0], lo[0], limit).shape, bool)
        for i in range(3):
            l, h, oi, di = lo[i] - tol, hi[i] + tol, o[i], d[i]
            zero = di == dt(0)
            iv = np.where(zero, dt(0), dt(1) / np.where(zero, dt(1), di))
            t1, t2 = (l - oi) * iv, (h - oi) * iv
            neg = iv < dt(0)
            t1, t2 = np.where(neg, t2, t1), np.where(neg, t1, t2)
            miss |= zero & ~((oi >= l) & (oi <= h))
            # smax / smin: NaN-ignoring (a NaN of t1 / t2 leaves the bound as it was)
            tmin = np.where(zero | (tmin > t1) | np.isnan(t1), tmin, t1)
            tmax = np.where(zero | (tmax < t2) | np.isnan(t2), tmax, t2)
        miss |= ~(tmin <= tmax) | (tmax < dt(0)) | ~(tmin <= limit)
        return np.where(miss, dt(np.inf), np.maximum(tmin, dt(0)))


def point_box(p, lo, hi, dt):
    """sp_point_box with the query's tolerance 64 eps * max |p| (broadcasting)."""
    tol = dt(64) * dt(np.finfo(dt).eps) * np.maximum(np.maximum(np.abs(p[0]), np.abs(p[1])), np.abs(p[2]))
    return np.logical_and.reduce([(p[i] >= lo[i] - tol) & (p[i] <= hi[i] + tol) for i in range(3)])
