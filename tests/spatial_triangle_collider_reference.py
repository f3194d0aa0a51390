"""numpy restatement of the spatial queries against Triangle COLLIDERS of include/avian_mi355x_spatial.h ("queries against triangle colliders"), in the
device's operation order (avn_spatial_triangle_pair.h: sp_tri_ray, sp_tri_point, sp_seg_tri_d2, sp_tricol_intersects, sp_tri_sat_cast,
sp_tri_sat_witness, sp_tricol_cast_exact; avn_triangle_pair.h: tri_closest_point, tri_seg_closest, tri_box_axis; k_spatial.hip: the CTRI branches of
the leaf tests), and brute-force versions of every entry point for snapshots that hold triangle colliders next to balls, cuboids and capsules.

Built on the existing references exactly as spatial_capsule_collider_reference is: vectors are tuples of three arrays, everything in the world's dtype with
no fused multiply-adds, the pair tests broadcast over (query, collider).  The rows of the other collider kinds are answered by
spatial_capsule_collider_reference (and through it by the older references) unchanged; the contacts against a triangle collider are the deepest point of
triangle_collider_reference.manifold (the narrow phase's) with the query as shape 1.  `patched(snapshot)` lends this module's pair functions to the existing
brute-force code for the length of one call.

The pair functions of the brute force receive (shape, half extents, pose) per collider and nothing that names the collider, so a snapshot made by
`with_triangles` carries, for its triangle colliders only, the collider's own index in half_extents.x (a triangle has no half extents: nothing else reads
them); the vertex table is looked up through it, whatever subset or broadcast of the colliders a caller passes.

closest_point here is triangle_collider_reference.closest_point evaluated for whole arrays (every branch in full, then selected in the order of its
tests); tests/test_spatial_triangle_colliders_cpu.py holds the two to each other bit for bit."""
from __future__ import annotations

import contextlib
import copy

import numpy as np

import spatial_capsule_collider_reference as K
import spatial_capsule_reference as C
import spatial_cast_reference as CA
import spatial_caster_reference as CS
import spatial_contact_reference as CR
import spatial_move_reference as M
import spatial_query_reference as R
import spatial_shape_reference as S
import triangle_collider_reference as T
from spatial_query_reference import add, dot, qinverse, qrot, scale, sub
from spatial_shape_reference import na_cross, na_dot, na_qmul, na_qrot, neg, support

SHAPE_TRIANGLE = 4
SHAPE_CAPSULE = 3
ROUNDS = K.ROUNDS
_w = np.where
_sel = C._sel

last_rounds = 0   # the most Newton rounds of a pair against a triangle collider since reset_rounds(): the tests' cap check reads it


def reset_rounds():
    global last_rounds
    last_rounds = 0


def _note_rounds(rounds, rows):
    global last_rounds
    if np.size(rounds) and np.any(rows):
        last_rounds = max(last_rounds, int(np.max(_w(rows, rounds, 0))))


# ---- the primitives (arrays; a, b, c, p: tuples of three arrays) ---------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt(na_dot(v, v))


def unit_normal(a, b, c):
    nrm = na_cross(sub(b, a), sub(c, a))
    l = _norm(nrm)
    return tuple(x / l for x in nrm)


def closest_point(a, b, c, p, dt):
    """tri_closest_point: (point, region) -- Ericson 5.1.5, every branch evaluated, the first test that holds wins."""
    zero = dt(0)
    ab, ac, ap = sub(b, a), sub(c, a), sub(p, a)
    d1, d2 = na_dot(ab, ap), na_dot(ac, ap)
    bp = sub(p, b)
    d3, d4 = na_dot(ab, bp), na_dot(ac, bp)
    vc = d1 * d4 - d3 * d2
    cp = sub(p, c)
    d5, d6 = na_dot(ab, cp), na_dot(ac, cp)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    nrm = na_cross(ab, ac)
    l = _norm(nrm)
    N = tuple(x / l for x in nrm)
    shp = np.broadcast(d1, d5).shape
    pt = tuple(np.broadcast_to(x, shp) for x in sub(p, scale(N, na_dot(N, ap))))
    rg = np.zeros(shp, np.int32)
    cases = [
        ((va <= zero) & ((d4 - d3) >= zero) & ((d5 - d6) >= zero), add(b, scale(sub(c, b), (d4 - d3) / ((d4 - d3) + (d5 - d6)))), 2),
        ((vb <= zero) & (d2 >= zero) & (d6 <= zero), add(a, scale(ac, d2 / (d2 - d6))), 3),
        ((d6 >= zero) & (d5 <= d6), c, 6),
        ((vc <= zero) & (d1 >= zero) & (d3 <= zero), add(a, scale(ab, d1 / (d1 - d3))), 1),
        ((d3 >= zero) & (d4 <= d3), b, 5),
        ((d1 <= zero) & (d2 <= zero), a, 4),
    ]
    for cond, q, region in cases:   # (the reference's tests in reverse: the earliest one that holds is applied last)
        pt = _sel(cond, q, pt)
        rg = _w(cond, region, rg)
    return pt, rg


def tri_ray(a, b, c, ol, dl, dt):
    """sp_tri_ray: (ok, t, local normal)."""
    zero = dt(0)
    N = unit_normal(a, b, c)
    den = na_dot(N, dl)
    ok = den != zero
    t = na_dot(N, sub(a, ol)) / den
    ok = ok & (t >= zero)
    dd = na_dot(dl, dl)
    ng = np.zeros(np.shape(den), bool)
    ps = np.zeros(np.shape(den), bool)
    for vk, vn in ((a, b), (b, c), (c, a)):
        m = scale(add(vk, vn), dt(0.5))
        o = add(ol, scale(dl, na_dot(dl, sub(m, ol)) / dd))
        s = na_dot(dl, na_cross(sub(vk, o), sub(vn, o)))
        ng = ng | ~(s >= zero)
        ps = ps | ~(s <= zero)
    ok = ok & ~(ng & ps)
    nl = _sel(den > zero, neg(N), N)
    return ok, t, nl


def tri_point(a, b, c, pl, dt):
    q, _ = closest_point(a, b, c, pl, dt)
    return (q[0] == pl[0]) & (q[1] == pl[1]) & (q[2] == pl[2])


def seg_closest(a, b, c, A, u, dt):
    """tri_seg_closest: (d2, p_seg, p_tri, region) -- the first smallest of the two ends and the three edges."""
    B = add(A, u)
    shp = np.broadcast(A[0], u[0], a[0]).shape
    best = np.full(shp, np.inf, dt)
    bc = lambda t: tuple(np.broadcast_to(x, shp) for x in t)
    ps, pt = bc(A), bc(a)
    rg = np.full(shp, 4, np.int32)

    def attempt(p_s, p_t, region):
        nonlocal best, ps, pt, rg
        d = sub(p_s, p_t)
        d2 = na_dot(d, d)
        upd = d2 < best
        best = _w(upd, d2, best); ps = _sel(upd, p_s, ps); pt = _sel(upd, p_t, pt); rg = _w(upd, region, rg)

    q0, r0 = closest_point(a, b, c, A, dt)
    attempt(A, q0, r0)
    q1, r1 = closest_point(a, b, c, B, dt)
    attempt(B, q1, r1)
    for k, (vk, vn) in enumerate(((a, b), (b, c), (c, a))):
        ek = sub(vn, vk)
        s, t = K.seg_seg(A, u, vk, ek, dt)
        attempt(add(A, scale(u, s)), add(vk, scale(ek, t)), _w(t == dt(0), 4 + k, _w(t == dt(1), 4 + (k + 1) % 3, 1 + k)))
    return best, ps, pt, rg


def seg_tri_d2(a, b, c, A, u, dt):
    """sp_seg_tri_d2: (d2, p_seg, p_tri)."""
    zero = dt(0)
    B = add(A, u)
    N = unit_normal(a, b, c)
    da, db = na_dot(N, sub(A, a)), na_dot(N, sub(B, a))
    X = add(A, scale(u, da / (da - db)))
    q, rg = closest_point(a, b, c, X, dt)
    cross = (((da > zero) & (db < zero)) | ((da < zero) & (db > zero))) & (rg == 0)
    d2, ps, pt, _ = seg_closest(a, b, c, A, u, dt)
    return _w(cross, zero, d2), _sel(cross, X, ps), _sel(cross, q, pt)


def box_axis(he, v0, v1, v2, L):
    """tri_box_axis's separation."""
    p0, p1, p2 = na_dot(L, v0), na_dot(L, v1), na_dot(L, v2)
    lt = p0 < p1
    tmin, tmax = _w(lt, p0, p1), _w(lt, p1, p0)
    tmin = _w(p2 < tmin, p2, tmin)
    tmax = _w(p2 > tmax, p2, tmax)
    rb = (np.abs(L[0]) * he[0] + np.abs(L[1]) * he[1]) + np.abs(L[2]) * he[2]
    sp, sm = tmin - rb, -tmax - rb
    return _w(sp >= sm, sp, sm)


def tri_cuboid_intersects(a, b, c, he2, qcr, qct, dt):
    """the cuboid branch of sp_tricol_intersects: (qcr, qct) the collider in the query's frame."""
    zero = dt(0)
    eps = dt(np.finfo(dt).eps)
    v = [add(na_qrot(qcr, x, dt), qct) for x in (a, b, c)]
    shp = np.broadcast(v[0][0], he2[0]).shape
    z, o = np.zeros(shp, dt), np.ones(shp, dt)
    sep = np.zeros(shp, bool)
    for L in ((o, z, z), (z, o, z), (z, z, o)):
        sep = sep | (box_axis(he2, v[0], v[1], v[2], L) > zero)
    sep = sep | (box_axis(he2, v[0], v[1], v[2], unit_normal(v[0], v[1], v[2])) > zero)
    for k in range(3):
        ek = sub(v[(k + 1) % 3], v[k])
        el = _norm(ek)
        for i in range(3):
            cx = (z, -ek[2], ek[1]) if i == 0 else ((ek[2], z, -ek[0]) if i == 1 else (-ek[1], ek[0], z))
            nl = _norm(cx)
            live = nl > eps * el
            sep = sep | (live & (box_axis(he2, v[0], v[1], v[2], tuple(x / nl for x in cx)) > zero))
    return ~sep


def tri_sat_cast(a, b, c, he2, qr, qt, dl, dt):
    """sp_tri_sat_cast: (ok, t, kin, n xyz, pen)."""
    zero, one, inf = dt(0), dt(1), dt(np.inf)
    eps = dt(np.finfo(dt).eps)
    shp = np.broadcast(a[0], he2[0], qr[0], qt[0], dl[0]).shape
    e = CA._units(shp, dt)
    u = [na_qrot(qr, x, dt) for x in e]
    N = unit_normal(a, b, c)
    edges = (sub(b, a), sub(c, b), sub(a, c))
    tin = np.full(shp, -inf, dt); tout = np.full(shp, inf, dt)
    kin = np.full(shp, -1, np.int32)
    nin = tuple(np.zeros(shp, dt) for _ in range(3))
    miss = np.zeros(shp, bool)
    for k in range(13):
        live = np.ones(shp, bool)
        if k == 0:
            ax = N
        elif k < 4:
            ax = u[k - 1]
        else:
            ib, ie = (k - 4) // 3, (k - 4) % 3
            axis = na_cross(edges[ie], u[ib])
            norm1 = _norm(axis)
            live = norm1 > eps
            ax = tuple(x / norm1 for x in axis)
        p0, p1, p2 = na_dot(ax, a), na_dot(ax, b), na_dot(ax, c)
        lt = p0 < p1
        lo, hi = _w(lt, p0, p1), _w(lt, p1, p0)
        lo = _w(p2 < lo, p2, lo)
        hi = _w(p2 > hi, p2, hi)
        s0, v = na_dot(ax, qt), na_dot(ax, dl)
        r2 = np.abs(na_dot(ax, u[0])) * he2[0] + np.abs(na_dot(ax, u[1])) * he2[1] + np.abs(na_dot(ax, u[2])) * he2[2]
        nz = v != zero
        inv = one / v
        t1, t2 = ((lo - r2) - s0) * inv, ((hi + r2) - s0) * inv
        ng = inv < zero
        t1, t2 = _w(ng, t2, t1), _w(ng, t1, t2)
        sg = _w(ng, one, -one)
        un = live & nz & (t1 > tin)
        uf = live & nz & (t2 < tout)
        tin = _w(un, t1, tin); kin = _w(un, k, kin)
        nin = tuple(_w(un, ax[j] * sg, nin[j]) for j in range(3))
        tout = _w(uf, t2, tout)
        miss = miss | (live & ~nz & ((s0 + r2 < lo) | (s0 - r2 > hi)))
    ok = ~miss & (tin <= tout) & ~(tout < zero)
    pen = tin < zero
    return ok, _w(pen, zero, tin), kin, nin, pen


def tri_sat_witness(a, b, c, he2, qr, tp, kin, n, dt):
    """sp_tri_sat_witness: (p1, p2) in the collider's frame."""
    zero, one = dt(0), dt(1)
    eps = dt(np.finfo(dt).eps)
    shp = np.broadcast(a[0], he2[0], qr[0], tp[0], kin, n[0]).shape
    bcs = lambda t: tuple(np.broadcast_to(x, shp) for x in t)
    qri = qinverse(qr)
    s2 = add(na_qrot(qr, support(he2, na_qrot(qri, neg(n), dt)), dt), tp)
    box_point = lambda p: add(na_qrot(qr, CA._clamp3(na_qrot(qri, sub(p, tp), dt), he2), dt), tp)
    # the triangle's face
    N = unit_normal(a, b, c)
    f2 = s2
    f1 = sub(s2, scale(N, na_dot(N, sub(s2, a))))
    _, frg = closest_point(a, b, c, f1, dt)
    f_in = frg == 0
    # a face of the query
    da, db, dc = na_dot(n, a), na_dot(n, b), na_dot(n, c)
    s1, dm = bcs(a), da + np.zeros(shp, dt)
    up = db > dm
    dm = _w(up, db, dm); s1 = _sel(up, bcs(b), s1)
    up = dc > dm
    s1 = _sel(up, bcs(c), s1)
    h = _w(kin == 1, he2[0], _w(kin == 2, he2[1], he2[2]))
    g1 = s1
    g2 = sub(s1, scale(n, na_dot(sub(s1, tp), n) + h))
    x = na_qrot(qri, sub(s1, tp), dt)
    g_in = np.logical_and.reduce([(kin == 1 + j) | (np.abs(x[j]) <= he2[j]) for j in range(3)])
    # an edge pair
    ke = _w(kin >= 4, kin - 4, 0)
    ib, ie = ke // 3, ke % 3
    vk = _sel(ie == 0, bcs(a), _sel(ie == 1, bcs(b), bcs(c)))
    vn = _sel(ie == 0, bcs(b), _sel(ie == 1, bcs(c), bcs(a)))
    ek = sub(vn, vk)
    eb = tuple(_w(ib == j, one, zero) + np.zeros(shp, dt) for j in range(3))
    ub = na_qrot(qr, eb, dt)
    w = sub(vk, s2)
    aa, bc, cc, dd, ee = na_dot(ek, ek), na_dot(ek, ub), na_dot(ub, ub), na_dot(ek, w), na_dot(ub, w)
    den = aa * cc - bc * bc
    cross = den > eps * (aa * cc)
    lam, mu = (bc * ee - cc * dd) / den, (aa * ee - bc * dd) / den
    h1 = _sel(cross, add(vk, scale(ek, lam)), add(vk, scale(ek, dt(0.5))))
    h2 = add(s2, scale(ub, mu))
    xe = na_qrot(qri, sub(h2, tp), dt)
    heb = _w(ib == 0, he2[0], _w(ib == 1, he2[1], he2[2]))
    xeb = _w(ib == 0, xe[0], _w(ib == 1, xe[1], xe[2]))
    h_in = cross & (lam >= zero) & (lam <= one) & (np.abs(xeb) <= heb)
    face1, face2 = kin == 0, kin < 4
    p1 = _sel(face1, f1, _sel(face2, g1, h1))
    p2 = _sel(face1, f2, _sel(face2, g2, h2))
    inside = _w(face1, f_in, _w(face2, g_in, h_in))
    # the common way out: onto the triangle, onto the box, once more onto the triangle, and the box's closest point to that
    c1, _ = closest_point(a, b, c, p1, dt)
    c1, _ = closest_point(a, b, c, box_point(c1), dt)
    return _sel(inside, p1, c1), _sel(inside, p2, box_point(c1))


# ---- the pair tests of a query shape against a triangle collider (broadcasting over (query, collider)) -------------------------------------------------
def _bc(shp):
    return lambda t: tuple(np.broadcast_to(x, shp) for x in t)


def tricol_intersects(kind, he2, r2, pos2, tri, pos1, rot1, dt):
    """sp_tricol_intersects: kind = the query's shape (0 / 1 / 3), r2 make_isometry's rotation of the query; tri = (a, b, c)."""
    a, b, c = tri
    with np.errstate(all="ignore"):
        _, qr, qt = C._relative(r2, pos2, pos1, rot1, dt)
        A, u = C.capsule_core(qr, qt, he2[1], dt)
        rr = he2[0] * he2[0]
        cap_hit = seg_tri_d2(a, b, c, A, u, dt)[0] <= rr
        q, _ = closest_point(a, b, c, qt, dt)
        d = sub(qt, q)
        ball_hit = na_dot(d, d) <= rr
        r2i = qinverse(r2)
        cub_hit = tri_cuboid_intersects(a, b, c, he2, na_qmul(r2i, rot1), na_qrot(r2i, sub(pos1, pos2), dt), dt)
    kind = np.asarray(kind)
    return _w(kind == SHAPE_CAPSULE, cap_hit, _w(kind == R.SHAPE_BALL, ball_hit, cub_hit))


def tricol_cast_exact(kind, he2, r2, pos2, d, max_distance, tri, pos1, rot1, dt):
    """sp_tricol_cast_exact for the three query kinds: (hit, toi, point1, point2, normal1, Newton rounds; 0 for a cuboid query)."""
    zero = dt(0)
    a, b, c = tri
    with np.errstate(all="ignore"):
        shp = np.broadcast(np.asarray(kind), he2[0], r2[0], pos2[0], d[0], max_distance, a[0], pos1[0], rot1[0]).shape
        bc = _bc(shp)
        he2, r2, pos2, d, pos1, rot1, a, b, c = bc(he2), bc(r2), bc(pos2), bc(d), bc(pos1), bc(rot1), bc(a), bc(b), bc(c)
        max_distance = np.broadcast_to(max_distance, shp)
        kind = np.broadcast_to(np.asarray(kind), shp)
        capsule, ball = kind == SHAPE_CAPSULE, kind == R.SHAPE_BALL
        zv = tuple(np.zeros(shp, dt) for _ in range(3))
        ri, qr, qt = C._relative(r2, pos2, pos1, rot1, dt)
        dl = na_qrot(ri, d, dt)
        r = he2[0]
        # a ball and a capsule: Newton on the distance of the centre / the core
        A, u = C.capsule_core(qr, qt, he2[1], dt)

        def closest_capsule(t):
            f, ps, pt = seg_tri_d2(a, b, c, add(A, scale(dl, t)), u, dt)
            return f, ps, pt

        def closest_ball(t):
            pa = add(qt, scale(dl, t))
            pb, _ = closest_point(a, b, c, pa, dt)
            df = sub(pa, pb)
            return na_dot(df, df), pa, pb

        outs = {}
        for name, rows, fn in (("ball", ball, closest_ball), ("capsule", capsule, closest_capsule)):
            if rows.any():
                outs[name] = K.newton_cast(fn, dl, r, max_distance, shp, dt)
            else:
                outs[name] = (np.zeros(shp, bool), np.zeros(shp, dt), zv, zv, zv, np.zeros(shp, bool), np.zeros(shp, np.int32))
        pick = lambda i: _w(capsule, outs["capsule"][i], outs["ball"][i])
        pickv = lambda i: _sel(capsule, outs["capsule"][i], outs["ball"][i])
        n_ok, n_t, n_n, n_pq, n_pc, n_pen, rounds = pick(0), pick(1), pickv(2), pickv(3), pickv(4), pick(5), pick(6)
        n_n1 = na_qrot(rot1, n_n, dt)
        n_p1 = add(na_qrot(rot1, n_pc, dt), pos1)
        n_p2 = add(na_qrot(rot1, sub(n_pq, scale(n_n, r)), dt), pos1)
        # a cuboid: the swept SAT
        s_ok, s_t, kin, s_n, s_pen = tri_sat_cast(a, b, c, he2, qr, qt, dl, dt)
        w1, w2 = tri_sat_witness(a, b, c, he2, qr, add(qt, scale(dl, s_t)), kin, s_n, dt)
        s_n1 = na_qrot(rot1, s_n, dt)
        s_p1 = add(na_qrot(rot1, w1, dt), pos1)
        s_p2 = add(na_qrot(rot1, w2, dt), pos1)
        newton = capsule | ball
        ok = _w(newton, n_ok, s_ok)
        t = _w(newton, n_t, s_t)
        pen = _w(newton, n_pen, s_pen)
        hit = ok & (t <= max_distance) & np.isfinite(t)
        keep = hit & ~pen
        n1 = _sel(keep, _sel(newton, n_n1, s_n1), zv)
        p1 = _sel(keep, _sel(newton, n_p1, s_p1), zv)
        p2 = _sel(keep, _sel(newton, n_p2, s_p2), zv)
    return hit, _w(hit, t, zero), p1, p2, n1, _w(newton, rounds, 0)


# ---- the snapshot's triangle table ---------------------------------------------------------------------------------------------------------------------
_table = None   # (vertices [C, 3, 3] in the snapshot's dtype, edge flags [C]) of the snapshot patched() was entered with
_base = {}      # the functions this module wraps while patched() is active
_depth = 0


def with_triangles(s: R.Snapshot, vertices, edge_flags=None):
    """The snapshot with its triangle table: vertices [C, 9] (read where shape == 4), edge flags [C] (None: all edges).  Its triangle colliders carry
    their own index in half_extents.x (see the module's docstring)."""
    o = copy.copy(s)
    tri = s.shape == SHAPE_TRIANGLE
    o.tri_vertices = np.asarray(vertices, s.dt).reshape(s.n, 3, 3)
    o.tri_flags = np.full(s.n, T.ALL_EDGES, np.uint8) if edge_flags is None else np.asarray(edge_flags, np.uint8)
    o.he = (np.where(tri, np.arange(s.n), s.he[0]).astype(s.dt), np.where(tri, 0, s.he[1]).astype(s.dt), np.where(tri, 0, s.he[2]).astype(s.dt))
    return o


def without_triangles(s: R.Snapshot):
    """The snapshot as the queries see it with the switch off: its triangle colliders are host shapes."""
    o = copy.copy(s)
    o.shape = np.where(s.shape == SHAPE_TRIANGLE, R.SHAPE_HOST, s.shape).astype(np.uint32)
    return o


def _tri_rows(shape, he):
    """(which rows are triangle colliders, their (a, b, c) from the table): shaped like the broadcast of shape and he.x."""
    tri = np.asarray(shape) == SHAPE_TRIANGLE
    if _table is None or not np.any(tri):
        return tri, None
    with np.errstate(all="ignore"):
        idx = np.where(tri, he[0], 0).astype(np.int64)
    tri = np.broadcast_to(tri, idx.shape)
    V = _table[0]
    return tri, tuple(tuple(V[idx, k, j] for j in range(3)) for k in range(3))


def shape_aabb(shape, h, pos, q, dt):
    mn, mx = _base["shape_aabb"](shape, h, pos, q, dt)
    tri, t = _tri_rows(shape, h)
    if t is None:
        return mn, mx
    pts = [add(pos, qrot(q, v, dt)) for v in t]
    lo = tuple(np.minimum(np.minimum(pts[0][j], pts[1][j]), pts[2][j]) for j in range(3))
    hi = tuple(np.maximum(np.maximum(pts[0][j], pts[1][j]), pts[2][j]) for j in range(3))
    return _sel(tri, lo, mn), _sel(tri, hi, mx)


def ray_exact(shape, he, pos, rot, o, d, max_distance, solid, dt):
    hit, toi, nw = _base["ray_exact"](shape, he, pos, rot, o, d, max_distance, solid, dt)
    tri, t = _tri_rows(shape, he)
    if t is None:
        return hit, toi, nw
    zero = dt(0)
    with np.errstate(all="ignore"):
        ci = qinverse(rot)
        ol = qrot(ci, sub(o, pos), dt)
        dl = qrot(ci, d, dt)
        ok, tt, nl = tri_ray(t[0], t[1], t[2], ol, dl, dt)
        t_hit = ok & (tt <= max_distance) & np.isfinite(tt)
        tn = qrot(rot, nl, dt)
        tn = tuple(_w(t_hit, x, zero) for x in tn)
    return _w(tri, t_hit, hit), _w(tri, _w(t_hit, tt, zero), toi), _sel(tri, tn, nw)


def point_exact(shape, he, pos, rot, p, dt):
    hit = _base["point_exact"](shape, he, pos, rot, p, dt)
    tri, t = _tri_rows(shape, he)
    if t is None:
        return hit
    with np.errstate(all="ignore"):
        pl = qrot(qinverse(rot), sub(p, pos), dt)
        return _w(tri, tri_point(t[0], t[1], t[2], pl, dt), hit)


def project_exact(shape, he, pos, rot, p, solid, dt):
    ok, dist, world, inside = _base["project_exact"](shape, he, pos, rot, p, solid, dt)
    tri, t = _tri_rows(shape, he)
    if t is None:
        return ok, dist, world, inside
    with np.errstate(all="ignore"):
        pl = qrot(qinverse(rot), sub(p, pos), dt)
        proj, _ = closest_point(t[0], t[1], t[2], pl, dt)
        t_in = (proj[0] == pl[0]) & (proj[1] == pl[1]) & (proj[2] == pl[2])
        diff = sub(pl, proj)
        t_dist = np.sqrt(dot(diff, diff))
        t_world = add(qrot(rot, proj, dt), pos)
    return _w(tri, np.isfinite(t_dist), ok), _w(tri, t_dist, dist), _sel(tri, t_world, world), _w(tri, t_in, inside)


def shape_exact(shape1, he1, r1, pos1, shape2, he2, pos2, rot2, dt):
    """a ball or a cuboid query (shape 1) against the colliders (shape 2)."""
    hit = _base["shape_exact"](shape1, he1, r1, pos1, shape2, he2, pos2, rot2, dt)
    tri, t = _tri_rows(shape2, he2)
    if t is None:
        return hit
    return _w(tri, tricol_intersects(shape1, he1, r1, pos1, t, pos2, rot2, dt), hit)


def capsule_intersects(r, h, r2, pos2, shape1, he1, pos1, rot1, dt):
    """a capsule query against the colliders (shape 1)."""
    hit = _base["capsule_intersects"](r, h, r2, pos2, shape1, he1, pos1, rot1, dt)
    tri, t = _tri_rows(shape1, he1)
    if t is None:
        return hit
    z = np.zeros_like(r)
    return _w(tri, tricol_intersects(SHAPE_CAPSULE, (r, h, z), r2, pos2, t, pos1, rot1, dt), hit)


def cast_exact(shape2, he2, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt):
    hit, toi, p1, p2, n1 = _base["cast_exact"](shape2, he2, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt)
    tri, t = _tri_rows(shape1, he1)
    if t is None:
        return hit, toi, p1, p2, n1
    k_hit, k_toi, k_p1, k_p2, k_n1, rounds = tricol_cast_exact(shape2, he2, r2, pos2, d, max_distance, t, pos1, rot1, dt)
    tri = np.broadcast_to(tri, k_hit.shape)
    _note_rounds(rounds, tri)
    return _w(tri, k_hit, hit), _w(tri, k_toi, toi), _sel(tri, k_p1, p1), _sel(tri, k_p2, p2), _sel(tri, k_n1, n1)


def capsule_cast_exact(r, h, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt):
    hit, toi, p1, p2, n1, rounds = _base["capsule_cast_exact"](r, h, r2, pos2, d, max_distance, shape1, he1, pos1, rot1, dt)
    tri, t = _tri_rows(shape1, he1)
    if t is None:
        return hit, toi, p1, p2, n1, rounds
    z = np.zeros_like(r)
    k_hit, k_toi, k_p1, k_p2, k_n1, k_rounds = tricol_cast_exact(SHAPE_CAPSULE, (r, h, z), r2, pos2, d, max_distance, t, pos1, rot1, dt)
    tri = np.broadcast_to(tri, k_hit.shape)
    _note_rounds(k_rounds, tri)
    return _w(tri, k_hit, hit), _w(tri, k_toi, toi), _sel(tri, k_p1, p1), _sel(tri, k_p2, p2), _sel(tri, k_n1, n1), _w(tri, k_rounds, rounds)


# ---- contacts: the narrow phase's triangle manifolds, the deepest point ---------------------------------------------------------------------------------
def _tri_manifold(shape1, he1, pos1, rot1, he2, pos2, rot2, pred, dt):
    """T.manifold of one (query, triangle collider) pair, the query as shape 1; he2.x names the collider.  (normal, points) or None."""
    c = int(he2[0])
    return T.manifold(int(shape1), he1, pos1, rot1, SHAPE_TRIANGLE, (0, 0, 0), pos2, rot2, pred, _table[0][c], _table[1][c], dt)


class _Manifolds:
    """contact_manifolds for a batch of (query shape, collider) pairs: the rows whose collider is a triangle come from triangle_collider_reference,
    the others from the manifolds in force before (spatial_capsule_collider_reference's)."""

    def __init__(self, bits):
        self.bits = bits

    def contact_manifolds(self, shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction):
        dt = np.float32 if self.bits == 32 else np.float64
        shape1, shape2 = np.asarray(shape1), np.asarray(shape2)
        k = len(shape1)
        A = lambda a, n: np.asarray(a, dt).reshape(k, n)
        he1, pos1, rot1, he2, pos2, rot2 = A(he1, 3), A(pos1, 3), A(rot1, 4), A(he2, 3), A(pos2, 3), A(rot2, 4)
        prediction = np.broadcast_to(np.asarray(prediction, dt), (k,))
        tri = shape2 == SHAPE_TRIANGLE
        m = {"point_count": np.zeros(k, np.uint32), "penetration": np.zeros((k, 16), dt), "normal": np.zeros((k, 3), dt),
             "point": np.zeros((k, 16, 3), dt), "anchor1": np.zeros((k, 16, 3), dt), "anchor2": np.zeros((k, 16, 3), dt)}
        i = np.nonzero(~tri)[0]
        if len(i):
            o = _base["oracle_world"](self.bits).contact_manifolds(shape1[i], he1[i], pos1[i], rot1[i], shape2[i], he2[i], pos2[i], rot2[i], prediction[i])
            for key in m:
                m[key][i] = o[key]
        for j in np.nonzero(tri)[0]:
            r = _tri_manifold(shape1[j], he1[j], pos1[j], rot1[j], he2[j], pos2[j], rot2[j], prediction[j], dt)
            if r is None:
                continue
            normal, pts = r
            p1 = tuple(dt(x) for x in pos1[j]); d12 = sub(p1, tuple(dt(x) for x in pos2[j]))
            m["point_count"][j] = len(pts)
            m["normal"][j] = normal
            for q, (a1, pen, _, _) in enumerate(pts):
                m["anchor1"][j, q] = a1; m["anchor2"][j, q] = add(a1, d12); m["point"][j, q] = add(p1, a1); m["penetration"][j, q] = pen
        return m


def contact_lists(s: R.Snapshot, shape, half_extents, position, rotation, prediction, mask=None, excluded=(), sensor=None, skip_sensors=False):
    """CR.contact_lists with triangle colliders: the other colliders' records from the contact lists in force before (the triangles out of their sight),
    the triangles' from _Manifolds; per query in ascending collider index."""
    from avian_amd.spatial_query import shape_contact_dtype
    dt = s.dt
    bits = CR._bits(dt)
    rd = shape_contact_dtype(bits)
    out = _base["contact_lists"](without_triangles(s), shape, half_extents, position, rotation, prediction, mask, excluded, sensor, skip_sensors)
    tcol = s.shape == SHAPE_TRIANGLE
    if not tcol.any():
        return out
    ok, he, pos, rot = S.shape_valid(shape, half_extents, position, rotation, dt)
    shape = np.asarray(shape)
    n = len(shape)
    pred = np.broadcast_to(np.asarray(prediction, dt), (n,)).copy()
    with np.errstate(all="ignore"):
        ok = ok & np.isfinite(pred) & (pred >= 0)
    cand = R._masks(s, n, mask, excluded, ok) & tcol[None, :]
    if skip_sensors and sensor is not None:
        cand = cand & ~(np.asarray(sensor) != 0)[None, :]
    with np.errstate(all="ignore"):
        cand = cand & CR.precondition(s, np.where(ok, shape, 0), np.where(ok[:, None], he, 0), np.where(ok[:, None], pos, 0),
                                      np.where(ok[:, None], rot, [0, 0, 0, 1]), np.where(ok, pred, 0))
    qi, ci = np.nonzero(cand)
    if not len(qi):
        return out
    cpos, crot, che = np.stack(s.pos, 1), np.stack(s.rot, 1), np.stack(s.he, 1)
    m = _Manifolds(bits).contact_manifolds(shape[qi], he[qi], pos[qi], rot[qi], s.shape[ci], che[ci], cpos[ci], crot[ci], pred[qi])
    rows = {}
    for j in range(len(qi)):
        cnt = int(m["point_count"][j])
        if cnt == 0:
            continue
        k = CR.deepest(m["penetration"][j], cnt)
        rec = np.zeros((), rd)
        rec["collider"] = ci[j]; rec["entity"] = s.entity[ci[j]]; rec["penetration"] = m["penetration"][j, k]
        rec["normal"] = -m["normal"][j]; rec["point"] = m["point"][j, k]; rec["anchor1"] = m["anchor1"][j, k]; rec["anchor2"] = m["anchor2"][j, k]
        rows.setdefault(int(qi[j]), []).append(rec)
    for q, l in rows.items():
        both = list(out[q]) + l
        both.sort(key=lambda r: int(r["collider"]))
        out[q] = np.array(both, rd)
    return out


@contextlib.contextmanager
def patched(s=None):
    """Lends this module's pair functions (on top of spatial_capsule_collider_reference's) to the existing references for one call; `s`: the snapshot
    (made by with_triangles) whose table the triangle rows are looked up in."""
    global _table, _depth
    with K.patched():
        if _depth:
            _depth += 1
            try:
                yield
            finally:
                _depth -= 1
            return
        saved = (R.shape_aabb, R.ray_exact, R.point_exact, S.project_exact, S.shape_exact, CA.cast_exact, C.capsule_intersects, C.capsule_cast_exact,
                 CR.contact_lists, CR.oracle_world)
        _base.update(shape_aabb=saved[0], ray_exact=saved[1], point_exact=saved[2], project_exact=saved[3], shape_exact=saved[4], cast_exact=saved[5],
                     capsule_intersects=saved[6], capsule_cast_exact=saved[7], contact_lists=saved[8], oracle_world=saved[9])
        _table = None if s is None or not hasattr(s, "tri_vertices") else (s.tri_vertices, s.tri_flags)
        (R.shape_aabb, R.ray_exact, R.point_exact, S.project_exact, S.shape_exact, CA.cast_exact, C.capsule_intersects, C.capsule_cast_exact,
         CR.contact_lists, CR.oracle_world) = (shape_aabb, ray_exact, point_exact, project_exact, shape_exact, cast_exact, capsule_intersects,
                                               capsule_cast_exact, contact_lists, _Manifolds)
        _depth = 1
        try:
            yield
        finally:
            _depth = 0
            _table = None
            (R.shape_aabb, R.ray_exact, R.point_exact, S.project_exact, S.shape_exact, CA.cast_exact, C.capsule_intersects, C.capsule_cast_exact,
             CR.contact_lists, CR.oracle_world) = saved


def _lend(fn):
    def call(s, *a, **kw):
        with patched(s), np.errstate(all="ignore"):
            return fn(s, *a, **kw)
    call.__doc__ = fn.__doc__
    return call


# ---- brute force: every entry point, for a snapshot whose triangle colliders are candidates ----------------------------------------------------------------
ray_queries = _lend(R.ray_queries)
cast_rays = _lend(R.cast_rays)
ray_hits = _lend(R.ray_hits)
point_intersections = _lend(R.point_intersections)
aabb_intersections = _lend(R.aabb_intersections)
project_points = _lend(S.project_points)
shape_intersections = _lend(C.shape_intersections)
cast_queries = _lend(CA.cast_queries)
shape_contacts = _lend(lambda s, shape, he, pos, rot, prediction, cap, **kw: CR.pad(CR.contact_lists(s, shape, he, pos, rot, prediction, **kw), cap, CR._bits(s.dt)))
contact_lists_of = _lend(lambda s, *a, **kw: CR.contact_lists(s, *a, **kw))
cast_moves = _lend(M.cast_moves)
move_and_slide = _lend(M.move_and_slide)
ray_casters = _lend(CS.ray_casters)
shape_casters = _lend(CS.shape_casters)
leaf_boxes = _lend(R.leaf_boxes)
