"""The spatial queries against Capsule COLLIDERS (include/avian_mi355x_spatial.h, "queries against capsule colliders") on the CPU:
tests/spatial_capsule_collider_reference.py, which restates the device's operations in order, is held to yardsticks it was not derived from.

1. Exact rational geometry (the bracketing of tests/test_spatial_capsule_cpu.py): the shapes grown and shrunk by the project's own
   band = 32 eps (|pos_q| + size_q + |pos_c| + size_c + distance) -- rays, point projection, intersections and cast distances of all three query kinds.
2. Role symmetry: a ball / cuboid query against a capsule collider agrees with the capsule query along -d against a ball / cuboid collider,
   which the tree already verifies.
3. h_c = 0: a capsule collider answers what a Ball collider of the same radius answers, up to rounding.
4. Contacts: the deepest point of capsule_collider_reference's manifold of the pair.
5. Casts never over-estimate (part of 1: the shrunk shapes do not touch before the reported distance).
6. The Newton rounds observed stay below the cap of 32."""
from fractions import Fraction as Q

import numpy as np
import pytest

from avian_amd.spatial_query import MISS, SHAPE_CAPSULE
from compound_helpers import compound_scene
from helpers import random_unit_quats
import capsule_collider_reference as K
import spatial_capsule_collider_reference as CC
import spatial_capsule_reference as C
import spatial_cast_reference as CA
import spatial_contact_reference as CR
import spatial_exact_geometry as X
import spatial_query_reference as R
import spatial_shape_reference as S
from test_spatial_capsule_cpu import Capsule, aimed_casts, band_of, collider, exact_seg_box_d2, exact_seg_point_d2, rcc, snapshot, within

DTYPES = [np.float32, np.float64]
I = [0.0, 0.0, 0.0, 1.0]
BALL, CUBOID = R.SHAPE_BALL, R.SHAPE_CUBOID
ROUNDS_OBSERVED = {np.float32: 12, np.float64: 15}     # the most Newton rounds of the 20 000 capsule-capsule casts below; the cap is 32


# ---- exact geometry --------------------------------------------------------------------------------------------------------------------------
def exact_seg_seg_d2(a1, u1, a2, u2):
    """min over (s, t) in [0, 1]^2 of |a1 + s u1 - a2 - t u2|^2 in Fractions: the interior critical point when it exists, else an edge of the square."""
    best = min(exact_seg_point_d2(a2, u2, a1), exact_seg_point_d2(a2, u2, X.add(a1, u1)), exact_seg_point_d2(a1, u1, a2), exact_seg_point_d2(a1, u1, X.add(a2, u2)))
    a, e, b = X.dot(u1, u1), X.dot(u2, u2), X.dot(u1, u2)
    den = a * e - b * b
    if den > 0:
        w = X.sub(a1, a2)
        c, f = X.dot(u1, w), X.dot(u2, w)
        s, t = (b * f - c * e) / den, (a * f - b * c) / den
        if 0 <= s <= 1 and 0 <= t <= 1:
            dv = X.sub(X.add(a1, X.scale(u1, s)), X.add(a2, X.scale(u2, t)))
            best = min(best, X.dot(dv, dv))
    return best


class Point:
    size = 0.0

    def __init__(self, p, dt):
        self.pos = X.vec([float(dt(x)) for x in p])


def core_d2(capc: Capsule, kind, q, shift=(0, 0, 0)):
    """The squared distance of the capsule collider's core to the query's core translated by `shift`: a Point / a ball (its centre), a cuboid
    (X.Collider: the box), a Capsule (its segment)."""
    sh = X.vec(shift)
    u = X.sub(capc.b, capc.a)
    if kind == SHAPE_CAPSULE:
        return exact_seg_seg_d2(capc.a, u, X.add(q.a, sh), X.sub(q.b, q.a))
    if kind == CUBOID:
        a, b = q.local(X.sub(capc.a, sh)), q.local(X.sub(capc.b, sh))
        return exact_seg_box_d2(a, X.sub(b, a), q.he)
    return exact_seg_point_d2(capc.a, u, X.add(q.pos, sh))


def query_of(kind, he, pos, rot, dt):
    """(exact query object, the radius its core is grown by)."""
    if kind == SHAPE_CAPSULE:
        c = Capsule(pos, rot, he[0], he[1], dt)
        return c, c.r
    if kind == BALL:
        c = collider(BALL, he, pos, rot, dt)
        return c, c.he[0]
    return collider(CUBOID, he, pos, rot, dt), Q(0)


def capsule_items(rng, n, spread=2.0, h_lo=0.0):
    return [(SHAPE_CAPSULE, [float(rng.uniform(0.05, 0.6)), float(rng.uniform(h_lo, 1.5)), 0.0], list(rng.uniform(-spread, spread, 3)),
             I if k % 4 == 0 else list(random_unit_quats(rng, 1)[0])) for k in range(n)]


def fvec(v):
    return X.vec([float(x) for x in v])


# ---- 1. rays ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_rays_bracketed_by_exact_geometry(dt):
    """Aimed rays, rays along the axis through the end caps and origins inside (solid and not): a hit point lies on the exact surface within band,
    nothing of the ray before it is inside the capsule shrunk by band, an exit leaves along the outward normal, a miss is an exact miss."""
    rng = np.random.default_rng(101)
    items = capsule_items(rng, 10)
    s = snapshot(items, dt)
    n = 400
    tgt = rng.integers(0, len(items), n)
    cen = np.array([it[2] for it in items])
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = cen[tgt] + rng.normal(size=(n, 3)) * 0.3 - d * rng.uniform(2, 5, n)[:, None]
    for k in range(0, 100):                                        # origins inside: on or near the core
        c = Capsule(*[items[tgt[k]][j] for j in (2, 3)], *items[tgt[k]][1][:2], dt)
        o[k] = np.array([float(x) for x in c.a]) + (np.array([float(x) for x in c.b]) - np.array([float(x) for x in c.a])) * rng.random() + rng.normal(size=3) * 0.02
    for k in range(100, 140):                                      # along the axis, through the end caps
        c = Capsule(*[items[tgt[k]][j] for j in (2, 3)], *items[tgt[k]][1][:2], dt)
        ax = np.array([float(x) for x in X.sub(c.b, c.a)])
        ax = ax / np.linalg.norm(ax) if np.linalg.norm(ax) > 0 else np.array([0, 1.0, 0])
        d[k] = ax; o[k] = cen[tgt[k]] - ax * 4.0
    o, d = o.astype(dt).astype(float), d.astype(dt).astype(float)
    solid = (np.arange(n) % 2).astype(np.uint8)
    col = lambda t: tuple(x[None, :] for x in t)
    with np.errstate(all="ignore"):
        hit, toi, nrm = CC.ray_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), tuple(o[:, i].astype(dt)[:, None] for i in range(3)),
                                     tuple(d[:, i].astype(dt)[:, None] for i in range(3)), dt(np.inf), (solid != 0)[:, None], dt)
    seen = dict(entry=0, exit=0, solid=0, miss=0, caps=0)
    for i in range(n):
        c = tgt[i]
        it = items[c]
        cap = Capsule(it[2], it[3], it[1][0], it[1][1], dt)
        u = X.sub(cap.b, cap.a)
        oq, dq = fvec(o[i]), fvec(d[i])
        at = lambda t: X.add(oq, X.scale(dq, t))
        band = band_of(dt, Point(o[i], dt), cap, float(toi[i, c]))
        inside0 = within(exact_seg_point_d2(cap.a, u, oq), cap.r - band)
        if not hit[i, c]:
            assert all(not within(exact_seg_point_d2(cap.a, u, at(Q(k, 16))), cap.r - 2 * band) for k in range(0, 160)), i
            seen["miss"] += 1
            continue
        t = X.q(float(toi[i, c]))
        nv = np.array([float(nrm[j][i, c]) for j in range(3)])
        if inside0 and solid[i]:
            assert t == 0 and not nv.any(), i
            seen["solid"] += 1
            continue
        if t == 0:
            assert within(exact_seg_point_d2(cap.a, u, oq), cap.r + band), i
            continue
        if abs(nv @ d[i]) < 0.05:
            continue                                                # grazing: the root is ill-conditioned
        p = at(t)
        d2 = exact_seg_point_d2(cap.a, u, p)
        assert within(d2, cap.r + 4 * band) and not within(d2, cap.r - 4 * band), (i, float(t))
        assert abs(np.linalg.norm(nv) - 1) < 64 * np.finfo(dt).eps
        if inside0:
            assert nv @ d[i] > 0, i                                 # the exit: along the outward normal
            assert within(exact_seg_point_d2(cap.a, u, at(t / 2)), cap.r + band)
            seen["exit"] += 1
        else:
            assert nv @ d[i] < 0, i
            assert not within(exact_seg_point_d2(cap.a, u, at(t - 16 * band)), cap.r - 4 * band), i   # never an over-estimate
            seen["entry"] += 1
            seen["caps"] += 100 <= i < 140
    assert seen["entry"] >= 100 and seen["exit"] >= 30 and seen["solid"] >= 30 and seen["miss"] >= 20 and seen["caps"] >= 30, seen


# ---- 1. projection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_point_projection_bracketed_by_exact_geometry(dt):
    rng = np.random.default_rng(103)
    items = capsule_items(rng, 8)
    s = snapshot(items, dt)
    n = 240
    tgt = rng.integers(0, len(items), n)
    pts = (np.array([items[c][2] for c in tgt]) + rng.normal(size=(n, 3)) * np.choose(np.arange(n) % 3, [0.1, 0.5, 1.5])[:, None]).astype(dt).astype(float)
    solid = (np.arange(n) % 2) != 0
    col = lambda t: tuple(x[None, :] for x in t)
    with np.errstate(all="ignore"):
        ok, dist, world, inside = CC.project_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), tuple(pts[:, i].astype(dt)[:, None] for i in range(3)), solid[:, None], dt)
    seen = dict(inside=0, outside=0, kept=0)
    for i in range(n):
        c = tgt[i]
        it = items[c]
        cap = Capsule(it[2], it[3], it[1][0], it[1][1], dt)
        u = X.sub(cap.b, cap.a)
        p = fvec(pts[i])
        band = band_of(dt, Point(pts[i], dt), cap, float(dist[i, c]))
        core = X.sqrt_q(exact_seg_point_d2(cap.a, u, p))
        assert ok[i, c]
        if abs(core - cap.r) > band:
            assert bool(inside[i, c]) == (core < cap.r), i
        w = fvec([world[j][i, c] for j in range(3)])
        if inside[i, c] and solid[i]:
            assert dist[i, c] == 0 and all(float(world[j][i, c]) == float(dt(pts[i, j])) for j in range(3))
            seen["kept"] += 1
            continue
        # the projection lies on the surface, at the reported distance from the point, which is | |p - core| - r |
        assert abs(X.sqrt_q(exact_seg_point_d2(cap.a, u, w)) - cap.r) <= 4 * band, i
        assert abs(X.norm(X.sub(w, p)) - X.q(float(dist[i, c]))) <= 4 * band, i
        if core > band:
            assert abs(abs(core - cap.r) - X.q(float(dist[i, c]))) <= 4 * band, i
        seen["inside" if inside[i, c] else "outside"] += 1
    assert seen["inside"] >= 20 and seen["outside"] >= 60 and seen["kept"] >= 20, seen


# ---- 1 and 5. intersections and casts of the three query kinds ----------------------------------------------------------------------------------------
def query_set(rng, items, n, dt):
    he, pos, rot, d, target = aimed_casts(rng, items, n)
    kind = np.array([BALL, CUBOID, SHAPE_CAPSULE], np.uint8)[np.arange(n) % 3]
    he[:, 2] = np.where(kind == CUBOID, rng.uniform(0.05, 0.6, n), he[:, 2])
    he[kind == CUBOID, 1] += 0.05
    return kind, he, pos.astype(dt).astype(float), rot, d.astype(dt).astype(float), target


def qmul_np(l, r):
    lx, ly, lz, lw = l
    rx, ry, rz, rw = r
    return [lw * rx + lx * rw + ly * rz - lz * ry, lw * ry - lx * rz + ly * rw + lz * rx, lw * rz + lx * ry - ly * rx + lz * rw, lw * rw - lx * rx - ly * ry - lz * rz]


TILTS = (0.0, 1e-7, 1e-4, 2e-4, 1e-3, 2e-3, 2.8e-3, 4e-3)


def near_parallel_pairs(rng, n):
    """Capsule queries whose axis is the collider's tilted by 0 (exactly parallel) to 4 mrad, about an axis perpendicular to it: beside the collider
    with the axes CONVERGING (the closest points are ends), and through it with the axes CROSSING inside both cores.  The single-precision parallel
    rule of sp_seg_seg (sin^2 <= 64 eps) holds up to about 2.8 mrad, the double-precision one up to 1.2e-7.
    Returns (collider item, he, rot, sideways unit vector, tilt) per pair; the caller places the query."""
    out = []
    for k in range(n):
        rc, hc = float(rng.uniform(0.2, 0.5)), float(rng.uniform(0.8, 1.6))
        rot_c = I if k % 3 == 0 else list(random_unit_quats(rng, 1)[0])
        item = (SHAPE_CAPSULE, [rc, hc, 0.0], list(rng.uniform(-1, 1, 3)), rot_c)
        th = TILTS[k % len(TILTS)] * (1 if k % 2 else -1)
        ang = rng.uniform(0, 2 * np.pi)
        side = np.array([np.cos(ang), 0.0, np.sin(ang)])                 # a direction perpendicular to the collider's axis, in its frame
        ax = np.cross([0, 1.0, 0], side) if k % 4 < 2 else side        # tilt towards / away from the collider (converging), or about the line between them
        tilt = list(ax * np.sin(th / 2)) + [np.cos(th / 2)]
        rot_q = qmul_np(rot_c, tilt)
        cap = Capsule(item[2], rot_c, rc, hc, np.float64)
        R3 = X.rotation(X.vec(rot_c))
        side_w = np.array([float(x) for x in X.mul(R3, X.vec(list(side)))])
        he = [float(rng.uniform(0.2, 0.5)), float(rng.uniform(0.8, 1.6)), 0.0]
        out.append((item, he, rot_q, side_w, th))
    return out


def check_near_parallel_intersections(dt):
    rng = np.random.default_rng(211)
    decided = {True: 0, False: 0}
    pairs = near_parallel_pairs(rng, 96)
    for k, (item, he, rot_q, side, th) in enumerate(pairs):
        cap = Capsule(item[2], item[3], item[1][0], item[1][1], dt)
        rr = item[1][0] + he[0]
        # beside the collider at a surface gap of -3 mm .. +3 mm at the nearest ends, and (every eighth) through it: the cores cross
        for gap in (-3e-3, -1e-3, -2e-4, 2e-4, 1e-3, 3e-3):
            lean = abs(np.sin(th)) * min(he[1], item[1][1])             # how far the converging end comes in
            off = 0.0 if k % 8 == 7 else rr + gap + lean
            pos = list(np.asarray(item[2]) + side * off + np.asarray([float(x) for x in X.sub(cap.b, cap.a)]) * (0.1 * (k % 5 - 2)))
            pos = [float(dt(x)) for x in pos]
            s = snapshot([item], dt)
            cnt = CC.shape_intersections(s, rcc(1), [he], [pos], [rot_q], 1)[1][0]
            q, rq = query_of(SHAPE_CAPSULE, he, pos, rot_q, dt)
            band = band_of(dt, q, cap)
            d2 = core_d2(cap, SHAPE_CAPSULE, q)
            if within(d2, rq + cap.r - 2 * band):
                assert cnt == 1, (k, th, gap, float(X.sqrt_q(d2)) - float(rq + cap.r))
                decided[True] += 1
            elif not within(d2, rq + cap.r + 2 * band):
                assert cnt == 0, (k, th, gap, float(X.sqrt_q(d2)) - float(rq + cap.r))
                decided[False] += 1
    assert decided[True] >= 150 and decided[False] >= 150, decided


def check_near_parallel_casts(dt):
    rng = np.random.default_rng(223)
    seen = 0
    for k, (item, he, rot_q, side, th) in enumerate(near_parallel_pairs(rng, 96)):
        cap = Capsule(item[2], item[3], item[1][0], item[1][1], dt)
        along = np.asarray([float(x) for x in X.sub(cap.b, cap.a)])
        pos = [float(dt(x)) for x in np.asarray(item[2]) + side * 3.0 + along * (0.1 * (k % 5 - 2))]
        d = -side + rng.normal(size=3) * 0.05
        d = (d / np.linalg.norm(d)).astype(dt).astype(float)
        s = snapshot([item], dt)
        with CC.patched(), np.errstate(all="ignore"):
            hit, toi, p1, p2, n1, ok = CA.cast_pairs(s, rcc(1), [he], [pos], [rot_q], [d])
        assert ok.all() and hit[0, 0], (k, th)
        q, rq = query_of(SHAPE_CAPSULE, he, pos, rot_q, dt)
        rr = rq + cap.r
        t = float(toi[0, 0])
        band = band_of(dt, q, cap, t)
        dq = fvec(d)
        assert t > 0
        assert within(core_d2(cap, SHAPE_CAPSULE, q, X.scale(dq, X.q(t))), rr + 2 * band), (k, th, t)       # not short of contact by more than band ...
        assert not within(core_d2(cap, SHAPE_CAPSULE, q, X.scale(dq, X.q(t) - band)), rr - 2 * band), (k, th, t)   # ... and never past it
        seen += 1
    assert seen == 96


@pytest.mark.parametrize("dt", DTYPES)
def test_intersections_bracketed_by_exact_geometry(dt):
    rng = np.random.default_rng(107)
    items = capsule_items(rng, 10)
    s = snapshot(items, dt)
    kind, he, pos, rot, d, tgt = query_set(rng, items, 300, dt)
    pos = (pos + d * rng.uniform(1.5, 5.5, 300)[:, None]).astype(dt).astype(float)      # near the colliders
    ids, cnt = CC.shape_intersections(s, kind, he, pos, rot, len(items))
    decided = {(k, v): 0 for k in (BALL, CUBOID, SHAPE_CAPSULE) for v in (True, False)}
    for i in range(300):
        q, rq = query_of(kind[i], he[i], pos[i], rot[i], dt)
        for c in (tgt[i], (tgt[i] + 1) % len(items)):
            it = items[c]
            cap = Capsule(it[2], it[3], it[1][0], it[1][1], dt)
            band = band_of(dt, q, cap)
            d2 = core_d2(cap, kind[i], q)
            got = c in ids[i, :cnt[i]]
            if within(d2, rq + cap.r - 2 * band):
                assert got, (i, c)
            elif not within(d2, rq + cap.r + 2 * band):
                assert not got, (i, c)
            else:
                continue
            decided[(kind[i], got)] += 1
    assert all(v >= 10 for v in decided.values()), decided
    check_near_parallel_intersections(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_cast_distances_bracketed_and_never_over_estimated(dt):
    """Per query kind: grown by band the exact shapes touch at the reported distance, shrunk by band they do not touch at distance - band (so the
    reported distance is at most the exact one and the gap there is within band); witnesses lie on their shapes; misses of the target are exact."""
    rng = np.random.default_rng(109)
    items = capsule_items(rng, 10)
    s = snapshot(items, dt)
    n = 360
    kind, he, pos, rot, d, tgt = query_set(rng, items, n, dt)
    CC.reset_rounds()
    with CC.patched(), np.errstate(all="ignore"):
        hit, toi, p1, p2, n1, ok = CA.cast_pairs(s, kind, he, pos, rot, d)
    assert ok.all() and 0 < CC.last_rounds < CC.ROUNDS
    seen = {k: 0 for k in (BALL, CUBOID, SHAPE_CAPSULE)}
    missed = overlap = 0
    for i in range(n):
        c = tgt[i]
        it = items[c]
        cap = Capsule(it[2], it[3], it[1][0], it[1][1], dt)
        q, rq = query_of(kind[i], he[i], pos[i], rot[i], dt)
        rr = rq + cap.r
        dq = fvec(d[i])
        if not hit[i, c]:
            band = band_of(dt, q, cap, 8.0)
            assert all(not within(core_d2(cap, kind[i], q, X.scale(dq, Q(k, 8))), rr - 2 * band) for k in range(0, 80)), i
            missed += 1
            continue
        t = float(toi[i, c])
        band = band_of(dt, q, cap, t)
        nv = np.array([float(n1[j][i, c]) for j in range(3)])
        if t == 0:
            assert not nv.any() and within(core_d2(cap, kind[i], q), rr + 2 * band), i
            overlap += 1
            continue
        assert abs(np.linalg.norm(nv) - 1) < 64 * np.finfo(dt).eps and nv @ d[i] < 0
        if -(nv @ d[i]) < 0.25:
            assert not within(core_d2(cap, kind[i], q, X.scale(dq, X.q(t) - 4096 * band)), rr - 2 * band), i
            continue
        assert within(core_d2(cap, kind[i], q, X.scale(dq, X.q(t))), rr + 2 * band), (i, kind[i], t)
        assert not within(core_d2(cap, kind[i], q, X.scale(dq, X.q(t) - band)), rr - 2 * band), (i, kind[i], t)
        # point1 on the collider's surface, point2 within the contact's width of it
        w1, w2 = fvec([p1[j][i, c] for j in range(3)]), fvec([p2[j][i, c] for j in range(3)])
        wb = 8 * band + Q(float(np.sqrt(float(2 * rr * band))))
        dc = exact_seg_point_d2(cap.a, X.sub(cap.b, cap.a), w1)
        assert within(dc, cap.r + wb) and not within(dc, cap.r - wb), i
        assert X.norm(X.sub(w1, w2)) <= 4 * wb, i
        seen[kind[i]] += 1
    assert all(v >= 30 for v in seen.values()) and missed >= 10, (seen, missed, overlap)
    check_near_parallel_casts(dt)


# ---- 2. role symmetry ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", [BALL, CUBOID])
def test_role_symmetry_with_the_capsule_query(dt, kind):
    """A ball / cuboid query cast along d against a capsule collider, and the capsule as the QUERY cast along -d against that ball / cuboid as the
    collider (spatial_capsule_reference, verified by tests/test_spatial_capsule_cpu.py): the same hit, the distance within band, the witnesses
    exchanged (in the frame of the other's start pose) and the normal negated; intersection booleans agree."""
    rng = np.random.default_rng(113 + int(kind))
    n = 150
    checked = inter = 0
    for i in range(n):
        cap_he = [float(rng.uniform(0.05, 0.6)), float(rng.uniform(0.0, 1.5)), 0.0]
        cap_pos = list(rng.uniform(-2, 2, 3)); cap_rot = I if i % 4 == 0 else list(random_unit_quats(rng, 1)[0])
        he = [float(rng.uniform(0.1, 0.7)), 0.0, 0.0] if kind == BALL else list(rng.uniform(0.1, 0.8, 3))
        rot = I if i % 5 == 0 else list(random_unit_quats(rng, 1)[0])
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        d = d.astype(dt).astype(float)
        pos = list(np.asarray(cap_pos) + rng.normal(size=3) * 0.4 - d * rng.uniform(0.0, 5.0))
        sa = snapshot([(SHAPE_CAPSULE, cap_he, cap_pos, cap_rot)], dt)
        sb = snapshot([(kind, he, pos, rot)], dt)
        with CC.patched(), np.errstate(all="ignore"):
            ha, ta, a1, a2, an, _ = CA.cast_pairs(sa, np.array([kind], np.uint8), [he], [pos], [rot], [d])
            ia = CC.shape_intersections(sa, np.array([kind], np.uint8), [he], [pos], [rot], 1)[1][0]
        with np.errstate(all="ignore"):
            hb, tb, b1, b2, bn, _ = C.cast_pairs(sb, rcc(1), [cap_he], [cap_pos], [cap_rot], [-d])
            ib = C.shape_intersections(sb, rcc(1), [cap_he], [cap_pos], [cap_rot], 1)[1][0]
        cap = Capsule(cap_pos, cap_rot, cap_he[0], cap_he[1], dt)
        q, rq = query_of(kind, he, pos, rot, dt)
        band = float(band_of(dt, q, cap, max(float(ta[0, 0]), float(tb[0, 0]))))
        gap = float(X.sqrt_q(core_d2(cap, kind, q))) - float(rq + cap.r)
        if abs(gap) > 2 * band:
            assert ia == ib == (1 if gap < 0 else 0), i
            inter += 1
        if ha[0, 0] != hb[0, 0] or not ha[0, 0]:
            assert ha[0, 0] == hb[0, 0] or abs(gap) <= 2 * band or min(float(ta[0, 0]), float(tb[0, 0])) > 0, i   # only a grazing pass may differ
            continue
        ta_, tb_ = float(ta[0, 0]), float(tb[0, 0])
        va, vb = np.array([float(an[j][0, 0]) for j in range(3)]), np.array([float(bn[j][0, 0]) for j in range(3)])
        if (ta_ == 0) != (tb_ == 0):
            assert abs(gap) <= 2 * band, i
            continue
        if ta_ == 0 or -(va @ d) < 0.25:
            continue
        assert abs(ta_ - tb_) <= 2 * band, (i, ta_, tb_)
        wb = 8 * band + float(np.sqrt(2 * float(rq + cap.r) * band))
        A1, A2 = (np.array([float(x[j][0, 0]) for j in range(3)]) for x in (a1, a2))
        B1, B2 = (np.array([float(x[j][0, 0]) for j in range(3)]) for x in (b1, b2))
        assert np.abs(va + vb).max() <= 4 * wb / max(float(rq + cap.r), wb), i                 # the normal is negated
        assert np.linalg.norm(A1 - (B2 + d * tb_)) <= 8 * wb and np.linalg.norm((A2 - d * ta_) - B1) <= 8 * wb, i   # the witnesses are exchanged
        checked += 1
    assert checked >= 40 and inter >= 100, (checked, inter)


# ---- 3. h_c = 0 is a Ball collider ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_zero_length_capsule_collider_equals_the_ball_collider(dt):
    rng = np.random.default_rng(127)
    m = 12
    caps = [(SHAPE_CAPSULE, [float(rng.uniform(0.2, 0.9)), 0.0, 0.0], list(rng.uniform(-3, 3, 3)), list(random_unit_quats(rng, 1)[0])) for _ in range(m)]
    balls = [(BALL, it[1], it[2], it[3]) for it in caps]
    sc, sb = snapshot(caps, dt), snapshot(balls, dt)
    n = 120
    eps = float(np.finfo(dt).eps)
    tol = lambda dist: X.BAND_EPS * eps * (4.0 + 1.0 + 3.0 + 0.9 + np.abs(dist))
    cen = np.array([it[2] for it in caps])
    # rays
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = cen[rng.integers(0, m, n)] + rng.normal(size=(n, 3)) * 0.25 - d * np.where(np.arange(n) % 4 == 0, 0.0, rng.uniform(1, 4, n))[:, None]
    solid = (np.arange(n) % 2).astype(np.uint8)
    a, b = CC.cast_rays(sc, o, d, None, solid), R.cast_rays(sb, o, d, None, solid)
    assert np.array_equal(a["collider"], b["collider"]) and (a["collider"] != MISS).sum() >= 60
    assert (np.abs(a["distance"] - b["distance"]) <= tol(b["distance"])).all()
    graze = np.abs((b["normal"] * d).sum(1)) < 0.25
    assert (np.abs(a["normal"] - b["normal"])[~graze] <= 1e3 * eps * 8).all()
    # points, boxes, projection
    pts = cen[rng.integers(0, m, n)] + rng.normal(size=(n, 3)) * 0.5
    pa, pb = CC.point_intersections(sc, pts, m), R.point_intersections(sb, pts, m)
    assert np.array_equal(pa[0], pb[0]) and pa[1].sum() >= 30
    lo, hi = pts - 0.3, pts + 0.3
    xa, xb = CC.aabb_intersections(sc, lo, hi, m), R.aabb_intersections(sb, lo, hi, m)
    assert np.array_equal(xa[1], xb[1]) and xa[1].sum() >= 30
    ja, jb = CC.project_points(sc, pts, solid), S.project_points(sb, pts, solid)
    assert np.array_equal(ja["collider"], jb["collider"]) and np.array_equal(ja["is_inside"], jb["is_inside"])
    assert (np.abs(ja["distance"] - jb["distance"]) <= tol(jb["distance"])).all() and (np.abs(ja["point"] - jb["point"]) <= 4 * tol(jb["distance"])[:, None]).all()
    # shape intersections, casts and contacts of the three query kinds
    kind, he, pos, rot, dd, tgt = query_set(rng, caps, n, dt)
    near = (pos + dd * rng.uniform(1.5, 5.5, n)[:, None])
    ia, ib = CC.shape_intersections(sc, kind, he, near, rot, m), C.shape_intersections(sb, kind, he, near, rot, m)
    assert np.array_equal(ia[0], ib[0]) and ia[1].sum() >= 30
    ca, cb = CC.cast_queries(sc, kind, he, pos, rot, dd)[0], C.cast_queries(sb, kind, he, pos, rot, dd)[0]
    both = (ca["collider"] != MISS) & (cb["collider"] != MISS)
    assert np.array_equal(ca["collider"], cb["collider"]) and both.sum() >= 60
    steep = both & (-(cb["normal1"] * dd).sum(1) > 0.25)
    assert (np.abs(ca["distance"] - cb["distance"])[steep] <= 2 * tol(cb["distance"])[steep]).all() and steep.sum() >= 40
    la, lb = CC.contact_lists(sc, kind, he, near, rot, 0.3), C.contact_lists(sb, kind, he, near, rot, 0.3)
    pairs = 0
    for x, y in zip(la, lb):
        keep = np.isin(x["collider"], y["collider"]); back = np.isin(y["collider"], x["collider"])
        assert (np.abs(x["penetration"][keep] - y["penetration"][back]) <= 8 * tol(0.0)).all()
        # (a list may differ only by a contact at the edge of the prediction distance or of "no direction")
        assert abs(len(x) - len(y)) <= 1
        pairs += keep.sum()
    assert pairs >= 40
    # the nearest-k lists: the same colliders in the same slots, the same counts, distances within band
    ra, rb = CC.ray_hits(sc, o, d, 4, None, solid), R.ray_hits(sb, o, d, 4, None, solid)
    assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[0]["collider"], rb[0]["collider"]) and (rb[1] > 1).sum() >= 10
    assert (np.abs(ra[0]["distance"] - rb[0]["distance"]) <= tol(rb[0]["distance"])).all()
    ha, hb = CC.cast_queries(sc, kind, he, pos, rot, dd, (4,))[1][4], C.cast_queries(sb, kind, he, pos, rot, dd, (4,))[1][4]
    assert np.array_equal(ha[1], hb[1]) and (hb[1] > 1).sum() >= 10
    same = ha[0]["collider"] == hb[0]["collider"]       # (two hits within band of each other may swap slots)
    assert same.mean() > 0.95 and (np.abs(ha[0]["distance"] - hb[0]["distance"])[same & (hb[0]["collider"] != MISS)] <= 64 * tol(hb[0]["distance"])[same & (hb[0]["collider"] != MISS)]).all()
    # cast_moves with the origin-penetration rule: the same collider, the safe distance within band / DOT_EPSILON's worth (skin / dot is the same quotient)
    mv = dd * 1.5
    near_mv = np.where((np.arange(n) % 2 == 0)[:, None], near, pos)                      # half of them start overlapping colliders
    info = {}
    ma, mb = CC.cast_moves(sc, kind, he, near_mv, rot, mv, 0.05), C.cast_moves(sb, kind, he, near_mv, rot, mv, 0.05, info=info)
    both = (ma["collider"] != MISS) & (mb["collider"] != MISS)
    # the one defined difference: a Ball collider whose centre is INSIDE a cuboid query has no contact (a hit at 0 without a normal), the capsule
    # manifold's crossing-core rule gives the h_c = 0 capsule one (which the origin-penetration rule may then ignore): those lanes are left out
    plain = info["no_contact"] == 0
    assert (kind[~plain] == CUBOID).all() and (~plain).sum() <= 5
    assert np.array_equal(ma["collider"][plain], mb["collider"][plain]) and both.sum() >= 40 and (mb["distance"][both] == 0).sum() >= 5
    steep = both & plain & (-(mb["normal1"] * dd).sum(1) > 0.25)
    assert (np.abs(ma["distance"] - mb["distance"])[steep] <= 64 * tol(mb["distance"])[steep]).all() and np.array_equal(ma["collision_distance"][plain], mb["collision_distance"][plain])
    # depenetrate: the same contact counts, the fixup within the contacts' tolerance times the iterations
    cfg = dict(skin_width=0.05, max_depenetration_error=1e-4, penetration_rejection_threshold=0.3, iterations=8)
    bits = 32 if dt == np.float32 else 64
    fa = CR.depenetrations(*CR.pad(CC.contact_lists(sc, kind, he, near, rot, 0.05), 64, bits), 0.05, 1e-4, 0.3, 8, bits)
    fb = CR.depenetrations(*CR.pad(C.contact_lists(sb, kind, he, near, rot, 0.05), 64, bits), 0.05, 1e-4, 0.3, 8, bits)
    eq = fa["count"] == fb["count"]
    assert eq.mean() > 0.95 and (np.abs(fa["fixup"] - fb["fixup"])[eq] <= 8 * 64 * tol(0.0)).all() and (np.abs(fb["fixup"]).max(1) > 0).sum() >= 20
    # NOT compared up to rounding: move_and_slide and the casters.  They are compositions of the calls above (depenetrate, cast_move, shape contacts,
    # project_velocity; a re-aim followed by cast_rays / ray_hits / cast_shapes / shape_hits) with discontinuous decisions in between -- the 1e-4 sweep
    # cut-off, the plane-similarity threshold, total_error < max_error, which contact makes a 64-slot list -- so two inputs a rounding apart may
    # legitimately take different branches; the GPU tests hold those entry points to the reference byte for byte instead.


# ---- 4. contacts ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_contacts_are_the_deepest_point_of_the_capsule_manifold(dt):
    rng = np.random.default_rng(131)
    items = capsule_items(rng, 10, h_lo=0.2)
    s = snapshot(items, dt)
    n = 150
    kind, he, pos, rot, d, tgt = query_set(rng, items, n, dt)
    pos = pos + d * rng.uniform(2.0, 5.5, n)[:, None]
    rot[::6] = np.array([items[c][3] for c in tgt[::6]])           # parallel capsules: two-point manifolds
    pred = np.where(np.arange(n) % 2, 0.3, 0.0)
    lists = CC.contact_lists(s, kind, he, pos, rot, pred)
    _, hev, posv, rotv = C.shape_valid(kind, he, pos, rot, dt)
    cpos, crot, che = np.stack(s.pos, 1), np.stack(s.rot, 1), np.stack(s.he, 1)
    seen = {k: 0 for k in (BALL, CUBOID, SHAPE_CAPSULE)}
    two = 0
    for i in range(n):
        ci = np.arange(s.n)
        m = K.manifolds(np.full(s.n, kind[i]), np.tile(hev[i], (s.n, 1)), np.tile(posv[i], (s.n, 1)), np.tile(rotv[i], (s.n, 1)), s.shape, che, cpos, crot,
                        np.full(s.n, pred[i]), dt)
        want =[c for c in ci if m["point_count"][c] > 0]
        got = list(lists[i]["collider"])
        assert set(got) <= set(want), i                              # (b), the exact-box precondition, may drop a contact at the prediction's edge
        for rec in lists[i]:
            c = rec["collider"]
            k = CR.deepest(m["penetration"][c], int(m["point_count"][c]))
            two += m["point_count"][c] == 2
            assert rec["penetration"] == m["penetration"][c, k] and (rec["normal"] == -m["normal"][c]).all()
            assert (rec["anchor1"] == m["anchor1"][c, k]).all() and (rec["anchor2"] == m["anchor2"][c, k]).all() and (rec["point"] == m["point"][c, k]).all()
            seen[kind[i]] += 1
    assert all(v >= 15 for v in seen.values()) and two >= 5, (seen, two)


# ---- 6. rounds ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_newton_rounds_of_20000_capsule_capsule_casts(dt):
    """Query centre uniform in +-6, collider centre in +-2, h in [0, 1.5], r in [0.05, 0.6], the direction aimed at the collider plus noise; a
    quarter exactly parallel axes, a quarter parallel to 1e-4, a quarter h_q = 0."""
    rng = np.random.default_rng(137)
    n = 20000
    pq, pc = rng.uniform(-6, 6, (n, 3)), rng.uniform(-2, 2, (n, 3))
    hq, hc = rng.uniform(0, 1.5, n), rng.uniform(0, 1.5, n)
    rq, rc = rng.uniform(0.05, 0.6, n), rng.uniform(0.05, 0.6, n)
    rotc, rotq = random_unit_quats(rng, n), random_unit_quats(rng, n)
    quarter = np.arange(n) % 4
    rotq[quarter == 0] = rotc[quarter == 0]
    tilt = np.c_[rng.normal(size=(n, 3)) * 1e-4, np.zeros(n)]
    near = rotc + tilt
    rotq[quarter == 1] = (near / np.linalg.norm(near, axis=1, keepdims=True))[quarter == 1]
    hq[quarter == 2] = 0.0
    d = pc - pq + rng.normal(size=(n, 3)) * 0.5
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    f = lambda a, k: tuple(np.asarray(a, dt).reshape(n, k)[:, i] for i in range(k))
    r2 = np.array([S.make_isometry_rotation(q, dt) for q in rotq.astype(dt)], dt)
    z = np.zeros(n, dt)
    hit, toi, _, _, _, rounds = CC.capcol_capsule_cast_exact(rq.astype(dt), hq.astype(dt), f(r2, 4), f(pq, 3), f(d, 3), np.full(n, np.inf, dt),
                                                             (rc.astype(dt), hc.astype(dt), z), f(pc, 3), f(rotc, 4), dt)
    print(f"{np.dtype(dt).name}: {hit.sum()} hits of {n}, at most {rounds.max()} Newton rounds")
    assert hit.sum() >= 10000 and (hit & (toi > 0)).sum() >= 8000
    assert rounds.max() == ROUNDS_OBSERVED[dt] < CC.ROUNDS, rounds.max()


# ---- padding on the compound scene with capsule children ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_padding_property_with_capsule_children(dt):
    """DESIGN.md 4.4.5 - 4.4.7 pair by pair on the compound (child-collider) scene with every third collider a capsule: a ray's / a cast's entry into
    the collider's padded leaf box is <= the computed distance, a point inside a capsule lies in its leaf box, a projection's lower bound holds,
    and the padded boxes of every intersecting or contacting pair overlap."""
    bodies, cols, tf = compound_scene(seed=3, n_bodies=40)
    cols = dict(cols)
    shape = np.array(cols["shape"]).copy()
    shape[::3] = SHAPE_CAPSULE
    cols["shape"] = shape
    s = R.Snapshot(bodies, cols, tf, dt)
    child = np.asarray(tf["is_child"]) != 0
    assert (child & (shape == SHAPE_CAPSULE)).sum() >= 10
    rng = np.random.default_rng(139)
    n = 240
    kind, he, pos, rot, d, tgt = query_set(rng, np.stack(s.pos, 1).astype(float), n, dt)
    col = lambda t: tuple(x[None, :] for x in t)
    q = lambda t: tuple(x[:, None] for x in t)
    caps = (s.shape == SHAPE_CAPSULE)[None, :]
    with CC.patched(), np.errstate(all="ignore"):
        lo, hi = R.leaf_boxes(s)
        # rays and points
        o3, d3 = tuple(pos[:, i].astype(dt)[:, None] for i in range(3)), tuple(d[:, i].astype(dt)[:, None] for i in range(3))
        hit, toi, _ = R.ray_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), o3, d3, dt(np.inf), np.zeros((n, 1), bool), dt)
        entry = R.ray_box(o3, d3, col(lo), col(hi), dt(np.inf), dt)
        assert (hit & caps).sum() >= 100 and not (hit & (entry > toi)).any()
        pts = (pos + d * 3.0).astype(dt)
        p3 = tuple(pts[:, i][:, None] for i in range(3))
        inside = R.point_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), p3, dt)
        assert (inside & caps).sum() >= 10 and not (inside & ~R.point_box(p3, col(lo), col(hi), dt)).any()
        ok, dist, _, _ = S.project_exact(s.shape[None, :], col(s.he), col(s.pos), col(s.rot), p3, np.zeros((n, 1), bool), dt)
        assert not (ok & (S.point_box_distance(p3, col(lo), col(hi), dt) > dist)).any()
        # casts
        chit, ctoi, _, _, _, okc = CA.cast_pairs(s, kind, he, pos, rot, d)
        _, hev, posv, rotv, dv, mdv = CA.cast_valid(kind, he, pos, rot, d, np.full(n, np.inf), dt)
        centre_q, hw = CA.cast_box(kind, hev, posv, rotv, dt)
        centry = CA.node_entry(q(centre_q), q(hw), tuple(dv[:, i][:, None] for i in range(3)), col(lo), col(hi), mdv[:, None], dt)
        assert okc.all() and (chit & caps).sum() >= 100 and not (chit & (centry > ctoi)).any()
        # intersections and contacts: the padded boxes overlap
        qlo, qhi = S.query_shape_aabb(kind, hev, pts, rotv, dt)
        ids, cnt = C.shape_intersections(s, kind, he, pts, rot, s.n)
        lists = C.contact_lists(s, kind, he, pts, rot, 0.25)
    assert cnt.sum() >= 50 and sum(len(l) for l in lists) >= cnt.sum()
    pad = dt(0.25) * (dt(1) + dt(64) * dt(np.finfo(dt).eps)) + dt(64) * dt(np.finfo(dt).eps) * np.maximum.reduce([np.abs(x) for x in qlo + qhi])
    for i in range(n):
        for c in ids[i, :cnt[i]]:
            assert all(lo[k][c] <= qhi[k][i] and hi[k][c] >= qlo[k][i] for k in range(3)), (i, c)
        for c in lists[i]["collider"]:
            assert all(lo[k][c] <= qhi[k][i] + pad[i] and hi[k][c] >= qlo[k][i] - pad[i] for k in range(3)), (i, c)


def test_the_patch_does_not_outlive_a_call():
    s = snapshot(capsule_items(np.random.default_rng(1), 3), np.float32)
    CC.cast_rays(s, [[0, 5.0, 0]], [[0, -1.0, 0]])
    assert R.ray_exact is CC._o["ray_exact"] and R.shape_aabb is CC._o["shape_aabb"] and CA.cast_exact is CC._o["cast_exact"]
    assert C.capsule_cast_exact is CC._o["capsule_cast_exact"] and CR.oracle_world is C._orig_oracle_world and S.shape_valid is C._orig_shape_valid
