"""Exact geometry of the spatial queries' per-collider tests (include/avian_mi355x_spatial.h), independent of the device's arithmetic.

Standard library only.  Every input float becomes a Fraction; a pose's rotation is the matrix of its quaternion divided by |q|^2, which is
rational and exactly orthogonal for any q != 0, and a child collider's pose composes the body's and the child's exactly (the quaternion
product).  The ball's square root is taken with `decimal` at 60 digits.  Nothing here follows the kernel's operation order: a ray is a
half-line o + t d, t >= 0, with d as given (not normalised), and a shape is the solid cuboid or ball.

Each answer carries MARGINS: how far, in length units, the ray, point or box can be translated before the decision changes.  They are
lower bounds of that distance:
  hit        the ray's decision (hit or miss, max_distance included)
  inside     whether the origin lies inside the shape (this picks distance 0, the entry or the exit)
  face       (cuboids) whether the entry (or, from inside, the exit) point stays on the same face: its distance from that face's edges,
             divided by how fast the point slides over the face when the ray moves
  For points and boxes only `hit`.

FORWARD-ERROR BOUND.  The device's answer in the world's scalar type (machine epsilon eps) is held to the exact one with
    scale = |o| + |pos| + max half-extent + |toi|          (max-norms; |toi| is the exact distance, 0 for points and boxes)
    band  = 32 eps * scale                                 (length units)
  * every decision whose margin exceeds `band` is the exact one;
  * where the decisions agree, |toi - toi_exact| <= band for cuboids, and band + min(sqrt(e), e / h) for balls, with e = 2 r band the
    error of the discriminant (per |d|^2) and h the exact half chord: the square root turns that error into e / h, and into sqrt(e) when
    the ray grazes (h -> 0);  each normal component is within 32 eps of the exact normal for cuboids, and within that distance bound / r
    for balls.
This is tighter than the tree's padding (64 eps times the box's and the query's largest coordinates, k_spatial.hip), so every pair the
float test accepts lies inside the boxes the traversal tests.  Parry's discriminant b^2 - a c breaks it: its rounding is eps |o - pos|^2,
which in f32 at 1 000 units accepts rays that miss a unit ball by 1.5 % of its radius (the band is 0.8 % there)."""
from __future__ import annotations

import decimal
from fractions import Fraction as Q

CUBOID, BALL = 0, 1
EPS = {32: 2.0 ** -23, 64: 2.0 ** -52}
BAND_EPS = 32
INF = float("inf")
_CTX = decimal.Context(prec=60)


def q(x):
    return Q(float(x))


def vec(v):
    return tuple(q(x) for x in v)


def sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def scale(a, s):
    return tuple(x * s for x in a)


def dot(a, b):
    return sum((x * y for x, y in zip(a, b)), Q(0))


def quat_mul(l, r):
    lx, ly, lz, lw = l
    rx, ry, rz, rw = r
    return (lw * rx + lx * rw + ly * rz - lz * ry, lw * ry - lx * rz + ly * rw + lz * rx, lw * rz + lx * ry - ly * rx + lz * rw, lw * rw - lx * rx - ly * ry - lz * rz)


def rotation(qt):
    """Rows of the rotation matrix of the (not necessarily unit) quaternion xyzw: the textbook matrix divided by |q|^2."""
    x, y, z, w = qt
    n = x * x + y * y + z * z + w * w
    return ((w * w + x * x - y * y - z * z) / n, 2 * (x * y - w * z) / n, 2 * (x * z + w * y) / n), \
           (2 * (x * y + w * z) / n, (w * w - x * x + y * y - z * z) / n, 2 * (y * z - w * x) / n), \
           (2 * (x * z - w * y) / n, 2 * (y * z + w * x) / n, (w * w - x * x - y * y + z * z) / n)


def mul(m, v):
    return tuple(dot(row, v) for row in m)


def mul_t(m, v):
    return tuple(sum((m[i][j] * v[i] for i in range(3)), Q(0)) for j in range(3))


def sqrt_q(x: Q) -> Q:
    """sqrt of a non-negative rational to 60 significant digits."""
    if x <= 0:
        return Q(0)
    r = (decimal.Decimal(x.numerator, _CTX) / decimal.Decimal(x.denominator, _CTX)).sqrt(_CTX)
    return Q(r)


def norm(v) -> Q:
    return sqrt_q(dot(v, v))


def maxabs(v) -> float:
    return max(abs(float(x)) for x in v)


class Collider:
    """A collider's exact pose: body position / rotation, optionally a child's ColliderTransform composed onto it."""

    def __init__(self, shape, half_extents, body_pos, body_rot, child=None):
        self.shape = int(shape)
        self.he = vec(half_extents)
        bp, bq = vec(body_pos), vec(body_rot)
        if child is not None:
            lp, lq = vec(child[0]), vec(child[1])
            self.pos = add(bp, mul(rotation(bq), lp))
            self.quat = quat_mul(bq, lq)
        else:
            self.pos, self.quat = bp, bq
        self.R = rotation(self.quat)
        self.size = max(float(self.he[0]), 0.0) if self.shape == BALL else max(float(h) for h in self.he)

    def local(self, p):
        return mul_t(self.R, sub(p, self.pos))


class Answer:
    def __init__(self, hit, toi=None, normal=None, margin=Q(0), inside=None, face=None, half_chord=None):
        self.hit = hit
        self.half_chord = half_chord  # balls: half the chord of the ray's line through the ball (the square root's conditioning)
        self.toi = toi            # Fraction (or None for a miss / point / box)
        self.normal = normal      # tuple of Fractions, (0, 0, 0) for solid hits from inside
        self.margins = {"hit": margin, "inside": inside, "face": face}

    def margin(self, key="hit"):
        return self.margins[key]

    def __repr__(self):
        m = {k: (None if v is None else float(v)) for k, v in self.margins.items()}
        return f"Answer(hit={self.hit}, toi={None if self.toi is None else float(self.toi)}, normal={None if self.normal is None else [float(x) for x in self.normal]}, margins={m})"


def bound(bits, o, col: Collider, toi=0, half_chord=None):
    """(band, distance bound, normal bound) of the module docstring for one pair (half_chord: the ball answer's; None = grazing)."""
    eps = EPS[bits]
    s = maxabs(o) + maxabs(col.pos) + col.size + abs(float(toi))
    band = BAND_EPS * eps * s
    if col.shape == BALL:
        r = float(col.he[0])
        e = 2 * band * r
        g = band + (e ** 0.5 if not half_chord else min(e ** 0.5, e / float(half_chord)))
        return band, g, (g / r if r > 0 else INF)
    return band, band, BAND_EPS * eps


# ---- rays --------------------------------------------------------------------------------------------------------------------------------
def _cuboid_l_inf(ol, dl, he, t):
    """L-inf excess of the local point at t over the box: > 0 outside, <= 0 inside."""
    return max(abs(ol[i] + t * dl[i]) - he[i] for i in range(3))


def _min_excess(ol, dl, he, t_hi):
    """min over t in [0, t_hi] of the L-inf excess: the L-inf distance of the ray segment from the box (negative: depth inside).  The excess
    is a max of lines in t, so its minimum lies at an end or where two of the lines cross."""
    lines = [(s * ol[i] - he[i], s * dl[i]) for i in range(3) for s in (1, -1)]
    ts = [Q(0)] + ([t_hi] if t_hi is not None else [])
    for i in range(len(lines)):
        for j in range(i + 1, len(lines)):
            (a0, a1), (b0, b1) = lines[i], lines[j]
            if a1 != b1:
                t = (b0 - a0) / (a1 - b1)
                if t >= 0 and (t_hi is None or t <= t_hi):
                    ts.append(t)
    return min(max(a + b * t for a, b in lines) for t in ts)


def _face_margin(p, dl, he, axis):
    """Distance of the point p (on the face normal to `axis`) from that face's edges, per unit of translation of the ray: a translation v
    moves the crossing point along the face by up to |v| (1 + |dl_j| / |dl_axis|) in component j."""
    m = None
    for j in range(3):
        if j == axis:
            continue
        slide = 1 + (abs(dl[j]) / abs(dl[axis]) if dl[axis] != 0 else Q(10 ** 30))
        v = (he[j] - abs(p[j])) / slide
        m = v if m is None else min(m, v)
    return m


def ray_cuboid(col: Collider, o, d, max_distance=INF, solid=True) -> Answer:
    he = col.he
    ol, dl = col.local(vec(o)), mul_t(col.R, vec(d))
    md = None if max_distance == INF else q(max_distance)
    dn = norm(dl)
    tmin, tmax, na, fa = None, None, -1, -1
    for i in range(3):
        if dl[i] == 0:
            if abs(ol[i]) > he[i]:
                tmin, tmax = Q(1), Q(0)   # outside a parallel slab: empty
                break
            continue
        t1, t2 = (-he[i] - ol[i]) / dl[i], (he[i] - ol[i]) / dl[i]
        if t1 > t2:
            t1, t2 = t2, t1
        if tmin is None or t1 > tmin:
            tmin, na = t1, i
        if tmax is None or t2 < tmax:
            tmax, fa = t2, i
    inside_excess = _cuboid_l_inf(ol, dl, he, Q(0))
    inside = inside_excess <= 0
    m_inside = abs(inside_excess)
    line_hits = tmin is None or tmin <= tmax   # (tmin None: d = 0 and the origin within every slab)
    if not line_hits or (tmax is not None and tmax < 0) or (tmin is None and not inside) or (inside and not solid and tmax is None):
        return Answer(False, margin=_min_excess(ol, dl, he, md), inside=m_inside)
    if inside:
        t, axis = (Q(0), -1) if solid else (tmax, fa)
    else:
        t, axis = tmin, na
    if md is not None and t > md:
        return Answer(False, margin=_min_excess(ol, dl, he, md), inside=m_inside)
    md_gap = (md - t) * abs(dl[axis]) if md is not None and axis >= 0 else None
    depth = -_min_excess(ol, dl, he, md)   # translations below the segment's L-inf depth inside the box keep the hit
    if axis < 0:                            # solid, from inside: distance 0 while the origin stays inside
        return Answer(True, t, (Q(0),) * 3, margin=max(depth, m_inside), inside=m_inside)
    p = tuple(ol[k] + t * dl[k] for k in range(3))
    out = 1 if inside else -1               # exit face: the normal along the ray; entry face: against it
    nl = tuple((Q(out) if dl[axis] > 0 else Q(-out)) if k == axis else Q(0) for k in range(3))
    face = _face_margin(p, dl, he, axis)
    # the origin stays inside / the ray keeps crossing the entry face at t >= 0 (a thin box can be crossed backwards: t |dl| caps it)
    keep = m_inside if inside else min(face, t * abs(dl[axis]))
    if md_gap is not None:
        keep = min(keep, md_gap)
    return Answer(True, t, mul(col.R, nl), margin=max(depth, keep), inside=m_inside, face=face)


def ray_ball(col: Collider, o, d, max_distance=INF, solid=True) -> Answer:
    r = col.he[0]
    ol, dl = sub(vec(o), col.pos), vec(d)   # the ball is round: the world frame is its local frame up to rotation
    md = None if max_distance == INF else q(max_distance)
    a, b = dot(dl, dl), dot(ol, dl)
    lo = norm(ol)
    inside = lo <= r
    m_inside = abs(lo - r)
    if a == 0:
        return Answer(solid and inside, Q(0) if solid and inside else None, (Q(0),) * 3 if solid and inside else None, margin=Q(0), inside=m_inside)
    f = sub(ol, scale(dl, b / a))          # the ray line's point nearest the centre, minus the centre
    near = norm(f) if b <= 0 else lo       # distance of the half-line from the centre
    if near > r:
        return Answer(False, margin=near - r, inside=m_inside)
    disc = a * (r * r - dot(f, f))
    sq = sqrt_q(disc)
    dn = sqrt_q(a)
    half = sq / dn                         # half chord, length units
    if inside and solid:
        t, nrm = Q(0), (Q(0),) * 3
    else:
        t = (-b + sq) / a if inside else (-b - sq) / a
        p = add(ol, scale(dl, t))
        lp = norm(p)
        nrm = scale(p, 1 / lp) if lp > 0 else (Q(0),) * 3
    keep = r - near
    if md is not None:
        slide = 1 + (r / half if half > 0 else Q(10 ** 30))
        gap = (md - t) * dn / slide
        if gap < 0:
            return Answer(False, margin=-gap, inside=m_inside)
        keep = min(keep, gap)
    return Answer(True, t, nrm, margin=keep, inside=m_inside, half_chord=half)


def ray(col: Collider, o, d, max_distance=INF, solid=True) -> Answer:
    if max_distance < 0:                    # every distance is >= 0: a miss whatever the ray does
        return Answer(False, margin=Q(10 ** 30))
    return (ray_ball if col.shape == BALL else ray_cuboid)(col, o, d, max_distance, solid)


# ---- points and boxes ------------------------------------------------------------------------------------------------------------------
def point(col: Collider, p) -> Answer:
    """Containment with its margin: the distance of the point from the shape's surface."""
    if col.shape == BALL:
        m = col.he[0] - norm(sub(vec(p), col.pos))
    else:
        pl = col.local(vec(p))
        m = min(col.he[i] - abs(pl[i]) for i in range(3))   # L-inf: a lower bound of the Euclidean distance outside, exact inside
    return Answer(m >= 0, margin=abs(m))


def shape_aabb(col: Collider):
    if col.shape == BALL:
        h = (col.he[0],) * 3
    else:
        h = tuple(sum((abs(col.R[i][j]) * col.he[j] for j in range(3)), Q(0)) for i in range(3))
    return sub(col.pos, h), add(col.pos, h)


def aabb(col: Collider, qmin, qmax) -> Answer:
    """Overlap of the exact shape AABB with the query box; margin: the overlap depth or the gap (min over axes)."""
    mn, mx = shape_aabb(col)
    lo, hi = vec(qmin), vec(qmax)
    m = min(min(hi[i] - mn[i], mx[i] - lo[i]) for i in range(3))
    return Answer(m >= 0, margin=abs(m))
