"""Exact geometry of shape casts (include/avian_mi355x_spatial.h), independent of the device's arithmetic.

Built on spatial_exact_geometry and spatial_shape_exact_geometry: every input float is a Fraction, a pose's rotation is the exactly orthogonal
matrix of its quaternion as given (the device sends the query's through make_isometry's axis-angle round trip), square roots are taken at 60
digits.  Nothing here follows an operation order.

sweep(query, d, col) is the closed interval of t (over the whole line) at which the query shape translated by t d intersects the collider:
  ball / ball      the roots of |c + t d|^2 = (r1 + r2)^2;
  ball and cuboid  the ball's centre against the cuboid rounded by r.  That set is convex, so its interval is [min entry, max exit] over convex
                   pieces that cover it: the three boxes he + r e_i, the twelve edge cylinders cut to their edges' extents, the eight corner
                   balls.  The module checks its own answer against the distance function of spatial_shape_exact_geometry: at the entry the
                   centre is r from the cuboid (to 1e-24: sqrt_q's quotient carries 28 digits);
  cuboid / cuboid  two cuboids intersect iff no one of the 15 SAT axes separates them; along each axis n (not normalised: no square root) that
                   is |n.(c + t d)| <= ra + rb, linear in t: the interval is the intersection of 15 rational intervals.
cast(query, d, col, max_distance) -> Cast: hit, toi = max(entry, 0), overlap (the shapes intersect at t = 0), and the CLASS of the contact.

DECIDED ANSWERS.  A translation of the query by less than `band` cannot turn a miss into a hit when the cast still misses with both shapes
grown by band (half extents and radii + band: a superset of the Minkowski sum with a ball of radius band) and the range grown by band; nor a
hit into a miss when it still hits with both shapes shrunk by band and the range shrunk.  decided(...) returns 'hit', 'miss' or None
(undecided: either answer is accepted).  The same with the interval at t = 0 decides the initial overlap.

FORWARD-ERROR BOUND.  With
    scale = |query position| + query size + |pos| + max half-extent + distance       (max-norms)
    band  = 32 eps * scale                                                            (BAND_EPS of spatial_exact_geometry, unchanged)
  * decided hit / miss / overlap answers are the exact ones;
  * where both hit at a positive distance, |distance - toi| <= band, plus for contacts on a round feature (any pair with a ball) the square
    root's term min(sqrt(e), e / h) with e = 2 r band and h the half chord of the centre's line through the rounded feature;
  * witnesses (decided hits, every class): point1 within wband of the collider's surface, point2 within wband of the cast shape's surface
    at the computed impact pose, each within wband of its shape's supporting plane along normal1, |point1 - point2| <= 2 wband, where
    wband = that distance bound, times 1 / sin^2 of the angle between the edges for an edge-edge contact (the closest points of two lines
    divide by it); normal2 = -normal1 exactly, | |n| - 1 | <= 32 eps, and along normal1 the collider's support lies within wband below the
    cast shape's.  The parallel-face class of the sets has equal or quarter-turned rotations: the clipped witnesses coincide there
    (faces turned about their common normal by another angle: test_parallel_faces_turned_about_the_normal pins what the clamps give).
WORST_OBSERVED records error / bound over the sets of test_spatial_casts_cpu.py, which asserts that they stay within four times it."""
from __future__ import annotations

from fractions import Fraction as Q

import spatial_exact_geometry as X
import spatial_shape_exact_geometry as XS
from spatial_exact_geometry import BALL, BAND_EPS, CUBOID, EPS, INF, Collider, add, dot, maxabs, mul, mul_t, norm, scale, sqrt_q, sub, vec
from spatial_shape_exact_geometry import Shape

# error / bound, the largest over the sets of test_spatial_casts_cpu.py (f32 and f64; the restatement on the CPU)
WORST_OBSERVED = {"distance": 0.03, "witness": 0.04, "undecided_fraction": 0.0}

CLASSES = ("face", "edge", "corner", "edge-edge", "face-vertex", "parallel-face", "overlap", "miss")


class Cast:
    def __init__(self, hit, toi=None, overlap=False, cls="miss", half_chord=None, sin2=None):
        self.hit, self.toi, self.overlap, self.cls, self.half_chord, self.sin2 = hit, toi, overlap, cls, half_chord, sin2

    def __repr__(self):
        return f"Cast(hit={self.hit}, toi={None if self.toi is None else float(self.toi)}, overlap={self.overlap}, cls={self.cls})"


def _quadratic(o, d, r, idx=(0, 1, 2)):
    """Interval of t with |o + t d| <= r over the components idx; None = empty; (None, None) = every t.  Also the half chord in length."""
    a = sum((d[i] * d[i] for i in idx), Q(0))
    b = sum((o[i] * d[i] for i in idx), Q(0))
    c = sum((o[i] * o[i] for i in idx), Q(0)) - r * r
    if a == 0:
        return ((None, None), None) if c <= 0 else (None, None)
    disc = b * b - a * c          # exact: no cancellation to fear in rationals
    if disc < 0:
        return None, None
    sq = sqrt_q(disc)
    return ((-b - sq) / a, (-b + sq) / a), sq / sqrt_q(a)


def _meet(a, b):
    """Intersection of two intervals with None ends = unbounded; None = empty."""
    if a is None or b is None:
        return None
    lo = a[0] if b[0] is None else (b[0] if a[0] is None else max(a[0], b[0]))
    hi = a[1] if b[1] is None else (b[1] if a[1] is None else min(a[1], b[1]))
    return None if (lo is not None and hi is not None and lo > hi) else (lo, hi)


def _slab(o, d, h):
    """Interval of t with |o + t d| <= h (one component)."""
    if d == 0:
        return (None, None) if abs(o) <= h else None
    t1, t2 = (-h - o) / d, (h - o) / d
    return (min(t1, t2), max(t1, t2))


def _round_box(o, d, he, r):
    """(interval, class of the entry, half chord of the round piece that gives the entry) of the line o + t d through the box rounded by r."""
    pieces = []
    for i in range(3):
        iv = (None, None)
        for j in range(3):
            iv = _meet(iv, _slab(o[j], d[j], he[j] + (r if j == i else 0)))
        pieces.append((iv, "face", None))
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        for sa in (1, -1):
            for sb in (1, -1):
                oo = list(o); oo[a] -= sa * he[a]; oo[b] -= sb * he[b]
                iv, half = _quadratic(oo, d, r, (a, b))
                pieces.append((_meet(iv, _slab(o[k], d[k], he[k])), "edge", half))
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                iv, half = _quadratic(sub(o, (sx * he[0], sy * he[1], sz * he[2])), d, r)
                pieces.append((iv, "corner", half))
    lo, hi, cls, half = None, None, None, None
    some = False
    for iv, c, h in pieces:
        if iv is None:
            continue
        if iv[0] is None or iv[1] is None:      # d = 0 inside a piece: every t
            return (None, None), c, h
        if not some or iv[0] < lo:
            lo, cls, half = iv[0], c, h
        hi = iv[1] if not some else max(hi, iv[1])
        some = True
    return ((lo, hi), cls, half) if some else (None, None, None)


def _axes(a: Collider, b: Collider):
    A = [tuple(a.R[i][j] for i in range(3)) for j in range(3)]
    B = [tuple(b.R[i][j] for i in range(3)) for j in range(3)]
    out = [(u, "face-vertex", None) for u in A] + [(u, "face-vertex", None) for u in B]
    for u in A:
        for v in B:
            c = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
            if dot(c, c) > Q(1, 10 ** 40):
                out.append((c, "edge-edge", dot(c, c)))     # |u x v|^2 = sin^2 of the angle between the edges
    return A, B, out


def _sat_sweep(query: Collider, d, col: Collider):
    A, B, axes = _axes(col, query)
    c = sub(query.pos, col.pos)
    iv, cls, sin2 = (None, None), None, None
    for n, kind, s2 in axes:
        rr = sum((abs(dot(n, A[i])) * col.he[i] for i in range(3)), Q(0)) + sum((abs(dot(n, B[i])) * query.he[i] for i in range(3)), Q(0))
        one = _slab(dot(n, c), dot(n, d), rr)
        if one is None:
            return None, None, None
        if one[0] is not None and (iv[0] is None or one[0] > iv[0]):
            cls, sin2 = kind, s2
        iv = _meet(iv, one)
        if iv is None:
            return None, None, None
    # parallel faces, or a face parallel to an edge: some axis of one cuboid is (anti)parallel or perpendicular to an axis of the other.  The
    # contact is then a segment or a polygon, several axes tie for the entry, and the witnesses are not unique
    if any(abs(abs(dot(u, v)) - 1) < Q(1, 10 ** 6) or abs(dot(u, v)) < Q(1, 10 ** 6) for u in A for v in B):
        cls = "parallel-face"
    return iv, cls, sin2


def sweep(query: Collider, d, col: Collider):
    """(interval or None, class of the entry, half chord or None, sin^2 or None)."""
    d = vec(d)
    if query.shape == BALL and col.shape == BALL:
        iv, half = _quadratic(sub(query.pos, col.pos), d, query.he[0] + col.he[0])
        return iv, "corner", half, None
    if query.shape == BALL:
        iv, cls, half = _round_box(col.local(query.pos), mul_t(col.R, d), col.he, query.he[0])
        if iv is not None and iv[0] is not None and query.he[0] > 0:
            assert abs(XS._cuboid_distance(col, add(query.pos, scale(d, iv[0]))) - query.he[0]) < Q(1, 10 ** 24)
        return iv, cls, half, None
    if col.shape == BALL:
        iv, cls, half = _round_box(query.local(col.pos), scale(mul_t(query.R, d), -1), query.he, col.he[0])
        return iv, cls, half, None
    iv, cls, sin2 = _sat_sweep(query, d, col)
    return iv, cls, None, sin2


def cast(query: Collider, d, col: Collider, max_distance=INF) -> Cast:
    iv, cls, half, sin2 = sweep(query, d, col)
    if iv is None or (iv[1] is not None and iv[1] < 0):
        return Cast(False)
    overlap = iv[0] is None or iv[0] <= 0
    toi = Q(0) if overlap else iv[0]
    if max_distance != INF and toi > X.q(max_distance):
        return Cast(False)
    return Cast(True, toi, overlap, "overlap" if overlap else cls, half, sin2)


def _resized(c: Collider, by):
    out = Collider(c.shape, (0, 0, 0), (0, 0, 0), (0, 0, 0, 1))
    out.pos, out.quat, out.R, out.size = c.pos, c.quat, c.R, c.size
    out.he = (c.he[0] + by,) * 3 if c.shape == BALL else tuple(h + by for h in c.he)
    return out if all(h >= 0 for h in (out.he[:1] if c.shape == BALL else out.he)) else None


def decided(query, d, col, max_distance, band):
    """('hit' | 'miss' | None, 'overlap' | 'apart' | None): the answers no translation of the query below `band` can change."""
    band = Q(band)
    md = INF if max_distance == INF else float(X.q(max_distance))
    big = cast(_resized(query, band), d, _resized(col, band), INF if md == INF else md + float(band))
    qs, cs = _resized(query, -band), _resized(col, -band)
    small = cast(qs, d, cs, INF if md == INF else md - float(band)) if qs is not None and cs is not None and (md == INF or md >= float(band)) else Cast(False)
    hit = "miss" if not big.hit else ("hit" if small.hit else None)
    start = "apart" if not (big.hit and big.overlap) else ("overlap" if small.hit and small.overlap else None)
    return hit, start


def scale_of(bits, query: Collider, col: Collider, distance=0):
    s = maxabs(query.pos) + query.size + maxabs(col.pos) + col.size + abs(float(distance))
    return s, BAND_EPS * EPS[bits] * s


def distance_bound(band, c: Cast, query: Collider, col: Collider):
    """band, plus the square root's grazing term when the contact is on a round feature."""
    if query.shape != BALL and col.shape != BALL:
        return band
    r = float(query.he[0] + col.he[0]) if (query.shape == BALL and col.shape == BALL) else float(query.he[0] if query.shape == BALL else col.he[0])
    if c.cls == "face" or r == 0:
        return band
    e = 2 * band * r
    return band + (e ** 0.5 if not c.half_chord else min(e ** 0.5, e / float(c.half_chord)))


# ---- witnesses -------------------------------------------------------------------------------------------------------------------------------
def surface_distance(c: Collider, p):
    """Signed distance of the world point p from the shape's surface (> 0 outside)."""
    if c.shape == BALL:
        return norm(sub(p, c.pos)) - c.he[0]
    return XS._cuboid_distance(c, p)


def support(c: Collider, n):
    """max of n.x over the shape."""
    if c.shape == BALL:
        return dot(n, c.pos) + c.he[0] * norm(n)
    return dot(n, c.pos) + sum((abs(dot(n, tuple(c.R[i][j] for i in range(3)))) * c.he[j] for j in range(3)), Q(0))


def moved(c: Collider, d, t):
    out = _resized(c, Q(0))
    out.pos = add(c.pos, scale(vec(d), X.q(t)))
    return out


def witness_errors(rec, query: Collider, d, col: Collider):
    """Errors of one record's witnesses against the exact shapes, the cast shape at the record's own distance: on-surface errors of point1 and
    point2, their distance apart, the error of the normal's length, how far the collider's support along normal1 passes the cast shape's, and
    the distances of the two points from the two supporting planes."""
    p1, p2, n1 = vec(rec["point1"]), vec(rec["point2"]), vec(rec["normal1"])
    qm = moved(query, d, rec["distance"])
    top = support(col, n1)
    bottom = -support(qm, scale(n1, -1))
    return dict(on1=abs(surface_distance(col, p1)), on2=abs(surface_distance(qm, p2)), apart=norm(sub(p1, p2)), unit=abs(norm(n1) - 1),
                separation=max(top - bottom, Q(0)), plane1=abs(dot(n1, p1) - top), plane2=abs(dot(n1, p2) - bottom))
