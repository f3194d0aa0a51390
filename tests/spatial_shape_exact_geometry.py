"""Exact geometry of point projection and shape intersection (include/avian_mi355x_spatial.h), independent of the device's arithmetic.

Built on spatial_exact_geometry: every input float is a Fraction, a pose's rotation is the exactly orthogonal matrix of its quaternion, square
roots are taken at 60 digits.  Nothing here follows an operation order: the query shape's pose is its quaternion as given (the device sends
it through make_isometry's axis-angle round trip), a cuboid pair is decided by the largest normalised separation over the 15 SAT axes.

Answers and their MARGINS (lower bounds of the translation of the query that can change the decision):
  project(col, p, solid) -> Projection: distance, world point, is_inside;  margins `inside` (the point's distance from the surface: it decides
      is_inside and, for solid queries, the distance 0) and `face` (hollow queries inside a cuboid: half the gap between the two smallest face
      distances, which decides the face; outside a cuboid and for balls away from the centre the projection is continuous: None).
  intersect(query, col) -> (hit, gap): ball pairs |c1 - c2| - (r1 + r2); ball / cuboid the distance of the centre from the cuboid minus r
      (inside: -(depth + r)); cuboid pairs the largest of the 15 separations along unit axes (edge axes that vanish are left out).  hit = gap
      <= 0; the margin is |gap|.

FORWARD-ERROR BOUND.  The restatement's (so the device's) answers in a scalar type of machine epsilon eps are held to these with
    scale = |query position| + query size + |pos| + max half-extent + distance      (max-norms; size and distance 0 where there is none)
    band  = 32 eps * scale                                                           (BAND_EPS of spatial_exact_geometry, unchanged)
  * is_inside, the chosen face and every intersection decision whose margin exceeds `band` are the exact ones;
  * where is_inside (and the face) agree, every coordinate of the projected point and the distance are within `band`; inside a hollow ball
    the scaling p_l * (r / |p_l|) turns the local point's error into r / |p_l| times it, so there the bound is band * max(1, r / d) with d
    the point's distance from the centre;
  * the collider a projection query answers has an exact distance within `band` of the exact minimum over the candidates.
Rounding count behind keeping 32 for two composed poses: the query's quaternion through make_isometry (an arctangent, a sine and a cosine of
<= 2 ulp each, two divisions, two products) moves the rotation by <= 8 eps, so a point of the query shape by 8 eps * size; the relative
rotation (one quaternion product, 7 roundings per component) and the relative translation (a difference of two positions, 1 eps of each,
then a rotation of ~10 roundings) add <= 12 eps * (|positions| + sizes); each SAT axis adds two more rotations of a support point, a sum
and a dot product: <= 10 eps * sizes.  The sum stays under 32 eps * scale because each term scales with ONE of the magnitudes that scale
adds up.  Worst error / (eps * scale) of the restatement over the sets of test_spatial_shapes_cpu.py: see WORST_OBSERVED below."""
from __future__ import annotations

from fractions import Fraction as Q

import spatial_exact_geometry as X
from spatial_exact_geometry import BALL, BAND_EPS, CUBOID, EPS, Collider, add, dot, maxabs, mul, norm, rotation, scale, sqrt_q, sub, vec

# error / (eps * scale), the largest over the random sets of test_spatial_shapes_cpu.py (f32 and f64, compound and far scenes):
# (projected point and distance, intersection decisions that disagree with the exact one have margins below this)
WORST_OBSERVED = {"projection": 1.4, "intersection": 0.1}


class Shape(Collider):
    """A query shape at its pose: a Collider without a body (kind, half extents / radius in x, position, rotation xyzw)."""

    def __init__(self, shape, half_extents, position, rot):
        super().__init__(shape, half_extents, position, rot)


class Projection:
    def __init__(self, distance, point, inside, m_inside, m_face):
        self.distance, self.point, self.is_inside = distance, point, inside
        self.margins = {"inside": m_inside, "face": m_face}


def project(col: Collider, p, solid=True) -> Projection:
    p = vec(p)
    if col.shape == BALL:
        r = col.he[0]
        v = sub(p, col.pos)
        d = norm(v)
        inside = d <= r
        m = abs(d - r)
        if inside and solid:
            return Projection(Q(0), p, True, m, None)
        if d == 0:
            return Projection(r, add(col.pos, mul(col.R, (Q(0), r, Q(0)))), True, m, None)
        # (hollow, near the centre the projection jumps when the point crosses it: d is that margin)
        return Projection(abs(d - r), add(col.pos, scale(v, r / d)), inside, m, d if inside else None)
    he = col.he
    pl = col.local(p)
    margins = [he[i] - abs(pl[i]) for i in range(3)]
    inside = all(m >= 0 for m in margins)
    if not inside:
        cl = tuple(max(-he[i], min(he[i], pl[i])) for i in range(3))
        d = norm(sub(pl, cl))
        return Projection(d, add(col.pos, mul(col.R, cl)), False, d, None)   # (L2 distance from the surface: the decision's margin)
    m_inside = min(margins)
    if solid:
        return Projection(Q(0), p, True, m_inside, None)
    order = sorted(range(3), key=lambda i: (margins[i], i))
    a = order[0]
    face = list(pl)
    face[a] = he[a] if pl[a] >= 0 else -he[a]
    # the face changes when another margin undercuts this one (translation changes a margin by at most |v|, their gap by 2 |v|) or when the
    # point crosses the centre plane of that axis
    m_face = min((margins[order[1]] - margins[a]) / 2, abs(pl[a]))
    return Projection(margins[a], add(col.pos, mul(col.R, tuple(face))), True, m_inside, m_face)


def _cuboid_distance(col: Collider, c):
    """Signed distance of the world point c from the cuboid: > 0 outside (Euclidean), <= 0 inside (minus the depth)."""
    pl = col.local(c)
    margins = [col.he[i] - abs(pl[i]) for i in range(3)]
    if all(m >= 0 for m in margins):
        return -min(margins)
    cl = tuple(max(-col.he[i], min(col.he[i], pl[i])) for i in range(3))
    return norm(sub(pl, cl))


def _sat_gap(a: Collider, b: Collider):
    """The largest separation of two cuboids over the 15 SAT axes, each normalised: > 0 disjoint (a lower bound of their distance), <= 0
    intersecting (minus a lower bound of the penetration)."""
    A = [tuple(a.R[i][j] for i in range(3)) for j in range(3)]   # columns: the cuboid's axes in world space
    B = [tuple(b.R[i][j] for i in range(3)) for j in range(3)]
    t = sub(b.pos, a.pos)
    axes = A + B
    for u in A:
        for v in B:
            c = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
            n2 = dot(c, c)
            if n2 > Q(1, 10 ** 40):
                axes.append(scale(c, 1 / sqrt_q(n2)))
    best = None
    for n in axes:
        ra = sum((abs(dot(n, A[i])) * a.he[i] for i in range(3)), Q(0))
        rb = sum((abs(dot(n, B[i])) * b.he[i] for i in range(3)), Q(0))
        s = abs(dot(n, t)) - ra - rb
        best = s if best is None or s > best else best
    return best


def intersect(query: Collider, col: Collider):
    """(hit, gap) of the module docstring; touching (gap == 0) is a hit."""
    if query.shape == BALL and col.shape == BALL:
        gap = norm(sub(query.pos, col.pos)) - (query.he[0] + col.he[0])
    elif query.shape == BALL:
        gap = _cuboid_distance(col, query.pos) - query.he[0]
    elif col.shape == BALL:
        gap = _cuboid_distance(query, col.pos) - col.he[0]
    else:
        gap = _sat_gap(query, col)
    return gap <= 0, gap


def scale_of(bits, query_pos, query_size, col: Collider, distance=0):
    """(scale, band) of the module docstring."""
    s = maxabs(query_pos) + float(query_size) + maxabs(col.pos) + col.size + abs(float(distance))
    return s, BAND_EPS * EPS[bits] * s
