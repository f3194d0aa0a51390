"""The capsule query shape (include/avian_mi355x_spatial.h, "capsule query shapes") on the CPU: tests/spatial_capsule_reference.py, which
restates the device's operations in order, is held to exact rational geometry in f32 and f64.

Exact side: every input float is a Fraction, a rotation is the exactly orthogonal matrix of its quaternion (spatial_exact_geometry), and the
squared distance of a segment to a point or a box is rational for rational inputs (a piecewise quadratic minimised interval by interval), so
"the shapes touch" is decided without a square root: dist <= T  <=>  T >= 0 and dist^2 <= T^2.
band = 32 eps * (|pos_q| + size_q + |pos_c| + size_c + distance), spatial_cast_exact_geometry's bound, with size_q = r + h."""
from fractions import Fraction as Q

import numpy as np
import pytest

from avian_amd.spatial_query import MISS, SHAPE_CAPSULE
from compound_helpers import compound_scene
from helpers import random_unit_quats
import spatial_capsule_reference as C
import spatial_cast_reference as CA
import spatial_contact_reference as CR
import spatial_exact_geometry as X
import spatial_query_reference as R
import spatial_scenes as SC
import spatial_shape_reference as S

DTYPES = [np.float32, np.float64]
BITS = {np.float32: 32, np.float64: 64}
I = [0.0, 0.0, 0.0, 1.0]
BALL, CUBOID = R.SHAPE_BALL, R.SHAPE_CUBOID


# ---- exact geometry --------------------------------------------------------------------------------------------------------------------------
def exact_seg_box_d2(a, u, he):
    """min over s in [0, 1] of the squared distance of a + s u to the box |x_i| <= he_i, in Fractions."""
    def f(s):
        return sum((max(abs(a[i] + s * u[i]) - he[i], Q(0)) ** 2 for i in range(3)), Q(0))
    cuts = {Q(0), Q(1)}
    for i in range(3):
        if u[i] != 0:
            for side in (-he[i], he[i]):
                s = (side - a[i]) / u[i]
                if 0 < s < 1:
                    cuts.add(s)
    cuts = sorted(cuts)
    best = min(f(s) for s in cuts)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m = [a[i] + (lo + hi) / 2 * u[i] for i in range(3)]
        act = [i for i in range(3) if abs(m[i]) > he[i]]
        den = sum((u[i] * u[i] for i in act), Q(0))
        if den > 0:
            num = sum((u[i] * (a[i] - (he[i] if m[i] > 0 else -he[i])) for i in act), Q(0))
            best = min(best, f(min(max(-num / den, lo), hi)))
    return best


def exact_seg_point_d2(a, u, c):
    uu = X.dot(u, u)
    s = Q(0) if uu == 0 else min(max(X.dot(X.sub(c, a), u) / uu, Q(0)), Q(1))
    e = X.sub(c, X.add(a, X.scale(u, s)))
    return X.dot(e, e)


class Capsule:
    """A capsule's exact pose: the world segment of its core."""

    def __init__(self, pos, rot, r, h, dt):
        f = lambda v: [float(dt(x)) for x in v]
        self.pos, self.r, self.h = X.vec(f(pos)), X.q(float(dt(r))), X.q(float(dt(h)))
        hv = X.mul(X.rotation(X.vec(f(rot))), (Q(0), self.h, Q(0)))
        self.a, self.b = X.sub(self.pos, hv), X.add(self.pos, hv)
        self.size = float(self.r + self.h)

    def core_d2(self, col, shift=(0, 0, 0)):
        """The squared distance of the core segment, translated by `shift`, to the collider's core (a ball's centre, a cuboid's box)."""
        sh = X.vec(shift)
        a, b = col.local(X.add(self.a, sh)), col.local(X.add(self.b, sh))
        u = X.sub(b, a)
        return exact_seg_point_d2(a, u, (Q(0),) * 3) if col.shape == BALL else exact_seg_box_d2(a, u, col.he)


def within(d2, T):
    """dist <= T for dist^2 = d2."""
    return T >= 0 and d2 <= T * T


def collider(shape, he, pos, rot, dt):
    f = lambda v: [float(dt(x)) for x in v]
    return X.Collider(shape, f(he), f(pos), f(rot))


def band_of(dt, cap, col, distance=0.0):
    return Q(X.BAND_EPS * X.EPS[BITS[dt]] * (X.maxabs(cap.pos) + cap.size + X.maxabs(col.pos) + col.size + abs(float(distance))))


def snapshot(items, dt):
    """A Snapshot of (shape, he, pos, rot) tuples, one static body each."""
    cols = dict(entity_index=np.arange(500, 500 + len(items), dtype=np.uint32), body=np.arange(len(items), dtype=np.int32),
                shape=np.array([i[0] for i in items], np.uint8), half_extents=np.array([i[1] for i in items], float))
    return R.Snapshot(SC.bodies_of([i[2] for i in items], [i[3] for i in items]), cols, None, dt)


def rcc(n):
    return np.full(n, SHAPE_CAPSULE, np.uint8)


def check_cast(dt, cap_pose, d, item, expect):
    """One capsule cast against one collider: the restatement's answer bracketed by the exact shapes grown / shrunk by band."""
    pos, rot, r, h = cap_pose
    s = snapshot([item], dt)
    d = np.asarray(d, float) / np.linalg.norm(d)
    hit, toi, p1, p2, n1, ok = C.cast_pairs(s, rcc(1), [[r, h, 9.0]], [pos], [rot], [d])
    assert ok.all() and (C.last_rounds < C.ROUNDS).all()
    cap, col = Capsule(pos, rot, r, h, dt), collider(*item, dt)
    rr = cap.r + (col.he[0] if col.shape == BALL else 0)
    dq = X.vec([float(dt(x)) for x in d])
    if expect == "miss":
        assert not hit[0, 0]
        return None
    assert hit[0, 0], expect
    t = float(toi[0, 0])
    band = band_of(dt, cap, col, t)
    nrm = np.array([n1[j][0, 0] for j in range(3)], float)
    if expect == "overlap":
        assert t == 0 and not nrm.any() and within(cap.core_d2(col), rr + 2 * band)
        return t
    assert t > 0 and abs(np.linalg.norm(nrm) - 1) < 64 * np.finfo(dt).eps
    # grown by band the exact shapes touch at the computed distance; shrunk by band they do not touch at distance - band
    assert within(cap.core_d2(col, X.scale(dq, X.q(t))), rr + 2 * band), (expect, t)
    assert not within(cap.core_d2(col, X.scale(dq, X.q(t) - band)), rr - 2 * band), (expect, t)
    # the witnesses: point1 on the collider, point2 on the capsule at the impact pose, normal2 = -normal1 along their difference
    w1 = X.vec([float(p1[j][0, 0]) for j in range(3)]); w2 = X.vec([float(p2[j][0, 0]) for j in range(3)])
    shifted = Capsule(pos, rot, r, h, dt)
    sh = X.scale(dq, X.q(t))
    a, b = X.add(shifted.a, sh), X.add(shifted.b, sh)
    d2 = exact_seg_point_d2(a, X.sub(b, a), w2)
    wb = 8 * band + Q(float(np.sqrt(float(2 * rr * band)))) if col.shape == BALL else 8 * band
    assert within(d2, cap.r + wb) and not within(d2, cap.r - wb), expect
    assert X.norm(X.sub(w1, w2)) <= 4 * wb, expect
    return t


def quat_to(v):
    """The rotation that takes the capsule's axis (0, 1, 0) to v."""
    v = np.asarray(v, float) / np.linalg.norm(v)
    ax = np.cross([0, 1, 0], v)
    s = np.linalg.norm(ax)
    if s < 1e-12:
        return I if v[1] > 0 else [1.0, 0.0, 0.0, 0.0]
    ang = np.arctan2(s, v[1])
    return list(ax / s * np.sin(ang / 2)) + [np.cos(ang / 2)]


BOX = (CUBOID, [1.0, 1.0, 1.0], [0.1, -0.2, 0.05], I)
TILTED = (CUBOID, [1.0, 0.7, 1.3], [0.1, -0.2, 0.05], list(np.array([0.1, 0.2, -0.15, 0.96]) / np.linalg.norm([0.1, 0.2, -0.15, 0.96])))
FLOOR = (CUBOID, [4.0, 0.5, 4.0], [0.0, -0.5, 0.0], I)
BALL_C = (BALL, [0.75, 0, 0], [0.2, 0.1, -0.3], I)
R_, H_ = 0.4, 0.5
# (class, (position, rotation, r, h), direction, collider, expectation)
CLASSES = [
    ("cap on a face", ([0.3, 3.0, -0.4], I, R_, H_), [0, -1, 0], FLOOR, "hit"),
    ("cap on a tilted face", ([0.3, 3.0, -0.4], quat_to([0.2, 1, 0.1]), R_, H_), [0.1, -1, 0.2], TILTED, "hit"),
    ("side on a face, parallel", ([0.3, 3.0, -0.4], quat_to([1, 0, 0]), R_, H_), [0, -1, 0], FLOOR, "hit"),
    ("side across an edge", ([3.1, 2.8, 0.3], quat_to([1, -1, 0]), R_, H_), [-1, -1, 0], BOX, "hit"),
    ("side along an edge", ([3.1, 2.8, 0.0], quat_to([0, 0, 1]), R_, H_), [-1, -1, 0], BOX, "hit"),
    ("cap on an edge", ([3.1, 2.8, 0.3], quat_to([1, 1, 0]), R_, H_), [-1, -1, 0], BOX, "hit"),
    ("cap on a corner", ([3.1, 2.8, 3.05], quat_to([1, 1, 1]), R_, H_), [-1, -1, -1], BOX, "hit"),
    ("side on a corner", ([3.1, 2.8, 3.05], quat_to([1, -1, 0]), R_, H_), [-1, -1, -1], BOX, "hit"),
    ("ball by the cap", ([0.3, 3.0, -0.4], I, R_, H_), [0, -1, 0], BALL_C, "hit"),
    ("ball by the side", ([0.3, 3.0, -0.4], quat_to([1, 0, 0.2]), R_, H_), [0, -1, 0], BALL_C, "hit"),
    ("a segment (r = 0) on a face", ([0.3, 3.0, -0.4], quat_to([1, 0.5, 0]), 0.0, H_), [0, -1, 0], FLOOR, "hit"),
    ("overlap at the start", ([0.3, 1.1, -0.4], I, R_, H_), [0, -1, 0], BOX, "overlap"),
    ("overlap with a ball", ([0.3, 1.0, -0.4], I, R_, H_), [0, -1, 0], BALL_C, "overlap"),
    ("cores crossing", ([0.3, 0.9, -0.4], quat_to([1, 1, 0.3]), R_, 1.5), [0, -1, 0], BOX, "overlap"),
    ("a miss beside the collider", ([3.0, 3.0, -0.4], I, R_, H_), [0, -1, 0], BOX, "miss"),
    ("a miss beside a ball", ([2.0, 3.0, -0.4], I, R_, H_), [0, -1, 0], BALL_C, "miss"),
    ("moving away", ([0.3, 3.0, -0.4], I, R_, H_), [0.1, 1, 0], BOX, "miss"),
    ("moving away from a ball", ([0.3, 3.0, -0.4], I, R_, H_), [0.1, 1, 0], BALL_C, "miss"),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CLASSES, ids=[c[0] for c in CLASSES])
def test_contact_classes_bracketed_by_exact_geometry(dt, case):
    _, pose, d, item, expect = case
    check_cast(dt, pose, d, item, expect)


@pytest.mark.parametrize("dt", DTYPES)
def test_upright_character_on_a_floor_bit_for_bit(dt):
    """Dyadic inputs: r = h = 0.5 at height 3 over a floor whose top is y = 0.  Round 0: dist = 2.5, t' = 2; round 1: dist = 0.5 <= r."""
    s = snapshot([FLOOR], dt)
    hit, toi, p1, p2, n1, _ = C.cast_pairs(s, rcc(1), [[0.5, 0.5, 0]], [[0.25, 3.0, -0.5]], [I], [[0, -1, 0]])
    assert hit[0, 0] and toi[0, 0] == dt(2.0) and C.last_rounds[0, 0] == 2
    assert [float(x[0, 0]) for x in n1] == [0.0, 1.0, 0.0]
    assert [float(x[0, 0]) for x in p1] == [0.25, 0.0, -0.5] and [float(x[0, 0]) for x in p2] == [0.25, 0.0, -0.5]
    # the same character resting: the contact at prediction 0.125 of a capsule whose cap is 0.0625 above the floor
    l = C.contact_lists(s, rcc(1), [[0.5, 0.5, 0]], [[0.25, 1.0625, -0.5]], [I], 0.125)[0]
    assert len(l) == 1 and l[0]["penetration"] == dt(-0.0625) and list(l[0]["normal"]) == [0, 1, 0]
    assert list(l[0]["anchor1"]) == [0, -1, 0] and list(l[0]["point"]) == [0.25, 0.0625, -0.5] and list(l[0]["anchor2"]) == [0.25, 0.5, -0.5]
    assert len(C.contact_lists(s, rcc(1), [[0.5, 0.5, 0]], [[0.25, 1.0625, -0.5]], [I], 0.03125)[0]) == 0


# ---- seeded sets ---------------------------------------------------------------------------------------------------------------------------------
def random_colliders(rng, n, spread=3.0, centre=(0, 0, 0)):
    items = []
    for k in range(n):
        rot = I if k % 4 == 0 else list(random_unit_quats(rng, 1)[0])
        pos = list(np.asarray(centre, float) + rng.uniform(-spread, spread, 3))
        if rng.random() < 0.4:
            items.append((BALL, [rng.uniform(0.2, 1.0), 0, 0], pos, rot))
        else:
            items.append((CUBOID, list(rng.uniform(0.2, 1.2, 3)), pos, rot))
    return items


def aimed_casts(rng, items, n, centre=(0, 0, 0)):
    """n capsule casts aimed near the colliders: (he [n, 3], pos, rot, d, target)."""
    he = np.c_[rng.uniform(0.05, 0.6, n), rng.uniform(0.0, 0.8, n), rng.uniform(-5, 5, n)]        # z is not read
    rot = random_unit_quats(rng, n)
    rot[::5] = I
    target = rng.integers(0, len(items), n)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    centres = items if isinstance(items, np.ndarray) else np.array([it[2] for it in items])      # (a list of colliders, or their positions)
    aim = centres[target] + rng.normal(size=(n, 3)) * 0.4
    pos = aim - d * rng.uniform(2.5, 6.0, n)[:, None]
    return he, pos, rot, d, target


@pytest.mark.parametrize("dt", DTYPES)
def test_seeded_casts_bracketed_and_newton_rounds(dt):
    """400 aimed casts per scalar type: every non-grazing hit on its target is bracketed by the exact shapes, misses of the target are exact
    misses, and no capsule-cuboid pair of the set comes near the cap of 32 rounds."""
    rng = np.random.default_rng(11)
    items = random_colliders(rng, 12)
    s = snapshot(items, dt)
    he, pos, rot, d, target = aimed_casts(rng, items, 400)
    hit, toi, p1, p2, n1, ok = C.cast_pairs(s, rcc(400), he, pos, rot, d)
    rounds = C.last_rounds
    assert ok.all() and rounds.max() < C.ROUNDS and rounds.max() <= 12, rounds.max()
    checked = missed = 0
    for i in range(0, 400, 2):
        c = target[i]
        cap, col = Capsule(pos[i], rot[i], he[i, 0], he[i, 1], dt), collider(*items[c], dt)
        rr = cap.r + (col.he[0] if col.shape == BALL else 0)
        dq = X.vec([float(dt(x)) for x in d[i]])
        if not hit[i, c]:
            # an exact miss: the core never comes within rr - band of the collider's over the range that matters (sampled finely), or moves away
            band = band_of(dt, cap, col, 8.0)
            assert all(not within(cap.core_d2(col, X.scale(dq, Q(k, 8))), rr - 2 * band) for k in range(0, 80)), i
            missed += 1
            continue
        t = float(toi[i, c])
        band = band_of(dt, cap, col, t)
        nrm = np.array([n1[j][i, c] for j in range(3)], float)
        if t == 0:
            assert within(cap.core_d2(col), rr + 2 * band), i
            continue
        if -(nrm @ d[i]) < 0.25:      # grazing: the root is ill-conditioned, the under-estimate is still sound but not within band
            assert not within(cap.core_d2(col, X.scale(dq, X.q(t) - 4096 * band)), rr - 2 * band), i
            continue
        assert within(cap.core_d2(col, X.scale(dq, X.q(t))), rr + 2 * band), (i, c, t)
        assert not within(cap.core_d2(col, X.scale(dq, X.q(t) - band)), rr - 2 * band), (i, c, t)
        checked += 1
    assert checked >= 100 and missed >= 10, (checked, missed)


@pytest.mark.parametrize("dt", DTYPES)
def test_segment_box_distance_against_exact(dt):
    """sp_seg_box on seeded segments, axis-parallel ones included: the distance agrees with the exact minimum within band and never undercuts a
    2001-sample brute force by more than that."""
    rng = np.random.default_rng(3)
    n = 300
    he = rng.uniform(0.1, 2, (n, 3)).astype(dt); a = rng.uniform(-4, 4, (n, 3)).astype(dt); u = rng.uniform(-3, 3, (n, 3)).astype(dt)
    for i in range(0, n, 3):
        u[i, rng.integers(3)] = 0
    u[5] = 0; a[7] = 0
    cols = lambda m: tuple(m[:, i] for i in range(3))
    with np.errstate(all="ignore"):
        f, sp, ps, pb = C.seg_box(cols(a), cols(u), cols(he), dt)
    assert ((sp >= 0) & (sp <= 1)).all()
    for i in range(n):
        A, U, HE = (X.vec([float(x) for x in v[i]]) for v in (a, u, he))
        ex = exact_seg_box_d2(A, U, HE)
        band = Q(X.BAND_EPS * X.EPS[BITS[dt]] * float(np.abs(a[i]).max() + np.abs(u[i]).max() + he[i].max()))
        dist = X.sqrt_q(ex)
        assert within(X.q(float(f[i])), dist + band) and within(ex, X.q(float(np.sqrt(f[i]))) + band), i


# ---- cores crossing: the contact separates the shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_cores_crossing_contact_separates_exactly(dt):
    """A capsule spawned inside a wall: translating it by (penetration + band) normal leaves the exact shapes disjoint, by (penetration - band)
    normal leaves them intersecting."""
    rng = np.random.default_rng(17)
    seen = 0
    for k in range(60):
        item = (CUBOID, list(rng.uniform(0.4, 1.5, 3)), list(rng.uniform(-1, 1, 3)), I if k % 3 == 0 else list(random_unit_quats(rng, 1)[0]))
        r, h = float(rng.uniform(0.05, 0.5)), float(rng.uniform(0.2, 2.0))
        pos = list(np.asarray(item[2]) + rng.uniform(-0.3, 0.3, 3) * np.asarray(item[1]))
        rot = list(random_unit_quats(rng, 1)[0]) if k % 4 else I
        s = snapshot([item], dt)
        l = C.contact_lists(s, rcc(1), [[r, h, 0]], [pos], [rot], 0.0)[0]
        cap, col = Capsule(pos, rot, r, h, dt), collider(*item, dt)
        assert cap.core_d2(col) == 0 and len(l) == 1
        pen, n = X.q(float(l[0]["penetration"])), X.vec([float(x) for x in l[0]["normal"]])
        band = band_of(dt, cap, col, float(pen))
        assert pen >= cap.r
        assert not within(cap.core_d2(col, X.scale(n, pen + band)), cap.r), k
        assert within(cap.core_d2(col, X.scale(n, pen - band)), cap.r), k
        # anchor1 on the capsule's surface, anchor2 on the box's supporting plane of the normal
        a1 = X.add(cap.pos, X.vec([float(x) for x in l[0]["anchor1"]]))
        assert abs(X.sqrt_q(exact_seg_point_d2(cap.a, X.sub(cap.b, cap.a), a1)) - cap.r) <= 8 * band
        seen += 1
    assert seen == 60


# ---- h == 0 is the Ball query --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_zero_length_capsule_equals_the_ball_query(dt):
    rng = np.random.default_rng(23)
    items = random_colliders(rng, 14)
    s = snapshot(items, dt)
    cols = [collider(*it, dt) for it in items]
    # queries whose exact gap to every collider is not within band of zero (asserted below: no case is left out)
    qs = []
    while len(qs) < 80:
        r = float(dt(rng.uniform(0.1, 0.8))); pos = [float(dt(x)) for x in rng.uniform(-3.5, 3.5, 3)]; rot = list(random_unit_quats(rng, 1)[0])
        cap = Capsule(pos, rot, r, 0.0, dt)
        gaps = []
        for col in cols:
            d = X.sqrt_q(cap.core_d2(col)) - cap.r - (col.he[0] if col.shape == BALL else 0)
            gaps.append(abs(d) > band_of(dt, cap, col))
        if all(gaps):
            qs.append((r, pos, rot))
    n = len(qs)
    he = np.array([[q[0], 0.0, 7.0] for q in qs]); pos = np.array([q[1] for q in qs]); rot = np.array([q[2] for q in qs])
    for i, (r, p, ro) in enumerate(qs):
        cap = Capsule(p, ro, r, 0.0, dt)
        for col in cols:
            gap = X.sqrt_q(cap.core_d2(col)) - cap.r - (col.he[0] if col.shape == BALL else 0)
            assert abs(gap) > band_of(dt, cap, col)
    balls = np.full(n, BALL, np.uint8)
    # intersections: the same ids and counts
    a = C.shape_intersections(s, rcc(n), he, pos, rot, 14)
    b = S.shape_intersections(s, balls, he, pos, rot, 14)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].sum() >= 30
    # casts: the same hit sets, distances within band
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        ch, ct, _, _, cn, _ = C.cast_pairs(s, rcc(n), he, pos, rot, d)
        bh, bt, _, _, bn, _ = CA.cast_pairs(s, balls, he, pos, rot, d)
    both = ch & bh
    scale = np.abs(pos).max(1)[:, None] + 1.0 + np.array([np.abs(it[2]).max() + max(it[1]) for it in items])[None, :] + np.maximum(ct, bt)
    tol = X.BAND_EPS * np.finfo(dt).eps * scale
    assert np.array_equal(ch, bh) and both.sum() >= 50
    assert (np.abs(ct - bt)[both] <= tol[both]).all()
    # the normals: each is (centre at the impact - core point) / its length, the length being r + r_c (a ball collider) or r (a cuboid); the two
    # impact centres differ by at most |ct - bt| <= band along d and each is within band of exact, so the quotients differ by at most
    # 2 * (band + band) / length
    moving = both & (ct > 0) & (bt > 0)
    length = he[:, :1] + np.array([it[1][0] if it[0] == BALL else 0.0 for it in items])[None, :]
    ntol = 4 * tol / length
    assert moving.sum() >= 30 and all((np.abs(cn[j] - bn[j])[moving] <= ntol[moving]).all() for j in range(3))
    # contacts at a prediction of 0.3: the same colliders; penetration and normal agree
    with np.errstate(all="ignore"):
        cl = C.contact_lists(s, rcc(n), he, pos, rot, 0.3)
        bl = CR.contact_lists(s, balls, he, pos, rot, 0.3)
    pairs = 0
    for x, y, p, r in zip(cl, bl, pos, he[:, 0]):
        # the Ball query has no contact where the ball's centre is inside a cuboid; the capsule's segment rule answers those
        inside = [c for c in x["collider"] if c not in y["collider"]]
        for c in inside:
            assert items[c][0] == CUBOID and all(abs(v) <= h for v, h in zip(collider(*items[c], dt).local(X.vec([float(dt(v)) for v in p])), collider(*items[c], dt).he))
        keep = np.isin(x["collider"], y["collider"])
        assert np.array_equal(x["collider"][keep], y["collider"])
        cs = y["collider"]
        band = X.BAND_EPS * np.finfo(dt).eps * (np.abs(p).max() + r + np.array([np.abs(items[c][2]).max() + max(items[c][1]) for c in cs]) + 0.3)
        assert (np.abs(x["penetration"][keep] - y["penetration"]) <= band).all()
        # the normal is (centre - core point) / dist with dist = r + r_c - penetration >= r - 0.3's worth of gap: two points within band each
        dist = np.maximum(r + np.array([items[c][1][0] if items[c][0] == BALL else 0.0 for c in cs]) - y["penetration"].astype(float), band)
        assert (np.abs(x["normal"][keep] - y["normal"]) <= (4 * band / dist)[:, None]).all()
        pairs += keep.sum()
    assert pairs >= 40


# ---- padding, nearest-k, layout and validity ------------------------------------------------------------------------------------------------------------
def padding_scenes(dt):
    """The compound scene of tests/test_spatial_casts_cpu.py (bodies with child colliders) and its far scene around 10^3, then two plain ones."""
    yield "compound", R.Snapshot(*compound_scene(seed=3, n_bodies=40), dt)
    yield "far compound", R.Snapshot(*SC.far_scene(7, n_bodies=24, spread=10.0, centre=(3000.0, -2000.0, 1000.0)), dt)
    rng = np.random.default_rng(31)
    yield "near", snapshot(random_colliders(rng, 30), dt)
    yield "around 1e3", snapshot(random_colliders(rng, 30, centre=(1000.0, -2000.0, 1500.0)), dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_padding_property_on_the_leaf_boxes(dt):
    """DESIGN.md 4.4.6, pair by pair: for every (capsule cast, collider) hit the cast ray's entry into that collider's leaf box grown by the
    capsule's padded half widths is <= the computed distance; and for every intersecting pair the padded boxes overlap."""
    for name, s in padding_scenes(dt):
        rng = np.random.default_rng(5)
        he, pos, rot, d, _ = aimed_casts(rng, np.stack(s.pos, 1).astype(float), 200)
        with np.errstate(all="ignore"):
            hit, toi, _, _, _, ok = C.cast_pairs(s, rcc(200), he, pos, rot, d)
            with C.patched():
                _, hev, posv, rotv, dv, mdv = CA.cast_valid(rcc(200), he, pos, rot, d, np.full(200, np.inf), dt)
                centre_q, hw = CA.cast_box(rcc(200), hev, posv, rotv, dt)
                pos2 = (pos + d * 3.0).astype(dt)          # poses near the colliders, for k_sp_shapes' box test
                qlo, qhi = S.query_shape_aabb(rcc(200), hev, pos2, rotv, dt)
            lo, hi = R.leaf_boxes(s)
            q = lambda t: tuple(x[:, None] for x in t)
            col = lambda t: tuple(x[None, :] for x in t)
            entry = CA.node_entry(q(centre_q), q(hw), tuple(dv[:, i][:, None] for i in range(3)), col(lo), col(hi), mdv[:, None], dt)
            ids, cnt = C.shape_intersections(s, rcc(200), he, pos2, rot, s.n)
        assert ok.all() and hit.sum() > 200 and (hit & (toi > 0)).sum() > 100, name
        assert not (hit & (entry > toi)).any(), f"{name}: {(hit & (entry > toi)).sum()} hits lie behind their leaf box's entry"
        # every intersecting pair's padded boxes overlap (k_sp_shapes' node test at the leaf)
        assert cnt.sum() >= 50, name
        for i in range(200):
            for c in ids[i, :cnt[i]]:
                assert all(lo[k][c] <= qhi[k][i] and hi[k][c] >= qlo[k][i] for k in range(3)), (name, i, c)


@pytest.mark.parametrize("dt", DTYPES)
def test_nearest_k_is_a_prefix_of_the_full_list(dt):
    rng = np.random.default_rng(41)
    items = random_colliders(rng, 20, spread=2.0)
    s = snapshot(items, dt)
    he, pos, rot, d, _ = aimed_casts(rng, items, 60)
    closest, many = C.cast_queries(s, rcc(60), he, pos, rot, d, (1, 3, 20))
    full, cnt = many[20]
    assert (cnt >= 3).sum() >= 10 and cnt.max() <= 20
    for k in (1, 3):
        h, c = many[k]
        assert np.array_equal(c, cnt) and h.tobytes() == np.ascontiguousarray(full[:, :k]).tobytes()
    assert closest.tobytes() == np.ascontiguousarray(full[:, 0]).tobytes()
    for row, c in zip(full, cnt):
        assert (np.diff(row["distance"][:c]) >= 0).all() and (row["collider"][c:] == MISS).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_layout_and_validity(dt):
    items = [BOX, BALL_C]
    s = snapshot(items, dt)
    n = 9
    shape = rcc(n)
    he = np.tile([0.4, 0.5, np.nan], (n, 1))          # z is not read: a NaN there is fine
    pos = np.tile([0.3, 1.0, -0.4], (n, 1)); rot = np.tile(I, (n, 1))
    he[1, 0] = -0.1; he[2, 1] = -0.1; he[3, 0] = np.nan; he[4, 1] = np.inf; pos[5, 0] = np.inf; rot[6, 3] = np.nan
    shape[7] = 2                                        # kind 2 stays invalid as a query shape
    he[8] = [0.0, 0.0, 0.0]; pos[8] = [0.1, -0.2, 0.05]  # a point (r = h = 0) inside the box and the ball: valid
    with np.errstate(all="ignore"):
        ok = C.shape_valid(shape, he, pos, rot, dt)[0]
        ids, cnt = C.shape_intersections(s, shape, he, pos, rot, 2)
        closest, _ = C.cast_queries(s, shape, he, pos, rot, np.tile([0, -1.0, 0], (n, 1)))
        lists = C.contact_lists(s, shape, he, pos, rot, 0.1)
    assert list(ok) == [True] + [False] * 7 + [True]
    assert cnt[0] == 2 and cnt[8] == 2 and not cnt[1:8].any() and (ids[1:8] == MISS).all()
    assert closest["collider"][0] != MISS and (closest["collider"][1:8] == MISS).all() and closest[1:8].tobytes() == closest[1:2].tobytes() * 7
    assert len(lists[0]) == 2 and all(len(l) == 0 for l in lists[1:8]) and len(lists[8]) == 2
    # a negative or non-finite prediction, a non-finite direction and a NaN max_distance: count 0 / a miss
    assert all(len(l) == 0 for l in C.contact_lists(s, rcc(3), he[:3] * 0 + [0.4, 0.5, 0], pos[:3], rot[:3], [-1.0, np.nan, np.inf]))
    with np.errstate(all="ignore"):
        c2, _ = C.cast_queries(s, rcc(2), he[:1].repeat(2, 0), pos[:2], rot[:2], [[0, np.nan, 0], [0, -1, 0]], max_distance=[1.0, np.nan])
    assert (c2["collider"] == MISS).all()
    # the patch does not outlive a call: the Ball / Cuboid references are themselves again
    assert S.shape_valid is C._orig_shape_valid and CA.cast_pairs is C._orig_cast_pairs and CR.contact_lists is C._orig_contact_lists
