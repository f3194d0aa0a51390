"""CPU: the capsule collider's reference (tests/capsule_collider_reference.py, the numpy restatement of include/avian_mi355x.h "capsule colliders")
against geometry that does not share its algorithm, and the oracle-hosted capsule scene whose coverage the GPU closed-loop test relies on."""
import numpy as np
import pytest

import capsule_collider_reference as CC
from helpers import F, oracle_lib, random_unit_quats

CUB, BALL, CAP = CC.SHAPE_CUBOID, CC.SHAPE_BALL, CC.SHAPE_CAPSULE
COMBOS = [(CAP, BALL), (BALL, CAP), (CAP, CUB), (CUB, CAP), (CAP, CAP)]
N_SAMPLES = 2001


# ---- exact geometry in float64 that shares nothing with the reference's algorithm -----------------------------------------------------------
def qrot(q, v):
    u = q[..., :3]
    return v + 2.0 * np.cross(u, np.cross(u, v) + q[..., 3:4] * v)


def point_segment(p, a, b):
    d = b - a
    dd = (d * d).sum(-1)
    t = np.clip(((p - a) * d).sum(-1) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
    return np.linalg.norm(p - (a + d * t[..., None]), axis=-1)


def point_box(p, he):
    return np.linalg.norm(p - np.clip(p, -he, he), axis=-1)


def core_distance(kind, he, pos, rot, p):
    """Exact distance of the world points p [k, 3] to the core of one shape (a ball's centre, a capsule's segment, the cuboid itself)."""
    local = qrot(np.array([-rot[0], -rot[1], -rot[2], rot[3]]), p - pos)
    if kind == BALL:
        return np.linalg.norm(local, axis=-1)
    if kind == CAP:
        return point_segment(local, np.array([0.0, -he[1], 0.0]), np.array([0.0, he[1], 0.0]))
    return point_box(local, he)


def radius(kind, he):
    return 0.0 if kind == CUB else float(he[0])


def sampled_core_distance(k1, he1, p1, r1, k2, he2, p2, r2):
    """(min over N samples of one shape's core of the exact distance to the other's core, the sampling bound |u| / (2 (N - 1))).  The sampled core
    is a capsule's segment (a ball's core is one point: no sampling error)."""
    if k1 != CAP:
        k1, he1, p1, r1, k2, he2, p2, r2 = k2, he2, p2, r2, k1, he1, p1, r1
    t = np.linspace(-1.0, 1.0, N_SAMPLES)[:, None]
    seg = p1 + qrot(r1, t * np.array([0.0, he1[1], 0.0]))
    return core_distance(k2, he2, p2, r2, seg).min(), 2.0 * he1[1] / (2.0 * (N_SAMPLES - 1))


def segment_crosses_box(he_c, p_c, r_c, he_b, p_b, r_b):
    """Exact slab clip of the capsule's segment against the box: do the cores intersect?"""
    inv = np.array([-r_b[0], -r_b[1], -r_b[2], r_b[3]])
    a = qrot(inv, p_c + qrot(r_c, np.array([0.0, -he_c[1], 0.0])) - p_b); b = qrot(inv, p_c + qrot(r_c, np.array([0.0, he_c[1], 0.0])) - p_b)
    lo, hi = 0.0, 1.0
    for i in range(3):
        d = b[i] - a[i]
        if d == 0.0:
            if abs(a[i]) > he_b[i]:
                return False
            continue
        t1, t2 = sorted(((-he_b[i] - a[i]) / d, (he_b[i] - a[i]) / d))
        lo, hi = max(lo, t1), min(hi, t2)
    return lo <= hi


def random_pairs(rng, k1, k2, n):
    """Random poses from far apart to deep overlap."""
    def he(kind):
        h = rng.uniform(0.1, 1.2, (n, 3))
        if kind == CAP:
            h[:, 0] = rng.uniform(0.05, 0.5, n); h[:, 2] = 0.0
        return h
    sep = rng.uniform(0.0, 3.0, (n, 1)) * random_unit_quats(rng, n)[:, :3]
    base = rng.uniform(-5, 5, (n, 3))
    return (np.full(n, k1), he(k1), base, random_unit_quats(rng, n), np.full(n, k2), he(k2), base + sep, random_unit_quats(rng, n), rng.uniform(0.0, 0.3, n))


def constructed_pairs():
    """The cases the GPU pair test lists, float64 (shape1, he1, pos1, rot1, shape2, he2, pos2, rot2, prediction) rows."""
    I = [0.0, 0.0, 0.0, 1.0]
    s = np.sqrt(0.5)
    Z90 = [0.0, 0.0, s, s]          # local y -> world -x: a capsule lying along x
    X90 = [s, 0.0, 0.0, s]          # local y -> world z
    tilt = lambda a: [0.0, 0.0, np.sin((np.pi / 2 + a) / 2), np.cos((np.pi / 2 + a) / 2)]
    box, capsule = [1.0, 0.5, 1.0], [0.25, 0.6, 0.0]
    rows = []
    add = lambda *r: rows.append(r)
    for other, heo in ((CUB, box), (BALL, [0.4, 0, 0]), (CAP, capsule)):
        for hc in ([0.25, 0.0, 0.0], [0.0, 0.6, 0.0], [0.0, 0.0, 0.0]):                      # h = 0, r = 0, both 0
            add(CAP, hc, [0.2, 0.9, 0.1], Z90, other, heo, [0, 0, 0], I, 0.1)
            add(other, heo, [0, 0, 0], I, CAP, hc, [0.2, 0.9, 0.1], Z90, 0.1)
    for rot in (Z90, tilt(1e-3)):                                                           # parallel to a box face: resting and tilted by 1e-3
        add(CAP, capsule, [0.1, 0.5 + 0.25, 0.2], rot, CUB, box, [0, 0, 0], I, 0.05)
        add(CUB, box, [0, 0, 0], I, CAP, capsule, [0.1, 0.5 + 0.25, 0.2], rot, 0.05)
        add(CAP, capsule, [0.9, 0.5 + 0.2, 0.2], rot, CUB, box, [0, 0, 0], I, 0.05)        # overhanging the face's edge: clipped
    add(CAP, capsule, [1.0 + 0.15, 0.5 + 0.15, 0.0], X90, CUB, box, [0, 0, 0], I, 0.05)     # parallel to a box edge
    add(CUB, box, [0, 0, 0], I, CAP, capsule, [1.0 + 0.15, 0.5 + 0.15, 0.0], X90, 0.05)
    add(CAP, [0.1, 2.0, 0.0], [0.1, 0.0, 0.2], I, CUB, box, [0, 0, 0], I, 0.0)              # the segment pierces the box
    add(CUB, box, [0, 0, 0], I, CAP, [0.1, 2.0, 0.0], [0.1, 0.0, 0.2], list(np.array([0.1, 0.0, 0.05, 0.99]) / np.linalg.norm([0.1, 0.0, 0.05, 0.99])), 0.0)
    add(CAP, [0.1, 0.5, 0.0], [0.3, 1.0, 0.2], I, CUB, box, [0, 0, 0], I, 0.0)              # a segment end exactly on a face
    add(CUB, box, [0, 0, 0], I, CAP, [0.1, 0.5, 0.0], [0.3, 1.0, 0.2], I, 0.0)
    for rot2 in (I, [0.0, 0.0, 1.0, 0.0]):                                                  # parallel / anti-parallel capsules
        for dy in (0.0, 0.7, 1.45):                                                         # full, partial, no overlap
            add(CAP, capsule, [0, 0, 0], I, CAP, [0.2, 0.6, 0.0], [0.4, dy, 0.0], rot2, 0.05)
    add(CAP, capsule, [0, 0, 0], I, CAP, capsule, [0.0, 0.1, 0.45], Z90, 0.05)              # crossed
    add(CAP, capsule, [0, 0, 0], I, CAP, capsule, [0, 0, 0], I, 0.05)                        # coincident cores
    add(CAP, capsule, [0, 0, 0], I, CAP, capsule, [0, 0.3, 0], I, 0.05)                      # collinear, overlapping
    add(CAP, capsule, [0, 0, 0], I, BALL, [0.3, 0, 0], [0.0, 0.25, 0.0], I, 0.05)           # a ball's centre on the segment
    add(BALL, [0.3, 0, 0], [0.0, 0.25, 0.0], I, CAP, capsule, [0, 0, 0], I, 0.05)
    add(CAP, capsule, [0, 0, 0], I, BALL, [0.25, 0, 0], [1.0, 0.0, 0.0], I, 0.5)            # prediction exactly at the acceptance boundary: 1.0 <= (0.25 + 0.25) + 0.5
    add(CAP, capsule, [0, 0, 0], I, CUB, box, [0.0, -1.25, 0.0], X90, 0.5)                   # 0.75 <= 0.25 + 0.5
    add(CAP, capsule, [0, 0, 0], I, CAP, capsule, [1.0, 0.0, 0.0], I, 0.5)
    for bad in (np.nan, np.inf):                                                            # non-finite poses
        add(CAP, capsule, [bad, 0, 0], I, CUB, box, [0, 0, 0], I, 0.05)
        add(CUB, box, [0, 0, 0], I, CAP, capsule, [0, 0.7, 0], [bad, 0, 0, 1], 0.05)
        add(CAP, capsule, [0, bad, 0], I, BALL, [0.3, 0, 0], [0, 0, 0], I, 0.05)
        add(CAP, capsule, [0, 0, 0], [0, bad, 0, 1], CAP, capsule, [0.3, 0, 0], I, 0.05)
    cols = list(zip(*rows))
    return (np.array(cols[0]), np.array(cols[1], np.float64), np.array(cols[2], np.float64), np.array(cols[3], np.float64),
            np.array(cols[4]), np.array(cols[5], np.float64), np.array(cols[6], np.float64), np.array(cols[7], np.float64), np.array(cols[8], np.float64))


def _swap(b):
    return (b[4], b[5], b[6], b[7], b[0], b[1], b[2], b[3], b[8])


def _check_against_brute_force(batch, label):
    """Test 1's properties for every row with finite inputs."""
    dt = np.float64
    m, ms = CC.manifolds(*batch, dt), CC.manifolds(*_swap(batch), dt)
    s1, he1, p1, r1, s2, he2, p2, r2, pred = batch
    TOL = 1e-9   # positions are O(10), float64: witnesses agree to ~1e-15 relative; 1e-9 leaves six decades
    n_manifolds = 0
    for i in range(len(s1)):
        if not (np.isfinite(p1[i]).all() and np.isfinite(p2[i]).all()):
            assert m["point_count"][i] == 0, f"{label} row {i}: a non-finite position has no manifold"
            continue
        if not (np.isfinite(r1[i]).all() and np.isfinite(r2[i]).all()):
            continue   # (make_isometry reads a non-finite rotation as the identity, as for every other pair kind: whatever comes out is compared on the GPU bit for bit)
        k1, k2 = int(s1[i]), int(s2[i])
        radii = radius(k1, he1[i]) + radius(k2, he2[i])
        d_s, bound = sampled_core_distance(k1, he1[i], p1[i], r1[i], k2, he2[i], p2[i], r2[i])
        crossing = CUB in (k1, k2) and (segment_crosses_box(he1[i], p1[i], r1[i], he2[i], p2[i], r2[i]) if k1 == CAP else segment_crosses_box(he2[i], p2[i], r2[i], he1[i], p1[i], r1[i]))
        pc = int(m["point_count"][i])
        assert pc == ms["point_count"][i], f"{label} row {i}: swapped point count"
        if pc == 0:
            # nothing within the prediction distance (the true distance is at least d_s - bound), or cores that touch without a direction
            assert d_s - radii > pred[i] - bound - 1e-9 or (d_s <= bound + 1e-9 and CUB not in (k1, k2)), f"{label} row {i}: no manifold at core distance {d_s}"
            continue
        n_manifolds += 1
        nrm = m["normal"][i]
        assert abs(np.linalg.norm(nrm) - 1.0) < 1e-12
        pen = m["penetration"][i, :pc]
        deepest = pen.max()
        assert np.allclose(ms["normal"][i], -nrm, atol=TOL, rtol=0), f"{label} row {i}: swapping the shapes negates the normal"
        assert abs(ms["penetration"][i, :pc].max() - deepest) <= 1e-12, f"{label} row {i}: swapping keeps the depth"
        if crossing:
            # the cores intersect (exact slab clip): the sampled distance is 0 and carries no depth; the definition's depth is the smallest overlap + r >= r
            assert deepest >= radii - 1e-12, f"{label} row {i}: crossing cores penetrate by at least the radius"
        else:
            assert d_s - bound - radii - 1e-12 <= -deepest <= d_s - radii + 1e-12, f"{label} row {i}: depth {deepest} vs sampled core distance {d_s}"
        rr1, rr2 = radius(k1, he1[i]), radius(k2, he2[i])
        for k in range(pc):
            dist = -pen[k]
            mid = p1[i] + m["anchor1"][i, k]
            assert np.allclose(m["anchor2"][i, k], m["anchor1"][i, k] + (p1[i] - p2[i]), atol=1e-12, rtol=0)
            surf1, surf2 = mid - nrm * dist * 0.5, mid + nrm * dist * 0.5
            # shape 1: the point is a point of its core displaced by its radius along the normal (on the surface where the core point's
            # outward direction is the normal: always for the deepest point; a clipped inner point of a tilted capsule lies r cos(tilt) from the axis)
            # (crossing cores with the cuboid as shape 1: the definition's point is the segment's end projected onto the box's supporting PLANE of the normal)
            if crossing and k1 == CUB:
                ln = qrot(np.array([-r1[i][0], -r1[i][1], -r1[i][2], r1[i][3]]), nrm); lp = qrot(np.array([-r1[i][0], -r1[i][1], -r1[i][2], r1[i][3]]), surf1 - p1[i])
                assert abs(ln @ lp - np.abs(ln) @ he1[i]) <= TOL, f"{label} row {i} point {k}: not on the box's supporting plane"
            else:
                assert core_distance(k1, he1[i], p1[i], r1[i], (surf1 - nrm * rr1)[None])[0] <= TOL, f"{label} row {i} point {k}: not on shape 1"
            if not crossing:
                # shape 2's supporting feature: the point's own depth along the normal ends on shape 2's core displaced by its radius
                assert core_distance(k2, he2[i], p2[i], r2[i], (surf2 + nrm * rr2)[None])[0] <= TOL, f"{label} row {i} point {k}: depth along the normal"
        if pc == 2:
            assert (m["feature_id1"][i, 0], m["feature_id2"][i, 0]) != (m["feature_id1"][i, 1], m["feature_id2"][i, 1]), "the two points have distinct ids"
        # the normal points from shape 1 to shape 2: stepping the deepest point's core point along it approaches shape 2's core
        if not crossing:
            k = int(np.argmax(pen))
            core1 = p1[i] + m["anchor1"][i, k] + nrm * pen[k] * 0.5 - nrm * rr1
            d0 = core_distance(k2, he2[i], p2[i], r2[i], core1[None])[0]
            assert d0 < 2e-3 or core_distance(k2, he2[i], p2[i], r2[i], (core1 + nrm * 1e-3)[None])[0] < d0, f"{label} row {i}: the normal's direction"
    return n_manifolds


@pytest.mark.parametrize("k1,k2", COMBOS)
def test_reference_against_sampled_geometry(k1, k2):
    """Test 1: ~2000 random pairs per kind combination in float64.  The core distance comes from N samples of the capsule's segment with exact
    point-box / point-segment distances; distance is 1-Lipschitz in the point, so the true minimum is within |u| / (2 (N - 1)) below the sampled one."""
    rng = np.random.default_rng(100 + 10 * k1 + k2)
    assert _check_against_brute_force(random_pairs(rng, k1, k2, 2000), f"{k1}-{k2}") > 300


def test_reference_on_the_constructed_cases():
    b = constructed_pairs()
    assert _check_against_brute_force(b, "constructed") > 25
    m = CC.manifolds(*b, np.float64)
    s1, s2 = b[0], b[4]
    two = m["point_count"] == 2
    assert (two & ((s1 == CUB) | (s2 == CUB))).sum() >= 4 and (two & (s1 == CAP) & (s2 == CAP)).sum() >= 3, "resting capsules get two points"


def test_reference_aabb_contains_the_capsule_and_is_tight():
    """Test 2: 10^4 surface points per capsule lie inside the reference box, and the box touches the capsule within 1e-12 along each axis (the
    support of a capsule along e_i is |R (0, h, 0)|_i + r: compared with the exact support, not with the samples)."""
    rng = np.random.default_rng(7)
    for _ in range(6):
        r, h = rng.uniform(0.05, 0.5), rng.uniform(0.0, 1.5)
        pos, rot = rng.uniform(-5, 5, 3), random_unit_quats(rng, 1)[0]
        col = lambda a: tuple(np.array([x]) for x in a)
        mn, mx = CC.aabb(col([r, h, 0.0]), col(pos), col(rot), np.float64)
        mn, mx = np.array([x[0] for x in mn]), np.array([x[0] for x in mx])
        d = rng.normal(size=(10000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        core = np.array([0.0, 1.0, 0.0]) * np.where(d[:, 1:2] >= 0, h, -h)     # the support point of the segment along d (local)
        surf = pos + qrot(rot, core) + qrot(rot, d) * r                           # NOT the support mapping of the world direction: just surface points
        assert (surf >= mn - 1e-12).all() and (surf <= mx + 1e-12).all()
        axis = qrot(rot, np.array([0.0, h, 0.0]))
        assert np.allclose(mx - pos, np.abs(axis) + r, atol=1e-12, rtol=0) and np.allclose(pos - mn, np.abs(axis) + r, atol=1e-12, rtol=0)


@pytest.mark.parametrize("bits", [32, 64])
def test_h_zero_is_a_ball(bits):
    """Test 3: a capsule with h = 0 against a Ball or a Cuboid, in either order, equals the oracle's Ball manifold (avo_contact_manifolds, kind 1).
    Both compute the same centre-to-core vector d = c - proj(c) and penetration = radii - |d|, the capsule in the capsule's (ball) or the cuboid's
    frame, the oracle in shape 1's or the cuboid's: each is a rotation of the same world vector, so |d| differs by the rounding of two quaternion
    rotations, a few eps |d|, and the penetration by the same amount plus an eps of the radii -- hence 4 eps of the operand magnitudes mag = |c1 - c2| + radii
    + extents for the penetration, the factor 4 for the chained rotations; the normal is d / |d|, so the same error of d is divided by |d|: 4 eps mag / |d|.  Excluded: a ball's centre inside the cuboid or on
    the other ball's centre, where contact_manifold_convex_ball / ball_ball have their own rules (no manifold / a fixed normal) and the capsule has its
    crossing-core rule."""
    dt = np.float32 if bits == 32 else np.float64
    eps = float(np.finfo(dt).eps)
    rng = np.random.default_rng(5)
    n = 400
    w = F.World(oracle_lib(), F.default_config(bits))
    checked = 0
    for other in (BALL, CUB):
        for order in (0, 1):
            heo = rng.uniform(0.2, 1.0, (n, 3))
            hc = np.zeros((n, 3)); hc[:, 0] = rng.uniform(0.1, 0.5, n)
            pc, rc = rng.uniform(-3, 3, (n, 3)), random_unit_quats(rng, n)
            po = pc + rng.uniform(0.6, 1.8, (n, 1)) * random_unit_quats(rng, n)[:, :3]
            ro = random_unit_quats(rng, n)
            pred = np.full(n, 0.2)
            a = (np.full(n, CAP), hc, pc, rc); b = (np.full(n, other), heo, po, ro)
            ab = (a + b) if order == 0 else (b + a)
            cap = CC.manifolds(*ab, pred, dt)
            as_ball = tuple(np.where(np.asarray(x) == CAP, BALL, x) if i in (0, 4) else x for i, x in enumerate(ab))
            ball = w.contact_manifolds(*as_ball, pred)
            # centre inside the cuboid: excluded (see above); exact test in float64
            inside = np.zeros(n, bool)
            if other == CUB:
                local = qrot(np.concatenate([-ro[:, :3], ro[:, 3:]], axis=1), pc - po)
                inside = (np.abs(local) <= heo).all(1)
            mag = np.linalg.norm(pc - po, axis=1) + hc[:, 0] + heo.max(1)
            both = (cap["point_count"] == 1) & (ball["point_count"] == 1) & ~inside
            # the acceptance boundaries differ by rounding only: a disagreement on the count needs the gap within the same tolerance of the prediction
            differ = (cap["point_count"] != ball["point_count"]) & ~inside
            if other == CUB:
                gap = point_box(qrot(np.concatenate([-ro[:, :3], ro[:, 3:]], axis=1), pc - po), heo) - hc[:, 0]
            else:
                gap = np.linalg.norm(pc - po, axis=1) - hc[:, 0] - heo[:, 0]
            assert np.all(np.abs(gap[differ] - pred[differ]) <= 4 * eps * mag[differ]), "the counts differ away from the acceptance boundary"
            core = gap + hc[:, 0] + (heo[:, 0] if other == BALL else 0.0)   # |d|: the centre's distance to the other core
            assert np.all(np.abs(cap["normal"][both].astype(np.float64) - ball["normal"][both]) <= (4 * eps * mag / core)[both, None]), "normal"
            assert np.all(np.abs(cap["penetration"][both, 0].astype(np.float64) - ball["penetration"][both, 0]) <= 4 * eps * mag[both]), "penetration"
            checked += int(both.sum())
    assert checked > 400


# ---- the oracle-hosted scene ------------------------------------------------------------------------------------------------------------------
SCENE = dict(n=24, seed=15, n_boxes=8, n_balls=4)   # (the seed: of 1..16 the one whose capsules end lowest on the oracle; several others leave a capsule lying across another, above the bound)
STEPS = 40           # the closed-loop comparison of tests/test_gpu_capsule_colliders.py runs these steps


def hosted_world(lib, bits, scene_kw=SCENE, sleeping=False):
    """The capsule_drop scene with its capsules held as AVN_SHAPE_HOST and answered by the reference callbacks."""
    from avian_amd import scenes
    sc = scenes.capsule_drop(**scene_kw)
    cols = sc.collider_kwargs()
    host = CC.CapsuleHost(cols["entity_index"], sc.shape, sc.half_extents)
    cols["shape"] = np.where(sc.shape == CAP, F.SHAPE_HOST, sc.shape).astype(np.uint8)
    w = F.World(lib, F.default_config(bits, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction, restitution=0.0)
    w.host_shapes_set(host.aabb, host.manifolds)
    w.pipeline_enable()
    if sleeping:
        w.sleeping_enable()
    return w, host, sc


class RowKinds:
    """Which contact rows hold a capsule: the colliders of every row id, collected from the broad phase's new pairs step by step."""

    def __init__(self, sc):
        self.capsule = set(int(e) for e in sc.collider_kwargs()["entity_index"][sc.shape == CAP])
        self.rows = {}

    def after_step(self, w):
        for p, i in zip(w.pairs_get(), w.pipeline_new_pair_ids()):
            self.rows[int(i)] = int(p["collider1"]) in self.capsule or int(p["collider2"]) in self.capsule

    def warm_start_share(self, w):
        """(the share of touching capsule rows whose first point carries an accumulated normal impulse, their number)."""
        _, handles = w.pipeline_handles()
        ids = np.sort(handles)
        rows = w.contacts_download(ids)
        sel = (rows["point_count"] > 0) & np.array([self.rows[int(i)] for i in ids], bool)
        return (float((rows["normal_impulse"][sel, 0] != 0).mean()) if sel.any() else 0.0), int(sel.sum())


# Manifold queries the reference alone answered over the first STEPS steps, by pair kind (capsule-capsule and capsule-ball: those that came back with a
# point).  Observed, f32 and f64 alike: two points 72, one point 164, capsule-capsule 221, capsule-ball 37, capsule-cuboid overall 311.  The floors
# are half of that (and never below the 1 / 20 the coverage condition asks for): a change of the scene or of the definitions shows here first.
COVERAGE_FLOOR = {"capsule-cuboid, two points": 36, "capsule-cuboid, one point": 82, "capsule-capsule": 110, "capsule-ball": 18, "capsule-cuboid": 155}


@pytest.mark.parametrize("bits", [32, 64])
def test_oracle_hosted_scene_covers_every_pair_kind_and_comes_to_rest(bits):
    """Test 4: 24 capsules, 8 boxes, 4 balls and the ground on the oracle, the capsules AVN_SHAPE_HOST answered by the reference."""
    w, host, sc = hosted_world(oracle_lib(), bits)
    kinds = RowKinds(sc)
    for step in range(240):
        w.step()
        kinds.after_step(w)
        if step == STEPS - 1:
            at_steps = dict(host.kinds)
    assert not w.host_shape_errors()
    count = lambda kinds, pcs=(0, 1, 2): sum(v for (k, c), v in at_steps.items() if k == kinds and c in pcs)
    got = {"capsule-cuboid, two points": count((CUB, CAP), (2,)), "capsule-cuboid, one point": count((CUB, CAP), (1,)), "capsule-capsule": count((CAP, CAP), (1, 2)),
           "capsule-ball": count((BALL, CAP), (1,)), "capsule-cuboid": count((CUB, CAP))}
    print("manifold queries by pair kind over", STEPS, "steps:", got)
    for k, floor in COVERAGE_FLOOR.items():
        assert got[k] >= floor, f"{k}: {got[k]} queries"
    b = w.bodies_download()
    caps = sc.shape == CAP
    r = 0.25
    y = b["position"][caps, 1]
    assert np.isfinite(b["position"]).all()
    assert (y > 0.0 + r - 0.03).all(), "no capsule sank into the ground"
    assert (y < 0.0 + r + 0.45).all(), "every capsule lies on the ground or leans on a neighbour"
    assert np.median(y) < 0.0 + r + 0.05
    # the cap the GPU sanity test holds the native capsules to; observed here: 1.0 of 33 rows (f32), 1.0 of 32 (f64)
    share, touching = kinds.warm_start_share(w)
    print("warm-started share of touching capsule rows at the last step:", share, "of", touching)
    assert share >= 0.9 and touching >= 20
