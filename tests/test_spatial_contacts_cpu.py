"""CPU: the definition of avn_spatial_shape_contacts / avn_spatial_depenetrate (include/avian_mi355x_spatial.h) through its brute force
(tests/spatial_contact_reference.py: filter, AABB precondition, the CPU oracle's contact_manifolds, the last-maximum fold) -- hand-computed
contacts, the deepest-point tie, a pair the manifold test accepts and the AABB precondition rejects, known answers of the depenetration,
and the library's exports and record layouts."""
import ctypes
import os
import re

import numpy as np
import pytest

from avian_amd import spatial_query as Q
from helpers import REPO, hip_lib, random_unit_quats
import spatial_contact_reference as CR
import spatial_query_reference as R
import spatial_scenes as SC

I = [0.0, 0.0, 0.0, 1.0]
BALL, CUBOID = R.SHAPE_BALL, R.SHAPE_CUBOID
DT = {32: np.float32, 64: np.float64}


def snapshot(pos, rot, shape, he, dt):
    n = len(pos)
    cols = dict(entity_index=np.arange(10, 10 + n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=np.array(shape, np.uint8),
                half_extents=np.array(he, float))
    return R.Snapshot(SC.bodies_of(pos, rot), cols, None, dt)


def record(bits, collider, entity, penetration, normal, point, anchor1, anchor2):
    r = np.zeros((), Q.shape_contact_dtype(bits))
    r["collider"], r["entity"], r["penetration"], r["normal"], r["point"], r["anchor1"], r["anchor2"] = collider, entity, penetration, normal, point, anchor1, anchor2
    return r


def same_bits(got, want, what):
    assert got.tobytes() == want.tobytes(), f"{what}: {got} expected {want}"


# Every quantity below is dyadic, so the expected records are exact literals.  The record's normal is the NEGATION of the manifold's normal,
# component by component: where the manifold's component is +0 the record holds -0, which is what `-np.array(...)` spells out.
@pytest.mark.parametrize("bits", [32, 64])
def test_ball_over_a_cuboid_face_bit_for_bit(bits):
    s = snapshot([[0, 0, 0]], [I], [CUBOID], [[1, 1, 1]], DT[bits])
    # radius 0.5, the cuboid's top face at y = 1, a gap of 0.25: the centre at y = 1.75.  The manifold normal (shape 1 = the ball) is (0, -1, 0)
    # and the raw point sits in the middle of the gap: anchor1 = (0, -0.5, 0) + (0, -1, 0) * 0.25 / 2
    (l,) = CR.contact_lists(s, [BALL], [[0.5, 0, 0]], [[0, 1.75, 0]], [I], 0.5)
    assert len(l) == 1
    same_bits(l[0], record(bits, 0, 10, -0.25, -np.array([0.0, -1.0, 0.0]), [0, 1.125, 0], [0, -0.625, 0], [0, 1.125, 0]), "ball over a face")
    # a prediction below the gap: nothing
    (l,) = CR.contact_lists(s, [BALL], [[0.5, 0, 0]], [[0, 1.75, 0]], [I], 0.125)
    assert len(l) == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_ball_inside_a_cuboid(bits):
    s = snapshot([[0, 0, 0]], [I], [CUBOID], [[1, 1, 1]], DT[bits])
    # the ball's lower half inside the cuboid, its centre 0.25 above the face: penetration 0.25, the point halfway between the two surfaces
    (l,) = CR.contact_lists(s, [BALL], [[0.5, 0, 0]], [[0, 1.25, 0]], [I], 0.0)
    assert len(l) == 1
    same_bits(l[0], record(bits, 0, 10, 0.25, -np.array([0.0, -1.0, 0.0]), [0, 0.875, 0], [0, -0.375, 0], [0, 0.875, 0]), "ball in a face")
    # The centre itself inside the cuboid: the narrow phase's convex / ball function projects an inside centre onto itself and returns no
    # manifold (avn_narrow.h, `if (!(dist > 0)) return false`), so the query reports no contact either.  Inherited, not chosen here.
    (l,) = CR.contact_lists(s, [BALL], [[0.5, 0, 0]], [[0, 0.5, 0]], [I], 0.0)
    assert len(l) == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_two_balls(bits):
    s = snapshot([[0, 0, 0]], [I], [BALL], [[1, 0, 0]], DT[bits])
    # radii 0.5 (query, at x = 2) and 1: a gap of 0.5; ball / ball needs dist < prediction, strictly
    (l,) = CR.contact_lists(s, [BALL], [[0.5, 0, 0]], [[2, 0, 0]], [I], 1.0)
    assert len(l) == 1
    same_bits(l[0], record(bits, 0, 10, -0.5, -np.array([-1.0, 0.0, 0.0]), [1.25, 0, 0], [-0.75, 0, 0], [1.25, 0, 0]), "two balls")
    (l,) = CR.contact_lists(s, [BALL], [[0.5, 0, 0]], [[2, 0, 0]], [I], 0.5)
    assert len(l) == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_deepest_point_tie_takes_the_later_point(bits):
    # a cuboid of half extents 0.5 sunk 0.25 into the top face of a cuboid of half extents 1, both axis-aligned: four vertex contacts, all 0.25 deep
    s = snapshot([[0, 0, 0]], [I], [CUBOID], [[1, 1, 1]], DT[bits])
    q = dict(shape=[CUBOID], he=[[0.5, 0.5, 0.5]], pos=[[0, 1.25, 0]], rot=[I])
    m = CR.oracle_world(bits).contact_manifolds(q["shape"], q["he"], q["pos"], q["rot"], [CUBOID], [[1, 1, 1]], [[0, 0, 0]], [I], [0.0])
    cnt = int(m["point_count"][0])
    pen = m["penetration"][0, :cnt]
    tied = np.nonzero(pen == pen.max())[0]
    assert cnt == 4 and len(tied) == 4 and pen.max() == 0.25, "the oracle's raw list no longer holds the tie this test is about"
    assert len({tuple(a) for a in m["anchor1"][0, :cnt]}) == 4     # four different points, so the choice shows
    assert CR.deepest(pen, cnt) == tied[-1] == 3
    (l,) = CR.contact_lists(s, q["shape"], q["he"], q["pos"], q["rot"], 0.0)
    assert len(l) == 1 and l[0]["penetration"] == 0.25
    assert np.array_equal(l[0]["anchor1"], m["anchor1"][0, 3]) and not np.array_equal(l[0]["anchor1"], m["anchor1"][0, 0])
    same_bits(l[0], record(bits, 0, 10, 0.25, -np.array([0.0, -1.0, 0.0]), [0.5, 0.875, -0.5], [0.5, -0.375, -0.5], [0.5, 0.875, -0.5]), "tie")
    # the fold itself: the later of equal maxima, the first point when it is strictly the deepest
    assert CR.deepest(np.array([1.0, 2.0, 2.0, 0.5]), 4) == 2 and CR.deepest(np.array([3.0, 2.0, 2.0]), 3) == 0 and CR.deepest(np.array([1.0]), 1) == 0


def facing_corner_pairs(seed, n, p):
    """Rotated cuboid pairs whose extreme vertices along x face each other across an AABB gap of 1.01 p .. 1.3 p."""
    rng = np.random.default_rng(seed)
    r1, r2 = random_unit_quats(rng, n), random_unit_quats(rng, n)
    he1, he2 = rng.uniform(0.5, 1.5, (n, 3)), rng.uniform(0.5, 1.5, (n, 3))

    def extreme(rot, he, sx):
        q = tuple(rot[:, i] for i in range(4))
        xl = R.qrot(R.qinverse(q), (np.full(n, sx), np.zeros(n), np.zeros(n)), np.float64)
        return np.stack(R.qrot(q, tuple(np.copysign(he[:, i], xl[i]) for i in range(3)), np.float64), 1)
    v1, v2 = extreme(r1, he1, 1.0), extreme(r2, he2, -1.0)
    gap = rng.uniform(1.01, 1.3, n) * p
    p2 = np.stack([v1[:, 0] - v2[:, 0] + gap, v1[:, 1] - v2[:, 1] + rng.normal(scale=0.05, size=n), v1[:, 2] - v2[:, 2] + rng.normal(scale=0.05, size=n)], 1)
    return he1, r1, he2, p2, r2


@pytest.mark.parametrize("bits", [32, 64])
def test_a_pair_the_manifold_test_accepts_and_the_aabb_precondition_rejects(bits):
    """The SAT of two cuboids is not a distance: with two corners facing each other it accepts pairs whose AABBs, and so whose true distance, are
    further apart than the prediction.  The AABB precondition is what rejects them, which is why it belongs to the definition."""
    n, p = 2000, 0.25
    he1, r1, he2, p2, r2 = facing_corner_pairs(7, n, p)
    z = np.zeros(n, np.uint8)
    m = CR.oracle_world(bits).contact_manifolds(z, he1, np.zeros((n, 3)), r1, z, he2, p2, r2, np.full(n, p))
    accepted = np.nonzero(m["point_count"] > 0)[0]
    rejected = []
    for j in accepted[:8]:
        s = snapshot([p2[j]], [r2[j]], [CUBOID], [he2[j]], DT[bits])
        if not CR.precondition(s, [CUBOID], [he1[j]], [[0, 0, 0]], [r1[j]], [p])[0, 0]:
            (l,) = CR.contact_lists(s, [CUBOID], [he1[j]], [[0, 0, 0]], [r1[j]], p)
            assert len(l) == 0
            # with a prediction that covers the gap the same pair is a contact
            (l,) = CR.contact_lists(s, [CUBOID], [he1[j]], [[0, 0, 0]], [r1[j]], 2 * p)
            assert len(l) == 1
            rejected.append(j)
    assert rejected, "no pair accepted by the manifold test and rejected by the AABB precondition: the case is vacuous"


def plane_records(bits, entries):
    r = np.zeros(len(entries), Q.shape_contact_dtype(bits))
    for k, (normal, pen) in enumerate(entries):
        r[k]["collider"] = k; r[k]["entity"] = k; r[k]["normal"] = normal; r[k]["penetration"] = pen
    return r


@pytest.mark.parametrize("bits", [32, 64])
def test_depenetrate_known_answers(bits):
    dt = DT[bits]
    # one plane: (pen + skin) n after one pass; the second pass finds no error and ends the loop
    fx, it = CR.depenetrate(plane_records(bits, [([0, 1, 0], 0.25)]), 0.125, 1e-4, 10.0, 8, bits)
    assert [float(x) for x in fx] == [0.0, 0.375, 0.0] and it == 2 and all(type(x) is dt for x in fx)
    # two perpendicular planes: each is resolved independently
    fx, it = CR.depenetrate(plane_records(bits, [([1, 0, 0], 0.5), ([0, 0, 1], 0.25)]), 0.125, 1e-4, 10.0, 8, bits)
    assert [float(x) for x in fx] == [0.625, 0.0, 0.375] and it == 2
    # a contact beyond the rejection threshold is ignored
    fx, it = CR.depenetrate(plane_records(bits, [([1, 0, 0], 0.5), ([0, 1, 0], 4.0)]), 0.125, 1e-4, 2.0, 8, bits)
    assert [float(x) for x in fx] == [0.625, 0.0, 0.0]
    # a single pass allowed: it is counted, and the loop does not run again
    fx, it = CR.depenetrate(plane_records(bits, [([0, 1, 0], 0.25)]), 0.125, 1e-4, 10.0, 1, bits)
    assert [float(x) for x in fx] == [0.0, 0.375, 0.0] and it == 1
    # iterations = 0: zero vectors, no pass
    fx, it = CR.depenetrate(plane_records(bits, [([0, 1, 0], 0.25)]), 0.125, 1e-4, 10.0, 0, bits)
    assert [float(x) for x in fx] == [0.0, 0.0, 0.0] and it == 0
    out = CR.depenetrations(plane_records(bits, [([0, 1, 0], 0.25)] * Q.MAX_HITS)[None, :], np.array([1], np.uint32), 0.125, 1e-4, 10.0, 0, bits)
    assert out.tobytes() == bytes(out.nbytes)
    # more contacts than MAX_HITS: the flag, and only the first MAX_HITS are read
    recs = plane_records(bits, [([0, 1, 0], 0.25)] * Q.MAX_HITS)[None, :]
    out = CR.depenetrations(recs, np.array([Q.MAX_HITS + 6], np.uint32), 0.125, 1e-4, 10.0, 4, bits)
    assert out[0]["truncated"] == 1 and out[0]["count"] == Q.MAX_HITS + 6 and list(out[0]["fixup"]) == [0.0, 0.375, 0.0]


def test_depenetrate_rounds_normals_through_f32_in_f64():
    n = np.array([0.1, 0.7, 0.3]) / np.linalg.norm([0.1, 0.7, 0.3])
    recs = plane_records(64, [(n, 0.25)])
    fx, _ = CR.depenetrate(recs, 0.125, 1e-4, 10.0, 1, 64)
    n32 = n.astype(np.float32).astype(np.float64)
    assert (n32 != n).all()
    assert [float(x) for x in fx] == [float(np.float64(0.375) * c) for c in n32] and [float(x) for x in fx] != [float(np.float64(0.375) * c) for c in n]
    # the records themselves keep the full-precision normal
    assert np.array_equal(recs[0]["normal"], n)
    # in an f32 world the rounding is a no-op
    fx32, _ = CR.depenetrate(plane_records(32, [(n, 0.25)]), 0.125, 1e-4, 10.0, 1, 32)
    assert [x for x in fx32] == [np.float32(0.375) * c for c in n.astype(np.float32)]


def test_library_exports_and_record_layouts():
    dll = ctypes.CDLL(hip_lib().path)
    for name in ("avn_spatial_shape_contacts", "avn_spatial_depenetrate"):
        assert name in Q.SYMBOLS and hasattr(dll, name), f"{hip_lib().path} does not export {name}"
    assert ctypes.sizeof(Q.avn_spatial_shape_contact_f32) == 60 and ctypes.sizeof(Q.avn_spatial_shape_contact_f64) == 120
    assert Q.shape_contact_dtype(32).itemsize == 60 and Q.shape_contact_dtype(64).itemsize == 120
    for bits, c in ((32, Q.avn_spatial_shape_contact_f32), (64, Q.avn_spatial_shape_contact_f64)):
        d = Q.shape_contact_dtype(bits)
        assert all(d.fields[name][1] == getattr(c, name).offset for name, _ in c._fields_), "numpy mirror and ctypes mirror disagree"
        assert sum(getattr(c, name).size for name, _ in c._fields_) == ctypes.sizeof(c), "implicit padding in the record"
    for bits, c in ((32, Q.avn_spatial_depenetration_f32), (64, Q.avn_spatial_depenetration_f64)):
        d = Q.depenetration_dtype(bits)
        assert d.itemsize == ctypes.sizeof(c) == (24 if bits == 32 else 40)
        assert all(d.fields[name][1] == getattr(c, name).offset for name, _ in c._fields_)
    text = open(os.path.join(REPO, "include", "avian_mi355x_spatial.h")).read()
    assert re.search(r"AVN_SPATIAL_SKIP_SENSORS\s*=\s*4\b", text) and Q.SKIP_SENSORS == 4
