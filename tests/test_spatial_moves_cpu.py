"""CPU: the definitions of avn_spatial_project_velocities / avn_spatial_cast_moves / avn_spatial_move_and_slide (include/avian_mi355x_spatial.h)
through their numpy restatement (tests/spatial_move_reference.py): the reference's own check_agreement of the cone projection, hand-computed
dyadic cases compared with ==, the three outcomes of the origin-penetration rule, the pull-back's two clamps, the populations the GPU test relies
on, and the library's exports and record layouts."""
import ctypes
import math

import numpy as np
import pytest

from avian_amd import spatial_query as Q
from helpers import hip_lib
import spatial_move_reference as M
import spatial_move_scenes as MS
import spatial_query_reference as R
import spatial_scenes as SC

I = MS.I
BALL, CUBOID = R.SHAPE_BALL, R.SHAPE_CUBOID
DT = {32: np.float32, 64: np.float64}
MISS = R.MISS


def snapshot(items, dt):
    """items: (shape, half extents, position) of axis-aligned colliders, entities 10, 11, ..."""
    n = len(items)
    cols = dict(entity_index=np.arange(10, 10 + n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=np.array([i[0] for i in items], np.uint8),
                half_extents=np.array([i[1] for i in items], float))
    return R.Snapshot(SC.bodies_of([i[2] for i in items], [I] * n), cols, None, dt)


FLOOR = (CUBOID, [4, 0.5, 4], [0, -0.5, 0])          # its top is y = 0
WALL_X = (CUBOID, [0.5, 2, 4], [1.5, 2, 0])          # its face is x = 1
WALL_Z = (CUBOID, [4, 2, 0.5], [0, 2, 1.5])          # its face is z = 1
HAND = dict(delta_time=1.0, skin_width=0.125, max_depenetration_error=1e-4, penetration_rejection_threshold=0.5, depenetration_iterations=8,
            plane_similarity_dot_threshold=0.999, max_planes=20)
BALL_Q = ([BALL], [[0.5, 0, 0]], [[0, 0.75, 0]], [I])


# ---- project_velocity: velocity_project.rs's own test, transcribed ---------------------------------------------------------------------------
def dir_of(x, y, z):
    """Dir::from_xyz: normalised in f32."""
    v = np.array([x, y, z], np.float32)
    return tuple(v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


NORMALS = [dir_of(*v) for v in [(0, 0, 1), (2, 0, 1), (-2, 0, 1), (0, 2, 1), (0, -2, 1), (1.5, 1.5, 1), (1.5, -1.5, 1), (-1.5, 1.5, 1), (-1.5, -1.5, 1), (1, 1.75, 1),
                                (1, -1.75, 1), (-1, 1.75, 1), (-1, -1.75, 1), (1.75, 1, 1), (1.75, -1, 1), (-1.75, 1, 1), (-1.75, -1, 1)]]


def quasi_random_directions(count, dt):
    """QuasiRandomDirection (velocity_project.rs, 3D) in the scalar dt."""
    plastic = dt(1.32471795724475)
    inv = dt(1) / plastic
    inv_sq = inv * inv
    i, j = dt(0), dt(0)
    for _ in range(count):
        phi = dt(2) * dt(math.pi) * j
        x, y = np.cos(phi), np.sin(phi)
        z = dt(2) * i - dt(1)
        rho = np.sqrt(dt(1) - z * z)
        i, j = np.fmod(i + inv, dt(1)), np.fmod(j + inv_sq, dt(1))
        yield (rho * x, rho * y, z)


def project_velocity_bruteforce(vs, normals, dt):
    """project_velocity_bruteforce (velocity_project.rs:15-110), transcribed for a batch of velocities vs [m, 3]."""
    eps = dt(M.DOT_EPSILON)
    ns = np.array(normals, dt)
    m = len(vs)
    inside = (vs @ ns.T >= -eps).all(1)
    best, best_d2 = np.zeros((m, 3), dt), np.full(m, np.inf)
    valid = lambda p: (p @ ns.T >= -eps).all(1)

    def take(p, ok):
        nonlocal best, best_d2
        d2 = ((vs - p) ** 2).sum(1)
        ok = ok & (d2 < best_d2) & valid(p)
        best = np.where(ok[:, None], p, best); best_d2 = np.where(ok, d2, best_d2)
    for n in ns:
        nv = vs @ n
        take(vs - nv[:, None] * n, nv < -eps)
    for a in range(len(ns)):
        for b in range(a + 1, len(ns)):
            e = np.cross(ns[a], ns[b])
            e2 = e.dot(e)
            if e2 < eps:
                continue
            take(e[None, :] * ((vs @ e) / e2)[:, None], np.ones(m, bool))
    return np.where(inside[:, None], vs, np.where(np.isfinite(best_d2)[:, None], best, dt(0)))


@pytest.mark.parametrize("bits", [32, 64])
def test_check_agreement_of_the_reference(bits):
    """17 normals, the first 1000 quasi-random directions: intrusion <= DOT_EPSILON and no worse than the brute force by more than DOT_EPSILON."""
    dt = DT[bits]
    vs = np.array(list(quasi_random_directions(1000, dt)), dt)
    for n in range(1, len(NORMALS) + 1):
        sel = NORMALS[:n]
        new = np.array([M.project_velocity(v, sel, dt) for v in vs], dt)
        assert new.dtype == dt
        intrusion = -(new @ np.array(sel, dt).T)
        assert (intrusion <= M.DOT_EPSILON).all(), f"{n} normals: input {vs[np.nonzero(intrusion > M.DOT_EPSILON)[0][:1]]} still points into a plane by {intrusion.max()}"
        old = project_velocity_bruteforce(vs, sel, dt)
        worse = np.sqrt(((new - vs) ** 2).sum(1)) - np.sqrt(((old - vs) ** 2).sum(1))
        assert (worse <= M.DOT_EPSILON).all(), f"{n} normals: {worse.max()} worse than the brute force for input {vs[worse.argmax()]}"


@pytest.mark.parametrize("bits", [32, 64])
def test_project_velocity_by_hand(bits):
    dt = DT[bits]
    up, west, south = (0, 1, 0), (-1, 0, 0), (0, 0, -1)
    eq = lambda got, want: [float(x) for x in got] == [float(x) for x in want] and all(type(x) is dt for x in got)
    assert eq(M.project_velocity([0, -1, 0], [up], dt), [0, 0, 0])
    assert np.signbit(M.project_velocity([0, -1, 0], [up], dt)[1])                  # blocked: -(+0)
    assert eq(M.project_velocity([1, -1, 0], [up], dt), [1, 0, 0])                   # slides
    assert eq(M.project_velocity([1, 1, 0], [up], dt), [1, 1, 0])                    # leaving: untouched
    assert eq(M.project_velocity([1, -1, 1], [up, west], dt), [0, 0, 1])             # along the crease
    out = M.project_velocity([1, -1, 1], [up, west, south], dt)                      # a corner: fully blocked, every component -0.0
    assert eq(out, [0, 0, 0]) and all(np.signbit(x) for x in out)
    assert eq(M.project_velocity([1, -1, 0], [], dt), [1, -1, 0])
    # the last maximum: two equal normals, and the result does not depend on which is taken; -0 < +0 under total_cmp
    assert eq(M.project_velocity([0, -2, 0], [up, up], dt), [0, 0, 0])
    assert M.total_key(dt(-0.0)) < M.total_key(dt(0.0)) and M.total_key(dt(1.0)) > M.total_key(dt(0.5)) and M.total_key(dt(-1.0)) < M.total_key(dt(-0.5))
    # non-finite inputs answer the velocity unchanged
    assert eq(M.project_velocity([1, -np.inf, 0], [up], dt), [1, -np.inf, 0])
    assert eq(M.project_velocity([1, -1, 0], [up, (np.nan, 0, 0)], dt), [1, -1, 0])
    # a Dir is f32 in an f64 world too
    d = M.dir_and_length([1.0, 2.0, 2.0])
    assert d[1] == np.float32(3) and d[0][0].dtype == np.float32 and M.dir_and_length([0, 0, 0]) is None and M.dir_and_length([np.inf, 0, 0]) is None
    assert M.dir_and_length([1e30, 0, 0]) is None                                    # the f32 length overflows


# ---- cast_move ----------------------------------------------------------------------------------------------------------------------------
def one_move(s, pos, movement, skin, **kw):
    return M.cast_moves(s, [BALL], [[0.5, 0, 0]], [pos], [I], [movement], skin, **kw)[0]


@pytest.mark.parametrize("bits", [32, 64])
def test_cast_move_by_hand(bits):
    s = snapshot([FLOOR], DT[bits])
    h = one_move(s, [0, 0.75, 0], [0, -1, 0], 0.125)
    assert h["collider"] == 0 and h["entity"] == 10 and h["distance"] == 0.125 and h["collision_distance"] == 1.0
    assert list(h["normal1"]) == [0, 1, 0] and list(h["normal2"]) == [0, -1, 0] and not np.signbit(h["normal2"][0])
    assert list(h["point1"]) == [0, 0, 0] and list(h["point2"]) == [0, 0, 0]
    # the movement ends before the floor: a miss, every byte but the ids 0
    m = one_move(s, [0, 0.75, 0], [0, -0.125, 0], 0.125)
    assert m["collider"] == MISS and m["entity"] == MISS and m.tobytes()[8:] == bytes(m.itemsize - 8)
    # a hit nearer than the skin: 0
    assert one_move(s, [0, 0.5625, 0], [0, -1, 0], 0.125)["distance"] == 0.0
    # a zero movement: (X, 0), a cast of length 0; clear of everything it is a miss, and a bad skin width or movement is one too
    assert one_move(s, [0, 0.75, 0], [0, 0, 0], 0.125)["collider"] == MISS
    for skin in (np.nan, np.inf, -0.125):
        assert one_move(s, [0, 0.75, 0], [0, -1, 0], skin)["collider"] == MISS
    assert one_move(s, [0, 0.75, 0], [0, -np.inf, 0], 0.125)["collider"] == MISS
    # a grazing normal: dot(dir, -normal1) = 2^-8 / |(1, 2^-8)| < DOT_EPSILON, so the skin is divided by DOT_EPSILON
    gap, slope, skin = 2.0 ** -10, 2.0 ** -8, 2.0 ** -11
    g = one_move(s, [-3, 0.5 + gap, 0], [2, -2 * slope, 0], skin)
    toi = gap / slope * math.sqrt(1 + slope * slope)
    assert g["collider"] == 0 and abs(g["distance"] - (toi - skin / M.DOT_EPSILON)) < 1e-5 and abs(g["distance"] - (toi - skin / slope)) > 0.02
    # self_entity, the shared excluded list, the mask and the sensor flag each make the floor invisible
    for kw in (dict(self_entity=[10]), dict(excluded=[10]), dict(mask=[2]), dict(sensor=[1])):
        assert one_move(s, [0, 0.75, 0], [0, -1, 0], 0.125, **kw)["collider"] == MISS
    assert one_move(s, [0, 0.75, 0], [0, -1, 0], 0.125, self_entity=[MISS])["collider"] == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_origin_penetration_rule_all_three_outcomes(bits):
    s = snapshot([FLOOR], DT[bits])
    # the ball's lower half in the floor (0.25 deep), on its way out: the floor is ignored, and nothing else is there
    info = {}
    out = M.cast_moves(s, [BALL], [[0.5, 0, 0]], [[0, 0.25, 0]], [I], [[0, 1, 0]], 0.125, info=info)[0]
    assert out["collider"] == MISS and info["ignored"][0] == 1
    # sideways along the surface (dir . n == 0) counts as leaving too
    assert one_move(s, [0, 0.25, 0], [1, 0, 0], 0.125)["collider"] == MISS
    # on its way in: distance 0 with the contact's normal and points
    info = {}
    h = M.cast_moves(s, [BALL], [[0.5, 0, 0]], [[0, 0.25, 0]], [I], [[0, -1, 0]], 0.125, info=info)[0]
    assert info["blocked"][0] == 1 and h["collider"] == 0 and h["distance"] == 0 and h["collision_distance"] == 1
    assert list(h["normal1"]) == [0, 1, 0] and list(h["normal2"]) == [0, -1, 0]
    assert list(h["point1"]) == [0, -0.125, 0] and list(h["point2"]) == [0, -0.125, 0]
    # the centre inside the cuboid: the pair has no contact (4.4.7 records why): distance 0 and zeros, whatever the direction
    for mv in ([0, -1, 0], [0, 1, 0]):
        info = {}
        z = M.cast_moves(s, [BALL], [[0.5, 0, 0]], [[0, -0.25, 0]], [I], [mv], 0.125, info=info)[0]
        assert info["no_contact"][0] == 1 and z["collider"] == 0 and z["entity"] == 10 and z["collision_distance"] == 1
        assert z.tobytes()[8:8 + z.dtype.fields["collision_distance"][1] - 8] == bytes(z.dtype.fields["collision_distance"][1] - 8)
        assert z.tobytes()[z.dtype.fields["point1"][1]:] == bytes(z.itemsize - z.dtype.fields["point1"][1])
    # an ordinary hit beside an ignored collider: leaving the floor upwards into a ceiling
    s2 = snapshot([FLOOR, (CUBOID, [4, 0.5, 4], [0, 2.0, 0])], DT[bits])
    c = one_move(s2, [0, 0.25, 0], [0, 2, 0], 0.125)
    assert c["collider"] == 1 and c["distance"] == 0.625 and list(c["normal1"]) == [0, -1, 0]


# ---- move_and_slide ---------------------------------------------------------------------------------------------------------------------------
def slide(s, velocity, iterations, q=BALL_Q, hit_cap=8, **kw):
    info = {}
    out, hits = M.move_and_slide(s, *q, [velocity], **dict(HAND, **kw), move_and_slide_iterations=iterations, hit_cap=hit_cap, info=info)
    return out[0], hits[0], info


@pytest.mark.parametrize("bits", [32, 64])
def test_ball_dropped_on_a_floor_by_hand(bits):
    """Radius 0.5 at height 0.75 over a floor whose top is y = 0, velocity (0, -1, 0), delta_time 1, skin_width 0.125: hit at 0.25, pulled back to
    0.125; position.y = 0.625, time_left = 0.875; the contact plane is the sweep's plane again, so one plane; the velocity is fully blocked."""
    s = snapshot([FLOOR], DT[bits])
    out, hits, info = slide(s, [0, -1, 0], 4)
    assert list(out["position"]) == [0, 0.625, 0] and list(out["projected_velocity"]) == [0, 0, 0] and np.signbit(out["projected_velocity"][1])
    assert out["iterations_run"] == 1 and out["hit_count"] == 1 and out["flags"] == 0 and info["max_planes"][0] == 1
    h = hits[0]
    assert (h["collider"], h["entity"], h["iteration"], h["kind"]) == (0, 10, 0, 0) and h["distance"] == 0.125 and h["collision_distance"] == 1
    assert list(h["normal"]) == [0, 1, 0] and list(h["point"]) == [0, 0.75, 0]      # point2 (0, 0, 0) + the position before the move
    assert hits[1]["collider"] == MISS and hits[1].tobytes()[8:] == bytes(hits[1].itemsize - 8)
    # iterations = 0: the two depenetrations only, and the ball is clear of the skin
    out0, _, _ = slide(s, [0, -1, 0], 0)
    assert list(out0["position"]) == [0, 0.75, 0] and list(out0["projected_velocity"]) == [0, -1, 0] and out0["iterations_run"] == 0 and out0["hit_count"] == 0
    # one iteration: the same as four, the second round would have had no movement left
    out1, _, _ = slide(s, [0, -1, 0], 1)
    assert out1.tobytes() == out.tobytes()
    # time_left: with the velocity halved by hand after the first round the rest of the sweep is 0.875 of the time
    o2, _, _ = slide(s, [1, -1, 0], 4)
    assert list(o2["projected_velocity"]) == [1, 0, 0] and o2["iterations_run"] == 2 and o2["hit_count"] == 1
    # it slides: (0.125, 0.625) after the first round up to rounding, then the rest of the sweep, 0.875, along x
    assert abs(o2["position"][0] - 1.0) < 1e-6 and abs(o2["position"][1] - 0.625) < 1e-6 and o2["position"][2] == 0
    # a depenetration pass first: the ball starts 0.25 deep and is lifted to skin_width above the floor before it moves
    o3, _, _ = slide(s, [0, 0, 0], 4, q=([BALL], [[0.5, 0, 0]], [[0, 0.25, 0]], [I]))
    assert list(o3["position"]) == [0, 0.625, 0] and o3["iterations_run"] == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_wall_after_floor_and_corner_by_hand(bits):
    s = snapshot([FLOOR, WALL_X], DT[bits])
    out, hits, info = slide(s, [1, -1, 1], 4)
    # the floor first, then the wall: two planes, the velocity runs along the crease
    assert info["max_planes"][0] == 2 and list(out["projected_velocity"]) == [0, 0, 1]
    kinds = [(int(h["collider"]), int(h["iteration"]), int(h["kind"])) for h in hits[:out["hit_count"]]]
    assert kinds == [(0, 0, 0), (1, 1, 0), (0, 1, 1)]          # sweep on the floor; sweep on the wall, then the floor's contact plane
    assert abs(out["position"][0] - 0.375) < 1e-5 and abs(out["position"][1] - 0.625) < 1e-5
    # max_planes = 1: the floor's contact plane of the second round is neither pushed nor logged; only the wall clips the velocity
    o1, h1, i1 = slide(s, [1, -1, 1], 4, max_planes=1)
    assert i1["max_planes"][0] == 1 and o1["hit_count"] == 2 == out["hit_count"] - 1 and list(o1["projected_velocity"]) == [0, 0, 1]
    # initial planes: a plane facing -z given in the configuration blocks the crease too
    o2, _, _ = slide(s, [1, -1, 1], 4, planes=[[0, 0, -1]])
    assert list(o2["projected_velocity"]) == [0, 0, 0]
    # a corner of three planes: nothing is left
    s3 = snapshot([FLOOR, WALL_X, WALL_Z], DT[bits])
    o3, _, i3 = slide(s3, [1, -1, 1], 6)
    assert i3["max_planes"][0] == 3 and list(o3["projected_velocity"]) == [0, 0, 0]
    # the log is truncated to hit_cap, the count is not
    o4, h4, _ = slide(s3, [1, -1, 1], 6, hit_cap=2)
    assert o4["hit_count"] == o3["hit_count"] > 2 and len(h4) == 2 and (h4["collider"] != MISS).all()


def test_a_character_that_cannot_be_simulated_keeps_its_inputs():
    s = snapshot([FLOOR], np.float32)
    q = (np.array([BALL, 2, BALL, CUBOID], np.uint8), [[0.5, 0, 0], [0.5, 0.5, 0.5], [0.5, 0, 0], [0.5, -0.5, 0.5]], [[0, np.nan, 0], [0, 0.75, 0], [0, 0.75, 0], [0, 0.75, 0]],
         [I, I, [0, np.inf, 0, 1], I])
    with np.errstate(all="ignore"):
        out, hits = M.move_and_slide(s, *q, [[0, -1, 0]] * 4, **HAND, move_and_slide_iterations=4, hit_cap=2)
    assert np.array_equal(out["position"], np.array(q[2], np.float32), equal_nan=True) and (out["projected_velocity"] == [0, -1, 0]).all()
    assert (out["iterations_run"] == 0).all() and (out["hit_count"] == 0).all() and (hits["collider"] == MISS).all()


# ---- the populations the GPU test relies on: seeds are chosen here, on the CPU -------------------------------------------------------------
def room_snapshot(bits, centre=(0.0, 0.0, 0.0)):
    bodies, cols, sensor = MS.room(centre)
    return R.Snapshot(bodies, cols, None, DT[bits]), cols, sensor


def slide_populations(out, info):
    ok = out["iterations_run"] > 0
    return dict(never_hit=int((ok & (out["hit_count"] == 0)).sum()), one_plane=int((info["max_planes"] == 1).sum()), more_planes=int((info["max_planes"] >= 2).sum()),
                leaving=int((info["ignored"] > 0).sum()), blocked=int((info["blocked"] > 0).sum()), no_contact=int((info["no_contact"] > 0).sum()))


MOVE_SEED, SLIDE_SEED = 3, 5


@pytest.mark.parametrize("bits", [32, 64])
def test_populations_of_the_room(bits):
    s, cols, sensor = room_snapshot(bits)
    assert s.n == 12 and sensor.sum() == 1 and (cols["entity_index"] == MS.SELF_ENTITY).sum() == 1
    shape, he, pos, rot, mv, skin, own = MS.moves(MOVE_SEED)
    info = {}
    hits = M.cast_moves(s, shape, he, pos, rot, mv, skin, own, sensor=sensor, info=info)
    assert (hits["collider"] == MISS).sum() >= 15 and (hits["collider"] != MISS).sum() >= 40
    assert (info["ignored"] > 0).sum() >= 8 and (info["blocked"] > 0).sum() >= 8 and (info["no_contact"] > 0).sum() >= 1
    assert ((hits["collider"] != MISS) & (hits["distance"] == 0)).sum() >= 8 and (hits["distance"] > 0).sum() >= 15
    assert hits["collider"][5] != 11 and not (hits["collider"] == 10).any()        # its own collider and the sensor are never hit
    assert len(set(hits["collider"])) >= 6
    shape, he, pos, rot, vel, own = MS.characters(SLIDE_SEED)
    info = {}
    out, log = M.move_and_slide(s, shape, he, pos, rot, vel, **MS.CFG, hit_cap=4, self_entity=own, sensor=sensor, info=info)
    p = slide_populations(out, info)
    assert p["never_hit"] >= 10 and p["one_plane"] >= 10 and p["more_planes"] >= 10 and p["leaving"] >= 5 and p["blocked"] >= 5 and p["no_contact"] >= 1, p
    assert info["live"][0] == 100 and info["live"][-1] >= 5 and (out["hit_count"] > 4).any() and (out["iterations_run"] == 4).any()


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_record_layouts():
    dll = ctypes.CDLL(hip_lib().path)
    for name in ("avn_spatial_project_velocities", "avn_spatial_cast_moves", "avn_spatial_move_and_slide"):
        assert name in Q.SYMBOLS and hasattr(dll, name), f"{hip_lib().path} does not export {name}"
    sizes = {"move_hit": (64, 120), "slide": (36, 64), "slide_hit": (48, 80)}
    for name, (s32, s64) in sizes.items():
        for bits, size in ((32, s32), (64, s64)):
            c = getattr(Q, f"avn_spatial_{name}_f{bits}")
            d = getattr(Q, f"{name}_dtype")(bits)
            assert ctypes.sizeof(c) == d.itemsize == size, name
            assert all(d.fields[f][1] == getattr(c, f).offset for f, _ in c._fields_ if f != "reserved"), "numpy mirror and ctypes mirror disagree"
            assert sum(getattr(c, f).size for f, _ in c._fields_) == ctypes.sizeof(c), "implicit padding in the record"
    assert Q.MAX_PLANES == 32 and Q.MAX_SLIDE_ITERATIONS == 16
