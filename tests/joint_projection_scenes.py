"""Scenes for the joint projection tests, the driver that records a world system by system, and the one check both the CPU test (oracle) and
the GPU test (HIP library) apply to such a record (tests/joint_projection_reference.py is the reference).

Formula scene: every joint on its own pair of bodies, ~40 variants per type, two substeps.  The pose of body 2 is built from chosen angles:
rot2 = rot1 * basis1 * R_rel * basis2^-1, so the two joint frames differ by R_rel exactly.

Schedule scenes: a comb, chains on both sides of the LDS ceiling of the level schedule, hubs -- all five joint types mixed, damping on.

Conditioning: a scene is finished by `conditioned`: the float64 reference runs next to the oracle, reports each joint's distance to every discontinuity
of the operation, and the joints that come too close are drawn again (deterministic: one seeded generator per scene).
"""
import numpy as np

import joint_projection_reference as R
import solver_second_opinion as S
from helpers import F, oracle_lib, random_spd_inverse_inertia, random_unit_quats

SUBSTEPS = 2
FACTOR = 16.0        # the bound: largest difference to the truth <= FACTOR * the reference's own rounding noise, per field and scene
SENSITIVITY = 1000.0  # median correction of a joint >= SENSITIVITY * tolerance

# what a generator keeps away from (drawn again below these) and what a test asserts (the issue's 5 degrees / 0.05 / 1e-3)
GENERATE = dict(wrap=np.radians(9.0), asin=1.0 - np.cos(np.radians(9.0)), twist_switch=0.09, ortho_z=0.05, ortho_xy=0.09, length=2e-3, w_sum=2e-3)
ASSERT = dict(wrap=np.radians(5.0), asin=1.0 - np.cos(np.radians(5.0)), twist_switch=0.05, ortho_z=0.05, ortho_xy=0.05, length=1e-3, w_sum=1e-3)

FIELDS = ("prepared", "delta_position", "delta_rotation", "linear_velocity", "angular_velocity", "total_lagrange", "total_rotation_lagrange", "force", "torque")


# ---- float64 helpers for building poses --------------------------------------------------------------------------------------------------------------
def q_axis_angle(axis, angle):
    axis = np.asarray(axis, float); axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])


def q_rotate(q, v):
    return R.quat_matrix(np.asarray(q, float)) @ np.asarray(v, float)


def perpendicular(rng, v):
    v = np.asarray(v, float) / np.linalg.norm(v)
    while True:
        p = rng.normal(size=3); p -= (p @ v) * v
        if np.linalg.norm(p) > 0.3:
            return p / np.linalg.norm(p)


def unit(rng, lo, hi):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v) * rng.uniform(lo, hi)


AXIS_PRESETS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.8, -0.0)]


def draw_axis(rng, k):
    a = (k * 3) % 11
    if a < len(AXIS_PRESETS):
        return np.array(AXIS_PRESETS[a], float)
    while True:
        v = unit(rng, 1.0, 1.0)
        if abs(v[2]) >= 0.08:
            return v


def draw_angle(rng, obtuse):
    return rng.choice([-1.0, 1.0]) * np.radians(rng.uniform(100.0, 165.0) if obtuse else rng.uniform(15.0, 75.0))


STATUS = ("absent", "inside", "below", "above", "equal")


def angle_limit(rng, status, theta):
    """[min, max] that puts the angle `theta` where `status` says."""
    if status in ("absent", "inside"): return theta - rng.uniform(0.2, 0.5), theta + rng.uniform(0.2, 0.4)
    if status == "below": return theta + rng.uniform(0.25, 0.4), theta + rng.uniform(0.6, 0.9)
    if status == "above": return theta - rng.uniform(0.6, 0.9), theta - rng.uniform(0.25, 0.4)
    lim = theta + rng.choice([-1.0, 1.0]) * rng.uniform(0.25, 0.5)
    return lim, lim


# ---- one body ---------------------------------------------------------------------------------------------------------------------------------------
def dynamic_body(rng):
    return dict(position=rng.uniform(-2, 2, 3), rotation=random_unit_quats(rng, 1)[0], linear_velocity=rng.normal(scale=0.5, size=3),
                angular_velocity=rng.normal(scale=1.0, size=3), inv_mass=rng.uniform(0.5, 2.0), inv_inertia_local=random_spd_inverse_inertia(rng, 1, 0.0)[0],
                rb_type=F.RB_DYNAMIC, center_of_mass=unit(rng, 0.02, 0.1), locked_axes=0, dominance=0, body_flags=0)


def make_static(b):
    b.update(rb_type=F.RB_STATIC, inv_mass=0.0, inv_inertia_local=np.zeros(6), linear_velocity=np.zeros(3), angular_velocity=np.zeros(3))


BODY_KEYS = ("position", "rotation", "linear_velocity", "angular_velocity", "inv_mass", "inv_inertia_local", "rb_type", "center_of_mass", "locked_axes", "dominance", "body_flags")
BODY_INT = dict(rb_type=np.uint8, locked_axes=np.uint8, dominance=np.int8, body_flags=np.uint8)
JOINT_KEYS = ("joint_type", "body1", "body2", "local_anchor1", "local_anchor2", "local_basis1", "local_basis2", "axis", "limit_min", "limit_max", "limit2_min",
              "limit2_max", "limit_flags", "compliance", "damping_linear", "damping_angular")
JOINT_INT = dict(joint_type=np.uint8, body1=np.int32, body2=np.int32, limit_flags=np.uint8)
BODY_VARIANTS = ("plain", "body1_static", "body2_kinematic", "both_static", "body1_disabled", "dominance_plus", "dominance_minus", "lock_t1_r2", "lock_t2_r1", "dominance_equal")
COMPLIANCE = (1e-3, 2e-4, 5e-5)   # three different values, one per lane


def stack(items, keys, ints):
    return {k: np.array([it[k] for it in items], ints.get(k, float)) for k in keys}


# ---- the formula scene: one joint per pair of bodies ---------------------------------------------------------------------------------------------------
def formula_pair(rng, t, k):
    """Variant `k` of joint type `t`: (body 1, body 2, joint, meta)."""
    b1, b2 = dynamic_body(rng), dynamic_body(rng)
    variant = BODY_VARIANTS[k % 10]
    if variant in ("body1_static", "both_static"): make_static(b1)
    if variant == "both_static": make_static(b2)
    if variant == "body2_kinematic": b2.update(rb_type=F.RB_KINEMATIC)
    if variant == "body1_disabled": b1.update(body_flags=F.BODY_DISABLED)
    if variant == "dominance_plus": b1.update(dominance=2)
    if variant == "dominance_minus": b2.update(dominance=3)
    if variant == "dominance_equal": b1.update(dominance=1); b2.update(dominance=1)
    if variant == "lock_t1_r2": b2.update(locked_axes=0b100000); b1.update(locked_axes=0b000011)
    if variant == "lock_t2_r1": b1.update(locked_axes=0b110000); b2.update(locked_axes=0b000100)
    axis = draw_axis(rng, k)
    basis1, basis2 = random_unit_quats(rng, 1)[0], random_unit_quats(rng, 1)[0]
    s1, s2 = STATUS[(k + k // 10) % 5], STATUS[(k // 2 + k // 10) % 5]
    obtuse1, obtuse2 = bool((k // 5) % 2), bool((k // 3) % 2)
    lim1, lim2, meta = (0.0, 0.0), (0.0, 0.0), dict(variant=variant, status1=s1, status2=s2)
    ortho = R.any_orthonormal_vector(axis)
    if t in (F.JOINT_FIXED, F.JOINT_PRISMATIC):
        rel = q_axis_angle(rng.normal(size=3), rng.uniform(0.05, 0.5))
    elif t == F.JOINT_REVOLUTE:
        theta = draw_angle(rng, obtuse1)
        rel = R.qmul(q_axis_angle(perpendicular(rng, axis), rng.uniform(0.02, 0.15)), q_axis_angle(axis, theta))
        lim1 = angle_limit(rng, s1, theta)
        meta.update(angle1=theta)
    elif t == F.JOINT_SPHERICAL:
        swing = np.radians(rng.uniform(130.0, 165.0) if obtuse1 else rng.uniform(20.0, 75.0))
        twist = draw_angle(rng, obtuse2)
        # the twist limit measures the twist axes projected along the bisector of the swing axes: seen from there, the plane perpendicular to the swing axis is
        # squashed by cos(swing / 2) across the swing's own axis m.  tau is the turn about the swing axis that shows as `twist` after the squash.
        m = perpendicular(rng, ortho)
        k_, c = R.cross(ortho, m), np.cos(swing / 2)
        psi1 = np.arctan2(axis @ k_, axis @ m)
        shown = np.arctan2(c * np.sin(psi1), np.cos(psi1)) + twist
        tau = np.arctan2(np.sin(shown) / c, np.cos(shown)) - psi1
        rel = R.qmul(q_axis_angle(m, swing), q_axis_angle(ortho, tau))
        lim1, lim2 = angle_limit(rng, s1, swing), angle_limit(rng, s2, twist)
        meta.update(angle1=swing, angle2=twist)
    else:
        rel = np.array([0.0, 0, 0, 1])
    if t != F.JOINT_DISTANCE:
        b2["rotation"] = R.qmul(R.qmul(R.qmul(b1["rotation"], basis1), rel), R.qconj(basis2))
    a1, a2 = unit(rng, 0.05, 0.3), unit(rng, 0.05, 0.3)
    if t == F.JOINT_PRISMATIC:
        u = q_rotate(R.qmul(b1["rotation"], basis1), axis)
        along, lim1 = dict(absent=(0.1, (-0.2, 0.4)), inside=(0.1, (-0.2, 0.4)), below=(-0.3, (-0.1, 0.4)), above=(0.5, (-0.2, 0.3)), equal=(0.1, (0.25, 0.25)))[s1]
        d = along * u + perpendicular(rng, u) * rng.uniform(0.05, 0.15)
    elif t == F.JOINT_DISTANCE:
        dist = rng.uniform(0.3, 0.8)
        d = unit(rng, dist, dist)
        lim1 = dict(absent=(0.0, 10.0), inside=(dist - 0.1, dist + 0.1), below=(dist + 0.1, dist + 0.3), above=(dist - 0.25, dist - 0.1), equal=(dist + 0.15, dist + 0.15))[s1]
    else:
        d = unit(rng, 0.05, 0.2)
    b2["position"] = b1["position"] + q_rotate(b1["rotation"], a1) + d - q_rotate(b2["rotation"], a2)
    flags = (F.JOINT_HAS_LIMIT1 if s1 != "absent" else 0) | (F.JOINT_HAS_LIMIT2 if s2 != "absent" else 0)
    lanes = (k // 2) % 8
    joint = dict(joint_type=t, local_anchor1=a1, local_anchor2=a2, local_basis1=basis1, local_basis2=basis2, axis=axis, limit_min=lim1[0], limit_max=lim1[1],
                 limit2_min=lim2[0], limit2_max=lim2[1], limit_flags=flags, compliance=[COMPLIANCE[i] if lanes >> i & 1 else 0.0 for i in range(3)],
                 damping_linear=(0.5, 2.0, 150.0, 300.0)[k % 4], damping_angular=(200.0, 1.0, 2.5, 140.0)[k % 4])
    return b1, b2, joint, meta


def right_angle_pair():
    """A swing of exactly 90 degrees from exactly representable rotations: identity and (1/2, 1/2, 1/2, 1/2), the turn by 120 degrees about (1, 1, 1) that
    sends y to z.  Twist axis x, swing axis any_orthonormal_vector(x) = y.  The anchors coincide and nothing moves the pair, so the point constraint leaves
    the delta rotations alone and the limit sees s = 1, n1.n2 = 0 exactly in the first substep."""
    rng = np.random.default_rng(0)
    b1, b2 = dynamic_body(rng), dynamic_body(rng)
    for b in (b1, b2):
        b.update(position=np.array([0.5, -1.25, 2.0]), linear_velocity=np.zeros(3), angular_velocity=np.zeros(3), center_of_mass=np.zeros(3), inv_mass=1.0,
                 inv_inertia_local=np.array([2.0, 0, 0, 2.0, 0, 2.0]))
    b1["rotation"] = np.array([0.0, 0, 0, 1]); b2["rotation"] = np.array([0.5, 0.5, 0.5, 0.5])
    ident = np.array([0.0, 0, 0, 1])
    joint = dict(joint_type=F.JOINT_SPHERICAL, local_anchor1=np.zeros(3), local_anchor2=np.zeros(3), local_basis1=ident, local_basis2=ident, axis=np.array([1.0, 0, 0]),
                 limit_min=-0.5, limit_max=0.5, limit2_min=0.0, limit2_max=0.0, limit_flags=F.JOINT_HAS_LIMIT1, compliance=[0.0, COMPLIANCE[1], 0.0],
                 damping_linear=1.0, damping_angular=1.0)
    return b1, b2, joint, dict(variant="right_angle", status1="above", status2="absent")


def assemble(pairs, with_damping=True, name="formula"):
    bodies = [b for p in pairs for b in p[:2]]
    joints = []
    for i, p in enumerate(pairs):
        joints.append(dict(p[2], body1=2 * i, body2=2 * i + 1))
    J = stack(joints, JOINT_KEYS, JOINT_INT)
    if not with_damping:
        del J["damping_linear"], J["damping_angular"]
    return dict(name=name, bodies=stack(bodies, BODY_KEYS, BODY_INT), joints=J, meta=[p[3] for p in pairs], substeps=SUBSTEPS)


_cache = {}


def formula_scene(with_damping=True):
    key = ("formula", with_damping)
    if key not in _cache:
        rng = np.random.default_rng(20200817)
        spec = [(t, k) for t in range(5) for k in range(40)]
        pairs = [formula_pair(rng, t, k) for t, k in spec] + [right_angle_pair()]

        def redraw(j):
            assert j < len(spec), "the deterministic right-angle case is not drawn"
            pairs[j] = formula_pair(rng, *spec[j])
        _cache[key] = conditioned(lambda: assemble(pairs, with_damping), redraw)
    return _cache[key]


# ---- schedule scenes: a joint graph given as edges, random joints of all five types on it ----------------------------------------------------------------
def schedule_joint(rng, types=(0, 1, 2, 3, 4)):
    t = int(rng.choice(types))
    while True:
        axis = unit(rng, 1.0, 1.0)
        if abs(axis[2]) >= 0.08: break
    lo = rng.uniform(0.1, 0.5) if t == F.JOINT_DISTANCE else rng.uniform(-1.5, 0.3)
    lo2 = rng.uniform(-1.5, 0.3)
    return dict(joint_type=t, local_anchor1=unit(rng, 0.05, 0.2), local_anchor2=unit(rng, 0.05, 0.2), local_basis1=random_unit_quats(rng, 1)[0],
                local_basis2=random_unit_quats(rng, 1)[0], axis=axis, limit_min=lo, limit_max=lo + rng.uniform(0.0, 1.2), limit2_min=lo2, limit2_max=lo2 + rng.uniform(0.0, 1.5),
                limit_flags=int(rng.integers(0, 4)), compliance=np.where(rng.random(3) < 0.5, 0.0, rng.uniform(1e-5, 1e-3, 3)),
                damping_linear=rng.choice([rng.uniform(0, 3), rng.uniform(130, 300)]), damping_angular=rng.choice([rng.uniform(0, 3), rng.uniform(130, 300)]))


def schedule_scene(name, n_bodies, edges, static=(), seed=1, types=None):
    """`types`: per edge the joint types to draw from (all five when None)."""
    key = (name, n_bodies, len(edges))
    types = types or [(0, 1, 2, 3, 4)] * len(edges)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        bodies = [dynamic_body(rng) for _ in range(n_bodies)]
        for b in bodies: b["position"] = rng.uniform(-0.6, 0.6, 3)
        for i in static: make_static(bodies[i])
        joints = [dict(schedule_joint(rng, ty), body1=a, body2=b) for (a, b), ty in zip(edges, types)]

        def build():
            return dict(name=name, bodies=stack(bodies, BODY_KEYS, BODY_INT), joints=stack(joints, JOINT_KEYS, JOINT_INT), meta=None, substeps=SUBSTEPS)

        def redraw(j):
            joints[j] = dict(schedule_joint(rng, types[j]), body1=edges[j][0], body2=edges[j][1])
        _cache[key] = conditioned(build, redraw)
        assert set(_cache[key]["joints"]["joint_type"]) == {0, 1, 2, 3, 4} or len(edges) < 20, "all five joint types in every case"
    return _cache[key]


def lds_bytes(n_bodies, n_joints, bits):
    """What the level schedule stages for one component: 4 vectors per body, 15 per joint (a vector is four scalars), and a 4-byte slot per body."""
    return (4 * n_bodies + 15 * n_joints) * 4 * (bits // 8) + 4 * n_bodies


LDS_CEILING = 64 * 1024


def straddling_chain_lengths(bits):
    nj = 1
    while lds_bytes(nj + 2, nj + 1, bits) <= LDS_CEILING: nj += 1
    return nj, nj + 1


def chain(first_body, n_joints):
    return [(first_body + i, first_body + i + 1) for i in range(n_joints)]


def comb_scene():
    """A path of 261 bodies, even edges uploaded first, then odd edges: one component, two levels of 130 joints (a 64-lane stride with a tail of 2).
    The solve runs type by type, so the even edges take the types fixed / revolute / spherical and the odd ones spherical / prismatic / distance: every
    even edge still precedes its two neighbours."""
    path = chain(0, 260)
    return schedule_scene("comb", 261, path[0::2] + path[1::2], seed=2, types=[(0, 1, 2)] * 130 + [(2, 3, 4)] * 130)


def chains_scene(bits):
    """The two chains on either side of the LDS ceiling alone."""
    fit, over = straddling_chain_lengths(bits)
    return schedule_scene(f"chains{bits}", fit + over + 2, chain(0, fit) + chain(fit + 1, over), seed=6)


def level_shape(scene):
    """The level schedule a scene asks for, worked out from the serial order alone (type by type, array order inside a type): per component of bodies that own
    a SolverBody the widths of its levels, a joint's level being one more than the last level that touched one of its bodies.  A joint without any such body
    is a component of its own."""
    J, B = scene["joints"], scene["bodies"]
    owns = (B["rb_type"] != F.RB_STATIC) & ((B["body_flags"] & F.BODY_DISABLED) == 0)
    parent = list(range(len(owns)))

    def find(x):
        while parent[x] != x: parent[x] = parent[parent[x]]; x = parent[x]
        return x
    for a, b in zip(J["body1"], J["body2"]):
        if owns[a] and owns[b]: parent[find(a)] = find(b)
    last, comps = {}, {}
    for j in sorted(range(len(J["body1"])), key=lambda j: J["joint_type"][j]):
        keys = [int(b) for b in (J["body1"][j], J["body2"][j]) if owns[b]]
        level = 1 + max([last.get(b, -1) for b in keys], default=-1)
        for b in keys: last[b] = level
        widths = comps.setdefault(find(keys[0]) if keys else ("alone", j), [])
        if level == len(widths): widths.append(0)
        widths[level] += 1
    return sorted(comps.values(), key=lambda w: (-sum(w), -len(w)))


def mixed_scene(bits):
    """A chain that fits the LDS ceiling, one that does not, twenty single-joint components and a joint between two static bodies -- in one world."""
    fit, over = straddling_chain_lengths(bits)
    edges = chain(0, fit); n = fit + 1
    edges += chain(n, over); n += over + 1
    for _ in range(20):
        edges.append((n, n + 1)); n += 2
    edges.append((n, n + 1)); n += 2
    return schedule_scene(f"mixed{bits}", n, edges, static=(n - 2, n - 1), seed=3)


def hub_scene(static_hub):
    """A star of 70 joints: on a dynamic hub 70 levels of one joint, on a static hub (no SolverBody) 70 one-joint components that skip staging."""
    rng = np.random.default_rng(4)
    edges = [(0, i) if rng.random() < 0.5 else (i, 0) for i in range(1, 71)]
    return schedule_scene("hub_static" if static_hub else "hub_dynamic", 71, edges, static=(0,) if static_hub else (), seed=5)


SCHEDULE_CASES = ("comb", "chains", "mixed", "hub_dynamic", "hub_static")


def schedule_case(case, bits):
    return dict(comb=comb_scene, chains=lambda: chains_scene(bits), mixed=lambda: mixed_scene(bits), hub_dynamic=lambda: hub_scene(False), hub_static=lambda: hub_scene(True))[case]()


# ---- recording a world system by system -----------------------------------------------------------------------------------------------------------------
def record(lib, bits, scene, whole_steps=0):
    w = F.World(lib, F.default_config(bits, substeps=scene["substeps"]))
    w.bodies_upload(**scene["bodies"])
    w.joints_upload(**scene["joints"])
    tr = dict(cfg=(int(w.cfg.dt_ns), int(w.cfg.substeps)), substeps=[])
    w.run_system("PREPARE_SOLVER_BODIES"); w.run_system("PREPARE_JOINTS")
    tr["prepared"] = w.joints_download()
    w.run_system("PRE_PROCESS_VELOCITY_INCREMENTS")
    for _ in range(scene["substeps"]):
        w.run_system("INTEGRATE_VELOCITIES"); w.run_system("INTEGRATE_POSITIONS")
        s = dict(before=w.solver_bodies_download())
        w.run_system("XPBD_SOLVE")
        s["solved"] = w.solver_bodies_download(); s["joints"] = w.joints_download()
        w.run_system("XPBD_VELOCITY_PROJECTION")
        s["projected"] = w.solver_bodies_download()
        w.run_system("JOINT_DAMPING")
        s["damped"] = w.solver_bodies_download()
        tr["substeps"].append(s)
    w.run_system("CLEAR_VELOCITY_INCREMENTS"); w.run_system("WRITEBACK_SOLVER_BODIES")
    tr["final"] = w.joints_download()
    tr["steps"] = []
    for _ in range(whole_steps):
        w.step(); w.synchronize()
        tr["steps"].append(dict(bodies=w.bodies_download(), joints=w.joints_download(), solver_bodies=w.solver_bodies_download()))
    w.close()
    return tr


_records = {}


def oracle_record(scene, bits):
    """The oracle's record of a scene (with two whole steps behind it), made once per process."""
    key = (scene["name"], id(scene), bits)
    if key not in _records:
        _records[key] = record(oracle_lib(), bits, scene, whole_steps=2)
    return _records[key]


def flatten(tr, prefix=""):
    if isinstance(tr, dict):
        for k, v in tr.items(): yield from flatten(v, f"{prefix}.{k}")
    elif isinstance(tr, (list, tuple)):
        for i, v in enumerate(tr): yield from flatten(v, f"{prefix}[{i}]")
    else:
        yield prefix, np.asarray(tr)


def assert_same_bits(a, b, what):
    fa, fb = dict(flatten(a)), dict(flatten(b))
    assert fa.keys() == fb.keys()
    for k in fa:
        assert np.array_equal(fa[k], fb[k], equal_nan=True), f"{what}: {k} differs"


# ---- the reference next to a record -------------------------------------------------------------------------------------------------------------------
def references(tr, scene, bits, types, mutation=None):
    Tw = np.float32 if bits == 32 else np.float64
    ts = S.time_scalars(S.Arith(bits), *tr["cfg"])
    as_world = lambda d, ints: {k: (np.asarray(v) if k in ints else np.asarray(v).astype(Tw)) for k, v in d.items()}
    joints, poses = as_world(scene["joints"], JOINT_INT), as_world(scene["bodies"], BODY_INT)
    return [R.JointReference(T, joints, poses, ts["h_adj"], ts["dt_adj"], tr["cfg"][1], mutation) for T in types]


def evaluate(tr, scene, bits, mutation=None):
    """Runs the reference in the next wider type (the truth) and in the world's own type (its noise) on the recorded inputs of every system.
    Returns ({field: (the world's largest difference to the truth, the noise)}, the truth's conditioning reports)."""
    Tw, Tt = (np.float32, np.float64) if bits == 32 else (np.float64, np.longdouble)
    truth, own = references(tr, scene, bits, (Tt, Tw), mutation)
    acc = {f: [0.0, 0.0] for f in FIELDS}

    def put(field, world, t, o):
        t = np.asarray(t)
        acc[field][0] = max(acc[field][0], float(np.abs(np.asarray(world).astype(Tt) - t).max()))
        acc[field][1] = max(acc[field][1], float(np.abs(np.asarray(o).astype(Tt) - t).max()))

    truth.prepare(); own.prepare()
    prep = lambda r: np.concatenate([r.world_r1, r.world_r2, r.center_difference])
    put("prepared", np.concatenate([tr["prepared"][k] for k in ("world_r1", "world_r2", "center_difference")]), prep(truth), prep(own))
    for s in tr["substeps"]:
        (tp, tq), (op, oq) = truth.solve(s["before"]), own.solve(s["before"])
        put("delta_position", s["solved"]["delta_position"], tp, op); put("delta_rotation", s["solved"]["delta_rotation"], tq, oq)
        put("total_lagrange", s["joints"]["total_lagrange"], truth.total_lagrange, own.total_lagrange)
        put("total_rotation_lagrange", s["joints"]["total_rotation_lagrange"], truth.total_rotation_lagrange(), own.total_rotation_lagrange())
        for stage, fn in (("projected", lambda r: r.project_velocities(s["solved"], s["before"])), ("damped", lambda r: r.damp(s["projected"]))):
            (tl, ta), (ol, oa) = fn(truth), fn(own)
            has = (np.asarray(s[stage]["flags"]) & R.NO_SOLVER_BODY) == 0   # a body without a SolverBody has no velocity here
            put("linear_velocity", s[stage]["linear_velocity"][has], tl[has], ol[has]); put("angular_velocity", s[stage]["angular_velocity"][has], ta[has], oa[has])
    (tf, tt), (of, ot) = truth.forces(), own.forces()
    put("force", tr["final"]["force"], tf, of); put("torque", tr["final"]["torque"], tt, ot)
    return {f: tuple(v) for f, v in acc.items()}, truth.report


def too_close(report, limits):
    """{joint: [the margins below `limits`]} over the substeps of a conditioning report."""
    bad = {}
    for sub, rep in enumerate(report):
        for j, m in rep.items():
            for key, lim in limits.items():
                # exactly 0 is no neighbourhood of a switch but an input: z = +-0 of the presets +-x, +-y, (x, y, -0), where the sign bit decides, and the
                # all-zero solver data of a joint that was never prepared (a disabled body), where every length is 0 in every type
                if m[key] < lim and not (key in ("ortho_z", "ortho_xy", "length") and m[key] == 0.0):
                    bad.setdefault(j, []).append((sub, key, m[key]))
    return bad


def conditioned(build, redraw, rounds=40):
    """Draws the joints that come too close to a discontinuity again until none does: the float64 reference on the oracle's f32 record."""
    for _ in range(rounds):
        scene = build()
        tr = record(oracle_lib(), 32, scene)
        truth, = references(tr, scene, 32, (np.float64,))
        truth.prepare()
        for s in tr["substeps"]: truth.solve(s["before"])
        bad = too_close(truth.report, GENERATE)
        if not bad:
            return scene
        for j in sorted(bad): redraw(j)
    raise AssertionError(f"{scene['name']}: joints stay close to a discontinuity: {bad}")


def check(tr, scene, bits, label, log=print):
    """The tolerance test: per field the world's largest difference to the truth is at most FACTOR * the reference's own noise; the truth keeps its distance
    from every discontinuity; the median correction of a joint is at least SENSITIVITY * the tolerance.  Returns {field: ratio}."""
    result, report = evaluate(tr, scene, bits)
    bad = too_close(report, ASSERT)
    assert not bad, f"{label}: too close to a discontinuity (change the generator): {bad}"
    ratios = {}
    for f, (err, noise) in result.items():
        ratios[f] = err / noise if noise > 0 else (0.0 if err == 0 else np.inf)
        log(f"{label} {scene['name']} f{bits} {f}: difference {err:.3e} noise {noise:.3e} ratio {ratios[f]:.2f}")
    tol = FACTOR * max(result["delta_position"][1], result["delta_rotation"][1])
    median = float(np.median([m["correction"] for rep in report for m in rep.values()]))
    log(f"{label} {scene['name']} f{bits}: median correction {median:.3e} = {median / tol:.0f} x tolerance")
    assert median >= SENSITIVITY * tol, f"{label}: the median correction {median:.3e} is within {SENSITIVITY:.0f} x the tolerance {tol:.3e}"
    over = {f: r for f, r in ratios.items() if not r <= FACTOR}
    assert not over, f"{label} {scene['name']} f{bits}: beyond {FACTOR:.0f} x the reference's noise: {over}"
    return ratios
