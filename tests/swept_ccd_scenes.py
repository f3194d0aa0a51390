"""Small scenes for the swept CCD tests (about ten bodies or fewer) and the two-world harness the GPU comparison uses: world B steps without
a SweptCcd list and supplies the pre-CCD state, world A steps with the list and must equal swept_ccd_reference's output byte for byte."""
from __future__ import annotations

import numpy as np

from helpers import F
import swept_ccd_reference as CR

DT_NS = 16666667   # Duration::from_secs_f64(1 / 60)
ENTITY0 = 100      # collider entity = ENTITY0 + slot: an entity index is never mistaken for a slot


class Scene:
    """Bodies and one collider list.  Every CCD body's own collider carries AVN_COLLIDER_SWEPT_CCD (as Avian's SweptCcd bodies do: the AABB
    then covers the whole motion, so the broad phase creates the pair the pass tests) and SpeculativeMargin(0), the setting Avian documents for
    pure sweep-based CCD: without it the speculative contact already stops the body and the sweep has nothing to do."""

    def __init__(self, gravity=(0.0, 0.0, 0.0), margin=None):
        self.pos, self.rot, self.lv, self.av, self.rb, self.flags = [], [], [], [], [], []
        self.c_body, self.c_shape, self.c_he, self.c_flags, self.c_child, self.c_lt, self.c_spec = [], [], [], [], [], [], []
        self.gravity, self.margin = gravity, margin

    def body(self, pos, rb=F.RB_DYNAMIC, lv=(0, 0, 0), av=(0, 0, 0), rot=(0, 0, 0, 1), flags=0):
        self.pos.append(pos); self.rot.append(rot); self.lv.append(lv); self.av.append(av); self.rb.append(rb); self.flags.append(flags)
        return len(self.pos) - 1

    def collider(self, body, shape, he, flags=0, child=None):
        self.c_spec.append(0.0 if flags & F.COLLIDER_SWEPT_CCD else -1.0)
        self.c_body.append(body); self.c_shape.append(shape); self.c_he.append(he if shape == F.SHAPE_CUBOID else (he, 0, 0)); self.c_flags.append(flags)
        self.c_child.append(0 if child is None else 1); self.c_lt.append((0, 0, 0) if child is None else child)
        return len(self.c_body) - 1

    def ball(self, pos, r, lv=(0, 0, 0), ccd=True, **kw):
        b = self.body(pos, lv=lv, **kw)
        self.collider(b, F.SHAPE_BALL, r, F.COLLIDER_SWEPT_CCD if ccd else 0)
        return b

    def cuboid(self, pos, he, rb=F.RB_STATIC, ccd=False, cflags=0, **kw):
        b = self.body(pos, rb=rb, **kw)
        self.collider(b, F.SHAPE_CUBOID, he, cflags | (F.COLLIDER_SWEPT_CCD if ccd else 0))
        return b

    # -- uploads ------------------------------------------------------------------------------------
    def body_kwargs(self):
        n = len(self.pos)
        rb = np.array(self.rb, np.uint8)
        inv_mass = np.where(rb == F.RB_DYNAMIC, 1.0, 0.0)
        ii = np.zeros((n, 6)); ii[rb == F.RB_DYNAMIC] = [2.5, 0, 0, 2.5, 0, 2.5]
        return dict(position=np.array(self.pos, float), rotation=np.array(self.rot, float), linear_velocity=np.array(self.lv, float), angular_velocity=np.array(self.av, float),
                    inv_mass=inv_mass, inv_inertia_local=ii, rb_type=rb, body_flags=np.array(self.flags, np.uint8))

    def collider_kwargs(self):
        c = len(self.c_body)
        return dict(entity_index=ENTITY0 + np.arange(c, dtype=np.uint32), body=np.array(self.c_body, np.int32), shape=np.array(self.c_shape, np.uint8),
                    half_extents=np.array(self.c_he, float), collider_flags=np.array(self.c_flags, np.uint8), speculative_margin=np.array(self.c_spec, float))

    def world(self, lib, bits, closed_loop=True):
        kw = dict(substeps=4, gravity=self.gravity, dt_ns=DT_NS)
        if self.margin is not None:
            kw["default_speculative_margin"] = self.margin
        w = F.World(lib, F.default_config(bits, **kw))
        w.bodies_upload(**self.body_kwargs()); w.colliders_upload(**self.collider_kwargs())
        if any(self.c_child):
            c = len(self.c_body)
            w.collider_transforms_upload(is_child=np.array(self.c_child, np.uint8), translation=np.array(self.c_lt, float), rotation=np.tile([0.0, 0, 0, 1], (c, 1)))
        w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5, restitution=0.0)
        if closed_loop:
            w.pipeline_enable()
        return w

    def reference_scene(self, pairs):
        """swept_ccd_reference's view: pairs = avn_pairs_get records in insertion order."""
        cols = dict(entity=ENTITY0 + np.arange(len(self.c_body)), body=np.array(self.c_body), shape=np.array(self.c_shape), half_extents=np.array(self.c_he, float),
                    child=np.array(self.c_child))
        return dict(colliders=cols, pairs=[(int(p["collider1"]) - ENTITY0, int(p["collider2"]) - ENTITY0) for p in pairs], rb_type=np.array(self.rb), body_flags=np.array(self.flags))

    def margin_cfg(self):
        return float(np.finfo(np.float64).max) if self.margin is None else self.margin


def entries_of(bodies, include_dynamic=1, linear_threshold=0.0, angular_threshold=0.0):
    b = lambda a, i: a[i] if isinstance(a, (list, tuple)) else a
    return [dict(body=x, include_dynamic=b(include_dynamic, i), linear_threshold=b(linear_threshold, i), angular_threshold=b(angular_threshold, i)) for i, x in enumerate(bodies)]


def upload(ccd, entries):
    ccd.upload([e["body"] for e in entries], include_dynamic=[e["include_dynamic"] for e in entries], linear_threshold=[e["linear_threshold"] for e in entries],
               angular_threshold=[e["angular_threshold"] for e in entries])


def reference_step(scene: Scene, bits, entries, world_b, pairs_before=(), info=None):
    """One step of world B (no list) and the reference's answer from its pre-CCD state: (records, delta_position, delta_rotation, B's solver bodies)."""
    start = world_b.bodies_download()
    world_b.step(); world_b.synchronize()
    pairs = list(pairs_before) + list(world_b.pairs_get())
    sb = world_b.solver_bodies_download()
    state = dict(position=start["position"], rotation=start["rotation"], linear_velocity=sb["linear_velocity"], angular_velocity=sb["angular_velocity"],
                 delta_position=sb["delta_position"], delta_rotation=sb["delta_rotation"])
    rec, dp, dq = CR.swept_ccd(bits, entries, scene.reference_scene(pairs), state, DT_NS, scene.margin_cfg(), info=info)
    return rec, dp, dq, sb


def assert_equals_reference(scene: Scene, bits, entries, world_a, ccd, world_b, info=None):
    """Steps both worlds once; A's records and delta_position / delta_rotation bytes must be the reference's.  Returns (records, A's solver bodies, B's)."""
    rec, dp, dq, sb_b = reference_step(scene, bits, entries, world_b, info=info)
    world_a.step(); world_a.synchronize()
    got = ccd.results()
    sb_a = world_a.solver_bodies_download()
    assert got.tobytes() == rec.tobytes(), (got, rec)
    assert sb_a["delta_position"].tobytes() == dp.tobytes(), (sb_a["delta_position"], dp)
    assert sb_a["delta_rotation"].tobytes() == dq.tobytes(), (sb_a["delta_rotation"], dq)
    for k in ("linear_velocity", "angular_velocity"):
        assert sb_a[k].tobytes() == sb_b[k].tobytes(), k   # velocities are never changed
    return got, sb_a, sb_b


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------
def tunnelling(speed=240.0):
    s = Scene()
    ball = s.ball((-1, 0, 0), 0.05, lv=(speed, 0, 0))
    s.cuboid((0, 0, 0), (0.05, 1, 2))
    return s, [ball]


def neutrality():
    """A static slab turned 45 degrees about z; two CCD balls inside its AABB that never reach it: one 0.8 off its face moving parallel to
    the face, one on the other side moving straight away."""
    s = Scene()
    h = float(np.sqrt(0.5))
    s.cuboid((0, 0, 0), (2, 0.1, 2), rot=(0, 0, float(np.sin(np.pi / 8)), float(np.cos(np.pi / 8))))
    n, t = np.array([-h, h, 0.0]), np.array([h, h, 0.0])
    a = s.ball(tuple(n * (0.1 + 0.2 + 0.8)), 0.2, lv=tuple(3.0 * t))
    b = s.ball(tuple(-n * 1.1), 0.2, lv=tuple(-3.0 * n))
    return s, [a, b]


def tie(incoming=False):
    """Two static wall halves sharing a seam at the ball's height: equal times of impact, bit for bit.  The broad phase names the collider
    with the smaller AABB min.x first.  incoming: the ball comes from +x just fast enough to reach the walls, so its swept AABB starts
    right of theirs and it is the SECOND collider of both pairs (its edges are then incoming ones)."""
    s = Scene()
    ball = s.ball((1, 0, 0), 0.05, lv=(-57.0, 0, 0)) if incoming else s.ball((-1, 0, 0), 0.05, lv=(240.0, 0, 0))
    s.cuboid((0, 0.5, 0), (0.05, 0.5, 2))
    s.cuboid((0, -0.5, 0), (0.05, 0.5, 2))
    return s, [ball]


def write_order():
    """Two bullets at different distances hit one awake dynamic cuboid that moves and spins."""
    s = Scene()
    a = s.ball((-1, 0, 0), 0.05, lv=(200.0, 0, 0))
    b = s.ball((0, 0, -2), 0.05, lv=(0, 0, 150.0))
    c = s.cuboid((0, 0, 0), (0.3, 0.3, 0.3), rb=F.RB_DYNAMIC, lv=(0, 3.0, 0), av=(0, 0, 2.0))
    return s, (a, b, c)


def target_kinds():
    """Three bullets in lanes far apart: a dynamic, a kinematic and a static cuboid in their way."""
    s = Scene()
    bullets = [s.ball((-1, 10.0 * k, 0), 0.05, lv=(240.0, 0, 0)) for k in range(3)]
    for k, rb in enumerate((F.RB_DYNAMIC, F.RB_KINEMATIC, F.RB_STATIC)):
        s.cuboid((0, 10.0 * k, 0), (0.05, 1, 1), rb=rb)
    return s, bullets


def wall_with(cflags=0, child=False):
    """The tunnelling scene with a sensor wall, or a wall that is a child collider of its (static) body."""
    s = Scene()
    ball = s.ball((-1, 0, 0), 0.05, lv=(240.0, 0, 0))
    if child:
        w = s.body((0, 0, 0), rb=F.RB_STATIC)
        s.collider(w, F.SHAPE_CUBOID, (0.05, 1, 2), child=(0.0, 0.0, 0.0))
    else:
        s.cuboid((0, 0, 0), (0.05, 1, 2), cflags=cflags)
    return s, [ball]


def sat_bullet():
    """A turned cuboid bullet against a wall turned 30 degrees about z: the swept SAT."""
    s = Scene()
    q = np.array([0.2, -0.3, 0.1, 0.9]); q = q / np.linalg.norm(q)
    b = s.body((-1.2, 0.1, 0.05), lv=(200.0, 20.0, 0), rot=tuple(q))
    s.collider(b, F.SHAPE_CUBOID, (0.05, 0.08, 0.06), F.COLLIDER_SWEPT_CCD)
    s.cuboid((0, 0, 0), (0.1, 1.5, 1.5), rot=(0, 0, float(np.sin(np.pi / 12)), float(np.cos(np.pi / 12))))
    return s, [b]


def moving_balls():
    """A CCD ball against a dynamic ball that comes to meet it: d = v2 - v1 with both non-zero."""
    s = Scene()
    a = s.ball((-1, 0, 0), 0.05, lv=(150.0, 0, 0))
    s.ball((1, 0.05, 0), 0.2, lv=(-60.0, 0, 0), ccd=False)
    return s, [a]


def overlapping(speed, margin, sensor=True):
    """A ball overlapping the wall's face by 0.01 at the start of the step.  sensor: the wall is a sensor, so no contact constraint takes the
    ball's velocity away before the pass sees it (against a solid wall the solver stops the ball inside the step: d = 0 and the origin rule
    answers nothing)."""
    s = Scene(margin=margin)
    ball = s.ball((-0.09, 0, 0), 0.05, lv=(speed, 0, 0))
    s.cuboid((0, 0, 0), (0.05, 1, 2), cflags=F.COLLIDER_SENSOR if sensor else 0)
    return s, [ball]
