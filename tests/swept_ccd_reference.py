"""numpy restatement of swept CCD as include/avian_mi355x_ccd.h defines it (k_ccd.hip is the device's side of the same definition).

Built on spatial_cast_reference.cast_exact (the closed-form pair cast), on the CPU oracle's contact_manifolds through
spatial_contact_reference (the origin-penetration rule's contact) and on a from_scaled_axis / quaternion product in the device's operation
order.  `apply_serial` is a plain transcription of the reference's loop (dynamics/ccd/mod.rs:644-683): entries in list order, each one
overwriting delta_position and multiplying delta_rotation of both bodies.  Everything is computed in the world's dtype with numpy scalars,
no fused multiply-adds.

The inputs are what a world WITHOUT a list holds after the same step: its step-start poses and its avn_solver_bodies_download (restitution 0
everywhere, so no restitution pass runs after the place the CCD pass takes).  The edge order is the emission order of avn_pairs_get, which
is the ContactGraph's insertion order when every edge of a CCD body is created in the step under test."""
from __future__ import annotations

import numpy as np

import spatial_cast_reference as CA
import spatial_contact_reference as CR
import spatial_shape_reference as S
from spatial_query_reference import qmul

MISS = 0xFFFFFFFF
RB_DYNAMIC, RB_STATIC, RB_KINEMATIC = 0, 1, 2
SHAPE_CUBOID, SHAPE_BALL, SHAPE_HOST = 0, 1, 2
BODY_SLEEPING, BODY_DISABLED = 1, 2


def result_dtype(bits):
    from avian_amd.swept_ccd import result_dtype as rd
    return rd(bits)


def dt_adjusted(dt_ns, dt):
    """StepParams::dt_adj: Time::delta_seconds_adjusted of the world's scalar (Duration::as_secs_f32 / as_secs_f64)."""
    secs, nanos = divmod(int(dt_ns), 1000000000)
    if dt == np.float32:
        return np.float32(secs) + np.float32(nanos) / np.float32(1e9)
    return np.float64(secs) + np.float64(nanos) / np.float64(1e9)


def from_scaled_axis(v, dt):
    """avn_math.h from_scaled_axis: xyzw."""
    ln = np.sqrt((v[0] * v[0]) + (v[1] * v[1]) + (v[2] * v[2]))
    if ln == dt(0):
        return (dt(0), dt(0), dt(0), dt(1))
    s, c = S.sin_cos(ln * dt(0.5), dt)
    return ((v[0] / ln) * s, (v[1] / ln) * s, (v[2] / ln) * s, c)


def has_solver_body(rb_type, body_flags):
    return (np.asarray(rb_type) != RB_STATIC) & ((np.asarray(body_flags) & (BODY_SLEEPING | BODY_DISABLED)) == 0)


def _v(a, dt):
    return tuple(dt(x) for x in a)


def _len2(a):
    return (a[0] * a[0]) + (a[1] * a[1]) + (a[2] * a[2])


def pair_cast(shape2, he2, pos2, rot2, d, max_t, shape1, he1, pos1, rot1, dt):
    """The header's shape cast for one pair: (hit, toi).  Collider 1 at its raw pose, the cast shape 2 through make_isometry."""
    one = lambda t: tuple(np.array([[dt(x)]], dt) for x in t)
    r2 = S.make_isometry_rotation(rot2, dt)
    with np.errstate(all="ignore"):
        hit, toi, _, _, _ = CA.cast_exact(np.array([[shape2]]), one(he2), one(r2), one(pos2), one(d), np.array([[max_t]], dt),
                                          np.array([[shape1]]), one(he1), one(pos1), one(rot1), dt)
    return bool(hit[0, 0]), dt(toi[0, 0])


def origin_contact_normal(bits, shape2, he2, pos2, rot2, shape1, he1, pos1, rot1, dt):
    """The pair's shape contact at prediction 0 with the cast shape as shape 1: n = -manifold.normal (from collider 1 towards 2), or None."""
    hq = [he2[0]] * 3 if shape2 == SHAPE_BALL else list(he2)
    a = lambda x, k: np.asarray(x, dt).reshape(1, k)
    m = CR.oracle_world(bits).contact_manifolds(np.array([shape2], np.uint8), a(hq, 3), a(pos2, 3), a(rot2, 4), np.array([shape1], np.uint8), a(he1, 3), a(pos1, 3), a(rot1, 4),
                                                np.zeros(1, dt))
    if int(m["point_count"][0]) == 0:
        return None
    return tuple(-dt(x) for x in m["normal"][0])


def entry_hit(bits, entry, scene, state, dt_step, margin, info=None):
    """Steps 1-5 for one entry: (toi, hit collider slot | None, tested).  scene: colliders (entity, body, shape, half_extents, child), pairs
    [(slot1, slot2)] in insertion order, rb_type, body_flags.  state: position, rotation (step start), linear_velocity, angular_velocity."""
    dt = np.float32 if bits == 32 else np.float64
    b1 = int(entry["body"])
    has_sb = has_solver_body(scene["rb_type"], scene["body_flags"])
    cols = scene["colliders"]
    if not has_sb[b1]:
        return dt(0), None, 0
    own = [s for s in range(len(cols["body"])) if cols["body"][s] == b1 and not cols["child"][s]]
    if not own:
        return dt(0), None, 0
    c1 = own[0]
    # the reference's `neighbors`: outgoing edges newest first, then incoming newest first
    pairs = list(scene["pairs"])
    edges = [(k, p[1]) for k, p in reversed(list(enumerate(pairs))) if p[0] == c1] + [(k, p[0]) for k, p in reversed(list(enumerate(pairs))) if p[1] == c1]
    lt, at = dt(entry["linear_threshold"]), dt(entry["angular_threshold"])
    lin2, ang2 = lt * lt, at * at
    v1, w1 = _v(state["linear_velocity"][b1], dt), _v(state["angular_velocity"][b1], dt)
    pos1, rot1 = _v(state["position"][b1], dt), _v(state["rotation"][b1], dt)
    shape1, he1 = int(cols["shape"][c1]), _v(cols["half_extents"][c1], dt)
    min_toi, winner, tested = dt_step, None, 0
    unbounded = not (margin < np.finfo(dt).max)
    with np.errstate(all="ignore"):
        for _, c2 in edges:
            b2 = int(cols["body"][c2])
            if cols["child"][c2] or shape1 == SHAPE_HOST or int(cols["shape"][c2]) == SHAPE_HOST:
                continue
            if not entry["include_dynamic"] and scene["rb_type"][b2] == RB_DYNAMIC:
                continue
            zero = (dt(0), dt(0), dt(0))
            v2 = _v(state["linear_velocity"][b2], dt) if has_sb[b2] else zero
            w2 = _v(state["angular_velocity"][b2], dt) if has_sb[b2] else zero
            dw, dv = tuple(a - b for a, b in zip(w1, w2)), tuple(a - b for a, b in zip(v1, v2))
            if _len2(dw) < ang2 and _len2(dv) < lin2:
                continue
            tested += 1
            shape2, he2 = int(cols["shape"][c2]), _v(cols["half_extents"][c2], dt)
            pos2, rot2 = _v(state["position"][b2], dt), _v(state["rotation"][b2], dt)
            d = tuple(a - b for a, b in zip(v2, v1))
            hit, t = pair_cast(shape2, he2, pos2, rot2, d, dt_step, shape1, he1, pos1, rot1, dt)
            if not hit:
                continue
            if t == dt(0):
                if info is not None:
                    info.setdefault("origin", []).append(c2)
                if unbounded:
                    continue
                n = origin_contact_normal(bits, shape2, he2, pos2, rot2, shape1, he1, pos1, rot1, dt)
                if n is not None and d[0] * n[0] + d[1] * n[1] + d[2] * n[2] >= dt(0):
                    continue
                hit, t = pair_cast(SHAPE_BALL, (margin, margin, margin), pos2, rot2, d, dt_step, shape1, he1, pos1, rot1, dt)
                if not hit:
                    continue
            # (every pair is cast with max_distance = dt; the reference narrows it to min_toi: the same winner under strict <)
            if t > dt(0) and t < dt_step and t < min_toi:
                min_toi, winner = t, c2
    if winner is None:
        return dt(0), None, tested
    return min_toi, winner, tested


def apply_serial(bits, hits, scene, state):
    """The reference's loop body after the search, entry by entry: hits = [(b1, b2 | None, toi)] in list order; entries without a hit are
    (b1, None, None).  Returns (delta_position, delta_rotation) arrays."""
    dt = np.float32 if bits == 32 else np.float64
    has_sb = has_solver_body(scene["rb_type"], scene["body_flags"])
    dp = np.array(state["delta_position"], dt).copy()
    dq = np.array(state["delta_rotation"], dt).copy()
    with np.errstate(all="ignore"):
        for b1, b2, toi in hits:
            if toi is None:
                continue
            t = dt(toi) * dt(1.0001)
            for b in (b1, b2):
                if b is None or not has_sb[b]:
                    continue   # (the reference's dummy SolverBody)
                v, w = _v(state["linear_velocity"][b], dt), _v(state["angular_velocity"][b], dt)
                dp[b] = [t * v[0], t * v[1], t * v[2]]
                dq[b] = qmul(from_scaled_axis((w[0] * t, w[1] * t, w[2] * t), dt), _v(dq[b], dt), dt)
    return dp, dq


def swept_ccd(bits, entries, scene, state, dt_ns, margin_cfg, length_unit=1.0, info=None):
    """The whole pass: (records in list order, delta_position, delta_rotation).  entries: a list of dicts (body, include_dynamic,
    linear_threshold, angular_threshold).  margin_cfg: avn_config::default_speculative_margin."""
    dt = np.float32 if bits == 32 else np.float64
    fmax = np.finfo(dt).max
    margin = fmax if margin_cfg >= float(fmax) else dt(length_unit) * dt(margin_cfg)
    dt_step = dt_adjusted(dt_ns, dt)
    rec = np.zeros(len(entries), result_dtype(bits))
    hits = []
    cols = scene["colliders"]
    for i, e in enumerate(entries):
        toi, c2, tested = entry_hit(bits, e, scene, state, dt_step, margin, info)
        rec[i]["tested"] = tested
        if c2 is None:
            rec[i]["toi"] = 0; rec[i]["hit_collider"] = MISS; rec[i]["hit_body"] = -1
            hits.append((int(e["body"]), None, None))
        else:
            rec[i]["toi"] = toi; rec[i]["hit_collider"] = cols["entity"][c2]; rec[i]["hit_body"] = cols["body"][c2]
            hits.append((int(e["body"]), int(cols["body"][c2]), toi))
    dp, dq = apply_serial(bits, hits, scene, state)
    return rec, dp, dq
