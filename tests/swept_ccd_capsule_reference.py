"""numpy restatement of swept CCD with Capsule colliders as include/avian_mi355x_ccd.h defines it ("capsule colliders"; k_ccd.hip's k_ccd_toi_cap,
k_ccd_toi_nl_cap, k_ccd_origin_cap and k_ccd_origin_nl_cap are the device's side of the same definition).

Built on swept_ccd_reference (the filters, the Ball / Cuboid cast, the tie rule, `apply_serial`) and swept_ccd_nonlinear_reference (N0, N1, N3, the
Ball / Cuboid gaps) by import.  A pair with a capsule goes, by role, to the pair casts of spatial_capsule_reference (a capsule cast against a
Ball / Cuboid collider) and spatial_capsule_collider_reference (anything cast against a capsule collider); its contact at prediction 0 is
capsule_collider_reference's manifold (the narrow phase's).  Those modules restate the device's operation order.  New here: the three capsule
arms of the gap N2, rho(capsule) = h + r, and the routing.  Everything is computed in the world's dtype, no fused multiply-adds.

With `capsules=False` a pair with a capsule is skipped, as a library without avn_swept_ccd_capsules_set (or with the switch off) does."""
from __future__ import annotations

import numpy as np

import capsule_collider_reference as K
import spatial_capsule_collider_reference as CC
import spatial_capsule_reference as C
import spatial_shape_reference as S
import swept_ccd_nonlinear_reference as NL
import swept_ccd_reference as CR
from spatial_query_reference import cross, dot, qinverse, qrot
from swept_ccd_nonlinear_reference import EXHAUSTED, HIT, MISSED, SWEEP_LINEAR, SWEEP_NON_LINEAR, _add, _div, _length, _neg, _scale, _sub
from swept_ccd_reference import MISS, RB_DYNAMIC, SHAPE_BALL, SHAPE_CUBOID, SHAPE_HOST

SHAPE_CAPSULE = 3
CCD_NL_ROUNDS = NL.CCD_NL_ROUNDS
SP_CAPSULE_ROUNDS = C.ROUNDS


def _arr(v, dt):
    return tuple(np.array([x], dt) for x in v)


def _sc(v, dt):
    return tuple(dt(np.asarray(x).reshape(-1)[0]) for x in v)


def rho(shape, he, dt):
    return dt(he[1]) + dt(he[0]) if shape == SHAPE_CAPSULE else NL.rho(shape, he, dt)


# ---- N2: the capsule arms -------------------------------------------------------------------------------------------------------------------
def gap(shape1, he1, p1, q1, shape2, he2, p2, q2, dt):
    """(g, n) as swept_ccd_nonlinear_reference.gap, with the capsule arms of sp_nl_gap_cap."""
    with np.errstate(all="ignore"):
        return _gap(shape1, he1, p1, q1, shape2, he2, p2, q2, dt)


def _gap(shape1, he1, p1, q1, shape2, he2, p2, q2, dt):
    cap1, cap2 = shape1 == SHAPE_CAPSULE, shape2 == SHAPE_CAPSULE
    if not (cap1 or cap2):
        return NL.gap(shape1, he1, p1, q1, shape2, he2, p2, q2, dt)
    up = (dt(0), dt(1), dt(0))
    zero = dt(0)
    if cap1 and cap2:
        ri = qinverse(q1)
        r12, t12 = S.na_qmul(ri, q2), S.na_qrot(ri, _sub(p2, p1), dt)         # iso_inv_mul
        A1, u1 = CC.capcol_core(np.array([he1[1]], dt), dt)
        A2, u2 = C.capsule_core(_arr(r12, dt), _arr(t12, dt), np.array([he2[1]], dt), dt)
        d2, pa, pb = CC.seg_seg_d2(A1, u1, A2, u2, dt)
        dist = np.sqrt(dt(d2[0]))
        n = S.na_qrot(q1, _div(_sub(_sc(pb, dt), _sc(pa, dt)), dist), dt) if dist > zero else up
        return dist - (he1[0] + he2[0]), n
    pc, po, hc, ho, qc, qo, so = (p1, p2, he1, he2, q1, q2, shape2) if cap1 else (p2, p1, he2, he1, q2, q1, shape1)
    if so == SHAPE_BALL:
        l = qrot(qinverse(qc), _sub(po, pc), dt)
        A, u = CC.capcol_core(np.array([hc[1]], dt), dt)
        _, s = C.seg_point(A, u, _arr(l, dt), dt)
        A, u, s = _sc(A, dt), _sc(u, dt), dt(s[0])
        df = _sub(l, _add(A, _scale(u, s)))
        dist = _length(df)
        if dist > zero:
            nw = qrot(qc, _div(df, dist), dt)
            n = nw if cap1 else _neg(nw)
        else:
            n = up
        return dist - (hc[0] + ho[0]), n
    ri = qinverse(qo)
    r, t = S.na_qmul(ri, qc), S.na_qrot(ri, _sub(pc, po), dt)                   # the capsule in the cuboid's frame
    A, u = C.capsule_core(_arr(r, dt), _arr(t, dt), np.array([hc[1]], dt), dt)
    f, _, ps, pb = C.seg_box(A, u, _arr(ho, dt), dt)
    dist = np.sqrt(dt(f[0]))
    if dist > zero:
        nw = qrot(qo, _div(_sub(_sc(ps, dt), _sc(pb, dt)), dist), dt)
        n = _neg(nw) if cap1 else nw
    else:
        n = up
    return dist - hc[0], n


# ---- N3 with the gap above ------------------------------------------------------------------------------------------------------------------
def advance(shape1, he1, m1, shape2, he2, m2, d, dt_step, tol, dt, cap=CCD_NL_ROUNDS, trace=None):
    """swept_ccd_nonlinear_reference.advance over this module's gap: (HIT | MISSED | EXHAUSTED, t, rounds)."""
    t = dt(0)
    with np.errstate(all="ignore"):
        for r in range(cap):
            p1, q1 = NL.pose(m1, t, dt)
            p2, q2 = NL.pose(m2, t, dt)
            g, n = gap(shape1, he1, p1, q1, shape2, he2, p2, q2, dt)
            if trace is not None:
                trace.append((t, g))
            if g <= tol:
                return HIT, t, r + 1
            B = (-dot(d, n) + _length(cross(m1["om"], n)) * m1["R"]) + _length(cross(m2["om"], n)) * m2["R"]
            if not B > dt(0):
                return MISSED, t, r + 1
            tn = t + g / B
            if tn > dt_step:
                return MISSED, t, r + 1
            if not tn > t:
                return HIT, t, r + 1
            t = tn
    return EXHAUSTED, t, cap


# ---- step 3 by role -------------------------------------------------------------------------------------------------------------------------
def pair_cast(shape2, he2, pos2, rot2, d, max_t, shape1, he1, pos1, rot1, dt):
    """The header's shape cast for one pair, capsules included: (hit, toi, Newton rounds | 0).  Collider 1 at its raw pose, the cast shape 2
    through make_isometry."""
    if shape1 != SHAPE_CAPSULE and shape2 != SHAPE_CAPSULE:
        hit, t = CR.pair_cast(shape2, he2, pos2, rot2, d, max_t, shape1, he1, pos1, rot1, dt)
        return hit, t, 0
    a = lambda v: _arr(v, dt)
    r2 = a(S.make_isometry_rotation(rot2, dt))
    mx = np.array([max_t], dt)
    with np.errstate(all="ignore"):
        if shape1 != SHAPE_CAPSULE:
            hit, toi, _, _, _, rounds = C.capsule_cast_exact(np.array([he2[0]], dt), np.array([he2[1]], dt), r2, a(pos2), a(d), mx, np.array([shape1]), a(he1), a(pos1), a(rot1), dt)
        elif shape2 != SHAPE_CAPSULE:
            hit, toi, _, _, _, rounds = CC.capcol_cast_exact(np.array([shape2]), a(he2), r2, a(pos2), a(d), mx, a(he1), a(pos1), a(rot1), dt)
        else:
            hit, toi, _, _, _, rounds = CC.capcol_capsule_cast_exact(np.array([he2[0]], dt), np.array([he2[1]], dt), r2, a(pos2), a(d), mx, a(he1), a(pos1), a(rot1), dt)
    return bool(hit[0]), dt(toi[0]), int(np.asarray(rounds).reshape(-1)[0])


def origin_contact_normal(bits, shape2, he2, pos2, rot2, shape1, he1, pos1, rot1, dt):
    """The pair's shape contact at prediction 0 with the cast shape as shape 1: n = -manifold.normal, or None.  A pair with a capsule: the
    narrow phase's capsule manifold (contact_manifolds_pair_sink<.., CAP = true>)."""
    if shape1 != SHAPE_CAPSULE and shape2 != SHAPE_CAPSULE:
        return CR.origin_contact_normal(bits, shape2, he2, pos2, rot2, shape1, he1, pos1, rot1, dt)
    hq = [he2[0]] * 3 if shape2 == SHAPE_BALL else list(he2)
    a = lambda x, k: np.asarray(x, dt).reshape(1, k)
    m = K.manifolds(np.array([shape2]), a(hq, 3), a(pos2, 3), a(rot2, 4), np.array([shape1]), a(he1, 3), a(pos1, 3), a(rot1, 4), np.zeros(1, dt), dt)
    if int(m["point_count"][0]) == 0:
        return None
    return tuple(-dt(x) for x in m["normal"][0])


# ---- the pass -------------------------------------------------------------------------------------------------------------------------------
def entry_hit(bits, entry, listed, scene, state, dt_step, margin, tol, stats, info=None, cap=CCD_NL_ROUNDS, capsules=True):
    """Steps 1 - 5 for one entry, both modes, capsule pairs included when `capsules`: (toi, hit collider slot | None, tested)."""
    dt = np.float32 if bits == 32 else np.float64
    b1 = int(entry["body"])
    has_sb = CR.has_solver_body(scene["rb_type"], scene["body_flags"])
    cols = scene["colliders"]
    if not has_sb[b1]:
        return dt(0), None, 0
    own = [s for s in range(len(cols["body"])) if cols["body"][s] == b1 and not cols["child"][s]]
    if not own:
        return dt(0), None, 0
    c1 = own[0]
    pairs = list(scene["pairs"])
    edges = [(k, p[1]) for k, p in reversed(list(enumerate(pairs))) if p[0] == c1] + [(k, p[0]) for k, p in reversed(list(enumerate(pairs))) if p[1] == c1]
    lt, at = dt(entry["linear_threshold"]), dt(entry["angular_threshold"])
    lin2, ang2 = lt * lt, at * at
    v = lambda a: tuple(dt(x) for x in a)
    zero = (dt(0), dt(0), dt(0))
    com = state.get("center_of_mass")
    com_of = lambda b: zero if com is None else v(com[b])
    v1, w1 = v(state["linear_velocity"][b1]), v(state["angular_velocity"][b1])
    pos1, rot1 = v(state["position"][b1]), v(state["rotation"][b1])
    shape1, he1 = int(cols["shape"][c1]), v(cols["half_extents"][c1])
    min_toi, winner, tested = dt_step, None, 0
    unbounded = not (margin < np.finfo(dt).max)
    allowed = (SHAPE_CUBOID, SHAPE_BALL, SHAPE_CAPSULE) if capsules else (SHAPE_CUBOID, SHAPE_BALL)
    ball = (margin, margin, margin)

    def count(res, rounds):
        stats["rounds_max"] = max(stats["rounds_max"], rounds)
        stats["exhausted"] += 1 if res == EXHAUSTED else 0
        stats.setdefault("rounds", []).append(rounds)

    with np.errstate(all="ignore"):
        for _, c2 in edges:
            b2 = int(cols["body"][c2])
            shape2 = int(cols["shape"][c2])
            if cols["child"][c2] or shape1 not in allowed or shape2 not in allowed:
                continue
            if not entry["include_dynamic"] and scene["rb_type"][b2] == RB_DYNAMIC:
                continue
            v2 = v(state["linear_velocity"][b2]) if has_sb[b2] else zero
            w2 = v(state["angular_velocity"][b2]) if has_sb[b2] else zero
            if CR._len2(_sub(w1, w2)) < ang2 and CR._len2(_sub(v1, v2)) < lin2:
                continue
            tested += 1
            he2 = v(cols["half_extents"][c2])
            pos2, rot2 = v(state["position"][b2]), v(state["rotation"][b2])
            d = _sub(v2, v1)
            if not NL.pair_is_nonlinear(entry.get("mode", SWEEP_LINEAR), b2, listed):
                hit, t, rounds = pair_cast(shape2, he2, pos2, rot2, d, dt_step, shape1, he1, pos1, rot1, dt)
                stats.setdefault("newton_rounds", []).append(rounds)
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
                    hit, t, _ = pair_cast(SHAPE_BALL, ball, pos2, rot2, d, dt_step, shape1, he1, pos1, rot1, dt)
                    if not hit:
                        continue
            else:
                stats["nonlinear_tested"] += 1
                m1 = NL.motion(pos1, rot1, com_of(b1), v1, w1, rho(shape1, he1, dt), dt)
                m2 = NL.motion(pos2, rot2, com_of(b2), v2, w2, rho(shape2, he2, dt), dt)
                res, t, rounds = advance(shape1, he1, m1, shape2, he2, m2, d, dt_step, tol, dt, cap)
                count(res, rounds)
                if res != HIT:
                    continue
                if t == dt(0):
                    if info is not None:
                        info.setdefault("origin", []).append(c2)
                    if unbounded:
                        continue
                    n = origin_contact_normal(bits, shape2, he2, pos2, rot2, shape1, he1, pos1, rot1, dt)
                    if n is not None and d[0] * n[0] + d[1] * n[1] + d[2] * n[2] >= dt(0):
                        continue
                    mb = NL.motion(pos2, rot2, com_of(b2), v2, w2, margin, dt)
                    res, t, rounds = advance(shape1, he1, m1, SHAPE_BALL, ball, mb, d, dt_step, tol, dt, cap)
                    count(res, rounds)
                    if res != HIT:
                        continue
            if t > dt(0) and t < dt_step and t < min_toi:
                min_toi, winner = t, c2
    if winner is None:
        return dt(0), None, tested
    return min_toi, winner, tested


def swept_ccd(bits, entries, scene, state, dt_ns, margin_cfg, tol_cfg=0.005, length_unit=1.0, info=None, cap=CCD_NL_ROUNDS, capsules=True):
    """The whole pass: (records in list order, delta_position, delta_rotation, stats), as swept_ccd_nonlinear_reference.swept_ccd."""
    dt = np.float32 if bits == 32 else np.float64
    fmax = np.finfo(dt).max
    margin = fmax if margin_cfg >= float(fmax) else dt(length_unit) * dt(margin_cfg)
    tol = dt(length_unit) * dt(tol_cfg)
    dt_step = CR.dt_adjusted(dt_ns, dt)
    listed = {int(e["body"]): int(e.get("mode", SWEEP_LINEAR)) for e in entries}
    stats = dict(nonlinear_tested=0, rounds_max=0, exhausted=0)
    rec = np.zeros(len(entries), CR.result_dtype(bits))
    hits = []
    cols = scene["colliders"]
    for i, e in enumerate(entries):
        toi, c2, tested = entry_hit(bits, e, listed, scene, state, dt_step, margin, tol, stats, info, cap, capsules)
        rec[i]["tested"] = tested
        if c2 is None:
            rec[i]["toi"] = 0; rec[i]["hit_collider"] = MISS; rec[i]["hit_body"] = -1
            hits.append((int(e["body"]), None, None))
        else:
            rec[i]["toi"] = toi; rec[i]["hit_collider"] = cols["entity"][c2]; rec[i]["hit_body"] = cols["body"][c2]
            hits.append((int(e["body"]), int(cols["body"][c2]), toi))
    dp, dq = CR.apply_serial(bits, hits, scene, state)
    return rec, dp, dq, stats
