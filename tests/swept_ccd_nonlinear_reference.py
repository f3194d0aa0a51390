"""numpy restatement of SweepMode::NonLinear of swept CCD as include/avian_mi355x_ccd.h defines it (N0 - N4; k_ccd.hip's k_ccd_toi_nl and
k_ccd_origin_nl are the device's side of the same definition).

Built on swept_ccd_reference (the filters, the Linear pair test, the tie rule, `apply_serial`, from_scaled_axis), on
spatial_shape_reference (sin_cos through from_scaled_axis, nalgebra's arithmetic) and on the CPU oracle's contact_manifolds through
swept_ccd_reference.origin_contact_normal.  The three SAT sweeps are avn_narrow.h's, written here with scalars because N2 needs the axis that
attains the separation, which spatial_shape_reference's broadcasting versions do not return; test_swept_ccd_nonlinear_cpu.py holds their
separations to those versions.  Everything is computed in the world's dtype with numpy scalars, no fused multiply-adds.

`advance` returns the rounds a pair took and whether it ran out of them, so avn_swept_ccd_stats can be compared."""
from __future__ import annotations

import numpy as np

import spatial_shape_reference as S
import swept_ccd_reference as CR
from spatial_query_reference import cross, dot, qinverse, qmul, qrot
from swept_ccd_reference import MISS, RB_DYNAMIC, SHAPE_BALL, SHAPE_CUBOID

SWEEP_LINEAR, SWEEP_NON_LINEAR = 0, 1
CCD_NL_ROUNDS = 64   # avn_kernels.h
HIT, MISSED, EXHAUSTED = 1, 0, 2


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _neg(a):
    return (-a[0], -a[1], -a[2])


def _scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def _div(a, s):
    return (a[0] / s, a[1] / s, a[2] / s)


def _length(a):
    return np.sqrt(dot(a, a))


# ---- N1 ---------------------------------------------------------------------------------------------------------------------------------------
def rho(shape, he, dt):
    return dt(he[0]) if shape == SHAPE_BALL else _length(tuple(dt(x) for x in he))


def motion(pos, rot, com, v, om, rho_k, dt):
    """The body's motion: pos / rot at the step start, local centre of mass, SolverBody velocities (zeros without one)."""
    f = lambda a: tuple(dt(x) for x in a)
    pos, rot, com, v, om = f(pos), f(rot), f(com), f(v), f(om)
    return dict(c0=_add(pos, qrot(rot, com, dt)), v=v, om=om, com=com, rot=rot, R=_length(com) + dt(rho_k))


def pose(m, t, dt):
    q = qmul(CR.from_scaled_axis(_scale(m["om"], t), dt), m["rot"], dt)
    p = _sub(_add(m["c0"], (t * m["v"][0], t * m["v"][1], t * m["v"][2])), qrot(q, m["com"], dt))
    return p, q


# ---- avn_narrow.h: the SAT sweeps with the axis that attains the separation (scalars) ------------------------------------------------------------
def _iso_point(r, t, p, dt):
    return _add(S.na_qrot(r, p, dt), t)


def sat_normal_oneway(he1, he2, r, t, dt):
    best, best_dir = -dt(np.finfo(dt).max), (dt(0), dt(0), dt(0))
    ri = qinverse(r)
    for i in range(3):
        sign = np.copysign(dt(1), t[i])
        axis1 = tuple(sign if k == i else dt(0) for k in range(3))
        axis2 = S.na_qrot(ri, _neg(axis1), dt)
        pt2 = _iso_point(r, t, S.support(he2, axis2), dt)
        sep = pt2[i] * sign - he1[i]
        if sep > best:
            best, best_dir = sep, axis1
    return best, best_dir


def sat_line_separation(he1, he2, r, t, axis1, dt):
    axis1_2 = S.na_qrot(qinverse(r), axis1, dt)
    pa = S.support(he1, axis1)
    pb = _iso_point(r, t, S.support(he2, _neg(axis1_2)), dt)
    sep1 = S.na_dot(_sub(pb, pa), axis1)
    pc = S.support(he1, _neg(axis1))
    pd = _iso_point(r, t, S.support(he2, axis1_2), dt)
    sep2 = S.na_dot(_sub(pd, pc), _neg(axis1))
    return (sep1, axis1) if sep1 > sep2 else (sep2, _neg(axis1))


def sat_edge_twoway(he1, he2, r, t, dt):
    z, one = dt(0), dt(1)
    e2 = [S.na_qrot(r, u, dt) for u in ((one, z, z), (z, one, z), (z, z, one))]
    best, best_dir = -dt(np.finfo(dt).max), (z, z, z)
    eps = dt(np.finfo(dt).eps)
    for b in range(3):
        for a in range(3):
            u = e2[b]
            axis = (z, -u[2], u[1]) if a == 0 else ((u[2], z, -u[0]) if a == 1 else (-u[1], u[0], z))
            norm1 = np.sqrt(S.na_dot(axis, axis))
            if norm1 > eps:
                sep, ax = sat_line_separation(he1, he2, r, t, _div(axis, norm1), dt)
                if sep > best:
                    best, best_dir = sep, ax
    return best, best_dir


# ---- N2 ---------------------------------------------------------------------------------------------------------------------------------------
def gap(shape1, he1, p1, q1, shape2, he2, p2, q2, dt):
    """(g, n): the gap and the unit axis (world, from collider 1 towards 2) at the given poses."""
    ball1, ball2 = shape1 == SHAPE_BALL, shape2 == SHAPE_BALL
    if ball1 and ball2:
        dv = _sub(p2, p1)
        dist = _length(dv)
        n = _div(dv, dist) if dist > dt(0) else (dt(0), dt(1), dt(0))
        return dist - (he1[0] + he2[0]), n
    if ball1 or ball2:
        pc, pb, he, qc = (p2, p1, he2, q2) if ball1 else (p1, p2, he1, q1)
        r = he1[0] if ball1 else he2[0]
        l = qrot(qinverse(qc), _sub(pb, pc), dt)
        cl = tuple(-h if x < -h else (h if x > h else x) for x, h in zip(l, he))
        df = _sub(l, cl)
        dist = _length(df)
        if dist > dt(0):
            nl, g = _div(df, dist), dist - r
        else:
            m, axis = he[0] - abs(l[0]), 0
            for i in (1, 2):
                mi = he[i] - abs(l[i])
                if mi < m:
                    m, axis = mi, i
            s = np.copysign(dt(1), l[axis])
            nl, g = tuple(s if k == axis else dt(0) for k in range(3)), -r
        nw = qrot(qc, nl, dt)
        return g, (_neg(nw) if ball1 else nw)
    ri = qinverse(q1)
    r12, t12 = S.na_qmul(ri, q2), S.na_qrot(ri, _sub(p2, p1), dt)          # iso_inv_mul
    r21 = qinverse(r12)
    t21 = S.na_qrot(r21, _neg(t12), dt)                                     # iso_inverse
    sep1, d1 = sat_normal_oneway(he1, he2, r12, t12, dt)
    sep2, d2 = sat_normal_oneway(he2, he1, r21, t21, dt)
    sep3, d3 = sat_edge_twoway(he1, he2, r12, t12, dt)
    best, g = d1, sep1
    if sep2 > sep1 and sep2 > sep3:
        best, g = S.na_qrot(r12, _neg(d2), dt), sep2
    elif sep3 > sep1:
        best, g = d3, sep3
    return g, S.na_qrot(q1, best, dt)


# ---- N3 ---------------------------------------------------------------------------------------------------------------------------------------
def advance(shape1, he1, m1, shape2, he2, m2, d, dt_step, tol, dt, cap=CCD_NL_ROUNDS, trace=None):
    """Conservative advancement from t = 0: (HIT | MISSED | EXHAUSTED, t, rounds)."""
    t = dt(0)
    with np.errstate(all="ignore"):
        for r in range(cap):
            p1, q1 = pose(m1, t, dt)
            p2, q2 = pose(m2, t, dt)
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


# ---- N0 and the pass --------------------------------------------------------------------------------------------------------------------------
def pair_is_nonlinear(entry_mode, b2, listed):
    """N0.  listed: {body: mode} of the whole list."""
    return entry_mode == SWEEP_NON_LINEAR or listed.get(int(b2), SWEEP_LINEAR) == SWEEP_NON_LINEAR


def entry_hit(bits, entry, listed, scene, state, dt_step, margin, tol, stats, info=None, cap=CCD_NL_ROUNDS):
    """Steps 1 - 5 for one entry, a NonLinear pair through N1 - N4: (toi, hit collider slot | None, tested)."""
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

    def count(res, rounds):
        stats["rounds_max"] = max(stats["rounds_max"], rounds)
        stats["exhausted"] += 1 if res == EXHAUSTED else 0
        stats.setdefault("rounds", []).append(rounds)

    with np.errstate(all="ignore"):
        for _, c2 in edges:
            b2 = int(cols["body"][c2])
            shape2 = int(cols["shape"][c2])
            if cols["child"][c2] or shape1 > SHAPE_BALL or shape2 > SHAPE_BALL:
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
            if not pair_is_nonlinear(entry.get("mode", SWEEP_LINEAR), b2, listed):
                hit, t = CR.pair_cast(shape2, he2, pos2, rot2, d, dt_step, shape1, he1, pos1, rot1, dt)
                if not hit:
                    continue
                if t == dt(0):
                    if info is not None:
                        info.setdefault("origin", []).append(c2)
                    if unbounded:
                        continue
                    n = CR.origin_contact_normal(bits, shape2, he2, pos2, rot2, shape1, he1, pos1, rot1, dt)
                    if n is not None and d[0] * n[0] + d[1] * n[1] + d[2] * n[2] >= dt(0):
                        continue
                    hit, t = CR.pair_cast(SHAPE_BALL, (margin, margin, margin), pos2, rot2, d, dt_step, shape1, he1, pos1, rot1, dt)
                    if not hit:
                        continue
            else:
                stats["nonlinear_tested"] += 1
                m1 = motion(pos1, rot1, com_of(b1), v1, w1, rho(shape1, he1, dt), dt)
                m2 = motion(pos2, rot2, com_of(b2), v2, w2, rho(shape2, he2, dt), dt)
                res, t, rounds = advance(shape1, he1, m1, shape2, he2, m2, d, dt_step, tol, dt, cap)
                count(res, rounds)
                if res != HIT:
                    continue
                if t == dt(0):
                    if info is not None:
                        info.setdefault("origin", []).append(c2)
                    if unbounded:
                        continue
                    n = CR.origin_contact_normal(bits, shape2, he2, pos2, rot2, shape1, he1, pos1, rot1, dt)
                    if n is not None and d[0] * n[0] + d[1] * n[1] + d[2] * n[2] >= dt(0):
                        continue
                    mb = motion(pos2, rot2, com_of(b2), v2, w2, margin, dt)
                    res, t, rounds = advance(shape1, he1, m1, SHAPE_BALL, (margin, margin, margin), mb, d, dt_step, tol, dt, cap)
                    count(res, rounds)
                    if res != HIT:
                        continue
            if t > dt(0) and t < dt_step and t < min_toi:
                min_toi, winner = t, c2
    if winner is None:
        return dt(0), None, tested
    return min_toi, winner, tested


def swept_ccd(bits, entries, scene, state, dt_ns, margin_cfg, tol_cfg=0.005, length_unit=1.0, info=None, cap=CCD_NL_ROUNDS):
    """The whole pass: (records in list order, delta_position, delta_rotation, stats).  entries: dicts as swept_ccd_reference's plus `mode`.
    state: swept_ccd_reference's plus an optional center_of_mass.  tol_cfg: avn_config::contact_tolerance."""
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
        toi, c2, tested = entry_hit(bits, e, listed, scene, state, dt_step, margin, tol, stats, info, cap)
        rec[i]["tested"] = tested
        if c2 is None:
            rec[i]["toi"] = 0; rec[i]["hit_collider"] = MISS; rec[i]["hit_body"] = -1
            hits.append((int(e["body"]), None, None))
        else:
            rec[i]["toi"] = toi; rec[i]["hit_collider"] = cols["entity"][c2]; rec[i]["hit_body"] = cols["body"][c2]
            hits.append((int(e["body"]), int(cols["body"][c2]), toi))
    dp, dq = CR.apply_serial(bits, hits, scene, state)
    return rec, dp, dq, stats
