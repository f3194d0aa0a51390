"""The round set of swept CCD with Capsule colliders (shared by test_swept_ccd_capsule_cpu.py and tools/swept_ccd_nonlinear_rounds.py) and a batched
form of the reference that runs it in seconds.

rounds_set() is the generator of test_swept_ccd_nonlinear_cpu.rounds_set with its parameters (|v| <= 300, |omega| <= 100, dt = 1 / 60, sizes
0.02 .. 2; a quarter each general, aimed to graze, pure spin, pure translation) and at least one capsule per pair: the five role / kind
combinations (collider 1, collider 2) = cuboid - capsule, ball - capsule, capsule - ball, capsule - cuboid, capsule - capsule in equal parts.

batch_advance / batch_newton_rounds do swept_ccd_capsule_reference's arithmetic (N1 - N3 with the capsule gaps; the Linear cast) on arrays over
the pairs, float64: the same operations in the same order, element by element, so the answers are the scalar reference's bit for bit
(test_6_the_batched_advancement_is_the_reference_bit_for_bit holds a slice of the set to that).  run_pair is the scalar reference itself.

The counts below are what tools/swept_ccd_nonlinear_rounds.py --capsules measured on this set (profiles/swept_ccd_capsule_rounds.txt)."""
from __future__ import annotations

import numpy as np

import spatial_capsule_collider_reference as CC
import spatial_capsule_reference as C
import spatial_shape_reference as S
import swept_ccd_capsule_reference as CAPR
import swept_ccd_nonlinear_reference as NL
import swept_ccd_reference as CR
from spatial_query_reference import add, cross, dot, qinverse, qmul, qrot, scale, sub

ROUNDS_SEED, ROUNDS_PAIRS, ROUNDS_MEASURE_CAP = 20261021, 20000, 4096
ROUNDS_EXHAUSTED_UNDER_CAP = 4         # pairs of the set that run out of CCD_NL_ROUNDS (64) rounds
ROUNDS_NEWTON_CAPPED = 0               # Linear Newton casts of the set that end on SP_CAPSULE_ROUNDS (32)
DT_NS, TOL = 16666667, 0.005
BALL, CUBOID, CAPSULE = CAPR.SHAPE_BALL, CAPR.SHAPE_CUBOID, CAPR.SHAPE_CAPSULE
COMBOS = ((CUBOID, CAPSULE), (BALL, CAPSULE), (CAPSULE, BALL), (CAPSULE, CUBOID), (CAPSULE, CAPSULE))
_w = np.where


def rounds_set(n=ROUNDS_PAIRS, seed=ROUNDS_SEED):
    rng = np.random.default_rng(seed)
    unit = lambda: (lambda x: x / np.linalg.norm(x))(rng.normal(size=3))
    unit4 = lambda: (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    out = []
    for i in range(n):
        kind, combo = i % 4, i % 5
        shapes = list(COMBOS[combo])
        hes, radii = [], []
        for s in shapes:
            size = np.exp(rng.uniform(np.log(0.02), np.log(2.0), 3))
            hes.append((size[0], 0.0, 0.0) if s == BALL else ((size[0], size[1], 0.0) if s == CAPSULE else tuple(size)))
            radii.append(size[0] if s == BALL else (size[0] + size[1] if s == CAPSULE else float(np.linalg.norm(size))))
        rots = [unit4() for _ in range(2)]
        speed = [rng.uniform(0, 300) for _ in range(2)]
        spin = [rng.uniform(0, 100) for _ in range(2)]
        if kind == 2:
            speed = [0.0, 0.0]
        if kind == 3:
            spin = [0.0, 0.0]
        reach = (speed[0] + speed[1]) / 60 + radii[0] + radii[1]
        u = unit()
        dist = rng.uniform(0.2, 1.0) * reach + (radii[0] + radii[1]) * rng.uniform(0.0, 0.3)
        p2 = u * dist
        if kind == 1:      # body 1 flies past body 2 so that the bounding spheres about graze
            side = np.cross(u, unit()); side /= np.linalg.norm(side)
            aim = p2 + side * (radii[0] + radii[1]) * rng.uniform(0.5, 1.05)
            v1, v2 = aim / np.linalg.norm(aim) * speed[0], np.zeros(3)
        else:
            v1, v2 = (u + 0.3 * unit()) * speed[0], (-u + 0.3 * unit()) * speed[1]
        out.append(dict(kind=kind, combo=combo, shape=shapes, he=hes, pos=[np.zeros(3), p2], rot=rots, v=[v1, v2], om=[unit() * spin[0], unit() * spin[1]],
                        com=[np.zeros(3), np.zeros(3)] if i % 8 < 4 else [unit() * 0.3 * radii[0], unit() * 0.3 * radii[1]]))
    return out


def run_pair(p, cap):
    """The scalar reference on one pair (float64): ((outcome, t, rounds) of the advancement, the Newton rounds of the Linear cast)."""
    dt = np.float64
    he = [tuple(dt(x) for x in h) for h in p["he"]]
    m = [NL.motion(p["pos"][k], p["rot"][k], p["com"][k], p["v"][k], p["om"][k], CAPR.rho(p["shape"][k], he[k], dt), dt) for k in range(2)]
    d = tuple(b - a for a, b in zip(m[0]["v"], m[1]["v"]))
    dt_step = CR.dt_adjusted(DT_NS, dt)
    adv = CAPR.advance(p["shape"][0], he[0], m[0], p["shape"][1], he[1], m[1], d, dt_step, dt(TOL), dt, cap)
    f = lambda a: tuple(dt(x) for x in a)
    _, _, newton = CAPR.pair_cast(p["shape"][1], he[1], f(p["pos"][1]), f(p["rot"][1]), d, dt_step, p["shape"][0], he[0], f(p["pos"][0]), f(p["rot"][0]), dt)
    return adv, newton


# ---- the batched form --------------------------------------------------------------------------------------------------------------------------
def _cols(pairs, key, k, width):
    a = np.array([np.asarray(p[key][k], np.float64) for p in pairs], np.float64).reshape(len(pairs), width)
    return tuple(np.ascontiguousarray(a[:, j]) for j in range(width))


def _take(t, idx):
    return tuple(x[idx] for x in t)


def _length(a):
    return np.sqrt(dot(a, a))


def _sin_cos(a):
    out = [S.sin_cos(np.float64(x), np.float64) for x in a]
    return np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.float64)


def _from_scaled_axis(v):
    ln = np.sqrt((v[0] * v[0]) + (v[1] * v[1]) + (v[2] * v[2]))
    s, c = _sin_cos(ln * np.float64(0.5))
    z = ln == 0
    return (_w(z, 0.0, (v[0] / ln) * s), _w(z, 0.0, (v[1] / ln) * s), _w(z, 0.0, (v[2] / ln) * s), _w(z, 1.0, c))


def _pose(m, t):
    dt = np.float64
    q = qmul(_from_scaled_axis(scale(m["om"], t)), m["rot"], dt)
    p = sub(add(m["c0"], (t * m["v"][0], t * m["v"][1], t * m["v"][2])), qrot(q, m["com"], dt))
    return p, q


def _gap(shape1, he1, p1, q1, shape2, he2, p2, q2):
    """swept_ccd_capsule_reference.gap over arrays; every pair holds a capsule."""
    dt = np.float64
    n_pairs = len(shape1)
    g = np.zeros(n_pairs, dt)
    n = [np.zeros(n_pairs, dt) for _ in range(3)]
    cap1, cap2 = shape1 == CAPSULE, shape2 == CAPSULE
    other = _w(cap1, shape2, shape1)
    up = (0.0, 1.0, 0.0)

    def put(idx, gg, nn, ok):
        g[idx] = gg
        for j in range(3):
            n[j][idx] = _w(ok, nn[j], up[j])

    idx = np.nonzero(cap1 & cap2)[0]
    if len(idx):
        a1, b1, c1, d1 = _take(he1, idx), _take(p1, idx), _take(q1, idx), _take(he2, idx)
        b2, c2 = _take(p2, idx), _take(q2, idx)
        ri = qinverse(c1)
        r12, t12 = S.na_qmul(ri, c2), S.na_qrot(ri, sub(b2, b1), dt)
        A1, u1 = CC.capcol_core(a1[1], dt)
        A2, u2 = C.capsule_core(r12, t12, d1[1], dt)
        d2, pa, pb = CC.seg_seg_d2(A1, u1, A2, u2, dt)
        dist = np.sqrt(d2)
        diff = sub(pb, pa)
        put(idx, dist - (a1[0] + d1[0]), S.na_qrot(c1, (diff[0] / dist, diff[1] / dist, diff[2] / dist), dt), dist > 0)
    for kind in (BALL, CUBOID):
        idx = np.nonzero((cap1 ^ cap2) & (other == kind))[0]
        if not len(idx):
            continue
        first = cap1[idx]
        sel = lambda a, b: tuple(_w(first, x[idx], y[idx]) for x, y in zip(a, b))
        pc, po, hc, ho, qc, qo = sel(p1, p2), sel(p2, p1), sel(he1, he2), sel(he2, he1), sel(q1, q2), sel(q2, q1)
        if kind == BALL:
            l = qrot(qinverse(qc), sub(po, pc), dt)
            A, u = CC.capcol_core(hc[1], dt)
            _, s = C.seg_point(A, u, l, dt)
            df = sub(l, add(A, scale(u, s)))
            dist = _length(df)
            nw = qrot(qc, (df[0] / dist, df[1] / dist, df[2] / dist), dt)
            put(idx, dist - (hc[0] + ho[0]), tuple(_w(first, x, -x) for x in nw), dist > 0)
        else:
            ri = qinverse(qo)
            r, t = S.na_qmul(ri, qc), S.na_qrot(ri, sub(pc, po), dt)
            A, u = C.capsule_core(r, t, hc[1], dt)
            f, _, ps, pb = C.seg_box(A, u, ho, dt)
            dist = np.sqrt(f)
            diff = sub(ps, pb)
            nw = qrot(qo, (diff[0] / dist, diff[1] / dist, diff[2] / dist), dt)
            put(idx, dist - hc[0], tuple(_w(first, -x, x) for x in nw), dist > 0)
    return g, tuple(n)


def _tables(pairs):
    dt = np.float64
    shape = [np.array([p["shape"][k] for p in pairs]) for k in range(2)]
    he = [_cols(pairs, "he", k, 3) for k in range(2)]
    ms = []
    for k in range(2):
        pos, rot, com, v, om = (_cols(pairs, key, k, w) for key, w in (("pos", 3), ("rot", 4), ("com", 3), ("v", 3), ("om", 3)))
        rho = _w(shape[k] == BALL, he[k][0], _w(shape[k] == CAPSULE, he[k][1] + he[k][0], _length(he[k])))
        ms.append(dict(c0=add(pos, qrot(rot, com, dt)), v=v, om=om, com=com, rot=rot, R=_length(com) + rho, pos=pos))
    return shape, he, ms


def batch_advance(pairs, cap):
    """N3 over the whole set: (outcome[n], t[n], rounds[n])."""
    dt = np.float64
    shape, he, ms = _tables(pairs)
    n_pairs = len(pairs)
    d_all = sub(ms[1]["v"], ms[0]["v"])
    dt_step, tol = CR.dt_adjusted(DT_NS, dt), dt(TOL)
    t = np.zeros(n_pairs, dt)
    res = np.full(n_pairs, CAPR.EXHAUSTED, np.int64)
    rounds = np.full(n_pairs, cap, np.int64)
    active = np.arange(n_pairs)
    with np.errstate(all="ignore"):
        for r in range(cap):
            if not len(active):
                break
            sub_m = [{k: (_take(v, active) if isinstance(v, tuple) else v[active]) for k, v in m.items()} for m in ms]
            ta = t[active]
            p1, q1 = _pose(sub_m[0], ta)
            p2, q2 = _pose(sub_m[1], ta)
            g, n = _gap(shape[0][active], _take(he[0], active), p1, q1, shape[1][active], _take(he[1], active), p2, q2)
            d = _take(d_all, active)
            B = (-dot(d, n) + _length(cross(sub_m[0]["om"], n)) * sub_m[0]["R"]) + _length(cross(sub_m[1]["om"], n)) * sub_m[1]["R"]
            tn = ta + g / B
            hit = g <= tol
            miss = ~hit & (~(B > 0) | (tn > dt_step))
            stuck = ~hit & ~miss & ~(tn > ta)
            done = hit | miss | stuck
            res[active[hit | stuck]] = CAPR.HIT
            res[active[miss]] = CAPR.MISSED
            rounds[active[done]] = r + 1
            go = ~done
            t[active[go]] = tn[go]
            active = active[go]
    return res, t, rounds


def batch_newton_rounds(pairs):
    """The Newton rounds of the Linear cast (step 3: collider = c1, cast shape = c2, d = v2 - v1, max_distance = dt) of every pair; 0 where the
    cast is closed-form (a ball on either side)."""
    dt = np.float64
    shape, he, ms = _tables(pairs)
    n_pairs = len(pairs)
    out = np.zeros(n_pairs, np.int64)
    d_all = sub(ms[1]["v"], ms[0]["v"])
    r2_all = np.array([S.make_isometry_rotation(p["rot"][1], dt) for p in pairs], dt)
    r2_all = tuple(np.ascontiguousarray(r2_all[:, j]) for j in range(4))
    mx = CR.dt_adjusted(DT_NS, dt)
    with np.errstate(all="ignore"):
        for combo, (s1, s2) in enumerate(COMBOS):
            idx = np.nonzero(np.array([p["combo"] == combo for p in pairs]))[0]
            if not len(idx):
                continue
            he1, he2, pos1, pos2, rot1, r2, d = (_take(x, idx) for x in (he[0], he[1], ms[0]["pos"], ms[1]["pos"], ms[0]["rot"], r2_all, d_all))
            mxa = np.full(len(idx), mx, dt)
            if s1 != CAPSULE:
                rounds = C.capsule_cast_exact(he2[0], he2[1], r2, pos2, d, mxa, shape[0][idx], he1, pos1, rot1, dt)[5]
            elif s2 != CAPSULE:
                rounds = CC.capcol_cast_exact(shape[1][idx], he2, r2, pos2, d, mxa, he1, pos1, rot1, dt)[5]
            else:
                rounds = CC.capcol_capsule_cast_exact(he2[0], he2[1], r2, pos2, d, mxa, he1, pos1, rot1, dt)[5]
            out[idx] = rounds
    return out
