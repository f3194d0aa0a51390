"""Numpy restatement of avn_spatial_project_velocities / avn_spatial_cast_moves / avn_spatial_move_and_slide (include/avian_mi355x_spatial.h,
"move and slide").

No geometry is restated here.  cast_moves composes spatial_cast_reference.cast_pairs (the per-pair shape cast), the CPU oracle's
contact_manifolds with spatial_contact_reference.deepest (the origin-penetration rule) and the pull-back; move_and_slide composes cast_moves,
spatial_contact_reference.contact_lists / depenetrate and project_velocity, which restates velocity_project.rs's cone projection in the
header's operation order with numpy scalars of the world's dtype.  Everything runs without a GPU."""
from __future__ import annotations

import numpy as np

from avian_amd.spatial_query import MAX_HITS, move_hit_dtype, slide_dtype, slide_hit_dtype
import spatial_cast_reference as CA
import spatial_contact_reference as CR
import spatial_query_reference as R
import spatial_shape_reference as S
from spatial_query_reference import MISS

DOT_EPSILON = 0.005
MIN_DISTANCE = 1e-4
f32 = np.float32


def _bits(dt):
    return 32 if dt == np.float32 else 64


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross3(a, b):
    """glam's cross."""
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def total_key(x):
    """Scalar::total_cmp as an integer key."""
    x = np.asarray(x)
    if x.dtype == np.float32:
        b = int(x.view(np.int32))
        return b ^ 0x7FFFFFFF if b < 0 else b
    b = int(x.view(np.int64))
    return b ^ 0x7FFFFFFFFFFFFFFF if b < 0 else b


def total_greater(a, b):
    """a > b under total_cmp; the key only where < and > do not decide (equal values, zeros of either sign, a NaN)."""
    if a > b:
        return True
    if a < b:
        return False
    return total_key(a) > total_key(b)


def dir_and_length(v):
    """Dir::new_and_length(v as f32): ((x, y, z) f32, length f32), or None when the length is not finite or not > 0."""
    with np.errstate(all="ignore"):
        x, y, z = f32(v[0]), f32(v[1]), f32(v[2])
        ln = np.sqrt(x * x + y * y + z * z)
        if not (np.isfinite(ln) and ln > f32(0)):
            return None
        return (x / ln, y / ln, z / ln), ln


def project_velocity(v, normals, dt):
    """project_velocity(v, normals): v three scalars, normals a sequence of f32 triples.  Returns three scalars of dtype dt."""
    v = [dt(x) for x in v]
    nrm = [tuple(f32(c) for c in n) for n in normals]
    if not all(np.isfinite(x) for x in v) or not all(np.isfinite(c) for n in nrm for c in n):
        return v
    nrm = [tuple(dt(c) for c in n) for n in nrm]
    eps = dt(DOT_EPSILON)
    with np.errstate(all="ignore"):
        x0 = [-x for x in v]
        s = list(x0)
        cone, n1, n2 = 0, None, None
        for _ in range(10):
            if dot3(s, s) < eps * eps or not nrm:
                break
            best, best_dot = 0, dot3(nrm[0], s)
            for k in range(1, len(nrm)):
                d = dot3(nrm[k], s)
                if not total_greater(best_dot, d):
                    best, best_dot = k, d
            if best_dot <= eps:
                break
            n = nrm[best]
            if cone == 0:
                d = dot3(n, x0)
                s = [x0[i] - d * n[i] for i in range(3)]
                n1, cone = n, 1
            elif cone == 1:
                c = cross3(n, n1)
                d, cc = dot3(x0, c), dot3(c, c)
                s = [d * c[i] / cc for i in range(3)]
                if d > dt(0):
                    n2, n1 = n1, n
                else:
                    n2 = n
                cone = 2
            else:
                c1 = cross3(n1, n)
                q1, d1 = dot3(c1, c1), dot3(x0, c1)
                c2 = cross3(n, n2)
                q2, d2 = dot3(c2, c2), dot3(x0, c2)
                if d1 <= dt(0) and d2 <= dt(0):
                    s = [dt(0), dt(0), dt(0)]
                    break
                if d1 * abs(d1) * q2 > d2 * abs(d2) * q1:
                    n2 = n
                    s = [d1 * c1[i] / q1 for i in range(3)]
                else:
                    n1 = n
                    s = [d2 * c2[i] / q2 for i in range(3)]
        return [-x for x in s]


def project_velocities(velocity, normals, counts, dt):
    """avn_spatial_project_velocities: velocity [n, 3], normals [n, stride, 3] f32, counts [n]."""
    velocity = np.asarray(velocity, dt).reshape(-1, 3)
    normals = np.asarray(normals, f32)
    out = np.zeros_like(velocity)
    for i in range(len(velocity)):
        k = min(int(counts[i]), normals.shape[1])
        out[i] = project_velocity(velocity[i], normals[i, :k], dt)
    return out


# ---- cast_move ------------------------------------------------------------------------------------------------------------------------------
def _candidates(s, n, ok, self_entity, mask, excluded, sensor):
    cand = R._masks(s, n, mask, excluded, ok)
    if sensor is not None:
        cand = cand & ~(np.asarray(sensor) != 0)[None, :]
    if self_entity is not None:
        se = np.asarray(self_entity, np.uint32)
        cand = cand & ~((s.entity[None, :] == se[:, None]) & (se != MISS)[:, None])
    return cand


def cast_moves(s: R.Snapshot, shape, half_extents, position, rotation, movement, skin_width, self_entity=None, mask=None, excluded=(), sensor=None, info=None):
    """avn_spatial_cast_moves by brute force.  info (a dict, optional) receives per query: 'ignored' / 'blocked' / 'no_contact' = colliders that
    overlapped at the start and were ignored, became hits with the contact's normal, or hits without a contact."""
    dt = s.dt
    bits = _bits(dt)
    shape = np.asarray(shape)
    n = len(shape)
    ok, he, pos, rot = S.shape_valid(shape, half_extents, position, rotation, dt)
    movement = np.asarray(movement, dt).reshape(-1, 3)
    skin = np.broadcast_to(np.asarray(skin_width, dt), (n,)).copy()
    with np.errstate(all="ignore"):
        ok = ok & np.isfinite(movement).all(1) & np.isfinite(skin) & (skin >= 0)
    dirs = np.zeros((n, 3), dt); dirs[:, 0] = 1
    dist = np.zeros(n, dt)
    for i in np.nonzero(ok)[0]:
        dl = dir_and_length(movement[i])
        if dl is not None:
            dirs[i] = [dt(c) for c in dl[0]]; dist[i] = dt(dl[1])
    with np.errstate(all="ignore"):
        hit, toi, p1, p2, n1, ok2 = CA.cast_pairs(s, shape, he, pos, rot, dirs, dist)
    hit = hit & _candidates(s, n, ok & ok2, self_entity, mask, excluded, sensor)
    P1, P2, N1 = np.stack(p1, 2), np.stack(p2, 2), np.stack(n1, 2)      # [n, C, 3]
    overlap = hit & (toi == 0) & (N1 == 0).all(2)
    qi, ci = np.nonzero(overlap)
    counts = {k: np.zeros(n, int) for k in ("ignored", "blocked", "no_contact")}
    if len(qi):
        cpos, crot, che = np.stack(s.pos, 1), np.stack(s.rot, 1), np.stack(s.he, 1)
        m = CR.oracle_world(bits).contact_manifolds(shape[qi].astype(np.uint8), he[qi], pos[qi], rot[qi], s.shape[ci].astype(np.uint8), che[ci], cpos[ci], crot[ci],
                                                    np.zeros(len(qi), dt))
        for j, (q, c) in enumerate(zip(qi, ci)):
            cnt = int(m["point_count"][j])
            if cnt == 0:
                counts["no_contact"][q] += 1
                continue
            k = CR.deepest(m["penetration"][j], cnt)
            cn = [-dt(x) for x in m["normal"][j]]
            d = [dt(x) for x in dirs[q]]
            if d[0] * cn[0] + d[1] * cn[1] + d[2] * cn[2] >= dt(0):
                hit[q, c] = False
                counts["ignored"][q] += 1
                continue
            counts["blocked"][q] += 1
            N1[q, c] = cn
            P1[q, c] = cpos[c] + m["anchor2"][j, k].astype(dt)
            P2[q, c] = m["point"][j, k]
    if info is not None:
        info.update(counts)
    out = np.zeros(n, move_hit_dtype(bits))
    out["collider"] = MISS; out["entity"] = MISS
    eps = dt(DOT_EPSILON)
    with np.errstate(all="ignore"):
        for q in range(n):
            idx = np.nonzero(hit[q])[0]
            if not len(idx):
                continue
            c = idx[np.lexsort((idx, toi[q, idx]))][0]
            nn = N1[q, c]
            safe = dt(0)
            if dist[q] != 0:
                d = dirs[q]
                dp = d[0] * (-nn[0]) + d[1] * (-nn[1]) + d[2] * (-nn[2])
                dm = dp if dp > eps else eps
                x = toi[q, c] - skin[q] / dm
                safe = x if x > dt(0) else dt(0)
            out[q] = (c, s.entity[c], safe, dist[q], tuple(P1[q, c]), tuple(P2[q, c]), tuple(nn), tuple(np.where(nn == 0, dt(0), -nn)))
    return out


# ---- move_and_slide -------------------------------------------------------------------------------------------------------------------------
def _own_removed(lists, s, self_entity, idx):
    """Per-query self exclusion of contact lists: a filter only removes candidates, so removing the records afterwards is the same list."""
    if self_entity is None:
        return lists
    se = np.asarray(self_entity, np.uint32)
    return [l[l["entity"] != se[i]] if se[i] != MISS and len(l) else l for l, i in zip(lists, idx)]


def move_and_slide(s: R.Snapshot, shape, half_extents, position, rotation, velocity, delta_time, skin_width, max_depenetration_error,
                   penetration_rejection_threshold, depenetration_iterations, move_and_slide_iterations=4, max_planes=20, plane_similarity_dot_threshold=0.999,
                   planes=None, hit_cap=0, self_entity=None, mask=None, excluded=(), sensor=None, info=None):
    """avn_spatial_move_and_slide: (slide records [n], hit records [n, hit_cap]).  info (a dict, optional) receives per character
    'max_planes' (the longest plane list of a round), 'live' (characters still live at the start of each round), and the overlap counters of the
    FIRST round's cast_move."""
    dt = s.dt
    bits = _bits(dt)
    shape = np.asarray(shape)
    n = len(shape)
    ok, he, pos_in, rot = S.shape_valid(shape, half_extents, position, rotation, dt)
    pos = pos_in.copy()
    vel = np.asarray(velocity, dt).reshape(-1, 3).copy()
    skin, thr = dt(skin_width), dt(plane_similarity_dot_threshold)
    time_left = np.full(n, dt(delta_time), dt)
    cfg_planes = [tuple(f32(c) for c in p) for p in (np.zeros((0, 3)) if planes is None else np.asarray(planes, f32).reshape(-1, 3))]
    slides = np.zeros(n, slide_dtype(bits))
    hits = np.zeros((n, hit_cap), slide_hit_dtype(bits))
    hits["collider"] = MISS; hits["entity"] = MISS
    iters, hit_count, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    most_planes = np.zeros(n, int)
    sub = lambda a, idx: None if a is None else np.asarray(a)[idx]
    valid = np.nonzero(ok)[0]

    def contacts(idx, prediction):
        with np.errstate(all="ignore"):
            lists = CR.contact_lists(s, shape[idx], he[idx], pos[idx], rot[idx], prediction, mask=sub(mask, idx), excluded=excluded, sensor=sensor,
                                     skip_sensors=sensor is not None)
        lists = _own_removed(lists, s, self_entity, idx)
        for l, i in zip(lists, idx):
            if len(l) > MAX_HITS:
                flags[i] |= 1
        return [l[:MAX_HITS] for l in lists]

    def depenetrate():
        if depenetration_iterations == 0 or not len(valid):
            pos[valid] = pos[valid] + dt(0)
            return
        for l, i in zip(contacts(valid, skin), valid):
            fx, _ = CR.depenetrate(l, skin, max_depenetration_error, penetration_rejection_threshold, depenetration_iterations, bits)
            with np.errstate(all="ignore"):
                pos[i] = [pos[i][k] + fx[k] for k in range(3)]

    def log(i, collider, entity, it, kind, point, normal, distance, collision_distance):
        k = int(hit_count[i])
        hit_count[i] += 1
        if k < hit_cap:
            hits[i, k] = (collider, entity, it, kind, tuple(point), tuple(normal), distance, collision_distance)

    depenetrate()
    live = ok.copy()
    live_per_round = []
    with np.errstate(all="ignore"):
        for it in range(move_and_slide_iterations):
            live_per_round.append(int(live.sum()))
            sweeps, dls = {}, {}
            for i in np.nonzero(live)[0]:
                sweep = [time_left[i] * vel[i][k] for k in range(3)]
                dl = dir_and_length(sweep)
                if dl is None or dt(dl[1]) < dt(MIN_DISTANCE):
                    live[i] = False
                    continue
                sweeps[i], dls[i] = sweep, dl
                iters[i] += 1
            idx = np.nonzero(live)[0]
            if not len(idx):
                continue
            cinfo = {}
            mh = cast_moves(s, shape[idx], he[idx], pos[idx], rot[idx], np.array([sweeps[i] for i in idx], dt), skin, sub(self_entity, idx), sub(mask, idx), excluded,
                            sensor, cinfo)
            if it == 0 and info is not None:
                for k, v in cinfo.items():
                    full = np.zeros(n, int); full[idx] = v
                    info[k] = full
            plane_lists, hit_of = {}, {}
            for h, i in zip(mh, idx):
                hit_of[i] = h
                if h["collider"] == MISS:
                    pos[i] = [pos[i][k] + sweeps[i][k] for k in range(3)]
                    live[i] = False
                    continue
                d, dist = [dt(c) for c in dls[i][0]], dt(dls[i][1])
                point = [h["point2"][k] + pos[i][k] for k in range(3)]
                time_left[i] = time_left[i] - time_left[i] * (h["distance"] / dist)
                pos[i] = [pos[i][k] + d[k] * h["distance"] for k in range(3)]
                nf = tuple(f32(c) for c in h["normal1"])
                log(i, h["collider"], h["entity"], it, 0, point, [dt(c) for c in nf], h["distance"], h["collision_distance"])
                plane_lists[i] = list(cfg_planes) + [nf]
            idx = np.nonzero(live)[0]
            if not len(idx):
                continue
            for l, i in zip(contacts(idx, skin * dt(2)), idx):
                pl, h = plane_lists[i], hit_of[i]
                v = [dt(c) for c in vel[i]]
                for r in l:
                    nf = tuple(f32(c) for c in r["normal"])
                    nv = [dt(c) for c in nf]
                    similar = False
                    for e in range(len(pl)):
                        if dt(nf[0] * pl[e][0] + nf[1] * pl[e][1] + nf[2] * pl[e][2]) >= thr:
                            if dot3(nv, v) < dot3([dt(c) for c in pl[e]], v):
                                pl[e] = nf
                            similar = True
                            break
                    if similar or len(pl) >= max_planes:
                        continue
                    log(i, r["collider"], r["entity"], it, 1, r["point"], nv, h["distance"], h["collision_distance"])
                    pl.append(nf)
                most_planes[i] = max(most_planes[i], len(pl))
                vel[i] = project_velocity(v, pl, dt)
    depenetrate()
    slides["position"] = pos
    slides["projected_velocity"] = vel
    slides["iterations_run"], slides["hit_count"], slides["flags"] = iters, hit_count, flags
    if info is not None:
        info["max_planes"] = most_planes
        info["live"] = live_per_round
    return slides, hits
