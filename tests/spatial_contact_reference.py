"""Brute force of avn_spatial_shape_contacts / avn_spatial_depenetrate (include/avian_mi355x_spatial.h, "shape contacts" and "depenetration").

No geometry is restated here.  Per query the brute force applies the filter (mask, excluded entities, candidate, sensor), the AABB
precondition with spatial_query_reference.shape_aabb in the world's dtype, ONE call of the CPU oracle's contact_manifolds (helpers.oracle_lib(),
the query as shape 1) over the surviving colliders, and the last-maximum fold over each manifold's raw points; records come in ascending
collider index.  `depenetrate` is MoveAndSlide::depenetrate_intersections in numpy scalars of the world's dtype."""
from __future__ import annotations

import numpy as np

from avian_amd.spatial_query import MAX_HITS, depenetration_dtype, shape_contact_dtype
from helpers import F, oracle_lib
import spatial_query_reference as R
import spatial_shape_reference as S
from spatial_query_reference import MISS

_worlds = {}


def oracle_world(bits):
    """One oracle world per scalar width: contact_manifolds is a stateless batch query."""
    if bits not in _worlds:
        _worlds[bits] = F.World(oracle_lib(), F.default_config(bits, substeps=4))
    return _worlds[bits]


def _bits(dt):
    return 32 if dt == np.float32 else 64


def deepest(penetration, count):
    """ContactManifold::find_deepest_contact as a fold over the raw points in emission order: the later point wins a tie."""
    best = 0
    for k in range(1, count):
        if not (penetration[best] > penetration[k]):
            best = k
    return best


def precondition(s: R.Snapshot, shape, he, pos, rot, prediction):
    """(b) per (query, collider): the query's shape_aabb grown by its prediction against the collider's shape_aabb, both exact boxes."""
    dt = s.dt
    cols = lambda a, k: tuple(np.asarray(a, dt).reshape(-1, k)[:, i] for i in range(k))
    p = np.asarray(prediction, dt)
    with np.errstate(all="ignore"):
        a, b = R.shape_aabb(np.asarray(shape), cols(he, 3), cols(pos, 3), cols(rot, 4), dt)
        qmin, qmax = tuple(x - p for x in a), tuple(x + p for x in b)
        mn, mx = R.shape_aabb(s.shape, s.he, s.pos, s.rot, dt)
        ok = np.ones((len(p), s.n), bool)
        for i in range(3):
            ok &= (mn[i][None, :] <= qmax[i][:, None]) & (mx[i][None, :] >= qmin[i][:, None])
    return ok


def contact_lists(s: R.Snapshot, shape, half_extents, position, rotation, prediction, mask=None, excluded=(), sensor=None, skip_sensors=False):
    """Per query the full list of contact records in ascending collider index (a list of structured arrays)."""
    dt = s.dt
    bits = _bits(dt)
    rd = shape_contact_dtype(bits)
    ok, he, pos, rot = S.shape_valid(shape, half_extents, position, rotation, dt)
    shape = np.asarray(shape)
    n = len(shape)
    pred = np.broadcast_to(np.asarray(prediction, dt), (n,)).copy()
    with np.errstate(all="ignore"):
        ok = ok & np.isfinite(pred) & (pred >= 0)
    cand = R._masks(s, n, mask, excluded, ok)
    if skip_sensors and sensor is not None:
        cand = cand & ~(np.asarray(sensor) != 0)[None, :]
    with np.errstate(all="ignore"):
        cand = cand & precondition(s, np.where(ok, shape, 0), np.where(ok[:, None], he, 0), np.where(ok[:, None], pos, 0),
                                   np.where(ok[:, None], rot, [0, 0, 0, 1]), np.where(ok, pred, 0))
    qi, ci = np.nonzero(cand)
    out = [np.zeros(0, rd) for _ in range(n)]
    if not len(qi):
        return out
    cpos, crot, che = np.stack(s.pos, 1), np.stack(s.rot, 1), np.stack(s.he, 1)
    m = oracle_world(bits).contact_manifolds(shape[qi].astype(np.uint8), he[qi], pos[qi], rot[qi], s.shape[ci].astype(np.uint8), che[ci], cpos[ci], crot[ci], pred[qi])
    rows = [[] for _ in range(n)]
    for j in range(len(qi)):
        cnt = int(m["point_count"][j])
        if cnt == 0:
            continue
        k = deepest(m["penetration"][j], cnt)
        rec = np.zeros((), rd)
        rec["collider"] = ci[j]; rec["entity"] = s.entity[ci[j]]; rec["penetration"] = m["penetration"][j, k]
        rec["normal"] = -m["normal"][j]; rec["point"] = m["point"][j, k]; rec["anchor1"] = m["anchor1"][j, k]; rec["anchor2"] = m["anchor2"][j, k]
        rows[qi[j]].append(rec)
    for q in range(n):
        if rows[q]:
            out[q] = np.array(rows[q], rd)
    return out


def pad(lists, cap, bits):
    """(records [n, cap] MISS-padded, true counts [n]) of per-query lists."""
    rd = shape_contact_dtype(bits)
    n = len(lists)
    rec = np.zeros((n, cap), rd)
    rec["collider"] = MISS; rec["entity"] = MISS
    count = np.zeros(n, np.uint32)
    for q, l in enumerate(lists):
        count[q] = len(l)
        k = min(cap, len(l))
        rec[q, :k] = l[:k]
    return rec, count


def shape_contacts(s: R.Snapshot, shape, half_extents, position, rotation, prediction, cap, **kw):
    """avn_spatial_shape_contacts by brute force."""
    return pad(contact_lists(s, shape, half_extents, position, rotation, prediction, **kw), cap, _bits(s.dt))


def depenetrate(records, skin_width, max_error, rejection, iterations, bits):
    """depenetrate_intersections over one query's records (at most MAX_HITS are read): (fixup xyz in the world's dtype, passes started)."""
    dt = np.float32 if bits == 32 else np.float64
    skin, max_error, rejection = dt(skin_width), dt(max_error), dt(rejection)
    fx = [dt(0), dt(0), dt(0)]
    it = 0
    with np.errstate(all="ignore"):
        while it < iterations:
            it += 1
            total = dt(0)
            for r in records[:MAX_HITS]:
                dist = dt(r["penetration"]) + skin
                if dist > rejection:
                    continue
                nv = [dt(np.float32(x)) for x in r["normal"]]    # Dir is f32: a no-op in an f32 world
                diff = dist - (fx[0] * nv[0] + fx[1] * nv[1] + fx[2] * nv[2])
                err = diff if diff > dt(0) else dt(0)
                total = total + err
                fx = [fx[i] + err * nv[i] for i in range(3)]
            if total < max_error:
                break
    return fx, it


def depenetrations(records, counts, skin_width, max_error, rejection, iterations, bits):
    """avn_spatial_depenetrate's records from contact records [n, MAX_HITS] and true counts [n]."""
    out = np.zeros(len(counts), depenetration_dtype(bits))
    if iterations == 0:
        return out
    for q, c in enumerate(counts):
        fx, it = depenetrate(records[q, :min(int(c), MAX_HITS)], skin_width, max_error, rejection, iterations, bits)
        out[q]["fixup"] = fx; out[q]["count"] = c; out[q]["iterations_run"] = it; out[q]["truncated"] = 1 if c > MAX_HITS else 0
    return out
