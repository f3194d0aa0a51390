"""numpy restatement of the casters of include/avian_mi355x_spatial.h ("Casters"): the re-aiming arithmetic in the world's dtype and the
per-caster answers.  It restates no geometry: a caster is re-aimed with spatial_query_reference's qrot / qmul / add, then answered by ONE
call of the batched references (spatial_query_reference.cast_rays / ray_hits, spatial_cast_reference.cast_shapes / shape_hits) with that
caster's own mask and its excluded list plus its self_entity, and the result is padded to hit_cap slots.

A set of casters is a dict: anchor_kind [n], anchor [n], origin [n, 3], direction [n, 3] (float32), max_distance [n], max_hits [n], hit_cap,
and optionally enabled [n], mask [n], self_entity [n] (MISS: none), excluded (a list of n arrays); ray casters add solid [n], shape casters
shape [n], half_extents [n, 3], shape_rotation [n, 4]."""
from __future__ import annotations

import numpy as np

from avian_amd.spatial_query import hit_dtype, shape_hit_dtype
import spatial_cast_reference as CR
import spatial_query_reference as R

MISS = R.MISS
WORLD, BODY, COLLIDER = 0, 1, 2


def _stack(t, dt):
    return np.stack([np.asarray(x, dt) for x in t], 1)


def reaim(s: R.Snapshot, bodies, anchor_kind, anchor, origin, direction, shape_rotation=None):
    """(global origins [n, 3] in s.dt, global directions [n, 3] float32, global shape rotations [n, 4] or None): a body anchor from the body's
    pose, a collider anchor from the snapshot's collider pose, a world anchor unchanged."""
    dt = s.dt
    kind = np.asarray(anchor_kind, np.uint8)
    n = len(kind)
    a = np.asarray(anchor, np.int64).reshape(n)
    ab, ac = np.where(kind == BODY, a, 0), np.where(kind == COLLIDER, a, 0)
    bpos = R._cols(np.asarray(bodies["position"], dt), dt, 3)
    brot = R._cols(np.asarray(bodies["rotation"], dt), dt, 4)
    pick = lambda b, c: np.where(kind == BODY, b[ab], c[ac]) if s.n else b[ab]      # (no colliders: no collider anchors)
    pos = tuple(pick(b, c) for b, c in zip(bpos, s.pos))
    rot = tuple(pick(b, c) for b, c in zip(brot, s.rot))
    o = R._cols(origin, dt, 3)
    d32 = np.asarray(direction, np.float32).reshape(n, 3)
    world = kind == WORLD
    with np.errstate(all="ignore"):
        go = R.add(pos, R.qrot(rot, o, dt))
        gd = R.qrot(rot, R._cols(d32.astype(dt), dt, 3), dt)          # widened, rotated in dt ...
        gd32 = _stack(gd, dt).astype(np.float32)                       # ... and rounded to float, not renormalised
        go = np.where(world[:, None], _stack(o, dt), _stack(go, dt))
        gd32 = np.where(world[:, None], d32, gd32)
        grot = None
        if shape_rotation is not None:
            sr = R._cols(shape_rotation, dt, 4)
            grot = np.where(world[:, None], _stack(sr, dt), _stack(R.qmul(sr, rot, dt), dt))   # the shape's rotation on the left
    return go, gd32, grot


def _filters(c, i):
    ex = list(np.asarray(c["excluded"][i], np.uint32)) if c.get("excluded") is not None else []
    own = MISS if c.get("self_entity") is None else int(c["self_entity"][i])
    if own != MISS:
        ex.append(np.uint32(own))
    mask = None if c.get("mask") is None else np.asarray(c["mask"], np.uint32)[i:i + 1]
    return mask, ex


def _live(c, i):
    k = min(int(c["max_hits"][i]), int(c["hit_cap"]))
    on = c.get("enabled") is None or bool(c["enabled"][i])
    return k if on else 0


def ray_casters(s: R.Snapshot, bodies, c):
    """(records [n, hit_cap], counts [n], global origins, global directions) of a set of ray casters."""
    dt = s.dt
    go, gd, _ = reaim(s, bodies, c["anchor_kind"], c["anchor"], c["origin"], c["direction"])
    n, cap = len(go), int(c["hit_cap"])
    hits = np.zeros((n, cap), hit_dtype(32 if dt == np.float32 else 64))
    hits["collider"] = MISS; hits["entity"] = MISS
    count = np.zeros(n, np.uint32)
    md = np.asarray(c["max_distance"], dt); solid = np.asarray(c["solid"])
    for i in range(n):
        k = _live(c, i)
        if k == 0:
            continue
        mask, ex = _filters(c, i)
        args = (s, go[i:i + 1], gd[i:i + 1].astype(dt))
        with np.errstate(all="ignore"):
            if k == 1:
                hits[i, 0] = R.cast_rays(*args, md[i:i + 1], solid[i:i + 1], mask, ex)[0]
                count[i] = hits[i, 0]["collider"] != MISS
            else:
                h, cnt = R.ray_hits(*args, k, md[i:i + 1], solid[i:i + 1], mask, ex)
                hits[i, :k] = h[0]; count[i] = cnt[0]
    return hits, count, go, gd


def shape_casters(s: R.Snapshot, bodies, c):
    """(records [n, hit_cap], counts [n], global origins, global directions, global rotations) of a set of shape casters."""
    dt = s.dt
    go, gd, grot = reaim(s, bodies, c["anchor_kind"], c["anchor"], c["origin"], c["direction"], c["shape_rotation"])
    n, cap = len(go), int(c["hit_cap"])
    hits = np.zeros((n, cap), shape_hit_dtype(32 if dt == np.float32 else 64))
    hits["collider"] = MISS; hits["entity"] = MISS
    count = np.zeros(n, np.uint32)
    md = np.asarray(c["max_distance"], dt)
    shape = np.asarray(c["shape"], np.uint8); he = np.asarray(c["half_extents"], dt).reshape(n, 3)
    for i in range(n):
        k = _live(c, i)
        if k == 0:
            continue
        mask, ex = _filters(c, i)
        args = (s, shape[i:i + 1], he[i:i + 1], go[i:i + 1], grot[i:i + 1], gd[i:i + 1].astype(dt))
        with np.errstate(all="ignore"):
            if k == 1:
                hits[i, 0] = CR.cast_shapes(*args, md[i:i + 1], mask, ex)[0]
                count[i] = hits[i, 0]["collider"] != MISS
            else:
                h, cnt = CR.shape_hits(*args, k, md[i:i + 1], mask, ex)
                hits[i, :k] = h[0]; count[i] = cnt[0]
    return hits, count, go, gd, grot
