"""Scenes and rays for the spatial-query edge tests (test_spatial_exact_cpu.py on the CPU, test_gpu_spatial_edges.py on the device): rotated
and thin cuboids, balls and child colliders, with rays from far away aimed within +-1 % of silhouettes, edges and faces."""
from __future__ import annotations

import numpy as np

from helpers import F, random_unit_quats
import spatial_exact_geometry as X
import spatial_query_reference as R

IDENTITY = (0.0, 0.0, 0.0, 1.0)


def bodies_of(pos, rot):
    """A bodies_upload argument set: static bodies at the given poses (the spatial tests never step them)."""
    n = len(pos)
    return dict(position=np.asarray(pos, float), rotation=np.asarray(rot, float), linear_velocity=np.zeros((n, 3)), angular_velocity=np.zeros((n, 3)),
                inv_mass=np.zeros(n), inv_inertia_local=np.zeros((n, 6)), rb_type=np.full(n, F.RB_STATIC, np.uint8))


def far_scene(seed, n_bodies=24, spread=20.0, centre=(0.0, 0.0, 0.0)):
    """Bodies within +-spread of centre, each with its own collider and 0-2 child colliders.  Cuboids have half extents from 1e-3 to 2,
    some of them 0 on one axis (plates) or 1e-3 (slivers); balls have radii from 0.05 to 2."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(centre, float) + rng.uniform(-spread, spread, (n_bodies, 3))
    rot = random_unit_quats(rng, n_bodies)
    rot[: n_bodies // 6] = IDENTITY   # axis-aligned ones: zero direction components in the local frame
    body, shape, he, child, lt, lr = [], [], [], [], [], []
    for b in range(n_bodies):
        for k in range(1 + int(rng.integers(0, 3))):
            body.append(b)
            if rng.random() < 0.4:
                shape.append(R.SHAPE_BALL); he.append([rng.uniform(0.05, 2.0), 0, 0])
            else:
                h = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), 3))
                u = rng.random()
                if u < 0.15:
                    h[rng.integers(0, 3)] = 0.0
                elif u < 0.3:
                    h[rng.integers(0, 3)] = 1e-3
                shape.append(R.SHAPE_CUBOID); he.append(list(h))
            child.append(1 if k else 0)
            lt.append(list(rng.uniform(-2, 2, 3)) if k else [0, 0, 0])
            lr.append(list(random_unit_quats(rng, 1)[0]) if k else list(IDENTITY))
    c = len(body)
    cols = dict(entity_index=np.arange(1000, 1000 + c, dtype=np.uint32), body=np.array(body, np.int32), shape=np.array(shape, np.uint8),
                half_extents=np.array(he, float))
    tf = dict(is_child=np.array(child, np.uint8), translation=np.array(lt, float), rotation=np.array(lr, float))
    return bodies_of(pos, rot), cols, tf


def exact_colliders(bodies, cols, tf, dt):
    """The exact poses (spatial_exact_geometry.Collider) of the values the world holds: every input rounded to the world's scalar type."""
    r = lambda a: np.asarray(a, float).astype(dt).astype(float)
    pos, rot = r(bodies["position"]), r(bodies["rotation"])
    he, lt, lr = r(cols["half_extents"]), r(tf["translation"]), r(tf["rotation"])
    out = []
    for c in range(len(cols["shape"])):
        b = int(cols["body"][c])
        child = (lt[c], lr[c]) if tf["is_child"][c] else None
        out.append(X.Collider(int(cols["shape"][c]), he[c], pos[b], rot[b], child))
    return out


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def aimed_rays(seed, s: R.Snapshot, n, dist_lo, dist_hi):
    """n rays, each aimed at one collider (returned as `target`): 45 % within +-1 % of a ball's silhouette or a cuboid's edge, 25 % at a
    face point, 15 % at the centre, 15 % from inside the shape; origins log-uniformly dist_lo .. dist_hi from the aimed point.  A quarter of
    the rays end (max_distance) within +-1 % of the aimed point; half are solid.  `aim` (the aimed points) doubles as point queries."""
    rng = np.random.default_rng(seed)
    pos = np.stack(s.pos, 1).astype(float)
    rot = np.stack(s.rot, 1).astype(float)
    he = np.stack(s.he, 1).astype(float)
    target = rng.integers(0, s.n, n)
    d = _unit(rng.normal(size=(n, 3)))
    kind = rng.random(n)
    aim = np.empty((n, 3))
    for i in range(n):
        c = target[i]
        if s.shape[c] == R.SHAPE_BALL:
            r = he[c, 0]
            u = _unit(np.cross(d[i], rng.normal(size=3)))
            if kind[i] < 0.45:
                local = u * r * (1 + rng.uniform(-0.01, 0.01))
            elif kind[i] < 0.7:
                local = u * r * rng.uniform(0, 0.99)
            else:
                local = u * r * rng.uniform(0, 0.5) * (kind[i] < 0.85)
            aim[i] = pos[c] + local
        else:
            h = he[c]
            sgn = rng.choice([-1.0, 1.0], 3)
            free = rng.integers(0, 3)
            if kind[i] < 0.45:        # an edge, +-1 %
                local = sgn * h * (1 + rng.uniform(-0.01, 0.01, 3))
                local[free] = rng.uniform(-1, 1) * h[free]
            elif kind[i] < 0.7:       # a face
                local = rng.uniform(-1, 1, 3) * h
                local[free] = sgn[free] * h[free]
            else:                     # the centre or a point inside
                local = rng.uniform(-0.5, 0.5, 3) * h * (kind[i] >= 0.85)
            aim[i] = pos[c] + R.qrot(tuple(rot[c]), tuple(local), np.float64)
    dist = np.exp(rng.uniform(np.log(dist_lo), np.log(dist_hi), n))
    inside = kind >= 0.85
    o = aim - d * np.where(inside, 0.0, dist)[:, None]
    md = np.full(n, np.inf)
    cut = rng.random(n) < 0.25
    md[cut] = np.where(inside[cut], rng.uniform(0, 1, cut.sum()), dist[cut] * (1 + rng.uniform(-0.01, 0.01, cut.sum())))
    solid = (rng.random(n) < 0.5).astype(np.uint8)
    return o, d, md, solid, target, aim
