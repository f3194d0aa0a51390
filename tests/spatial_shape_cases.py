"""Hand-computed cases of point projection and shape intersection (include/avian_mi355x_spatial.h), shared by test_spatial_shapes_cpu.py
(the numpy restatement) and test_gpu_spatial_shapes.py (the device).

The world: five static bodies far from each other, one collider each.
  0  cuboid he (1, 2, 3) at (10, 0, 0), rotation (1/2, 1/2, 1/2, 1/2): 120 degrees about (1, 1, 1), which maps local x -> world y, local y ->
     world z, local z -> world x and is exact in binary floating point.  Its world box is [7, 13] x [-1, 1] x [-2, 2].
  1  ball r = 2 at (-10, 0, 0)
  2, 3  two identical cubes he 1 at (0, 20, 0)
  4  cube he 1 at (40, 0, 3), rotated 45 degrees about y
Every coordinate of the first four is a small dyadic number, so every expected value below is exact in f32 and f64 unless it says sqrt."""
from __future__ import annotations

import numpy as np

from spatial_scenes import bodies_of
import spatial_query_reference as R

S22, C22 = np.sin(np.pi / 8), np.cos(np.pi / 8)    # half of 45 degrees


def world():
    pos = [[10, 0, 0], [-10, 0, 0], [0, 20, 0], [0, 20, 0], [40, 0, 3]]
    rot = [[0.5, 0.5, 0.5, 0.5], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, S22, 0, C22]]
    cols = dict(entity_index=np.arange(700, 705, dtype=np.uint32), body=np.arange(5, dtype=np.int32),
                shape=np.array([R.SHAPE_CUBOID, R.SHAPE_BALL, R.SHAPE_CUBOID, R.SHAPE_CUBOID, R.SHAPE_CUBOID], np.uint8),
                half_extents=np.array([[1, 2, 3], [2, 0, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1]], float))
    tf = dict(is_child=np.zeros(5, np.uint8), translation=np.zeros((5, 3)), rotation=np.tile([0.0, 0, 0, 1], (5, 1)))
    return bodies_of(pos, rot), cols, tf


# (name, point, solid, collider, is_inside, projected point, distance or ("sqrt", x))
PROJECTIONS = [
    ("outside a face of the rotated cuboid", (15, 0.5, 1), 1, 0, 0, (13, 0.5, 1), 2.0),
    ("outside an edge", (15, 3, 1), 1, 0, 0, (13, 1, 1), ("sqrt", 8.0)),
    ("outside a corner", (15, 3, 5), 0, 0, 0, (13, 1, 2), ("sqrt", 17.0)),
    ("inside, solid: the point itself", (11, 0.25, 0.5), 1, 0, 1, (11, 0.25, 0.5), 0.0),
    # local point (0.25, 0.5, 1): margins 0.75, 1.5, 2 -> the +x local face, which is world y = 1
    ("inside, hollow: the nearest face", (11, 0.25, 0.5), 0, 0, 1, (11, 1, 0.5), 0.75),
    # local point (0.5, 1.5, 0): margins 0.5, 0.5, 3 -> x beats y
    ("inside, hollow, equidistant from two faces: x beats y", (10, 0.5, 1.5), 0, 0, 1, (10, 1, 1.5), 0.5),
    ("a hollow ball's centre: (0, r, 0)", (-10, 0, 0), 0, 1, 1, (-10, 2, 0), 2.0),
    ("a solid ball's centre", (-10, 0, 0), 1, 1, 1, (-10, 0, 0), 0.0),
    ("outside a ball", (-10, 0, 5), 1, 1, 0, (-10, 0, 2), 3.0),
    ("two identical colliders: the lower index", (0, 23, 0), 1, 2, 0, (0, 21, 0), 2.0),
    ("inside two identical colliders, solid: the lower index at distance 0", (0.5, 20, 0), 1, 2, 1, (0.5, 20, 0), 0.0),
]


def projection_arrays():
    pts = np.array([c[1] for c in PROJECTIONS], float)
    solid = np.array([c[2] for c in PROJECTIONS], np.uint8)
    return pts, solid


def expected_projections(dt):
    from avian_amd.spatial_query import projection_dtype
    out = np.zeros(len(PROJECTIONS), projection_dtype(32 if dt == np.float32 else 64))
    for i, (_, _, _, col, inside, pt, dist) in enumerate(PROJECTIONS):
        d = np.sqrt(dt(dist[1])) if isinstance(dist, tuple) else dt(dist)
        out[i] = (col, 700 + col, inside, pt, d)
    return out


def past(x, towards, dt):
    return float(np.nextafter(dt(x), dt(towards)))


def shape_cases(dt):
    """(name, shape, half extents, position, rotation, expected collider ids) in the scalar type dt (the one-ulp case depends on it)."""
    ident = (0, 0, 0, 1)
    tilt_x = (S22, 0, 0, C22)   # 45 degrees about x
    return [
        ("a ball tangent to a ball", R.SHAPE_BALL, (1, 0, 0), (-7, 0, 0), ident, [1]),
        ("one ulp past tangent", R.SHAPE_BALL, (1, 0, 0), (past(-7, 0, dt), 0, 0), ident, []),
        ("a ball tangent to a cuboid's face", R.SHAPE_BALL, (1, 0, 0), (14, 0, 0), ident, [0]),
        ("a ball one ulp past the face", R.SHAPE_BALL, (1, 0, 0), (past(14, 20, dt), 0, 0), ident, []),
        ("a ball inside the cuboid", R.SHAPE_BALL, (0.25, 0, 0), (10, 0, 0), ident, [0]),
        ("a cuboid query around a ball collider's centre", R.SHAPE_CUBOID, (0.5, 0.5, 0.5), (-10, 0.25, 0), ident, [1]),
        ("a cuboid query touching a ball collider", R.SHAPE_CUBOID, (0.5, 0.5, 0.5), (-7.5, 0, 0), ident, [1]),
        ("a cuboid query one ulp off a ball collider", R.SHAPE_CUBOID, (0.5, 0.5, 0.5), (past(-7.5, 0, dt), 0, 0), ident, []),
        ("axis-aligned cuboids sharing a face", R.SHAPE_CUBOID, (1, 1, 1), (2, 20, 0), ident, [2, 3]),
        ("axis-aligned cuboids one ulp apart", R.SHAPE_CUBOID, (1, 1, 1), (past(2, 3, dt), 20, 0), ident, []),
        # a cube tilted 45 degrees about x under collider 4 (tilted 45 degrees about y, 3 above): the cubes' nearest edges run along x and y
        # and cross at distance 3 - 2 sqrt 2 = 0.17; every face axis overlaps (the tilted faces up to h = 1 + sqrt 2 + ... = 3.83)
        ("cuboids separated only along an edge-edge axis", R.SHAPE_CUBOID, (1, 1, 1), (40, 0, 0), tilt_x, []),
        ("the same pair half a unit closer", R.SHAPE_CUBOID, (1, 1, 1), (40, 0, 0.5), tilt_x, [4]),
    ]


def shape_arrays(dt):
    cs = shape_cases(dt)
    return (np.array([c[1] for c in cs], np.uint8), np.array([c[2] for c in cs], float), np.array([c[3] for c in cs], float),
            np.array([c[4] for c in cs], float), [c[5] for c in cs])
