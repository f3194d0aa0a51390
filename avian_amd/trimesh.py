"""Static triangle meshes as triangle colliders: one collider per face (parry's Triangle, a convex shape with one manifold per pair), all on one static
body, with per-edge flags from the mesh's adjacency so that the interior edges of a bag of triangles raise no ghost collisions.  The manifolds such a
collider answers with are defined in tests/triangle_collider_reference.py; today it is held as a host shape (SHAPE_HOST), on every backend."""
from __future__ import annotations

import numpy as np


def triangle_colliders(vertices, indices):
    """Per face of the mesh (`vertices` [V, 3], `indices` [F, 3], counter-clockwise seen from the side the normal points to): the local vertices
    [F, 3, 3] (a, b, c) and the edge flags [F] (uint8; bit k: edge k of ab, bc, ca is a real edge).
      a boundary edge (one face)                    -> set
      an edge shared by two faces                   -> set iff the neighbour's opposite vertex lies strictly below this face's plane (convex)
                                                       coplanar or concave -> clear
      an edge shared by more than two faces         -> set"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(indices, np.int64).reshape(-1, 3)
    tri = v[f]                                                    # [F, 3, 3]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    users = {}                                                    # undirected edge -> [(face, edge index)]
    for i in range(len(f)):
        for k in range(3):
            a, b = int(f[i, k]), int(f[i, (k + 1) % 3])
            users.setdefault((min(a, b), max(a, b)), []).append((i, k))
    flags = np.zeros(len(f), np.uint8)
    for faces in users.values():
        if len(faces) != 2:
            for i, k in faces:
                flags[i] |= 1 << k
            continue
        for (i, k), (j, kj) in (faces, faces[::-1]):
            opposite = v[f[j, (kj + 2) % 3]]                      # the neighbour's vertex that is not on the shared edge
            if np.dot(normal[i], opposite - tri[i, 0]) < 0.0:
                flags[i] |= 1 << k
    return tri, flags
