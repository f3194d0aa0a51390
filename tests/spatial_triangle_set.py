"""The case set of the spatial queries against triangle colliders, shared by tests/test_gpu_spatial_triangle_colliders.py (the queries it sends to the
device) and tests/test_spatial_triangle_host.py (the same queries paired with the mesh's faces, as rows for tests/spatial_triangle_main.cpp), plus random rows and the
row file format of that program.

The scene: scenes.trimesh_drop(n_boxes=6, n_balls=6, n_capsules=6, nx=4, nz=4) over a bumpy ground: 32 faces on the static body 0 and 18 bodies.  Body 0 is
moved and tilted, so that the faces' frame is not the world's."""
import functools

import numpy as np

from avian_amd import scenes
from helpers import random_unit_quats
import spatial_shape_reference as S
import spatial_triangle_collider_reference as TC

N = 512
CUB, BALL, CAP, TRI = 0, 1, 3, 4
I = [0.0, 0.0, 0.0, 1.0]
OPS = dict(ray=0, project=1, intersects=2, cast=3, segment=4)
W = 10


def bumpy(x, z):
    return 0.2 * np.sin(1.7 * x + 0.3) * np.cos(1.1 * z) + 0.05 * x


@functools.lru_cache(maxsize=None)
def scene():
    sc = scenes.trimesh_drop(n_boxes=6, n_balls=6, n_capsules=6, nx=4, nz=4, height_fn=bumpy, seed=11)
    sc.position[0] = [0.25, -0.125, 0.375]
    sc.rotation[0] = [0.02, 0.11, -0.04, 1.0] / np.linalg.norm([0.02, 0.11, -0.04, 1.0])
    return sc


def faces_local(sc):
    """[n_faces, 3, 3] vertices of the mesh in body 0's frame (the table's)."""
    return np.asarray(sc.vertices[:sc.n_faces], np.float64)


def faces_of(sc):
    """[n_faces, 3, 3] world vertices of the mesh (float64, for aiming)."""
    f = faces_local(sc)
    return np.array([[_qrot(sc.rotation[0], v) + sc.position[0] for v in t] for t in f])


def targets(rng, sc, n):
    """n points ON the mesh: a third inside faces, a third on edges (shared ones among them), a third at vertices -- with the face each was made from."""
    f = faces_of(sc)
    face = rng.integers(0, len(f), n)
    kind = np.arange(n) % 3
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    w[kind == 1, 2] = 0.0                                   # on edge ab
    w[kind == 1] /= w[kind == 1].sum(1, keepdims=True)
    w[kind == 2] = np.eye(3)[rng.integers(0, 3, (kind == 2).sum())]   # a vertex
    return np.einsum("nk,nkj->nj", w, f[face]), face, kind


def rays_of(rng, sc, with_face=False):
    """512 rays: from above and from below at faces, shared edges and vertices; parallel to a face's plane; origins on a face; some at the bodies; NaN lanes."""
    p, face, kind = targets(rng, sc, N)
    f = faces_of(sc)
    d = rng.normal(size=(N, 3)); d[:, 1] = -np.abs(d[:, 1]) - 0.3
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    up = np.arange(N) % 4 == 3
    d[up] = -d[up]                                           # from below: the faces are two-sided
    o = p - d * rng.uniform(0.5, 3.0, N)[:, None]
    straight = np.arange(N) % 8 == 1                         # straight down: exactly representable origins over the grid's vertices and edges
    d[straight] = [0.0, -1.0, 0.0]
    o[straight] = np.round(p[straight] * 2) / 2 + [0.0, 2.0, 0.0]
    par = np.arange(0, N, 16)                                # in the plane of its face (coplanar) or parallel above it
    for k in par:
        a, b, c = f[face[k]]
        d[k] = (b - a) / np.linalg.norm(b - a)
        o[k] = a - d[k] * 0.5 + (np.cross(b - a, c - a) * 0.3 if k % 32 else 0.0)
    on = np.arange(5, N, 32)                                 # the origin on the face
    o[on] = p[on]
    md = np.where(rng.random(N) < 0.25, rng.uniform(0.3, 3, N), np.inf)
    solid = (np.arange(N) % 2).astype(np.uint8)
    o[77, 1] = np.nan; d[78, 0] = np.inf
    return (o, d, md, solid, face) if with_face else (o, d, md, solid)


def shapes_of(rng, sc, with_face=False):
    """512 query shapes of the three kinds over faces, shared edges and vertices: resting near the surface (some overlapping it), and cast towards it from up
    to 2 m away; capsules lying along edges; invalid lanes."""
    p, face, kind = targets(rng, sc, N)
    shape = rng.choice(np.array([CUB, BALL, CAP], np.uint8), N)
    he = rng.uniform(0.1, 0.4, (N, 3))
    he[::9, 1] = 0.0
    rot = random_unit_quats(rng, N)
    rot[::4] = I
    lift = np.choose(np.arange(N) % 4, [0.05, 0.3, 0.8, 2.0])
    d = rng.normal(size=(N, 3)) * 0.3; d[:, 1] = -1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = p - d * lift[:, None]
    side = np.arange(N) % 16 == 7                            # sideways, grazing over the surface
    d[side] = [1.0, 0.0, 0.0]
    pos[side] = p[side] + [-1.5, 0.0, 0.0] + np.c_[np.zeros(side.sum()), he[side, 0] + rng.uniform(-0.02, 0.02, side.sum()), np.zeros(side.sum())]
    md = np.where(rng.random(N) < 0.3, rng.uniform(0.5, 4, N), np.inf)
    shape[[200, 300]] = CAP; he[200, 0] = -0.1; he[300, 1] = np.nan; shape[400] = 2      # invalid lanes
    return (shape, he, pos, rot, d, md, face) if with_face else (shape, he, pos, rot, d, md)


# ---- rows for tests/spatial_triangle_main.cpp ---------------------------------------------------------------------------------------------------------
def rows(op, kind, tri, pos1, rot1, he2, pos2, rot2, d, md):
    n = len(op)
    A = lambda a, k: np.asarray(a, np.float64).reshape(n, k)
    return dict(op=np.asarray(op, np.uint8), kind=np.asarray(kind, np.uint8), tri=A(tri, 9), pos1=A(pos1, 3), rot1=A(rot1, 4), he2=A(he2, 3), pos2=A(pos2, 3),
                rot2=A(rot2, 4), d=A(d, 3), md=np.asarray(md, np.float64).reshape(n))


def concat(rs):
    return {k: np.concatenate([r[k] for r in rs]) for k in rs[0]}


def gpu_case_rows(seed=1):
    """The GPU test's rays and query shapes, each paired with the face it was aimed at and with two more faces of the mesh.  The ray and projection rows take
    their origins and directions carried into body 0's frame (in float64: the program's inputs, not the kernel's own rounding of that step)."""
    sc = scene()
    rng = np.random.default_rng(seed)
    f = faces_local(sc)
    nf = len(f)
    out = []
    p0, q0 = np.asarray(sc.position[0], float), np.asarray(sc.rotation[0], float)
    qi = np.array([-q0[0], -q0[1], -q0[2], q0[3]])
    o, d, md, solid, rface = rays_of(rng, sc, True)
    shape, he, pos, rot, sd, smd, sface = shapes_of(rng, sc, True)
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    valid = np.isin(shape, [CUB, BALL, CAP]) & np.isfinite(he).all(1) & (he >= 0).all(1)
    for shift in (0, 1, 7):
        fr, fs = (rface + shift) % nf, (sface + shift) % nf   # (shift 0: the face the lane was aimed at; 1: the other face of its quad or the next quad's)
        z3, zq = np.zeros((N, 3)), np.tile(I, (N, 1))
        ol = np.array([_qrot(qi, x - p0) for x in np.nan_to_num(o)]); dl = np.array([_qrot(qi, x) for x in np.nan_to_num(d, posinf=0.0)])
        out.append({k: v[ok] for k, v in rows(np.full(N, OPS["ray"]), np.zeros(N), f[fr], z3, zq, z3, ol, zq, dl, md).items()})
        out.append({k: v[ok] for k, v in rows(np.full(N, OPS["project"]), np.zeros(N), f[fr], z3, zq, z3, ol, zq, dl, md).items()})
        for name in ("intersects", "cast"):
            out.append({k: v[valid] for k, v in rows(np.full(N, OPS[name]), shape, f[fs], np.tile(p0, (N, 1)), np.tile(q0, (N, 1)), he, pos, rot, sd, smd).items()})
    return concat(out)


def random_rows(rng, n):
    """n rows of every op: random triangles in posed collider frames, queries within a few units of them; every sixth triangle a sliver, every ninth query
    touching or crossing the face."""
    tri = rng.normal(size=(n, 3, 3)) * rng.choice([0.3, 1.0, 3.0], n)[:, None, None]
    sliver = np.arange(n) % 6 == 5
    tri[sliver, 2] = tri[sliver, 0] + (tri[sliver, 1] - tri[sliver, 0]) * 0.5 + rng.normal(size=(sliver.sum(), 3)) * 1e-3
    op = rng.integers(0, 5, n).astype(np.uint8)
    kind = rng.choice(np.array([CUB, BALL, CAP], np.uint8), n)
    pos1 = rng.normal(size=(n, 3)) * 2
    rot1 = random_unit_quats(rng, n)
    he2 = rng.uniform(0.05, 0.6, (n, 3))
    he2[::11, 1] = 0.0
    rot2 = random_unit_quats(rng, n)
    rot2[::5] = I
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    on_tri = np.einsum("nk,nkj->nj", w, tri)
    local = (op == OPS["ray"]) | (op == OPS["project"]) | (op == OPS["segment"])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(0.0, 3.0, n)
    dist[::9] = 0.0
    # (ray, projection and segment rows work in the collider's frame; the others place the query in the world, aimed at the posed triangle)
    world = np.array([_qrot(q, v) for q, v in zip(rot1, on_tri)]) + pos1
    wd = np.array([_qrot(q, v) for q, v in zip(rot1, d)])
    miss = rng.normal(size=(n, 3)) * np.where(np.arange(n) % 3 == 0, 0.6, 0.0)[:, None]
    pos2 = np.where(local[:, None], on_tri - d * dist[:, None] + miss, world - wd * dist[:, None] + miss)
    dd = np.where(local[:, None], d, wd)
    vtx = (op == OPS["project"]) & (np.arange(n) % 4 == 1)   # a projected point that IS a vertex: the one place where a random point is on the triangle exactly
    pos2[vtx] = tri[vtx, np.arange(n)[vtx] % 3]
    at_a = (op == OPS["ray"]) & (np.arange(n) % 7 == 3)      # a ray that starts AT vertex a: t = 0 exactly
    pos2[at_a] = tri[at_a, 0]
    seg = op == OPS["segment"]
    dd[seg] *= rng.uniform(0.0, 4.0, seg.sum())[:, None]
    md = np.where(rng.random(n) < 0.3, rng.uniform(0.2, 3, n), np.inf)
    return rows(op, kind, tri, pos1, rot1, he2, pos2, rot2, dd, md)


def _qrot(q, v):
    b = np.asarray(q[:3], float)
    return v * (q[3] * q[3] - b @ b) + b * (2 * (v @ b)) + np.cross(b, v) * (2 * q[3])


def write_rows(path, r, bits):
    dt = np.float32 if bits == 32 else np.float64
    with open(path, "wb") as f:
        np.array([bits, len(r["op"])], np.int32).tofile(f)
        r["op"].tofile(f); r["kind"].tofile(f)
        for k in ("tri", "pos1", "rot1", "he2", "pos2", "rot2", "d", "md"):
            np.ascontiguousarray(r[k], dt).tofile(f)


def read_answers(path, n, bits):
    dt = np.float32 if bits == 32 else np.float64
    with open(path, "rb") as f:
        hit = np.fromfile(f, np.uint8, n)
        res = np.fromfile(f, dt, W * n).reshape(n, W)
    return hit, res


def reference(r, bits):
    """The answers of spatial_triangle_collider_reference for the rows, in the program's layout."""
    dt = np.float32 if bits == 32 else np.float64
    n = len(r["op"])
    col = lambda a, k: tuple(np.asarray(a, dt).reshape(n, k)[:, i] for i in range(k))
    t9 = np.asarray(r["tri"], dt).reshape(n, 3, 3)
    tri = tuple(tuple(t9[:, k, j] for j in range(3)) for k in range(3))
    pos1, rot1, he2, pos2, d = col(r["pos1"], 3), col(r["rot1"], 4), col(r["he2"], 3), col(r["pos2"], 3), col(r["d"], 3)
    md = np.asarray(r["md"], dt)
    rot2 = np.asarray(r["rot2"], dt).reshape(n, 4)
    r2 = col(np.array([S.make_isometry_rotation(q, dt) for q in rot2], dt).reshape(n, 4), 4)
    op, kind = r["op"], r["kind"]
    hit = np.zeros(n, np.uint8)
    res = np.zeros((n, W), dt)
    put = lambda rows_, at, v: [res.__setitem__((rows_, at + j), v[j][rows_]) for j in range(3)]
    with np.errstate(all="ignore"):
        ok, t, nl = TC.tri_ray(*tri, pos2, d, dt)
        m = (op == OPS["ray"]) & ok
        hit[m] = 1; res[m, 0] = t[m]; put(m, 1, nl)
        q, rg = TC.closest_point(*tri, pos2, dt)
        m = op == OPS["project"]
        hit[m] = TC.tri_point(*tri, pos2, dt)[m]; put(m, 0, q); res[m, 3] = rg[m]
        m = op == OPS["intersects"]
        hit[m] = TC.tricol_intersects(kind, he2, r2, pos2, tri, pos1, rot1, dt)[m]
        TC.reset_rounds()
        c_hit, c_t, p1, p2, n1, rounds = TC.tricol_cast_exact(kind, he2, r2, pos2, d, md, tri, pos1, rot1, dt)
        m = (op == OPS["cast"]) & c_hit
        hit[m] = 1; res[m, 0] = c_t[m]; put(m, 1, p1); put(m, 4, p2); put(m, 7, n1)
        d2, ps, pt = TC.seg_tri_d2(*tri, pos2, d, dt)
        m = op == OPS["segment"]
        hit[m] = 1; res[m, 0] = d2[m]; put(m, 1, ps); put(m, 4, pt)
    return hit, res, np.where(op == OPS["cast"], rounds, 0)
