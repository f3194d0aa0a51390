"""GPU: the staging arena behind the host-facing calls (World<T>::StagePlan, avian_amd/csrc/avn_stage.h).  One world reuses one arena for calls of
very different sizes and array lists; whatever an earlier call left there, every answer has to be the one a world that never used its arena
gives, byte for byte.  Optional outputs and the caller's own device pointers take no arena space and change no other output."""
import ctypes as C

import numpy as np
import pytest

from avian_amd.spatial_query import MISS, SpatialQuery
from helpers import F, hip_lib, random_unit_quats

pytestmark = pytest.mark.gpu

STEPS = 3
SIZES = (65, 1, 0, 64, 63, 65)   # rays, shapes, casts, points or contact ids of a call
SIZED = ("cast_rays", "shape_intersections", "cast_shapes", "project_points", "contacts_download")
UNSIZED = ("bodies_download", "solver_bodies_download")


def scene():
    """Eight cuboids and one ball resting on a static floor."""
    m = 10
    pos = np.zeros((m, 3)); he = np.zeros((m, 3)); shape = np.zeros(m, np.uint8)
    pos[0] = [0, -0.5, 0]; he[0] = [8, 0.5, 8]
    for k in range(1, m):
        i, j = divmod(k - 1, 3)
        he[k] = [0.4 + 0.01 * k, 0.5, 0.45]
        pos[k] = [1.25 * (i - 1), 0.5, 1.25 * (j - 1)]
    shape[9] = F.SHAPE_BALL; he[9] = [0.5, 0, 0]
    rot = np.tile([0.0, 0, 0, 1], (m, 1))
    rb = np.zeros(m, np.uint8); rb[0] = F.RB_STATIC
    mass = np.where(shape == F.SHAPE_BALL, 4 / 3 * np.pi * he[:, 0] ** 3, 8 * he.prod(1).clip(1e-9))
    ii = np.zeros((m, 6))
    for k in range(1, m):
        hx, hy, hz = he[k]
        d = [2 / 5 * mass[k] * hx * hx] * 3 if shape[k] == F.SHAPE_BALL else [mass[k] / 3 * (hy * hy + hz * hz), mass[k] / 3 * (hx * hx + hz * hz), mass[k] / 3 * (hx * hx + hy * hy)]
        ii[k] = [1 / d[0], 0, 0, 1 / d[1], 0, 1 / d[2]]
    inv_mass = 1.0 / mass; inv_mass[0] = 0.0
    bodies = dict(position=pos, rotation=rot, linear_velocity=np.zeros((m, 3)), angular_velocity=np.zeros((m, 3)), inv_mass=inv_mass, inv_inertia_local=ii, rb_type=rb)
    colliders = dict(entity_index=np.arange(m, dtype=np.uint32) + 100, body=np.arange(m, dtype=np.int32), shape=shape, half_extents=he)
    return bodies, colliders


def fresh(bits):
    """(world, its spatial queries, the contact ids of its constraints): the closed loop over scene(), stepped until contacts exist, snapshot taken."""
    bodies, colliders = scene()
    w = F.World(hip_lib(), F.default_config(bits, substeps=4))
    w.bodies_upload(**bodies); w.colliders_upload(**colliders)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.6, restitution=0.0)
    w.pipeline_enable()
    for _ in range(STEPS):
        w.step()
    sq = SpatialQuery(w)
    sq.update()
    _, ids = w.pipeline_handles()
    assert ids.size >= 9   # every body rests on the floor
    return w, sq, ids


def query_shapes(rng, n):
    shape = (rng.random(n) < 0.5).astype(np.uint8)
    he = rng.uniform(0.1, 0.6, (n, 3))
    pos = rng.uniform([-2.5, 0.0, -2.5], [2.5, 2.0, 2.5], (n, 3))
    return shape, he, pos, random_unit_quats(rng, n)


def call(kind, size, w, sq, ids, dev=False):
    """One call of `kind` with `size` items (inputs fixed by kind and size); its outputs as a list of byte strings."""
    rng = np.random.default_rng(1000 * size + (SIZED + UNSIZED).index(kind))
    if dev:
        import torch
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()
    else:
        t = lambda a: a
    s = lambda a: np.asarray(a, w.dtype)
    if kind == "cast_rays":
        o = rng.uniform([-2.5, 2.0, -2.5], [2.5, 3.0, 2.5], (size, 3)); d = rng.normal(size=(size, 3)) * [0.3, 0, 0.3] + [0, -1, 0]
        out = [sq.cast_rays(t(s(o)), t(s(d / np.linalg.norm(d, axis=1, keepdims=True))))]
    elif kind == "shape_intersections":
        shape, he, pos, rot = query_shapes(rng, size)
        out = list(sq.shape_intersections(t(shape), t(s(he)), t(s(pos)), t(s(rot)), 4))
    elif kind == "cast_shapes":
        shape, he, pos, rot = query_shapes(rng, size)
        out = [sq.cast_shapes(t(shape), t(s(he)), t(s(pos + [0, 2.5, 0])), t(s(rot)), t(s(np.tile([0.0, -1, 0], (size, 1)))))]
    elif kind == "project_points":
        out = [sq.project_points(t(s(rng.uniform([-2.5, 0.0, -2.5], [2.5, 2.0, 2.5], (size, 3)))), t((rng.random(size) < 0.5).astype(np.uint8)))]
    elif kind == "contacts_download":
        out = list(w.contacts_download(np.resize(ids, size)).values())
    elif kind == "bodies_download":
        out = list(w.bodies_download().values())
    else:
        out = list(w.solver_bodies_download().values())
    return [(a.cpu().numpy() if dev else a).tobytes() for a in out]


@pytest.mark.parametrize("bits", [32, 64])
def test_arena_reuse_across_sizes(bits):
    # every sized kind meets at least three of the sizes; the downloads (their size is the world's) sit between them
    seq = [(kind, size) for i, size in enumerate(SIZES) for kind in [SIZED[(i + k) % 5] for k in range(3)] + [UNSIZED[i % 2]]]
    assert {k for k, _ in seq} == set(SIZED + UNSIZED) and all(len({n for k, n in seq if k == kind}) >= 3 for kind in SIZED)
    w, sq, ids = fresh(bits)
    got = [call(kind, size, w, sq, ids) for kind, size in seq]
    hits = 0
    for (kind, size), g in zip(seq, got):
        w2, sq2, ids2 = fresh(bits)
        assert np.array_equal(ids2, ids)
        ref = call(kind, size, w2, sq2, ids2)
        w2.close()
        assert [len(b) for b in g] == [len(b) for b in ref] and g == ref, f"{kind} with {size} items differs from a fresh world's answer"
        if kind == "cast_rays":
            hits += int((np.frombuffer(g[0], sq.hit_dtype)["collider"] != MISS).sum())
    assert hits > 100   # (the rays do look at the scene)
    w.close()


def one_field_at_a_time(fn, cls, full, head=()):
    """The C call `fn(*head, &out)` once per field of `cls` with only that pointer set: the bytes of `full[field]`."""
    for name, _ in cls._fields_:
        a = np.full_like(full[name], 0x5A if full[name].dtype.itemsize == 1 else 77)
        o = cls(**{name: F._ptr(a)})
        st = fn(*head, C.byref(o))
        assert st == 0, f"{cls.__name__}.{name}: status {st}"
        assert a.tobytes() == full[name].tobytes(), f"{cls.__name__}.{name} alone differs from the call with every field"


@pytest.mark.parametrize("bits", [32, 64])
def test_optional_outputs_and_device_pointers(bits):
    w, sq, ids = fresh(bits)
    lib = w.lib
    full = w.contacts_download(ids)
    assert full["point_count"].any() and len(full) == len(F.avn_contacts_out._fields_)
    one_field_at_a_time(lib.fn("contacts_download"), F.avn_contacts_out, full, (w.handle, F._ptr(ids), ids.size))
    full = w.solver_bodies_download()
    one_field_at_a_time(lib.fn("solver_bodies_download"), F.avn_solver_bodies_out, full, (w.handle,))
    # contact_manifolds: every body against the floor and against its neighbour
    b, c = scene()
    i1 = np.r_[np.arange(1, 10), np.arange(1, 9)]; i2 = np.r_[np.zeros(9, int), np.arange(2, 10)]
    n = len(i1)
    ins = [np.ascontiguousarray(a) for a in (c["shape"][i1], c["half_extents"][i1].astype(w.dtype), b["position"][i1].astype(w.dtype), b["rotation"][i1].astype(w.dtype),
                                               c["shape"][i2], c["half_extents"][i2].astype(w.dtype), b["position"][i2].astype(w.dtype), b["rotation"][i2].astype(w.dtype),
                                               np.full(n, 0.25, w.dtype))]
    full = w.contact_manifolds(*ins)
    assert full["point_count"][:9].all()
    pin = F.avn_shape_pairs(n, *[F._ptr(a) for a in ins])
    one_field_at_a_time(lib.fn("contact_manifolds"), F.avn_query_manifolds_out, full, (w.handle, C.byref(pin)))
    # the spatial calls: the caller's device buffers (torch tensors) instead of host arrays, the same records
    for kind in SIZED[:4]:
        host = call(kind, 65, w, sq, ids)
        assert call(kind, 65, w, sq, ids, dev=True) == host, f"{kind}: AVN_SPATIAL_DEVICE_POINTERS changes the answer"
    w.close()
