"""The triangle collider kind's bindings where no GPU is needed: the oracle has no such kind (its library does not export the entry points of
include/avian_mi355x_trimesh.h), so asking it for native triangles raises; MeshScene.collider_kwargs(native_triangles=True) returns kind 4 plus the table, and
the default call is what it always was."""
import ctypes as C

import numpy as np
import pytest

from avian_amd import scenes
from helpers import F, oracle_lib

TRI = F.SHAPE_TRIANGLE


def test_the_oracle_refuses_native_triangles():
    lib = oracle_lib()
    assert not any(hasattr(lib.dll, name) for name in F.TRIMESH_SYMBOLS) and not F.declare_trimesh(lib.dll)
    sc = scenes.trimesh_drop(n_boxes=1, n_balls=1, n_capsules=1, nx=2, nz=2)
    w = F.World(lib, F.default_config(32))
    w.bodies_upload(**sc.body_kwargs())
    with pytest.raises(ValueError, match="no triangle collider kind"):
        w.colliders_upload(**sc.collider_kwargs(host_capsules=True, native_triangles=True))
    with pytest.raises(ValueError):   # without the table kind 4 is refused as ever, whatever the backend
        w.colliders_upload(**dict(sc.collider_kwargs(), shape=sc.col_shape))
    with pytest.raises(ValueError, match="no triangle collider kind"):
        w.triangle_manifolds([TRI], [[0, 0, 0]], [[0, 0, 0]], [[0, 0, 0, 1]], [F.SHAPE_BALL], [[0.3, 0, 0]], [[0.2, 0.2, 0.2]], [[0, 0, 0, 1]], 0.1, vertices1=[[0, 0, 0, 0, 0, 1, 1, 0, 0]])
    with pytest.raises(ValueError, match="no triangle collider kind"):
        w.collider_triangles_upload(np.zeros((0, 9)))
    w.colliders_upload(**sc.collider_kwargs(host_capsules=True))   # the hosted form still goes up


def test_collider_kwargs_native_triangles_returns_kind_four_and_the_table():
    sc = scenes.trimesh_drop(n_boxes=2, n_balls=1, n_capsules=1, nx=3, nz=2)
    c = len(sc.col_shape)
    kw = sc.collider_kwargs(native_triangles=True)
    assert set(kw) == {"entity_index", "body", "shape", "half_extents", "triangles"}
    assert np.array_equal(kw["shape"], sc.col_shape) and (kw["shape"] == TRI).sum() == 12 and kw["shape"].dtype == np.uint8
    t = kw["triangles"]
    assert set(t) == {"vertices", "edge_flags"} and t["vertices"].shape == (c, 9) and t["edge_flags"].shape == (c,) and t["edge_flags"].dtype == np.uint8
    assert np.array_equal(t["vertices"].reshape(c, 3, 3), sc.vertices) and np.array_equal(t["edge_flags"], sc.edge_flags) and (t["edge_flags"] <= 7).all()
    both = sc.collider_kwargs(host_capsules=True, native_triangles=True)
    assert (both["shape"][sc.col_shape == F.SHAPE_CAPSULE] == F.SHAPE_HOST).all() and (both["shape"][sc.col_shape == TRI] == TRI).all()


def test_the_default_collider_kwargs_are_unchanged():
    sc = scenes.trimesh_drop(n_boxes=2, n_balls=1, n_capsules=1, nx=3, nz=2)
    kw = sc.collider_kwargs()
    assert set(kw) == {"entity_index", "body", "shape", "half_extents"}
    tri = sc.col_shape == TRI
    assert (kw["shape"][tri] == F.SHAPE_HOST).all() and np.array_equal(kw["shape"][~tri], sc.col_shape[~tri])
    hosted = sc.collider_kwargs(host_capsules=True)
    assert (hosted["shape"][sc.col_shape == F.SHAPE_CAPSULE] == F.SHAPE_HOST).all() and "triangles" not in hosted


def test_the_struct_mirrors_have_the_headers_layout():
    assert C.sizeof(F.avn_collider_triangles) == 24 and F.avn_collider_triangles.vertices.offset == 8 and F.avn_collider_triangles.edge_flags.offset == 16
    assert C.sizeof(F.avn_triangle_pairs) == 8 + 13 * 8 and F.avn_triangle_pairs.shape1.offset == 8 and F.avn_triangle_pairs.edge_flags2.offset == 8 + 12 * 8
