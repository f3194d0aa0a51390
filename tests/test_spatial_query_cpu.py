"""CPU checks of the spatial queries (include/avian_mi355x_spatial.h): known answers of the numpy restatement of the exact per-collider
tests (tests/spatial_query_reference.py), the library's exports and the ctypes mirror of the header's structs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import REPO, hip_lib
from avian_amd import spatial_query as S
import spatial_query_reference as R

DTYPES = [np.float32, np.float64]
SQ2 = np.sqrt(0.5)


def one(shape, he, pos=(0, 0, 0), rot=(0, 0, 0, 1), dt=np.float32, child=None, memberships=None):
    """A world of one collider on one body (child: (translation, rotation) of a ColliderTransform)."""
    bodies = dict(position=np.array([pos], float), rotation=np.array([rot], float))
    cols = dict(entity_index=np.array([7], np.uint32), body=np.array([0], np.int32), shape=np.array([shape], np.uint8), half_extents=np.array([he], float))
    if memberships is not None:
        cols["memberships"] = np.array([memberships], np.uint32)
    tf = None
    if child is not None:
        tf = dict(is_child=np.array([1], np.uint8), translation=np.array([child[0]], float), rotation=np.array([child[1]], float))
    return R.Snapshot(bodies, cols, tf, dt)


def ray(s, o, d, solid=True, max_distance=np.inf, **kw):
    return R.cast_rays(s, np.array([o], float), np.array([d], float), np.array([max_distance]), np.array([solid], np.uint8), **kw)[0]


def close(a, b, dt):
    return np.allclose(np.asarray(a, float), np.asarray(b, float), rtol=0, atol=1e-5 if dt == np.float32 else 1e-12)


@pytest.mark.parametrize("dt", DTYPES)
def test_cuboid_face_hit_from_outside(dt):
    h = ray(one(R.SHAPE_CUBOID, (0.5, 0.5, 0.5), dt=dt), (0, 0, -5), (0, 0, 1))
    assert h["collider"] == 0 and h["entity"] == 7
    assert h["distance"] == dt(4.5) and list(h["normal"]) == [0, 0, -1]
    assert h["distance"].dtype == dt


@pytest.mark.parametrize("dt", DTYPES)
def test_cuboid_origin_inside_solid_and_not_solid(dt):
    s = one(R.SHAPE_CUBOID, (0.5, 0.5, 0.5), dt=dt)
    h = ray(s, (0, 0, 0.1), (0, 0, 1), solid=True)
    assert h["collider"] == 0 and h["distance"] == 0 and list(h["normal"]) == [0, 0, 0]
    h = ray(s, (0, 0, 0.1), (0, 0, 1), solid=False)
    assert h["collider"] == 0 and close(h["distance"], 0.4, dt) and list(h["normal"]) == [0, 0, 1]
    h = ray(s, (0, 0, 0.1), (0, 0, 1), solid=False, max_distance=0.3)   # the exit lies past max_distance
    assert h["collider"] == R.MISS


@pytest.mark.parametrize("dt", DTYPES)
def test_ball_head_on_and_from_inside(dt):
    s = one(R.SHAPE_BALL, (1.0, 0, 0), pos=(2, 0, 0), dt=dt)
    h = ray(s, (-3, 0, 0), (1, 0, 0))
    assert h["distance"] == dt(4) and list(h["normal"]) == [-1, 0, 0]
    h = ray(s, (2, 0, 0), (1, 0, 0), solid=False)
    assert h["distance"] == dt(1) and list(h["normal"]) == [1, 0, 0]
    h = ray(s, (2, 0, 0), (1, 0, 0), solid=True)
    assert h["distance"] == 0 and list(h["normal"]) == [0, 0, 0]
    assert ray(s, (-3, 0, 0), (-1, 0, 0))["collider"] == R.MISS          # pointing away (c > 0 && b > 0)
    assert ray(s, (-3, 1.5, 0), (1, 0, 0))["collider"] == R.MISS         # passes above (negative discriminant)
    assert ray(s, (-3, 0, 0), (1, 0, 0), max_distance=3.5)["collider"] == R.MISS


@pytest.mark.parametrize("dt", DTYPES)
def test_axis_parallel_rays_are_slabs_not_nan(dt):
    s = one(R.SHAPE_CUBOID, (0.5, 0.5, 0.5), dt=dt)
    h = ray(s, (0.2, 0.3, -5), (0, 0, 1))
    assert h["distance"] == dt(4.5) and list(h["normal"]) == [0, 0, -1]
    assert ray(s, (2, 0, -5), (0, 0, 1))["collider"] == R.MISS         # parallel to the x slab, outside it
    h = ray(s, (0.5, 0, -5), (0, 0, 1))                                   # grazing the +x face: on the slab boundary counts
    assert h["collider"] == 0 and h["distance"] == dt(4.5)


@pytest.mark.parametrize("dt", DTYPES)
def test_edge_tie_takes_the_first_axis(dt):
    s = one(R.SHAPE_CUBOID, (0.5, 0.5, 0.5), dt=dt)
    h = ray(s, (-5, -5, 0), (SQ2, SQ2, 0))   # exactly onto the edge x = y = -0.5: the x face wins the tie (strict >)
    assert h["collider"] == 0 and list(h["normal"]) == [-1, 0, 0]
    assert close(h["distance"], 4.5 / SQ2, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_rotated_cuboid(dt):
    c, sn = np.cos(np.pi / 8), np.sin(np.pi / 8)   # 45 degrees about z: a diamond in the xy plane, vertices at +-sqrt(1/2)
    s = one(R.SHAPE_CUBOID, (0.5, 0.5, 0.5), rot=(0, 0, sn, c), dt=dt)
    h = ray(s, (-5, 0.2, 0), (1, 0, 0))            # hits the upper-left edge x = y - sqrt(1/2): local +y face
    assert h["collider"] == 0 and close(h["distance"], 5 + 0.2 - SQ2, dt)
    assert close(h["normal"], (-SQ2, SQ2, 0), dt)
    assert ray(s, (-5, 0.8, 0), (1, 0, 0))["collider"] == R.MISS   # above the diamond's top vertex
    ids, cnt = R.point_intersections(s, np.array([[0.6, 0.0, 0.0], [0.5, 0.5, 0.0]]), 4)
    assert list(cnt) == [1, 0] and ids[0, 0] == 0


@pytest.mark.parametrize("dt", DTYPES)
def test_child_collider_pose(dt):
    q = (0, 0, np.sin(np.pi / 4), np.cos(np.pi / 4))   # body turned 90 degrees about z: the child's +x offset points along +y
    s = one(R.SHAPE_BALL, (0.5, 0, 0), pos=(1, 0, 0), rot=q, dt=dt, child=((1, 0, 0), (0, 0, 0, 1)))
    assert close([s.pos[0][0], s.pos[1][0], s.pos[2][0]], (1, 1, 0), dt)
    h = ray(s, (1, 1, -5), (0, 0, 1))
    assert h["collider"] == 0 and close(h["distance"], 4.5, dt) and close(h["normal"], (0, 0, -1), dt)
    assert ray(s, (2, 0, -5), (0, 0, 1))["collider"] == R.MISS   # where the child would be without its transform


@pytest.mark.parametrize("dt", DTYPES)
def test_filters_ties_and_nearest_k(dt):
    # three unit cubes on the z axis + one in the same place as the first (tie: equal distance, the lower index first)
    bodies = dict(position=np.array([[0, 0, 0], [0, 0, 3], [0, 0, 6], [0, 0, 0]], float), rotation=np.tile([0, 0, 0, 1.0], (4, 1)))
    cols = dict(entity_index=np.array([10, 11, 12, 13], np.uint32), body=np.arange(4, dtype=np.int32), shape=np.zeros(4, np.uint8),
                half_extents=np.full((4, 3), 0.5), memberships=np.array([1, 2, 1, 4], np.uint32))
    s = R.Snapshot(bodies, cols, None, dt)
    o, d = np.array([[0, 0, -5.0]]), np.array([[0, 0, 1.0]])
    assert R.cast_rays(s, o, d)[0]["collider"] == 0
    assert R.cast_rays(s, o, d, excluded=[10])[0]["collider"] == 3
    assert R.cast_rays(s, o, d, mask=np.array([2]))[0]["collider"] == 1
    h, cnt = R.ray_hits(s, o, d, 3)
    assert cnt[0] == 4 and list(h[0]["collider"]) == [0, 3, 1]
    h, cnt = R.ray_hits(s, o, d, 8, mask=np.array([5]))
    assert cnt[0] == 3 and list(h[0]["collider"][:4]) == [0, 3, 2, R.MISS]
    closest, many = R.ray_queries(s, o, d, ks=(1, 3))
    assert closest[0]["collider"] == 0 and list(many[3][0][0]["collider"]) == [0, 3, 1] and many[1][1][0] == 4
    ids, cnt = R.point_intersections(s, np.array([[0, 0, 0.2], [0, 0, 1.5]]), 1)
    assert list(cnt) == [2, 0] and list(ids[:, 0]) == [0, R.MISS]
    ids, cnt = R.aabb_intersections(s, np.array([[-1, -1, 0.0]]), np.array([[1, 1, 2.5]]), 4)
    assert cnt[0] == 3 and list(ids[0]) == [0, 1, 3, R.MISS]   # touching counts (<=)


def test_host_shapes_are_never_candidates():
    bodies = dict(position=np.zeros((2, 3)), rotation=np.tile([0, 0, 0, 1.0], (2, 1)))
    cols = dict(entity_index=np.array([1, 2], np.uint32), body=np.arange(2, dtype=np.int32), shape=np.array([R.SHAPE_HOST, R.SHAPE_BALL], np.uint8),
                half_extents=np.array([[1, 1, 1], [0.5, 0, 0]], float))
    s = R.Snapshot(bodies, cols)
    assert R.cast_rays(s, np.array([[0, 0, -5.0]]), np.array([[0, 0, 1.0]]))[0]["collider"] == 1
    assert list(R.point_intersections(s, np.zeros((1, 3)), 4)[1]) == [1]


def spatial_header_symbols():
    text = open(os.path.join(REPO, "include", "avian_mi355x_spatial.h")).read()
    return sorted(set(re.findall(r"AVN_API\s+avn_status\s+(avn_spatial_\w+)\s*\(", text)))


def test_every_spatial_entry_point_is_exported():
    syms = spatial_header_symbols()
    assert syms == sorted(S.SYMBOLS)
    dll = ctypes.CDLL(hip_lib().path)
    for s in syms:
        assert hasattr(dll, s), f"{hip_lib().path} does not export {s}"


def test_spatial_structs_match_the_ctypes_mirror(tmp_path):
    names = [c.__name__ for c in S.STRUCTS]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "avian_mi355x_spatial.h"\nint main(void) {\n' +
                   "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for c in S.STRUCTS:
        assert int(got[c.__name__]) == ctypes.sizeof(c), f"{c.__name__}: header {got[c.__name__]} B, binding {ctypes.sizeof(c)} B"
    assert S.hit_dtype(32).itemsize == ctypes.sizeof(S.avn_spatial_hit_f32) and S.hit_dtype(64).itemsize == ctypes.sizeof(S.avn_spatial_hit_f64)


def test_main_header_does_not_declare_the_spatial_queries():
    text = open(os.path.join(REPO, "include", "avian_mi355x.h")).read()
    assert "spatial" not in re.findall(r"AVN_FN\((\w+)\)", text)
    assert not any("spatial" in s for s in re.findall(r"AVN_FN\((\w+)\)", text))
