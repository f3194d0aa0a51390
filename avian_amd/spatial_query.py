"""ctypes binding of ``include/avian_mi355x_spatial.h``: device spatial queries (ray casts, ray hits, point and AABB intersections, point
projection, shape intersections, shape casts, shape contacts, depenetration, velocity projection, cast_move and move_and_slide) over the
colliders a :class:`avian_amd._ffi.World` holds on the device, and the persistent RayCaster / ShapeCaster tables re-aimed and cast by
``casters_run``.

Numpy arrays in and out (copied through the library's staging), or torch tensors on the world's GPU (``AVN_SPATIAL_DEVICE_POINTERS``: the
library reads and writes the tensors in place).  These entry points are not part of ``_ffi.ABI_SYMBOLS``: they live in their own header.
"""
from __future__ import annotations

import os

import ctypes as C

import numpy as np

from . import _ffi as F

vp = C.c_void_p

DEVICE_POINTERS = 1
SKIP_HOST_SHAPES = 2
SKIP_SENSORS = 4      # shape_contacts / depenetrate only
MAX_HITS = 64
MAX_PLANES = 32
MAX_SLIDE_ITERATIONS = 16
SLIDE_TRUNCATED = 1
MISS = 0xFFFFFFFF
ANCHOR_WORLD, ANCHOR_BODY, ANCHOR_COLLIDER = 0, 1, 2
CASTER_RAY, CASTER_SHAPE = 0, 1
# query-shape kinds: a capsule is a query shape only (half_extents = (r, h, .): the radius in x, the half length of its y segment in y)
SHAPE_CUBOID, SHAPE_BALL, SHAPE_CAPSULE = 0, 1, 3


class avn_spatial_filter(C.Structure):
    _fields_ = [("mask", vp), ("excluded", vp), ("n_excluded", C.c_uint32)]


class avn_spatial_rays(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("origin", vp), ("direction", vp), ("max_distance", vp), ("solid", vp),
                ("filter", avn_spatial_filter)]


class avn_spatial_points(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("point", vp), ("filter", avn_spatial_filter)]


class avn_spatial_aabbs(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("min", vp), ("max", vp), ("filter", avn_spatial_filter)]


class avn_spatial_solid_points(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("point", vp), ("solid", vp), ("filter", avn_spatial_filter)]


class avn_spatial_shapes(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("shape", vp), ("half_extents", vp), ("position", vp), ("rotation", vp),
                ("filter", avn_spatial_filter)]


class avn_spatial_shape_casts(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("shape", vp), ("half_extents", vp), ("position", vp), ("rotation", vp),
                ("direction", vp), ("max_distance", vp), ("filter", avn_spatial_filter)]


class avn_spatial_shape_hit_f32(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("distance", C.c_float), ("point1", C.c_float * 3), ("point2", C.c_float * 3),
                ("normal1", C.c_float * 3), ("normal2", C.c_float * 3)]


class avn_spatial_shape_hit_f64(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("distance", C.c_double), ("point1", C.c_double * 3), ("point2", C.c_double * 3),
                ("normal1", C.c_double * 3), ("normal2", C.c_double * 3)]


class avn_spatial_shape_contact_queries(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("shape", vp), ("half_extents", vp), ("position", vp), ("rotation", vp),
                ("prediction_distance", vp), ("filter", avn_spatial_filter)]


class avn_spatial_shape_contact_f32(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("penetration", C.c_float), ("normal", C.c_float * 3), ("point", C.c_float * 3),
                ("anchor1", C.c_float * 3), ("anchor2", C.c_float * 3)]


class avn_spatial_shape_contact_f64(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("penetration", C.c_double), ("normal", C.c_double * 3), ("point", C.c_double * 3),
                ("anchor1", C.c_double * 3), ("anchor2", C.c_double * 3), ("reserved", C.c_uint32 * 2)]


class avn_spatial_shape_contacts_out(C.Structure):
    _fields_ = [("contacts", vp), ("count", vp)]


class avn_spatial_depenetration_config(C.Structure):
    _fields_ = [("skin_width", C.c_double), ("max_depenetration_error", C.c_double), ("penetration_rejection_threshold", C.c_double),
                ("iterations", C.c_uint32)]


class avn_spatial_depenetration_f32(C.Structure):
    _fields_ = [("fixup", C.c_float * 3), ("count", C.c_uint32), ("iterations_run", C.c_uint32), ("truncated", C.c_uint32)]


class avn_spatial_depenetration_f64(C.Structure):
    _fields_ = [("fixup", C.c_double * 3), ("count", C.c_uint32), ("iterations_run", C.c_uint32), ("truncated", C.c_uint32), ("reserved", C.c_uint32)]


class avn_spatial_depenetrations_out(C.Structure):
    _fields_ = [("depenetration", vp)]


class avn_spatial_velocity_projections(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("stride", C.c_uint32), ("velocity", vp), ("normals", vp), ("normal_count", vp)]


class avn_spatial_velocities_out(C.Structure):
    _fields_ = [("velocity", vp)]


class avn_spatial_moves(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("shape", vp), ("half_extents", vp), ("position", vp), ("rotation", vp),
                ("movement", vp), ("skin_width", vp), ("self_entity", vp), ("filter", avn_spatial_filter)]


class avn_spatial_move_hit_f32(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("distance", C.c_float), ("collision_distance", C.c_float), ("point1", C.c_float * 3),
                ("point2", C.c_float * 3), ("normal1", C.c_float * 3), ("normal2", C.c_float * 3)]


class avn_spatial_move_hit_f64(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("distance", C.c_double), ("collision_distance", C.c_double), ("point1", C.c_double * 3),
                ("point2", C.c_double * 3), ("normal1", C.c_double * 3), ("normal2", C.c_double * 3)]


class avn_spatial_move_hits_out(C.Structure):
    _fields_ = [("hits", vp)]


class avn_spatial_characters(C.Structure):
    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("shape", vp), ("half_extents", vp), ("position", vp), ("rotation", vp),
                ("velocity", vp), ("self_entity", vp), ("filter", avn_spatial_filter)]


class avn_spatial_move_and_slide_config(C.Structure):
    _fields_ = [("delta_time", C.c_double), ("skin_width", C.c_double), ("max_depenetration_error", C.c_double), ("penetration_rejection_threshold", C.c_double),
                ("plane_similarity_dot_threshold", C.c_double), ("planes", vp), ("n_planes", C.c_uint32), ("max_planes", C.c_uint32),
                ("move_and_slide_iterations", C.c_uint32), ("depenetration_iterations", C.c_uint32)]


class avn_spatial_slide_f32(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("projected_velocity", C.c_float * 3), ("iterations_run", C.c_uint32), ("hit_count", C.c_uint32), ("flags", C.c_uint32)]


class avn_spatial_slide_f64(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("projected_velocity", C.c_double * 3), ("iterations_run", C.c_uint32), ("hit_count", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class avn_spatial_slide_hit_f32(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("iteration", C.c_uint32), ("kind", C.c_uint32), ("point", C.c_float * 3), ("normal", C.c_float * 3),
                ("distance", C.c_float), ("collision_distance", C.c_float)]


class avn_spatial_slide_hit_f64(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("iteration", C.c_uint32), ("kind", C.c_uint32), ("point", C.c_double * 3), ("normal", C.c_double * 3),
                ("distance", C.c_double), ("collision_distance", C.c_double)]


class avn_spatial_slides_out(C.Structure):
    _fields_ = [("slides", vp), ("hits", vp)]


class avn_spatial_shape_hits_out(C.Structure):
    _fields_ = [("hits", vp), ("count", vp)]


class avn_spatial_projection_f32(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("is_inside", C.c_uint32), ("point", C.c_float * 3), ("distance", C.c_float)]


class avn_spatial_projection_f64(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("is_inside", C.c_uint32), ("reserved", C.c_uint32), ("point", C.c_double * 3), ("distance", C.c_double)]


class avn_spatial_projections_out(C.Structure):
    _fields_ = [("projection", vp)]


class avn_spatial_hit_f32(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("distance", C.c_float), ("normal", C.c_float * 3)]


class avn_spatial_hit_f64(C.Structure):
    _fields_ = [("collider", C.c_uint32), ("entity", C.c_uint32), ("distance", C.c_double), ("normal", C.c_double * 3)]


class avn_spatial_hits_out(C.Structure):
    _fields_ = [("hits", vp), ("count", vp)]


class avn_spatial_ids_out(C.Structure):
    _fields_ = [("collider", vp), ("count", vp)]


class avn_spatial_stats(C.Structure):
    _fields_ = [("colliders", C.c_uint32), ("nodes", C.c_uint32), ("host_skipped", C.c_uint32), ("valid", C.c_uint32),
                ("nodes_visited", C.c_uint64), ("leaves_visited", C.c_uint64)]


class avn_spatial_ray_casters(C.Structure):
    _fields_ = [("count", C.c_uint32), ("hit_cap", C.c_uint32), ("anchor_kind", vp), ("anchor", vp), ("origin", vp), ("direction", vp), ("max_distance", vp),
                ("max_hits", vp), ("solid", vp), ("enabled", vp), ("mask", vp), ("self_entity", vp), ("excluded_offset", vp), ("excluded", vp)]


class avn_spatial_shape_casters(C.Structure):
    _fields_ = [("count", C.c_uint32), ("hit_cap", C.c_uint32), ("anchor_kind", vp), ("anchor", vp), ("origin", vp), ("direction", vp), ("max_distance", vp),
                ("max_hits", vp), ("shape", vp), ("half_extents", vp), ("shape_rotation", vp), ("enabled", vp), ("mask", vp), ("self_entity", vp),
                ("excluded_offset", vp), ("excluded", vp)]


class avn_spatial_caster_poses_out(C.Structure):
    _fields_ = [("origin", vp), ("direction", vp), ("rotation", vp)]


STRUCTS = [avn_spatial_filter, avn_spatial_rays, avn_spatial_points, avn_spatial_aabbs, avn_spatial_hit_f32, avn_spatial_hit_f64,
           avn_spatial_hits_out, avn_spatial_ids_out, avn_spatial_stats, avn_spatial_solid_points, avn_spatial_shapes,
           avn_spatial_projection_f32, avn_spatial_projection_f64, avn_spatial_projections_out, avn_spatial_shape_casts,
           avn_spatial_shape_hit_f32, avn_spatial_shape_hit_f64, avn_spatial_shape_hits_out, avn_spatial_shape_contact_queries,
           avn_spatial_shape_contact_f32, avn_spatial_shape_contact_f64, avn_spatial_shape_contacts_out, avn_spatial_depenetration_config,
           avn_spatial_depenetration_f32, avn_spatial_depenetration_f64, avn_spatial_depenetrations_out, avn_spatial_velocity_projections,
           avn_spatial_velocities_out, avn_spatial_moves, avn_spatial_move_hit_f32, avn_spatial_move_hit_f64, avn_spatial_move_hits_out,
           avn_spatial_characters, avn_spatial_move_and_slide_config, avn_spatial_slide_f32, avn_spatial_slide_f64, avn_spatial_slide_hit_f32,
           avn_spatial_slide_hit_f64, avn_spatial_slides_out, avn_spatial_ray_casters, avn_spatial_shape_casters, avn_spatial_caster_poses_out]
SYMBOLS = ["avn_spatial_update", "avn_spatial_capsule_colliders_set", "avn_spatial_triangle_colliders_set", "avn_spatial_cast_rays", "avn_spatial_ray_hits", "avn_spatial_point_intersections",
           "avn_spatial_aabb_intersections", "avn_spatial_stats_get", "avn_spatial_project_points", "avn_spatial_shape_intersections",
           "avn_spatial_cast_shapes", "avn_spatial_shape_hits", "avn_spatial_shape_contacts", "avn_spatial_depenetrate", "avn_spatial_project_velocities",
           "avn_spatial_cast_moves", "avn_spatial_move_and_slide", "avn_spatial_ray_casters_upload", "avn_spatial_shape_casters_upload",
           "avn_spatial_casters_run", "avn_spatial_ray_caster_hits_get", "avn_spatial_shape_caster_hits_get", "avn_spatial_caster_poses_get"]


def hit_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_hit_fNN."""
    s = np.float32 if bits == 32 else np.float64
    return np.dtype([("collider", np.uint32), ("entity", np.uint32), ("distance", s), ("normal", s, (3,))], align=True)


def projection_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_projection_fNN (f64: the 4 bytes after is_inside are the record's `reserved` word, always 0)."""
    s = np.float32 if bits == 32 else np.float64
    return np.dtype([("collider", np.uint32), ("entity", np.uint32), ("is_inside", np.uint32), ("point", s, (3,)), ("distance", s)], align=True)


def shape_hit_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_shape_hit_fNN (60 / 112 bytes, no padding)."""
    s = np.float32 if bits == 32 else np.float64
    return np.dtype([("collider", np.uint32), ("entity", np.uint32), ("distance", s), ("point1", s, (3,)), ("point2", s, (3,)),
                     ("normal1", s, (3,)), ("normal2", s, (3,))], align=True)


def shape_contact_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_shape_contact_fNN (60 / 120 bytes, no padding; f64: two reserved words at the end, always 0)."""
    s = np.float32 if bits == 32 else np.float64
    f = [("collider", np.uint32), ("entity", np.uint32), ("penetration", s), ("normal", s, (3,)), ("point", s, (3,)), ("anchor1", s, (3,)),
         ("anchor2", s, (3,))]
    return np.dtype(f + ([("reserved", np.uint32, (2,))] if bits == 64 else []), align=True)


def depenetration_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_depenetration_fNN (24 / 40 bytes; f64: a reserved word at the end, always 0)."""
    s = np.float32 if bits == 32 else np.float64
    f = [("fixup", s, (3,)), ("count", np.uint32), ("iterations_run", np.uint32), ("truncated", np.uint32)]
    return np.dtype(f + ([("reserved", np.uint32)] if bits == 64 else []), align=True)


def move_hit_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_move_hit_fNN (64 / 120 bytes, no padding)."""
    s = np.float32 if bits == 32 else np.float64
    return np.dtype([("collider", np.uint32), ("entity", np.uint32), ("distance", s), ("collision_distance", s), ("point1", s, (3,)), ("point2", s, (3,)),
                     ("normal1", s, (3,)), ("normal2", s, (3,))], align=True)


def slide_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_slide_fNN (36 / 64 bytes; f64: a reserved word at the end, always 0)."""
    s = np.float32 if bits == 32 else np.float64
    f = [("position", s, (3,)), ("projected_velocity", s, (3,)), ("iterations_run", np.uint32), ("hit_count", np.uint32), ("flags", np.uint32)]
    return np.dtype(f + ([("reserved", np.uint32)] if bits == 64 else []), align=True)


def slide_hit_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_spatial_slide_hit_fNN (48 / 80 bytes, no padding)."""
    s = np.float32 if bits == 32 else np.float64
    return np.dtype([("collider", np.uint32), ("entity", np.uint32), ("iteration", np.uint32), ("kind", np.uint32), ("point", s, (3,)), ("normal", s, (3,)),
                     ("distance", s), ("collision_distance", s)], align=True)


def _declare(dll):
    # (AVN_AB_OLDER_LIBRARY=1 with AVN_LIB_PATH, as in _ffi.Library: an A/B run against a build from before the switch; otherwise a missing symbol is an error)
    older = bool(os.environ.get("AVN_AB_OLDER_LIBRARY"))
    switch = hasattr(dll, "avn_spatial_capsule_colliders_set") or not older
    tri_switch = hasattr(dll, "avn_spatial_triangle_colliders_set") or not older
    for name in SYMBOLS:
        if (switch or name != "avn_spatial_capsule_colliders_set") and (tri_switch or name != "avn_spatial_triangle_colliders_set"):
            getattr(dll, name).restype = C.c_int32
    dll.avn_spatial_update.argtypes = [vp]
    if switch:
        dll.avn_spatial_capsule_colliders_set.argtypes = [vp, C.c_uint32]
    if tri_switch:
        dll.avn_spatial_triangle_colliders_set.argtypes = [vp, C.c_uint32]
    dll.avn_spatial_cast_rays.argtypes = [vp, vp, vp]
    dll.avn_spatial_ray_hits.argtypes = [vp, vp, C.c_uint32, vp]
    dll.avn_spatial_point_intersections.argtypes = [vp, vp, C.c_uint32, vp]
    dll.avn_spatial_aabb_intersections.argtypes = [vp, vp, C.c_uint32, vp]
    dll.avn_spatial_stats_get.argtypes = [vp, vp]
    dll.avn_spatial_project_points.argtypes = [vp, vp, vp]
    dll.avn_spatial_shape_intersections.argtypes = [vp, vp, C.c_uint32, vp]
    dll.avn_spatial_cast_shapes.argtypes = [vp, vp, vp]
    dll.avn_spatial_shape_hits.argtypes = [vp, vp, C.c_uint32, vp]
    dll.avn_spatial_shape_contacts.argtypes = [vp, vp, C.c_uint32, vp]
    dll.avn_spatial_depenetrate.argtypes = [vp, vp, vp, vp]
    dll.avn_spatial_project_velocities.argtypes = [vp, vp, vp]
    dll.avn_spatial_cast_moves.argtypes = [vp, vp, vp]
    dll.avn_spatial_move_and_slide.argtypes = [vp, vp, vp, C.c_uint32, vp]
    dll.avn_spatial_ray_casters_upload.argtypes = [vp, vp]
    dll.avn_spatial_shape_casters_upload.argtypes = [vp, vp]
    dll.avn_spatial_casters_run.argtypes = [vp, C.c_uint32]
    dll.avn_spatial_ray_caster_hits_get.argtypes = [vp, C.c_uint32, vp]
    dll.avn_spatial_shape_caster_hits_get.argtypes = [vp, C.c_uint32, vp]
    dll.avn_spatial_caster_poses_get.argtypes = [vp, C.c_uint32, C.c_uint32, vp]


class SpatialQuery:
    """The spatial queries of one world (``SpatialQueryPipeline`` / ``SpatialQuery``).  Call :meth:`update` to snapshot the poses the
    device holds; the queries answer against the last snapshot.

    Arguments that are torch tensors on the GPU select the device-pointer path: every array of that call must then be a contiguous tensor on
    the world's device (scalars in the world's dtype, ``solid`` uint8, masks / excluded entities int32 read as uint32), outputs come back
    as tensors.  Otherwise everything is numpy.

    ``capsule_colliders=True`` switches the world's capsule colliders in as candidates of every query (:meth:`set_capsule_colliders`); the
    default leaves the world's switch as it is, which is off in a new world: capsule colliders are then left out as host shapes are.
    ``triangle_colliders=True`` does the same for the world's triangle colliders (:meth:`set_triangle_colliders`); the two switches are independent."""

    def __init__(self, world: F.World, capsule_colliders: bool = False, triangle_colliders: bool = False):
        self.world = world
        self.dll = world.lib.dll
        if not hasattr(self.dll, "avn_spatial_update"):
            raise ImportError(f"{world.lib.path} does not export the spatial queries (include/avian_mi355x_spatial.h)")
        _declare(self.dll)
        self.bits = world.cfg.scalar_bits
        self.dtype = world.dtype
        self.hit_dtype = hit_dtype(self.bits)
        self.projection_dtype = projection_dtype(self.bits)
        self.shape_hit_dtype = shape_hit_dtype(self.bits)
        self.shape_contact_dtype = shape_contact_dtype(self.bits)
        self.depenetration_dtype = depenetration_dtype(self.bits)
        self.move_hit_dtype = move_hit_dtype(self.bits)
        self.slide_dtype = slide_dtype(self.bits)
        self.slide_hit_dtype = slide_hit_dtype(self.bits)
        self._keep = []
        self._casters = {CASTER_RAY: (0, 1), CASTER_SHAPE: (0, 1)}   # (count, hit_cap) of the last uploads
        if capsule_colliders:
            self.set_capsule_colliders(True)
        if triangle_colliders:
            self.set_triangle_colliders(True)

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, st: int):
        self._keep = []
        self.world._check(st)

    @staticmethod
    def _is_tensor(a) -> bool:
        return type(a).__module__.startswith("torch") and hasattr(a, "is_cuda") and a.is_cuda

    def _arr(self, a, dt, dev, shape=None):
        if a is None:
            return None
        if dev:
            import torch
            tdt = {np.float32: torch.float32, np.float64: torch.float64, np.uint8: torch.uint8, np.uint32: torch.int32}[dt]
            t = a.to(tdt).contiguous()
            if shape is not None:
                t = t.reshape(shape)
            self._keep.append(t)
            return vp(t.data_ptr())
        x = np.ascontiguousarray(a, dtype=dt)
        if shape is not None:
            x = x.reshape(shape)
        self._keep.append(x)
        return x.ctypes.data_as(vp)

    def _out(self, shape, dt, dev, like=None):
        if dev:
            import torch
            if isinstance(dt, np.dtype):   # a record: bytes
                t = torch.empty(tuple(shape) + (dt.itemsize,), dtype=torch.uint8, device=like.device)
            else:
                t = torch.empty(shape, dtype={np.uint32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}[dt], device=like.device)
            return t, vp(t.data_ptr())
        x = np.empty(shape, dt)
        return x, x.ctypes.data_as(vp)

    def _filter(self, n, mask, excluded, dev):
        f = avn_spatial_filter()
        f.mask = self._arr(mask, np.uint32, dev, (n,)) if mask is not None else None
        if excluded is not None and len(excluded):
            f.excluded = self._arr(excluded, np.uint32, dev)
            f.n_excluded = len(excluded)
        return f

    def _flags(self, dev, skip_host_shapes, skip_sensors=False):
        return (DEVICE_POINTERS if dev else 0) | (SKIP_HOST_SHAPES if skip_host_shapes else 0) | (SKIP_SENSORS if skip_sensors else 0)

    @staticmethod
    def _sync_torch(dev):
        if dev:
            import torch
            torch.cuda.synchronize()   # the caller's writes to the inputs are complete before the library's stream reads them

    # -- entry points --------------------------------------------------------------------------
    def update(self):
        """avn_spatial_update: the LBVH of every collider at the poses the device holds now."""
        self._check(self.dll.avn_spatial_update(self.world.handle))

    def set_capsule_colliders(self, enabled: bool):
        """avn_spatial_capsule_colliders_set: whether capsule colliders are candidates of the queries.  Sticky; it invalidates the snapshot, so
        call :meth:`update` (or :meth:`casters_run`) before the next query."""
        if not hasattr(self.dll, "avn_spatial_capsule_colliders_set"):
            raise ImportError(f"{self.world.lib.path} is older than avn_spatial_capsule_colliders_set")
        self._check(self.dll.avn_spatial_capsule_colliders_set(self.world.handle, 1 if enabled else 0))

    def set_triangle_colliders(self, enabled: bool):
        """avn_spatial_triangle_colliders_set: whether triangle colliders (``World.colliders_upload(triangles=...)``) are candidates of the queries.
        Sticky and independent of :meth:`set_capsule_colliders`; it invalidates the snapshot, so call :meth:`update` (or :meth:`casters_run`)
        before the next query."""
        if not hasattr(self.dll, "avn_spatial_triangle_colliders_set"):
            raise ImportError(f"{self.world.lib.path} is older than avn_spatial_triangle_colliders_set")
        self._check(self.dll.avn_spatial_triangle_colliders_set(self.world.handle, 1 if enabled else 0))

    def _rays(self, origin, direction, max_distance, solid, mask, excluded, skip_host_shapes):
        dev = self._is_tensor(origin)
        n = int(origin.shape[0])
        r = avn_spatial_rays()
        r.count = n
        r.flags = self._flags(dev, skip_host_shapes)
        r.origin = self._arr(origin, self.dtype, dev, (n, 3))
        r.direction = self._arr(direction, self.dtype, dev, (n, 3))
        if max_distance is None:
            max_distance = np.full(n, np.inf) if not dev else origin.new_full((n,), float("inf"))
        if solid is None:
            solid = np.ones(n, np.uint8) if not dev else origin.new_ones((n,))
        r.max_distance = self._arr(max_distance, self.dtype, dev, (n,))
        r.solid = self._arr(solid, np.uint8, dev, (n,))
        r.filter = self._filter(n, mask, excluded, dev)
        return r, n, dev

    def cast_rays(self, origin, direction, max_distance=None, solid=None, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::cast_ray per ray: a structured array of hit records (``hit_dtype``; collider == MISS: no hit).  Device
        tensors in: a uint8 tensor [n, itemsize] of the same records out."""
        r, n, dev = self._rays(origin, direction, max_distance, solid, mask, excluded, skip_host_shapes)
        hits, hp = self._out((n,), self.hit_dtype, dev, origin)
        o = avn_spatial_hits_out(hp, None)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_cast_rays(self.world.handle, C.byref(r), C.byref(o)))
        return hits

    def ray_hits(self, origin, direction, max_hits, max_distance=None, solid=None, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::ray_hits: (records [n, max_hits] nearest first, true hit counts [n])."""
        r, n, dev = self._rays(origin, direction, max_distance, solid, mask, excluded, skip_host_shapes)
        hits, hp = self._out((n, max(int(max_hits), 1)), self.hit_dtype, dev, origin)
        cnt, cp = self._out((n,), np.uint32, dev, origin)
        o = avn_spatial_hits_out(hp, cp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_ray_hits(self.world.handle, C.byref(r), int(max_hits), C.byref(o)))
        return hits, cnt

    def point_intersections(self, point, cap, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::point_intersections: (collider indices [n, cap] ascending, MISS-padded; true counts [n])."""
        dev = self._is_tensor(point)
        n = int(point.shape[0])
        p = avn_spatial_points()
        p.count = n
        p.flags = self._flags(dev, skip_host_shapes)
        p.point = self._arr(point, self.dtype, dev, (n, 3))
        p.filter = self._filter(n, mask, excluded, dev)
        ids, ip = self._out((n, int(cap)), np.uint32, dev, point)
        cnt, cp = self._out((n,), np.uint32, dev, point)
        o = avn_spatial_ids_out(ip, cp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_point_intersections(self.world.handle, C.byref(p), int(cap), C.byref(o)))
        return ids, cnt

    def aabb_intersections(self, aabb_min, aabb_max, cap, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::aabb_intersections_with_aabb: (collider indices [n, cap] ascending, MISS-padded; true counts [n])."""
        dev = self._is_tensor(aabb_min)
        n = int(aabb_min.shape[0])
        b = avn_spatial_aabbs()
        b.count = n
        b.flags = self._flags(dev, skip_host_shapes)
        b.min = self._arr(aabb_min, self.dtype, dev, (n, 3))
        b.max = self._arr(aabb_max, self.dtype, dev, (n, 3))
        b.filter = self._filter(n, mask, excluded, dev)
        ids, ip = self._out((n, int(cap)), np.uint32, dev, aabb_min)
        cnt, cp = self._out((n,), np.uint32, dev, aabb_min)
        o = avn_spatial_ids_out(ip, cp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_aabb_intersections(self.world.handle, C.byref(b), int(cap), C.byref(o)))
        return ids, cnt

    def project_points(self, point, solid=None, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::project_point per point: a structured array of projection records (``projection_dtype``; collider == MISS:
        no candidate).  ``solid`` defaults to 1.  Device tensors in: a uint8 tensor [n, itemsize] of the same records out."""
        dev = self._is_tensor(point)
        n = int(point.shape[0])
        p = avn_spatial_solid_points()
        p.count = n
        p.flags = self._flags(dev, skip_host_shapes)
        p.point = self._arr(point, self.dtype, dev, (n, 3))
        if solid is None:
            solid = np.ones(n, np.uint8) if not dev else point.new_ones((n,))
        p.solid = self._arr(solid, np.uint8, dev, (n,))
        p.filter = self._filter(n, mask, excluded, dev)
        rec, rp = self._out((n,), self.projection_dtype, dev, point)
        o = avn_spatial_projections_out(rp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_project_points(self.world.handle, C.byref(p), C.byref(o)))
        return rec

    def shape_intersections(self, shape, half_extents, position, rotation, cap, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::shape_intersections per query shape (AVN_SHAPE_CUBOID = 0 / AVN_SHAPE_BALL = 1, a ball's radius in
        half_extents[:, 0] / SHAPE_CAPSULE = 3, ``half_extents`` = (r, h, .): the radius and the half length of the y segment): (collider indices [n, cap] ascending, MISS-padded; true counts [n])."""
        dev = self._is_tensor(position)
        n = int(position.shape[0])
        q = avn_spatial_shapes()
        q.count = n
        q.flags = self._flags(dev, skip_host_shapes)
        q.shape = self._arr(shape, np.uint8, dev, (n,))
        q.half_extents = self._arr(half_extents, self.dtype, dev, (n, 3))
        q.position = self._arr(position, self.dtype, dev, (n, 3))
        q.rotation = self._arr(rotation, self.dtype, dev, (n, 4))
        q.filter = self._filter(n, mask, excluded, dev)
        ids, ip = self._out((n, int(cap)), np.uint32, dev, position)
        cnt, cp = self._out((n,), np.uint32, dev, position)
        o = avn_spatial_ids_out(ip, cp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_shape_intersections(self.world.handle, C.byref(q), int(cap), C.byref(o)))
        return ids, cnt

    def _casts(self, shape, half_extents, position, rotation, direction, max_distance, mask, excluded, skip_host_shapes):
        dev = self._is_tensor(position)
        n = int(position.shape[0])
        q = avn_spatial_shape_casts()
        q.count = n
        q.flags = self._flags(dev, skip_host_shapes)
        q.shape = self._arr(shape, np.uint8, dev, (n,))
        q.half_extents = self._arr(half_extents, self.dtype, dev, (n, 3))
        q.position = self._arr(position, self.dtype, dev, (n, 3))
        q.rotation = self._arr(rotation, self.dtype, dev, (n, 4))
        q.direction = self._arr(direction, self.dtype, dev, (n, 3))
        if max_distance is None:
            max_distance = np.full(n, np.inf) if not dev else position.new_full((n,), float("inf"))
        q.max_distance = self._arr(max_distance, self.dtype, dev, (n,))
        q.filter = self._filter(n, mask, excluded, dev)
        return q, n, dev

    def cast_shapes(self, shape, half_extents, position, rotation, direction, max_distance=None, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::cast_shape per cast (AVN_SHAPE_CUBOID = 0 / AVN_SHAPE_BALL = 1, a ball's radius in half_extents[:, 0] /
        SHAPE_CAPSULE = 3, ``half_extents`` = (r, h, .)): a
        structured array of shape-hit records (``shape_hit_dtype``; collider == MISS: no hit).  Device tensors in: a uint8 tensor
        [n, itemsize] of the same records out."""
        q, n, dev = self._casts(shape, half_extents, position, rotation, direction, max_distance, mask, excluded, skip_host_shapes)
        hits, hp = self._out((n,), self.shape_hit_dtype, dev, position)
        o = avn_spatial_shape_hits_out(hp, None)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_cast_shapes(self.world.handle, C.byref(q), C.byref(o)))
        return hits

    def shape_hits(self, shape, half_extents, position, rotation, direction, max_hits, max_distance=None, mask=None, excluded=None, skip_host_shapes=False):
        """SpatialQueryPipeline::shape_hits: (records [n, max_hits] nearest first, true hit counts [n])."""
        q, n, dev = self._casts(shape, half_extents, position, rotation, direction, max_distance, mask, excluded, skip_host_shapes)
        hits, hp = self._out((n, max(int(max_hits), 1)), self.shape_hit_dtype, dev, position)
        cnt, cp = self._out((n,), np.uint32, dev, position)
        o = avn_spatial_shape_hits_out(hp, cp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_shape_hits(self.world.handle, C.byref(q), int(max_hits), C.byref(o)))
        return hits, cnt

    def shape_contacts(self, shape, half_extents, position, rotation, prediction_distance, cap, mask=None, excluded=None, skip_host_shapes=False,
                       skip_sensors=False):
        """MoveAndSlide::intersections per query shape: (contact records [n, cap] in ascending collider index, ``shape_contact_dtype``, unused
        slots MISS; true counts [n]).  ``prediction_distance`` is a scalar or [n].  Shapes as in :meth:`shape_intersections` (a capsule:
        ``half_extents`` = (r, h, .)).  Device tensors in: a uint8 tensor [n, cap, itemsize] out."""
        dev = self._is_tensor(position)
        n = int(position.shape[0])
        q = avn_spatial_shape_contact_queries()
        q.count = n
        q.flags = self._flags(dev, skip_host_shapes, skip_sensors)
        q.shape = self._arr(shape, np.uint8, dev, (n,))
        q.half_extents = self._arr(half_extents, self.dtype, dev, (n, 3))
        q.position = self._arr(position, self.dtype, dev, (n, 3))
        q.rotation = self._arr(rotation, self.dtype, dev, (n, 4))
        if not self._is_tensor(prediction_distance) and np.ndim(prediction_distance) == 0:
            prediction_distance = np.full(n, prediction_distance) if not dev else position.new_full((n,), float(prediction_distance))
        q.prediction_distance = self._arr(prediction_distance, self.dtype, dev, (n,))
        q.filter = self._filter(n, mask, excluded, dev)
        rec, rp = self._out((n, int(cap)), self.shape_contact_dtype, dev, position)
        cnt, cp = self._out((n,), np.uint32, dev, position)
        o = avn_spatial_shape_contacts_out(rp, cp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_shape_contacts(self.world.handle, C.byref(q), int(cap), C.byref(o)))
        return rec, cnt

    def depenetrate(self, shape, half_extents, position, rotation, skin_width, max_depenetration_error, penetration_rejection_threshold, iterations,
                    mask=None, excluded=None, skip_host_shapes=False, skip_sensors=False):
        """MoveAndSlide::depenetrate per query shape: a structured array of ``depenetration_dtype`` records (fixup, count, iterations_run,
        truncated).  The caller applies PhysicsLengthUnit to the configuration.  A capsule: ``half_extents`` = (r, h, .).  Device tensors in: a uint8 tensor [n, itemsize] out."""
        dev = self._is_tensor(position)
        n = int(position.shape[0])
        q = avn_spatial_shapes()
        q.count = n
        q.flags = self._flags(dev, skip_host_shapes, skip_sensors)
        q.shape = self._arr(shape, np.uint8, dev, (n,))
        q.half_extents = self._arr(half_extents, self.dtype, dev, (n, 3))
        q.position = self._arr(position, self.dtype, dev, (n, 3))
        q.rotation = self._arr(rotation, self.dtype, dev, (n, 4))
        q.filter = self._filter(n, mask, excluded, dev)
        cfg = avn_spatial_depenetration_config(float(skin_width), float(max_depenetration_error), float(penetration_rejection_threshold), int(iterations))
        rec, rp = self._out((n,), self.depenetration_dtype, dev, position)
        o = avn_spatial_depenetrations_out(rp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_depenetrate(self.world.handle, C.byref(q), C.byref(cfg), C.byref(o)))
        return rec

    def project_velocities(self, velocity, normals, normal_count=None):
        """project_velocity (velocity_project.rs) per query: ``velocity`` [n, 3] in the world's dtype, ``normals`` [n, stride, 3] float32 unit
        vectors (Dir is f32), ``normal_count`` [n] (default: stride).  Returns the projected velocities [n, 3].  Needs no snapshot."""
        dev = self._is_tensor(velocity)
        n = int(velocity.shape[0])
        stride = int(normals.shape[1]) if n else 0
        p = avn_spatial_velocity_projections()
        p.count = n
        p.flags = self._flags(dev, False)
        p.stride = stride
        p.velocity = self._arr(velocity, self.dtype, dev, (n, 3))
        p.normals = self._arr(normals, np.float32, dev, (n, stride, 3)) if stride else None
        if normal_count is None:
            normal_count = np.full(n, stride, np.uint32) if not dev else velocity.new_full((n,), stride)
        p.normal_count = self._arr(normal_count, np.uint32, dev, (n,))
        res, rp = self._out((n, 3), self.dtype, dev, velocity)
        o = avn_spatial_velocities_out(rp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_project_velocities(self.world.handle, C.byref(p), C.byref(o)))
        return res

    def cast_moves(self, shape, half_extents, position, rotation, movement, skin_width, self_entity=None, mask=None, excluded=None, skip_host_shapes=False):
        """MoveAndSlide::cast_move per move: a structured array of ``move_hit_dtype`` records (collider == MISS: the way is free).  ``skin_width``
        is a scalar or [n]; ``self_entity`` [n] is the entity each query never hits (MISS: none).  A capsule: ``half_extents`` = (r, h, .).  Device tensors in: a uint8 tensor
        [n, itemsize] out."""
        dev = self._is_tensor(position)
        n = int(position.shape[0])
        q = avn_spatial_moves()
        q.count = n
        q.flags = self._flags(dev, skip_host_shapes)
        q.shape = self._arr(shape, np.uint8, dev, (n,))
        q.half_extents = self._arr(half_extents, self.dtype, dev, (n, 3))
        q.position = self._arr(position, self.dtype, dev, (n, 3))
        q.rotation = self._arr(rotation, self.dtype, dev, (n, 4))
        q.movement = self._arr(movement, self.dtype, dev, (n, 3))
        if not self._is_tensor(skin_width) and np.ndim(skin_width) == 0:
            skin_width = np.full(n, skin_width) if not dev else position.new_full((n,), float(skin_width))
        q.skin_width = self._arr(skin_width, self.dtype, dev, (n,))
        q.self_entity = self._arr(self_entity, np.uint32, dev, (n,)) if self_entity is not None else None
        q.filter = self._filter(n, mask, excluded, dev)
        rec, rp = self._out((n,), self.move_hit_dtype, dev, position)
        o = avn_spatial_move_hits_out(rp)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_cast_moves(self.world.handle, C.byref(q), C.byref(o)))
        return rec

    def move_and_slide(self, shape, half_extents, position, rotation, velocity, delta_time, skin_width, max_depenetration_error,
                       penetration_rejection_threshold, depenetration_iterations, move_and_slide_iterations=4, max_planes=20,
                       plane_similarity_dot_threshold=0.999, planes=None, hit_cap=0, self_entity=None, mask=None, excluded=None, skip_host_shapes=False):
        """MoveAndSlide::move_and_slide per character: (``slide_dtype`` records [n], ``slide_hit_dtype`` records [n, hit_cap]: what on_hit would
        have been called with).  ``planes`` [k, 3] float32 are the configuration's initial planes, shared by the call.  A capsule character
        (Collider::capsule(radius, length)): shape SHAPE_CAPSULE, ``half_extents`` = (radius, length / 2, .).  The caller applies
        PhysicsLengthUnit to the configuration.  Device tensors in: uint8 tensors [n, itemsize] and [n, hit_cap, itemsize] out."""
        dev = self._is_tensor(position)
        n = int(position.shape[0])
        q = avn_spatial_characters()
        q.count = n
        q.flags = self._flags(dev, skip_host_shapes)
        q.shape = self._arr(shape, np.uint8, dev, (n,))
        q.half_extents = self._arr(half_extents, self.dtype, dev, (n, 3))
        q.position = self._arr(position, self.dtype, dev, (n, 3))
        q.rotation = self._arr(rotation, self.dtype, dev, (n, 4))
        q.velocity = self._arr(velocity, self.dtype, dev, (n, 3))
        q.self_entity = self._arr(self_entity, np.uint32, dev, (n,)) if self_entity is not None else None
        q.filter = self._filter(n, mask, excluded, dev)
        pl = np.ascontiguousarray(np.zeros((0, 3)) if planes is None else planes, dtype=np.float32).reshape(-1, 3)   # (host memory, always)
        self._keep.append(pl)
        cfg = avn_spatial_move_and_slide_config(float(delta_time), float(skin_width), float(max_depenetration_error), float(penetration_rejection_threshold),
                                                float(plane_similarity_dot_threshold), pl.ctypes.data_as(vp) if len(pl) else None, len(pl), int(max_planes),
                                                int(move_and_slide_iterations), int(depenetration_iterations))
        rec, rp = self._out((n,), self.slide_dtype, dev, position)
        hits, hp = self._out((n, int(hit_cap)), self.slide_hit_dtype, dev, position)
        o = avn_spatial_slides_out(rp, hp if hit_cap else None)
        self._sync_torch(dev)
        self._check(self.dll.avn_spatial_move_and_slide(self.world.handle, C.byref(q), C.byref(cfg), int(hit_cap), C.byref(o)))
        return rec, hits

    # -- casters ---------------------------------------------------------------------------------
    def _caster_common(self, c, n, hit_cap, anchor_kind, anchor, origin, direction, max_distance, max_hits, enabled, mask, self_entity, ignore_self,
                       excluded):
        c.count = n
        c.hit_cap = int(hit_cap)
        anchor_kind = np.full(n, ANCHOR_WORLD, np.uint8) if anchor_kind is None else anchor_kind
        c.anchor_kind = self._arr(anchor_kind, np.uint8, False, (n,))
        c.anchor = self._arr(np.zeros(n, np.uint32) if anchor is None else anchor, np.uint32, False, (n,))
        c.origin = self._arr(origin, self.dtype, False, (n, 3))
        c.direction = self._arr(direction, np.float32, False, (n, 3))
        c.max_distance = self._arr(np.full(n, np.inf) if max_distance is None else max_distance, self.dtype, False, (n,))
        mh = np.full(n, MISS, np.uint32) if max_hits is None else np.minimum(np.asarray(max_hits, np.uint64), MISS).astype(np.uint32)   # (Avian's default: u32::MAX)
        c.max_hits = self._arr(mh, np.uint32, False, (n,))
        c.enabled = self._arr(enabled, np.uint8, False, (n,)) if enabled is not None else None
        c.mask = self._arr(mask, np.uint32, False, (n,)) if mask is not None else None
        if self_entity is not None:
            own = np.asarray(self_entity, np.uint32).reshape(n)
            if ignore_self is not None:   # RayCaster::ignore_self = false: the caster may hit its own entity
                own = np.where(np.broadcast_to(np.asarray(ignore_self, bool), (n,)), own, np.uint32(MISS)).astype(np.uint32)
            c.self_entity = self._arr(own, np.uint32, False, (n,))
        if excluded is not None:
            if len(excluded) != n:
                raise ValueError("excluded: one array of entity indices per caster")
            off = np.zeros(n + 1, np.uint32)
            off[1:] = np.cumsum([len(e) for e in excluded])
            flat = np.concatenate([np.asarray(e, np.uint32).reshape(-1) for e in excluded]) if n else np.zeros(0, np.uint32)
            c.excluded_offset = self._arr(off, np.uint32, False)
            c.excluded = self._arr(flat if len(flat) else np.zeros(1, np.uint32), np.uint32, False)

    def ray_casters_upload(self, origin, direction, anchor_kind=None, anchor=None, max_distance=None, max_hits=None, solid=None, hit_cap=1, enabled=None,
                           mask=None, self_entity=None, ignore_self=None, excluded=None):
        """avn_spatial_ray_casters_upload: the world's RayCasters (numpy only: configuration).  ``origin`` [n, 3] and ``direction`` [n, 3]
        (float32) are local to the anchor (``anchor_kind`` ANCHOR_WORLD / ANCHOR_BODY / ANCHOR_COLLIDER, ``anchor`` the table index);
        ``max_hits`` defaults to u32::MAX (read as ``hit_cap``); ``self_entity`` [n] with ``ignore_self`` (a bool or [n], default True) is the
        entity a caster never hits; ``excluded`` is a list of n arrays of entity indices.  n == 0 clears the table."""
        n = int(np.asarray(origin).reshape(-1, 3).shape[0])
        c = avn_spatial_ray_casters()
        self._caster_common(c, n, hit_cap, anchor_kind, anchor, origin, direction, max_distance, max_hits, enabled, mask, self_entity, ignore_self, excluded)
        c.solid = self._arr(np.ones(n, np.uint8) if solid is None else solid, np.uint8, False, (n,))
        self._check(self.dll.avn_spatial_ray_casters_upload(self.world.handle, C.byref(c)))
        self._casters[CASTER_RAY] = (n, max(int(hit_cap), 1))   # (only now: a rejected upload leaves the library's table, and the getters' sizes, as they were)

    def shape_casters_upload(self, shape, half_extents, origin, shape_rotation, direction, anchor_kind=None, anchor=None, max_distance=None, max_hits=None,
                             hit_cap=1, enabled=None, mask=None, self_entity=None, ignore_self=None, excluded=None):
        """avn_spatial_shape_casters_upload: the world's ShapeCasters (AVN_SHAPE_CUBOID = 0 / AVN_SHAPE_BALL = 1, a ball's radius in
        half_extents[:, 0] / SHAPE_CAPSULE = 3, ``half_extents`` = (r, h, .); ``shape_rotation`` [n, 4] xyzw, local); the other arguments as in :meth:`ray_casters_upload`."""
        n = int(np.asarray(origin).reshape(-1, 3).shape[0])
        c = avn_spatial_shape_casters()
        self._caster_common(c, n, hit_cap, anchor_kind, anchor, origin, direction, max_distance, max_hits, enabled, mask, self_entity, ignore_self, excluded)
        c.shape = self._arr(shape, np.uint8, False, (n,))
        c.half_extents = self._arr(half_extents, self.dtype, False, (n, 3))
        c.shape_rotation = self._arr(shape_rotation, self.dtype, False, (n, 4))
        self._check(self.dll.avn_spatial_shape_casters_upload(self.world.handle, C.byref(c)))
        self._casters[CASTER_SHAPE] = (n, max(int(hit_cap), 1))

    def casters_run(self, skip_host_shapes=False):
        """avn_spatial_casters_run: a new snapshot, every caster re-aimed from its anchor's pose, the enabled ones cast.  Only enqueues: the
        results stay on the device until :meth:`ray_caster_hits` / :meth:`shape_caster_hits` / :meth:`caster_poses` fetch them."""
        self._check(self.dll.avn_spatial_casters_run(self.world.handle, SKIP_HOST_SHAPES if skip_host_shapes else 0))

    def _like(self, device):
        import torch
        return torch.empty(0, device=torch.device("cuda", max(int(self.world.cfg.device), 0)) if device is True else device)

    def _caster_hits(self, kind, fn, rec_dtype, out_cls, device):
        n, cap = self._casters[kind]
        dev = device is not None and device is not False
        like = self._like(device) if dev else None
        hits, hp = self._out((n, cap), rec_dtype, dev, like)
        cnt, cp = self._out((n,), np.uint32, dev, like)
        o = out_cls(hp, cp)
        self._check(fn(self.world.handle, DEVICE_POINTERS if dev else 0, C.byref(o)))
        return hits, cnt

    def ray_caster_hits(self, device=None):
        """RayHits of the last run: (records [n, hit_cap] nearest first, ``hit_dtype``; counts [n]).  ``device`` (True or a torch device): the
        answers as tensors on the GPU (records as uint8 [n, hit_cap, itemsize]), copied device to device."""
        return self._caster_hits(CASTER_RAY, self.dll.avn_spatial_ray_caster_hits_get, self.hit_dtype, avn_spatial_hits_out, device)

    def shape_caster_hits(self, device=None):
        """ShapeHits of the last run: (records [n, hit_cap], ``shape_hit_dtype``; counts [n]); ``device`` as in :meth:`ray_caster_hits`."""
        return self._caster_hits(CASTER_SHAPE, self.dll.avn_spatial_shape_caster_hits_get, self.shape_hit_dtype, avn_spatial_shape_hits_out, device)

    def caster_poses(self, kind, device=None):
        """The re-aimed casters of the last run: (global origins [n, 3], global directions [n, 3] float32) for CASTER_RAY, plus the global shape
        rotations [n, 4] for CASTER_SHAPE."""
        n, _ = self._casters[kind]
        dev = device is not None and device is not False
        like = self._like(device) if dev else None
        org, op = self._out((n, 3), self.dtype, dev, like)
        dr, dp = self._out((n, 3), np.float32, dev, like)
        rot, rp = self._out((n, 4), self.dtype, dev, like)
        o = avn_spatial_caster_poses_out(op, dp, rp)
        self._check(self.dll.avn_spatial_caster_poses_get(self.world.handle, int(kind), DEVICE_POINTERS if dev else 0, C.byref(o)))
        return (org, dr, rot) if kind == CASTER_SHAPE else (org, dr)

    def stats(self) -> avn_spatial_stats:
        s = avn_spatial_stats()
        self._check(self.dll.avn_spatial_stats_get(self.world.handle, C.byref(s)))
        return s
