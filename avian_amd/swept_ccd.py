"""ctypes binding of ``include/avian_mi355x_ccd.h``: the SweptCcd list of a :class:`avian_amd._ffi.World` in device closed-loop mode and
the records its pass leaves per step (``SweepMode::Linear`` and, behind :meth:`SweptCcd.set_non_linear`, ``SweepMode::NonLinear``; Ball /
Cuboid colliders and, behind :meth:`SweptCcd.set_capsules`, Capsule colliders)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi as F

SWEEP_LINEAR, SWEEP_NON_LINEAR = 0, 1
MISS = 0xFFFFFFFF


def result_dtype(bits: int) -> np.dtype:
    """numpy mirror of avn_swept_ccd_result_fNN (16 / 24 bytes, no implicit padding)."""
    if bits == 32:
        return np.dtype([("toi", np.float32), ("hit_collider", np.uint32), ("hit_body", np.int32), ("tested", np.uint32)])
    return np.dtype([("toi", np.float64), ("hit_collider", np.uint32), ("hit_body", np.int32), ("tested", np.uint32), ("reserved", np.uint32)])


class SweptCcd:
    """The SweptCcd components of one world, in the order of Avian's ``Query<Entity, With<SweptCcd>>``."""

    def __init__(self, world: F.World, non_linear: bool = False, capsules: bool = False):
        self.world = world
        self.dll = world.lib.dll
        if not hasattr(self.dll, "avn_swept_ccd_upload"):
            raise ImportError(f"{world.lib.path} does not export swept CCD (include/avian_mi355x_ccd.h)")
        F.declare_swept_ccd(self.dll)
        self.result_dtype = result_dtype(world.cfg.scalar_bits)
        self.count = 0
        if non_linear:
            self.set_non_linear(True)
        if capsules:
            self.set_capsules(True)

    def set_non_linear(self, enabled: bool):
        """avn_swept_ccd_non_linear_set: whether :meth:`upload` accepts ``SWEEP_NON_LINEAR`` (sticky, off in a new world).  Turning it off while
        the list in force holds a NonLinear entry raises (AVN_ERR_STATE)."""
        if not hasattr(self.dll, "avn_swept_ccd_non_linear_set"):
            raise ImportError(f"{self.world.lib.path} is older than avn_swept_ccd_non_linear_set")
        self.world._check(self.dll.avn_swept_ccd_non_linear_set(self.world.handle, 1 if enabled else 0))

    def set_capsules(self, enabled: bool):
        """avn_swept_ccd_capsules_set: whether pairs with a Capsule collider on either side are tested (sticky, off in a new world; may be
        toggled between steps, it takes effect from the next pass)."""
        if not hasattr(self.dll, "avn_swept_ccd_capsules_set"):
            raise ImportError(f"{self.world.lib.path} is older than avn_swept_ccd_capsules_set")
        self.world._check(self.dll.avn_swept_ccd_capsules_set(self.world.handle, 1 if enabled else 0))

    def stats(self) -> dict:
        """avn_swept_ccd_stats_get: nonlinear_tested, rounds_max and exhausted of the last step's pass (waits for it)."""
        if not hasattr(self.dll, "avn_swept_ccd_stats_get"):
            raise ImportError(f"{self.world.lib.path} is older than avn_swept_ccd_stats_get")
        o = F.avn_swept_ccd_stats(C.sizeof(F.avn_swept_ccd_stats), 0, 0, 0)
        self.world._check(self.dll.avn_swept_ccd_stats_get(self.world.handle, C.byref(o)))
        return dict(nonlinear_tested=int(o.nonlinear_tested), rounds_max=int(o.rounds_max), exhausted=int(o.exhausted))

    def upload(self, body, mode=None, include_dynamic=None, linear_threshold=None, angular_threshold=None):
        """Replaces the list; an empty ``body`` clears it.  Defaults are SweptCcd::default(): Linear, include_dynamic, thresholds 0."""
        body = np.ascontiguousarray(body, np.uint32).reshape(-1)
        n = len(body)
        if n == 0:
            self.world._check(self.dll.avn_swept_ccd_upload(self.world.handle, None))
            self.count = 0
            return
        full = lambda a, dt, default: np.ascontiguousarray(np.broadcast_to(np.asarray(default if a is None else a, dt), (n,)))
        keep = [body, full(mode, np.uint32, SWEEP_LINEAR), full(include_dynamic, np.uint32, 1), full(linear_threshold, np.float64, 0.0),
                full(angular_threshold, np.float64, 0.0)]
        l = F.avn_swept_ccd(C.sizeof(F.avn_swept_ccd), n, *[a.ctypes.data_as(C.c_void_p) for a in keep])
        self.world._check(self.dll.avn_swept_ccd_upload(self.world.handle, C.byref(l)))
        self.count = n

    def clear(self):
        self.upload(np.zeros(0, np.uint32))

    def results(self) -> np.ndarray:
        """The records of the last step's pass, in list order (empty before the first pass)."""
        o = F.avn_swept_ccd_results_out(None, 0, 0)
        self.world._check(self.dll.avn_swept_ccd_results_get(self.world.handle, C.byref(o)))
        rec = np.zeros(o.count, self.result_dtype)
        if o.count:
            o = F.avn_swept_ccd_results_out(rec.ctypes.data_as(C.c_void_p), o.count, 0)
            self.world._check(self.dll.avn_swept_ccd_results_get(self.world.handle, C.byref(o)))
        return rec
