"""Frozen-manifold steps of other shapes than the benchmark's, for A/Bs of what runs beside the solver (k_sweep's footprint bound):
cfg2 with 1, 2 or 4 substeps, and a sparse scene -- 100 352 boxes in two layers of separated columns, 1.0 manifolds per collider against cfg2's 6.8.
Wall time per step over settled steps, no profiler.  (AVN_LIB_PATH selects the build; the `make measure` build reads AVN_SWEEP_WG_PER_CU and
AVN_SWEEP_BOUND_MIN_WORK.)

    python tools/frozen_shapes.py --scene cfg2|sparse --substeps S
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, avian_amd
from avian_amd import _ffi as F, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="cfg2", choices=["cfg2", "sparse"])
ap.add_argument("--substeps", type=int, default=4)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
lib = avian_amd.load_library()
sc = scenes.box_stack(50, 40, 50) if args.scene == "cfg2" else scenes.box_stack(224, 2, 224, spacing_xz=1.5)
w = F.World(lib, F.default_config(32, substeps=args.substeps, use_graph=1))
meta = bench.setup_world(w, lib, sc)
for _ in range(5):
    w.step()
w.synchronize()
best = []
for rep in range(args.reps):
    t0 = time.perf_counter()
    for _ in range(args.steps):
        w.step()
    w.synchronize()
    best.append((time.perf_counter() - t0) / args.steps * 1e3)
print("%s substeps %d: %d colliders, %d manifolds; wall ms/step %s" % (args.scene, args.substeps, sc.n, meta["n_manifolds"], " ".join("%.4f" % b for b in best)), flush=True)
