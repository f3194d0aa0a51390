"""Settled frozen-manifold cfg2 steps, for a kernel trace or a wall-clock figure: graph replay by default, direct launches with --no-graph.
(The library is avian_amd's: AVN_LIB_PATH selects an A/B build, and the `make measure` build reads the AVN_* switches.)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, avian_amd
from avian_amd import _ffi as F

ap = argparse.ArgumentParser()
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=2)
args = ap.parse_args()
lib = avian_amd.load_library()
sc, substeps, _ = bench.build_inputs(lib, "cfg2_box_stack_100k")
w = F.World(lib, F.default_config(32, substeps=substeps, use_graph=0 if args.no_graph else 1))
bench.setup_world(w, lib, sc)
for _ in range(5):
    w.step()
w.synchronize()
for rep in range(args.reps):
    t0 = time.perf_counter()
    for _ in range(args.steps):
        w.step()
    w.synchronize()
    print("wall/step %.4f ms" % ((time.perf_counter() - t0) / args.steps * 1e3), flush=True)
