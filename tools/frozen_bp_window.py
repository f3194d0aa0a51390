"""Where the broad phase's chain runs inside a settled frozen-manifold cfg2 step WITHOUT a profiler attached: the step's own events
(`make measure` build, AVN_HOST_TRACE=1: avn_timers_get prints the chain's start and end relative to the step's start event).

    AVN_LIB_PATH=avian_amd/csrc/measure/libavian_mi355x.so AVN_HOST_TRACE=1 python tools/frozen_bp_window.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, avian_amd
from avian_amd import _ffi as F

lib = avian_amd.load_library()
sc, substeps, _ = bench.build_inputs(lib, "cfg2_box_stack_100k")
w = F.World(lib, F.default_config(32, substeps=substeps, use_graph=0 if "--no-graph" in sys.argv else 1))
bench.setup_world(w, lib, sc)
for rep in range(5):
    for _ in range(12):
        w.step()
    t = w.timers()   # synchronises; prints the last step's windows to stderr
    print("step %.4f ms, broad phase chain %.4f ms" % (t.step_ms, t.broad_phase_ms), flush=True)
