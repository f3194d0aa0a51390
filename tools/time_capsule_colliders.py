#!/usr/bin/env python3
"""Native capsule colliders in the closed loop: cfg2's 100 000 boxes (scenes.box_stack(50, 40, 50)) plus 1 000 and 10 000 AVN_SHAPE_CAPSULE colliders lying
in a grid beside the stack (the layout of examples/host_shapes_demo.cpp: rows one diameter apart, so capsules also meet capsules), ms per step over the
last 20 of 140 steps (settled), next to the boxes alone.  Then, on the same box, the compiled demo in both of its modes: the capsules hosted through its
callbacks (the figures of DESIGN.md 4.4.1) and the same capsules native.  The demo's callback geometry is simpler than the native definition, so the two are
compared for TIME only.  Prints one JSON line; --out also writes it to a file.

    python tools/time_capsule_colliders.py [--counts 1000 10000] [--steps 140] [--timed 20] [--no-demo] [--out profiles/capsule_colliders.json]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def scene_with_capsules(n_caps, dims):
    from avian_amd import _ffi as F, scenes
    sc = scenes.box_stack(*dims)
    if not n_caps:
        return sc, np.zeros(0, int)
    r, h = 0.25, 0.4
    side = int(np.ceil(np.sqrt(n_caps)))
    c = np.arange(n_caps)
    pos = np.stack([0.5 * dims[0] + 3.0 + 1.45 * (c % side), 0.6 + 0.05 * (c % 3), 0.5 * (c // side) - 0.25 * side], axis=1)
    ang = 1.5707963 + 0.1 * ((c * 7) % 5) - 0.2           # the axis turned towards world x with a small tilt
    rot = np.stack([np.zeros(n_caps), np.zeros(n_caps), np.sin(0.5 * ang), np.cos(0.5 * ang)], axis=1)
    mass, (ixx, iyy, izz) = scenes.capsule_mass_properties(r, h)
    inv_i = np.zeros((n_caps, 6)); inv_i[:, 0] = 1.0 / ixx; inv_i[:, 3] = 1.0 / iyy; inv_i[:, 5] = 1.0 / izz
    cat = lambda a, b: np.concatenate([a, b])
    out = scenes.Scene(cat(sc.position, pos), cat(sc.rotation, rot), cat(sc.linear_velocity, np.zeros((n_caps, 3))), cat(sc.angular_velocity, np.zeros((n_caps, 3))),
                       cat(sc.inv_mass, np.full(n_caps, 1.0 / mass)), cat(sc.inv_inertia_local, inv_i), cat(sc.rb_type, np.zeros(n_caps, np.uint8)),
                       cat(sc.half_extents, np.tile([r, h, 0.0], (n_caps, 1))), cat(sc.shape, np.full(n_caps, F.SHAPE_CAPSULE, np.uint8)), friction=0.5)
    return out, np.arange(sc.n, sc.n + n_caps)


def time_world(n_caps, dims, steps, timed):
    import avian_amd
    from avian_amd import _ffi as F
    sc, caps = scene_with_capsules(n_caps, dims)
    w = F.World(avian_amd.load_library(), F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**sc.collider_kwargs())
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction)
    w.pipeline_enable()
    for _ in range(steps - timed):
        w.step()
    w.synchronize()
    t0 = time.perf_counter()
    for _ in range(timed):
        w.step()
    w.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / timed
    y = w.bodies_download()["position"][caps, 1] if n_caps else np.zeros(0)
    res = {"capsules": int(n_caps), "ms_per_step": round(ms, 4), "steps": steps, "timed": timed}
    if n_caps:
        res["worst_centre_height_error"] = round(float(np.abs(y - 0.25).max()), 5)
    w.close()
    return res


def run_demo(dims, n_caps, steps, native):
    exe = os.path.join(REPO, "examples", "host_shapes_demo")
    if not os.path.exists(exe):
        return {"status": "examples/host_shapes_demo is not built"}
    p = subprocess.run([exe, *map(str, dims), str(n_caps), str(steps)] + (["native"] if native else []), capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    ms = [float(x) for x in re.findall(r"capsules: ([0-9.]+) ms per step", p.stdout)]
    return {"capsules": n_caps, "mode": "native" if native else "hosted", "boxes_alone_ms": ms[0] if ms else None, "with_capsules_ms": ms[1] if len(ms) > 1 else None,
            "ok": "HOST_SHAPES_DEMO_OK" in p.stdout}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="*", default=[1000, 10000])
    ap.add_argument("--dims", type=int, nargs=3, default=[50, 40, 50])
    ap.add_argument("--steps", type=int, default=140)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--no-demo", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"scene": "box_stack(%d, %d, %d) + capsules (r 0.25, h 0.4) lying beside it" % tuple(a.dims), "python_worlds": [time_world(n, a.dims, a.steps, a.timed) for n in [0] + a.counts]}
    if not a.no_demo:
        res["demo"] = [run_demo(a.dims, n, a.steps, native) for n in a.counts for native in (False, True)]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
