#!/usr/bin/env python3
"""Triangle colliders in the closed loop, native (AVN_SHAPE_TRIANGLE, include/avian_mi355x_trimesh.h) against hosted (the same faces as AVN_SHAPE_HOST, answered
by the callbacks of tests/triangle_collider_reference.py: TriangleHost -- the only hosted triangle in the tree, written in numpy scalars): ms per step at f32 over
the same steps of the same scene, the two worlds alternating on one device.  Scenes: scenes.trimesh_drop at a few face and body counts (dropped from 0.1 above the
ground's highest point and warmed up until they lie on it, so the timed steps hold triangle pairs), and cfg2's boxes (scenes.box_stack(50, 40, 50)) standing on a flat 64 x 64-quad mesh in the place of their ground
slab.  The hosted world pays two round trips per step and one Python callback per face (AABB) and per triangle pair (manifold): it is timed over few steps.
Prints one JSON line; --out also writes it to a file.

    python tools/time_trimesh.py [--configs small large cfg2] [--warm 24] [--timed 20] [--hosted-timed 3] [--repeats 2] [--out profiles/trimesh_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

CONFIGS = {
    "small": dict(kind="drop", n_boxes=8, n_balls=8, n_capsules=8, nx=8, nz=8),            # 128 faces, 24 bodies
    "medium": dict(kind="drop", n_boxes=167, n_balls=167, n_capsules=166, nx=32, nz=32),   # 2 048 faces, 500 bodies
    "large": dict(kind="drop", n_boxes=667, n_balls=667, n_capsules=666, nx=64, nz=64),    # 8 192 faces, 2 000 bodies
    "cfg2": dict(kind="stack", dims=(50, 40, 50), nx=64, nz=64, warm=3),                   # 8 192 faces, 100 000 boxes (they stand on the mesh from the first step)
}


def bumps(x, z):
    """The bumps of the tested ground (test_triangle_collider_cpu.bumps) WITHOUT its rising border, which grows with the square of the distance from the centre:
    at 64 x 64 quads it would be a wall 500 high and the bodies, dropped from above the mesh's highest point, would never land in the timed steps."""
    return 0.15 * np.sin(1.3 * x) * np.cos(0.9 * z)


def build_scene(cfg):
    from avian_amd import _ffi as F, scenes
    from avian_amd.trimesh import triangle_colliders
    if cfg["kind"] == "drop":
        kw = {k: v for k, v in cfg.items() if k not in ("kind", "warm")}
        return scenes.trimesh_drop(**kw, height_fn=bumps, drop_height=0.1, seed=1)
    sc = scenes.box_stack(*cfg["dims"])
    gv, gi = scenes.trimesh_ground(cfg["nx"], cfg["nz"], 1.0)
    tri, flags = triangle_colliders(gv, gi)
    nf, n = len(tri), sc.n
    pos = sc.position.copy(); pos[0] = 0.0          # the mesh's frame is body 0's: its top, y = 0, is where the slab's top was
    shape = sc.shape.copy(); shape[0] = F.SHAPE_TRIANGLE
    c = nf + n - 1
    verts = np.zeros((c, 3, 3)); verts[:nf] = tri
    ef = np.full(c, F.TRIANGLE_ALL_EDGES, np.uint8); ef[:nf] = flags
    return scenes.MeshScene(pos, sc.rotation, sc.linear_velocity, sc.angular_velocity, sc.inv_mass, sc.inv_inertia_local, sc.rb_type, sc.half_extents, shape, friction=sc.friction,
                            col_entity=np.arange(c, dtype=np.uint32), col_body=np.concatenate([np.zeros(nf, np.int32), np.arange(1, n, dtype=np.int32)]),
                            col_shape=np.concatenate([np.full(nf, F.SHAPE_TRIANGLE, np.uint8), sc.shape[1:]]), col_half_extents=np.concatenate([np.zeros((nf, 3)), sc.half_extents[1:]]),
                            vertices=verts, edge_flags=ef, grid=(cfg["nx"], cfg["nz"], 1.0, gv[:, 1].reshape(cfg["nx"] + 1, cfg["nz"] + 1)))


def time_world(sc, native, warm, timed):
    import avian_amd
    import triangle_collider_reference as TR
    from avian_amd import _ffi as F
    w = F.World(avian_amd.load_library(), F.default_config(32, substeps=4))
    cols = sc.collider_kwargs(native_triangles=native)
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction, restitution=0.0)
    host = None
    if not native:
        host = TR.TriangleHost(cols["entity_index"], sc.col_shape, sc.col_half_extents, sc.vertices, sc.edge_flags)
        w.host_shapes_set(host.aabb, host.manifolds)
    w.pipeline_enable()
    for _ in range(warm):
        w.step()
    w.synchronize()
    before = host.manifold_queries if host else 0
    t0 = time.perf_counter()
    for _ in range(timed):
        w.step()
    w.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / timed
    res = {"mode": "native" if native else "hosted", "ms_per_step": round(ms, 4), "warm": warm, "timed": timed, "contact_rows": int(len(w.pipeline_handles()[1])),
           "finite": bool(np.isfinite(w.bodies_download()["position"]).all())}
    if host:
        res["triangle_pairs_per_step"] = round((host.manifold_queries - before) / timed, 1)
        res["last_callback_ms"] = round(float(w.host_shape_stats().last_callback_ms), 3)
    w.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["small", "large", "cfg2"], choices=sorted(CONFIGS))
    ap.add_argument("--warm", type=int, default=24)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--hosted-timed", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"scalar_bits": 32, "not_measured": "f64; the shares of the AABB and the narrow phase inside a step; scenes other than these", "configs": []}
    for name in a.configs:
        sc = build_scene(CONFIGS[name])
        warm = min(a.warm, CONFIGS[name].get("warm", a.warm))
        runs = []
        for _ in range(a.repeats):   # alternating: native, hosted, native, hosted ...
            runs.append(time_world(sc, True, warm, a.timed))
            runs.append(time_world(sc, False, warm, a.hosted_timed))
            print(name, runs[-2], runs[-1], file=sys.stderr, flush=True)
        best = lambda mode: min(r["ms_per_step"] for r in runs if r["mode"] == mode)
        res["configs"].append({"config": name, "faces": sc.n_faces, "bodies": int(sc.n - 1), "native_ms_per_step": best("native"), "hosted_ms_per_step": best("hosted"),
                               "hosted_over_native": round(best("hosted") / best("native"), 1), "runs": runs})
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
