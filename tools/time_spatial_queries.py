#!/usr/bin/env python3
"""Timing of the device spatial queries (include/avian_mi355x_spatial.h); prints one JSON object.

  avn_spatial_update at cfg2 (100 k cuboids after 20 closed-loop steps) and cfg4 (10^6 mixed, sparse_mixed)
  cast_rays, 10^6 random rays into cfg2: short (sensor-like, <= 2 m) and long (through the pile)
  ray_hits k = 16, 64 k rays;  point and AABB intersections, 10^6 queries each
  project_points, 10^6 points into cfg2 (the points of point_intersections);  shape_intersections, 10^6 query shapes, half balls and half
  cuboids with sizes like the AABB query's boxes, cap 16 -- reported beside the point and AABB figures of the same run
  shape_contacts (prediction 0.05 m, cap 16) and depenetrate (skin 0.05 m, 4 iterations) with the SAME 10^6 query shapes as
  shape_intersections, which shares the traversal and has the cheaper leaf: the yardstick of the two
  cast_shapes, 10^6 casts into cfg2 from the rays' origins along the rays' directions, short (<= 2 m) and long (200 m), half balls and half
  cuboids of half extent <= 0.25 m;  shape_hits k = 16, 64 k long casts -- reported beside cast_rays / ray_hits of the same run
  project_velocities, 10^6 velocities against 0 .. 4 planes;  cast_moves and move_and_slide (4 rounds) for a crowd of 262144 characters in cfg2,
  beside the same work done through the older entry points (two depenetrate, then per round cast_shapes + shape_contacts), with the share of
  characters still live in each round
  casters: 65536 ray casters with max_hits 1, 16384 with max_hits 4 and 16384 shape casters on random bodies of cfg2, all with ignore_self:
  casters_run + the getters through device pointers, beside the same answers through the older entry points (bodies_download, the re-aiming in
  numpy, ray_hits / shape_hits with k + 1 and the caster's own entity dropped on the host, uploads included; and the cheaper cast_rays /
  ray_hits / cast_shapes with k, which cannot ignore the own entity), the two alternating, in wall-clock windows closed by a device
  synchronisation; the host-side duration of the casters_run call alone, and the share of the run that is the LBVH build
  capsule query shapes: shape_intersections, cast_shapes short and long, shape_contacts and move_and_slide with the reference character's capsule
  (Collider::capsule(0.4, 1.0): r = 0.4, h = 0.5) on the poses of the legs above, each beside the same call with a Cuboid query of the capsule's
  bounding box (0.4, 0.9, 0.4) from the same run, with the node and leaf counts; and the mean Newton rounds per capsule-cuboid pair, from the
  numpy restatement (tests/spatial_capsule_reference.py) on a sample of the timed long casts
  capsule colliders (`capcol`: this leg alone): the cfg2 poses once as they are (all cuboids) and once with every fourth collider an
  AVN_SHAPE_CAPSULE of r = 0.3, h = 0.2 (inside the cuboid it replaces) and avn_spatial_capsule_colliders_set on, the same 262144 queries into
  both: update, cast_rays short / long, ray_hits k = 16, point and AABB intersections, project_points, shape_intersections, shape_contacts,
  depenetrate, cast_shapes, shape_hits k = 16, cast_moves, move_and_slide with Ball / Cuboid query shapes, and cast_shapes, shape_contacts and
  move_and_slide with the capsule character -- per entry point the two figures side by side, the second being the CCAP instantiations' cost

  triangle colliders (`tricol`: this leg alone): cfg2's boxes at their poses once on their single cuboid ground (the existing scene, the yardstick) and
  once on the flat 8 192-face mesh of tools/time_trimesh.py with avn_spatial_triangle_colliders_set on, the same 262144 queries into both, the entry
  points of `capcol` -- per entry point the two figures and their ratio, the CTRI instantiations' cost with a mesh under the pile

Every figure is the median over `reps` warmed-up calls.  The queries take torch tensors on the GPU (AVN_SPATIAL_DEVICE_POINTERS: no
staging copies), so a call is its launches plus one stream synchronisation; the update is timed with avn_synchronize behind it.  Device
events bracket the calls on torch's stream after a synchronisation of it, which the library's own stream joins at the call's end.
bytes_floor: the bytes each call must move at least (inputs, outputs, the snapshot records a query touches once), for a roofline fraction
against MI355X's 8 TB/s HBM.
usage: python tools/time_spatial_queries.py [reps] [casters] [capcol] [tricol] [nocapsule]
       (`casters` / `capcol` / `tricol`: that leg alone; `nocapsule`: without the capsule legs, for an A/B run of a library from before them;
        AVN_LIB_PATH=path AVN_AB_OLDER_LIBRARY=1: time that (older) build of libavian_mi355x.so instead of the tree's)"""
import json
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402
import avian_amd  # noqa: E402
from avian_amd import _ffi as F, scenes  # noqa: E402
from avian_amd.spatial_query import ANCHOR_BODY, MISS, SHAPE_CAPSULE, SpatialQuery  # noqa: E402

HBM = 8.0e12


def timed(fn, reps):
    fn()   # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        out.append(max(a.elapsed_time(b), 0.0) or wall)
    return float(np.median(out))


def qrot_np(q, v):
    """avn_math.h's qrot over rows, in the arrays' dtype."""
    b, w = q[:, :3], q[:, 3:4]
    return v * (w * w - (b * b).sum(1, keepdims=True)) + b * ((v * b).sum(1, keepdims=True) * 2) + np.cross(b, v) * (w * 2)


def qmul_np(l, r):
    """avn_math.h's qmul (f32: glam's association) over rows."""
    lx, ly, lz, lw = l.T
    rx, ry, rz, rw = r.T
    return np.stack([(lw * rx + lx * rw) + (ly * rz + -(lz * ry)), (lw * ry + -(lx * rz)) + (ly * rw + lz * rx), (lw * rz + lx * ry) + (-(ly * rx) + lz * rw),
                     (lw * rw + -(lx * rx)) + (-(ly * ry) + -(lz * rz))], 1)


def drop_own(hits, own, k):
    """The first k records of each row whose entity is not the caster's own (what ignore_self costs a host that has k + 1 records)."""
    keep = hits["entity"] != own[:, None]
    order = np.argsort(~keep, axis=1, kind="stable")[:, :k]
    out = np.take_along_axis(hits, order, 1)
    out[~np.take_along_axis(keep, order, 1)] = (MISS, MISS, *([0] * (len(hits.dtype.names) - 2)))
    return out


def casters_leg(res, w2, sq, sc, reps):
    rng = np.random.default_rng(7)
    ent = np.asarray(sc.collider_kwargs()["entity_index"], np.uint32)
    cbody = np.asarray(sc.collider_kwargs()["body"], np.int64)
    own_of_body = np.full(w2.n_bodies, MISS, np.uint32); own_of_body[cbody] = ent
    n1, n4, ns = 65536, 16384, 16384
    nr = n1 + n4

    def table(n):
        a = rng.integers(1, w2.n_bodies, n).astype(np.uint32)
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        return a, (rng.normal(size=(n, 3)) * 0.1).astype(np.float32), d.astype(np.float32), np.full(n, 2.0, np.float32), own_of_body[a]
    ra, ro, rd, rmd, rown = table(nr)
    rk = np.r_[np.ones(n1, np.uint32), np.full(n4, 4, np.uint32)]
    sa, so, sd, smd, sown = table(ns)
    skind = (np.arange(ns) & 1).astype(np.uint8)
    she = rng.uniform(0.05, 0.25, (ns, 3)).astype(np.float32)
    srot = rng.normal(size=(ns, 4)); srot = (srot / np.linalg.norm(srot, axis=1, keepdims=True)).astype(np.float32)
    sq.ray_casters_upload(ro, rd, anchor_kind=np.full(nr, ANCHOR_BODY, np.uint8), anchor=ra, max_distance=rmd, max_hits=rk, hit_cap=4, self_entity=rown)
    sq.shape_casters_upload(skind, she, so, srot, sd, anchor_kind=np.full(ns, ANCHOR_BODY, np.uint8), anchor=sa, max_distance=smd, max_hits=np.ones(ns, np.uint32), hit_cap=1,
                            self_entity=sown)
    got = {}

    def casters():
        sq.casters_run()
        got["rays"] = sq.ray_caster_hits(device=True)
        got["shapes"] = sq.shape_caster_hits(device=True)

    def reaimed():
        b = w2.bodies_download()
        return (b["position"][ra] + qrot_np(b["rotation"][ra], ro), qrot_np(b["rotation"][ra], rd), b["position"][sa] + qrot_np(b["rotation"][sa], so), qrot_np(b["rotation"][sa], sd),
                qmul_np(srot, b["rotation"][sa]))

    def emulated():          # the same answers: k + 1 records, the own entity dropped on the host
        go, gd, gso, gsd, gsr = reaimed()
        sq.update()
        solid = np.ones(nr, np.uint8)
        h1, _ = sq.ray_hits(go[:n1], gd[:n1], 2, rmd[:n1], solid[:n1])
        h4, _ = sq.ray_hits(go[n1:], gd[n1:], 5, rmd[n1:], solid[n1:])
        hs, _ = sq.shape_hits(skind, she, gso, gsr, gsd, 2, smd)
        got["emulated"] = drop_own(h1, rown[:n1], 1), drop_own(h4, rown[n1:], 4), drop_own(hs, sown, 1)

    def emulated_hitting_itself():   # the cheaper calls with k, which cannot ignore the own entity
        go, gd, gso, gsd, gsr = reaimed()
        sq.update()
        solid = np.ones(nr, np.uint8)
        sq.cast_rays(go[:n1], gd[:n1], rmd[:n1], solid[:n1]); sq.ray_hits(go[n1:], gd[n1:], 4, rmd[n1:], solid[n1:]); sq.cast_shapes(skind, she, gso, gsr, gsd, smd)

    def upd():
        sq.update()

    def run_only():
        sq.casters_run()
    fns = {"casters_run_and_getters": casters, "emulated_k_plus_1": emulated, "emulated_hitting_itself": emulated_hitting_itself, "update_alone": upd, "casters_run_alone": run_only}
    times = {k: [] for k in fns}
    enqueue = []
    for it in range(reps + 1):       # (round 0 warms every variant up)
        for name, fn in fns.items():  # the variants alternate
            torch.cuda.synchronize(); w2.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            w2.synchronize(); torch.cuda.synchronize()
            if it:
                times[name].append((time.perf_counter() - t0) * 1e3)
                if name == "casters_run_alone":
                    enqueue.append((t1 - t0) * 1e3)
    for name in fns:
        res[f"casters_{name}_ms"] = float(np.median(times[name]))
    res["casters_run_host_side_ms"] = float(np.median(enqueue))
    res["casters_build_share_of_run"] = res["casters_update_alone_ms"] / res["casters_casters_run_alone_ms"]
    res["casters_emulated_over_casters"] = res["casters_emulated_k_plus_1_ms"] / res["casters_casters_run_and_getters_ms"]
    res["casters_timing"] = "median ms over reps rounds after a warm-up round, wall clock between device synchronisations, the variants alternating inside a round"
    res["casters_counts"] = {"ray_max_hits_1": n1, "ray_max_hits_4": n4, "shape": ns}
    casters()
    st = sq.stats()
    res["casters_leaves_per_caster"], res["casters_nodes_per_caster"] = st.leaves_visited / (nr + ns), st.nodes_visited / (nr + ns)
    hr = got["rays"][0].cpu().numpy().reshape(-1).view(sq.hit_dtype).reshape(nr, 4)
    hsd = got["shapes"][0].cpu().numpy().reshape(-1).view(sq.shape_hit_dtype).reshape(ns, 1)
    res["casters_hit_share"] = {"rays": float((hr[:, 0]["collider"] != MISS).mean()), "shapes": float((hsd[:, 0]["collider"] != MISS).mean())}
    # the emulation re-aims in numpy's operation order, not the device's: the colliders agree except where a rounding decides
    e1, e4, es = got["emulated"]
    res["casters_emulation_agreement"] = {"rays_k1": float((e1[:, 0]["collider"] == hr[:n1, 0]["collider"]).mean()), "rays_k4": float((e4["collider"] == hr[n1:]["collider"]).mean()),
                                          "shapes": float((es[:, 0]["collider"] == hsd[:, 0]["collider"]).mean())}
    sq.ray_casters_upload(np.zeros((0, 3)), np.zeros((0, 3), np.float32))
    sq.shape_casters_upload(np.zeros(0, np.uint8), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 4)), np.zeros((0, 3), np.float32))
    sq.update()


def capsule_legs(res, w2, sq, sc, dev, p, o, d, rot, short, long, cv, nc, mcfg, rounds, reps):
    n = p.shape[0]
    pred = torch.full((n,), 0.05, device=dev)
    keys = ("shapes_1m", "cast_shapes_short", "cast_shapes_long", "contacts_1m", "move_and_slide_256k")
    for name, kind_v, he_v in (("capsule", SHAPE_CAPSULE, (0.4, 0.5, 0.0)), ("cuboid", 0, (0.4, 0.9, 0.4))):
        kind = torch.full((n,), kind_v, dtype=torch.uint8, device=dev)
        he = torch.tensor(he_v, device=dev).repeat(n, 1).contiguous()
        ck, che, cp, cr = kind[:nc].contiguous(), he[:nc].contiguous(), o[:nc].contiguous(), rot[:nc].contiguous()
        calls = (lambda: sq.shape_intersections(kind, he, p, rot, 16), lambda: sq.cast_shapes(kind, he, o, rot, d, short), lambda: sq.cast_shapes(kind, he, o, rot, d, long),
                 lambda: sq.shape_contacts(kind, he, p, rot, pred, 16), lambda: sq.move_and_slide(ck, che, cp, cr, cv, **mcfg, move_and_slide_iterations=rounds, hit_cap=0))
        for key, fn in zip(keys, calls):
            count = nc if key.startswith("move") else n
            res[f"{name}_query_{key}_ms"] = timed(fn, reps)
            st = sq.stats()
            res[f"{name}_query_{key}_leaves_per_query"], res[f"{name}_query_{key}_nodes_per_query"] = st.leaves_visited / count, st.nodes_visited / count
    for key in keys:
        res[f"capsule_over_cuboid_{key}"] = res[f"capsule_query_{key}_ms"] / res[f"cuboid_query_{key}_ms"]
    res.update(newton_rounds_sample(sc.collider_kwargs(), w2.bodies_download(), o[:64].cpu().numpy(), d[:64].cpu().numpy(), rot[:64].cpu().numpy()))


def newton_rounds_sample(cols, bodies, oo, dd, rr, reach=10.0, radius=2.0):
    """Newton rounds of the capsule-cuboid pair test, from the numpy restatement: the given casts of the reference capsule over `reach` metres against
    the colliders whose centre lies within `radius` of a cast's path (every pair the cast can reach there, and many it merely passes)."""
    sys.path.insert(0, os.path.join(R, "tests"))
    import spatial_capsule_reference as CAP
    import spatial_query_reference as REF
    m = len(oo)
    nc = len(cols["shape"])
    centre = np.asarray(bodies["position"], float)[np.asarray(cols["body"], np.int64)]
    near = np.zeros(nc, bool)
    for i in range(m):
        t = np.clip((centre - oo[i]) @ dd[i], 0.0, reach)
        near |= np.linalg.norm(centre - (oo[i] + t[:, None] * dd[i]), axis=1) < radius
    idx = np.nonzero(near)[0]
    sub = {k: np.asarray(v)[idx] for k, v in cols.items() if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == nc}
    snap = REF.Snapshot(bodies, sub, None, np.float32)
    with np.errstate(all="ignore"):
        hit = CAP.cast_pairs(snap, np.full(m, SHAPE_CAPSULE, np.uint8), np.tile([0.4, 0.5, 0.0], (m, 1)), oo, rr, dd, np.full(m, reach))[0]
    rounds = CAP.last_rounds
    ran = rounds > 0
    return {"capsule_newton_rounds_mean_per_pair": float(rounds[ran].mean()) if ran.any() else 0.0,
            "capsule_newton_rounds_mean_per_hit_pair": float(rounds[hit & ran].mean()) if (hit & ran).any() else 0.0,
            "capsule_newton_rounds_max": int(rounds.max()) if rounds.size else 0, "capsule_newton_rounds_pairs": int(ran.sum()), "capsule_newton_rounds_casts": m}


def capsule_colliders_leg(res, sc, w_box, reps, dev):
    """The same queries into the all-cuboid cfg2 poses and into those poses with every fourth collider a capsule, the switch on."""
    b = w_box.bodies_download()
    n_col = sc.n
    shape = np.array(sc.shape, np.uint8).copy(); he = np.array(sc.half_extents, float).copy()
    caps = np.arange(n_col) % 4 == 1
    shape[caps] = SHAPE_CAPSULE; he[caps] = (0.3, 0.2, 0.0)
    w_cap = F.World(w_box.lib, F.default_config(32, substeps=4))
    w_cap.bodies_upload(**dict(sc.body_kwargs(), **b)); w_cap.colliders_upload(**dict(sc.collider_kwargs(), shape=shape, half_extents=he))
    g = torch.Generator(device=dev).manual_seed(3)
    n = 262144
    pos = torch.from_numpy(b["position"]).to(dev)
    o = pos[torch.randint(1, n_col, (n,), device=dev, generator=g)] + torch.randn(n, 3, device=dev, generator=g) * 0.7
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    solid = (torch.arange(n, device=dev) & 1).to(torch.uint8)
    short = torch.rand(n, device=dev, generator=g) * 2.0
    long = torch.full((n,), 200.0, device=dev)
    ext = torch.rand(n, 3, device=dev, generator=g)
    small = ext * 0.25
    kind = (torch.arange(n, device=dev) & 1).to(torch.uint8)
    rot = torch.nn.functional.normalize(torch.randn(n, 4, device=dev, generator=g), dim=1)
    pred = torch.full((n,), 0.05, device=dev)
    skin = torch.full((n,), 0.01, device=dev)
    ckind = torch.full((n,), SHAPE_CAPSULE, dtype=torch.uint8, device=dev)
    che = torch.tensor([0.4, 0.5, 0.0], device=dev).repeat(n, 1)
    upright = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).repeat(n, 1)
    cv = (d * 4.0).contiguous()
    mcfg = dict(delta_time=0.1, skin_width=0.01, max_depenetration_error=1e-4, penetration_rejection_threshold=0.5, depenetration_iterations=4)
    nk = 65536
    res["capcol_queries"] = n
    res["capcol_capsule_colliders"] = int(caps.sum())
    for name, w in (("boxes", w_box), ("capsules", w_cap)):
        sq = SpatialQuery(w, capsule_colliders=name == "capsules")

        def upd():
            sq.update(); w.synchronize()
        calls = {
            "update": upd,
            "cast_rays_short": lambda: sq.cast_rays(o, d, short, solid), "cast_rays_long": lambda: sq.cast_rays(o, d, long, solid),
            "ray_hits_k16_64k": lambda: sq.ray_hits(o[:nk], d[:nk], 16, long[:nk], solid[:nk]),
            "point_intersections": lambda: sq.point_intersections(o, 8), "aabb_intersections": lambda: sq.aabb_intersections(o - ext, o + ext, 16),
            "project_points": lambda: sq.project_points(o, solid),
            "shape_intersections": lambda: sq.shape_intersections(kind, ext, o, rot, 16), "shape_contacts": lambda: sq.shape_contacts(kind, ext, o, rot, pred, 16),
            "depenetrate": lambda: sq.depenetrate(kind, ext, o, rot, 0.05, 1e-4, 0.5, 4),
            "cast_shapes_short": lambda: sq.cast_shapes(kind, small, o, rot, d, short), "shape_hits_k16_64k": lambda: sq.shape_hits(kind[:nk], small[:nk], o[:nk], rot[:nk], d[:nk], 16, long[:nk]),
            "cast_moves": lambda: sq.cast_moves(kind, small, o, rot, cv * 0.1, skin),
            "move_and_slide": lambda: sq.move_and_slide(kind, small, o, rot, cv, **mcfg, move_and_slide_iterations=4, hit_cap=0),
            "capsule_query_cast_shapes_short": lambda: sq.cast_shapes(ckind, che, o, upright, d, short),
            "capsule_query_shape_contacts": lambda: sq.shape_contacts(ckind, che, o, upright, pred, 16),
            "capsule_query_move_and_slide": lambda: sq.move_and_slide(ckind, che, o, upright, cv, **mcfg, move_and_slide_iterations=4, hit_cap=0),
        }
        for key, fn in calls.items():
            res[f"capcol_{name}_{key}_ms"] = timed(fn, reps)
            if key != "update":
                st = sq.stats()
                res[f"capcol_{name}_{key}_leaves_per_query"] = st.leaves_visited / (nk if key.endswith("64k") else n)
        res[f"capcol_{name}_host_skipped"] = sq.stats().host_skipped
    for key in calls:
        res[f"capcol_ratio_{key}"] = res[f"capcol_capsules_{key}_ms"] / res[f"capcol_boxes_{key}_ms"]


def triangle_colliders_leg(res, sc, w_box, reps, dev):
    """The same queries into cfg2's boxes standing on their single cuboid ground (the existing scene: the yardstick) and into the same boxes at the same
    poses on the flat 8 192-face mesh of tools/time_trimesh.py (its top where the slab's top is), the triangle switch on."""
    sys.path.insert(0, os.path.join(R, "tools"))
    import time_trimesh
    b = w_box.bodies_download()
    msc = time_trimesh.build_scene(time_trimesh.CONFIGS["cfg2"])
    nf = msc.n_faces
    bm = {k: np.array(v).copy() for k, v in b.items()}
    bm["position"][0] = 0.0                                  # (body 0 carries the mesh: its frame's y = 0 is the slab's top)
    w_tri = F.World(w_box.lib, F.default_config(32, substeps=4))
    w_tri.bodies_upload(**dict(msc.body_kwargs(), **bm)); w_tri.colliders_upload(**msc.collider_kwargs(native_triangles=True))
    n_col = sc.n
    g = torch.Generator(device=dev).manual_seed(3)
    n = 262144
    pos = torch.from_numpy(b["position"]).to(dev)
    o = pos[torch.randint(1, n_col, (n,), device=dev, generator=g)] + torch.randn(n, 3, device=dev, generator=g) * 0.7
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    solid = (torch.arange(n, device=dev) & 1).to(torch.uint8)
    short = torch.rand(n, device=dev, generator=g) * 2.0
    long = torch.full((n,), 200.0, device=dev)
    ext = torch.rand(n, 3, device=dev, generator=g)
    small = ext * 0.25
    kind = (torch.arange(n, device=dev) & 1).to(torch.uint8)
    rot = torch.nn.functional.normalize(torch.randn(n, 4, device=dev, generator=g), dim=1)
    pred = torch.full((n,), 0.05, device=dev)
    skin = torch.full((n,), 0.01, device=dev)
    ckind = torch.full((n,), SHAPE_CAPSULE, dtype=torch.uint8, device=dev)
    che = torch.tensor([0.4, 0.5, 0.0], device=dev).repeat(n, 1)
    upright = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).repeat(n, 1)
    cv = (d * 4.0).contiguous()
    mcfg = dict(delta_time=0.1, skin_width=0.01, max_depenetration_error=1e-4, penetration_rejection_threshold=0.5, depenetration_iterations=4)
    nk = 65536
    res["tricol_queries"] = n
    res["tricol_faces"] = nf
    keep = {}
    for name, w in (("ground", w_box), ("mesh", w_tri)):
        sq = SpatialQuery(w, triangle_colliders=name == "mesh")

        def upd():
            sq.update(); w.synchronize()
        calls = {
            "update": upd,
            "cast_rays_short": lambda: sq.cast_rays(o, d, short, solid), "cast_rays_long": lambda: keep.__setitem__(name, sq.cast_rays(o, d, long, solid)),
            "ray_hits_k16_64k": lambda: sq.ray_hits(o[:nk], d[:nk], 16, long[:nk], solid[:nk]),
            "point_intersections": lambda: sq.point_intersections(o, 8), "aabb_intersections": lambda: sq.aabb_intersections(o - ext, o + ext, 16),
            "project_points": lambda: sq.project_points(o, solid),
            "shape_intersections": lambda: sq.shape_intersections(kind, ext, o, rot, 16), "shape_contacts": lambda: sq.shape_contacts(kind, ext, o, rot, pred, 16),
            "depenetrate": lambda: sq.depenetrate(kind, ext, o, rot, 0.05, 1e-4, 0.5, 4),
            "cast_shapes_short": lambda: sq.cast_shapes(kind, small, o, rot, d, short), "shape_hits_k16_64k": lambda: sq.shape_hits(kind[:nk], small[:nk], o[:nk], rot[:nk], d[:nk], 16, long[:nk]),
            "cast_moves": lambda: sq.cast_moves(kind, small, o, rot, cv * 0.1, skin),
            "move_and_slide": lambda: sq.move_and_slide(kind, small, o, rot, cv, **mcfg, move_and_slide_iterations=4, hit_cap=0),
            "capsule_query_cast_shapes_short": lambda: sq.cast_shapes(ckind, che, o, upright, d, short),
            "capsule_query_shape_contacts": lambda: sq.shape_contacts(ckind, che, o, upright, pred, 16),
            "capsule_query_move_and_slide": lambda: sq.move_and_slide(ckind, che, o, upright, cv, **mcfg, move_and_slide_iterations=4, hit_cap=0),
        }
        for key, fn in calls.items():
            res[f"tricol_{name}_{key}_ms"] = timed(fn, reps)
            if key != "update":
                st = sq.stats()
                res[f"tricol_{name}_{key}_leaves_per_query"] = st.leaves_visited / (nk if key.endswith("64k") else n)
        res[f"tricol_{name}_host_skipped"] = sq.stats().host_skipped
        hits = keep[name].cpu().numpy().reshape(-1).view(sq.hit_dtype)
        ground = hits["collider"] < nf if name == "mesh" else hits["collider"] == 0
        res[f"tricol_{name}_long_rays_answered_by_the_ground_share"] = float(((hits["collider"] != MISS) & ground).mean())
        res[f"tricol_{name}_long_rays_hit_share"] = float((hits["collider"] != MISS).mean())
    for key in calls:
        res[f"tricol_ratio_{key}"] = res[f"tricol_mesh_{key}_ms"] / res[f"tricol_ground_{key}_ms"]


def world(sc, steps):
    lib = avian_amd.load_library()
    w = F.World(lib, F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**sc.collider_kwargs())
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    if steps:
        w.pipeline_enable()
        for _ in range(steps):
            w.step()
    w.synchronize()
    return w


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = torch.device("cuda", 0)
    res = {"reps": reps, "timing": "median ms per call (device events on torch's stream around a synchronous call)"}
    sc2 = scenes.box_stack(50, 40, 50)
    w2 = world(sc2, 20)
    C = w2.n_colliders
    sq = SpatialQuery(w2)
    if "casters" in sys.argv[2:]:
        del res["timing"]          # (device events: the other legs'; this one's is res["casters_timing"])
        casters_leg(res, w2, sq, sc2, reps)
        print(json.dumps(res))
        return
    if "capcol" in sys.argv[2:]:
        capsule_colliders_leg(res, sc2, w2, reps, dev)
        print(json.dumps(res))
        return
    if "tricol" in sys.argv[2:]:
        triangle_colliders_leg(res, sc2, w2, reps, dev)
        print(json.dumps(res))
        return

    def upd():
        sq.update(); w2.synchronize()
    res["update_cfg2_ms"] = timed(upd, reps)
    res["update_cfg2_colliders"] = C
    b = w2.bodies_download()
    pos = torch.from_numpy(b["position"]).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    n = 1_000_000
    o = pos[torch.randint(1, C, (n,), device=dev, generator=g)] + torch.randn(n, 3, device=dev, generator=g) * 0.7
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    solid = torch.ones(n, dtype=torch.uint8, device=dev)
    short = torch.rand(n, device=dev, generator=g) * 2.0
    long = torch.full((n,), 200.0, device=dev)
    rec = 24
    for name, md in (("short", short), ("long", long)):
        ms = timed(lambda: sq.cast_rays(o, d, md, solid), reps)
        st = sq.stats()
        res[f"cast_rays_{name}_rays_per_s"] = n / (ms * 1e-3)
        res[f"cast_rays_{name}_ms"] = ms
        res[f"cast_rays_{name}_leaves_per_ray"] = st.leaves_visited / n
        res[f"cast_rays_{name}_nodes_per_ray"] = st.nodes_visited / n
        res[f"cast_rays_{name}_bytes_floor"] = n * (28 + 1 + rec)
    nk = 65536
    ms = timed(lambda: sq.ray_hits(o[:nk], d[:nk], 16, long[:nk], solid[:nk]), reps)
    res["ray_hits_k16_64k_ms"] = ms
    res["ray_hits_k16_64k_rays_per_s"] = nk / (ms * 1e-3)
    res["ray_hits_k16_leaves_per_ray"] = sq.stats().leaves_visited / nk
    res["ray_hits_k16_bytes_floor"] = nk * (28 + 1 + 16 * rec + 4)
    p = o
    ms = timed(lambda: sq.point_intersections(p, 8), reps)
    res["points_1m_ms"] = ms
    res["points_per_s"] = n / (ms * 1e-3)
    res["points_bytes_floor"] = n * (12 + 8 * 4 + 4)
    st = sq.stats()
    res["points_leaves_per_query"], res["points_nodes_per_query"] = st.leaves_visited / n, st.nodes_visited / n
    ext = torch.rand(n, 3, device=dev, generator=g)
    lo, hi = p - ext, p + ext
    ms = timed(lambda: sq.aabb_intersections(lo, hi, 16), reps)
    res["aabbs_1m_ms"] = ms
    res["aabbs_per_s"] = n / (ms * 1e-3)
    res["aabbs_bytes_floor"] = n * (24 + 16 * 4 + 4)
    st = sq.stats()
    res["aabbs_leaves_per_query"], res["aabbs_nodes_per_query"] = st.leaves_visited / n, st.nodes_visited / n
    for name, sol in (("solid", solid), ("hollow", torch.zeros_like(solid))):
        ms = timed(lambda: sq.project_points(p, sol), reps)
        st = sq.stats()
        res[f"project_{name}_1m_ms"] = ms
        res[f"project_{name}_per_s"] = n / (ms * 1e-3)
        res[f"project_{name}_leaves_per_query"], res[f"project_{name}_nodes_per_query"] = st.leaves_visited / n, st.nodes_visited / n
    res["project_bytes_floor"] = n * (12 + 1 + 28)
    kind = (torch.arange(n, device=dev) & 1).to(torch.uint8)                 # half cuboids (0), half balls (1)
    rot = torch.nn.functional.normalize(torch.randn(n, 4, device=dev, generator=g), dim=1)
    ms = timed(lambda: sq.shape_intersections(kind, ext, p, rot, 16), reps)
    st = sq.stats()
    res["shapes_1m_ms"] = ms
    res["shapes_per_s"] = n / (ms * 1e-3)
    res["shapes_leaves_per_query"], res["shapes_nodes_per_query"] = st.leaves_visited / n, st.nodes_visited / n
    res["shapes_bytes_floor"] = n * (1 + 12 + 12 + 16 + 16 * 4 + 4)
    # shape contacts and depenetration: the same query shapes (leaves = colliders that passed the filter, before the AABB precondition)
    pred = torch.full((n,), 0.05, device=dev)
    ms = timed(lambda: sq.shape_contacts(kind, ext, p, rot, pred, 16), reps)
    st = sq.stats()
    res["contacts_1m_ms"] = ms
    res["contacts_per_s"] = n / (ms * 1e-3)
    res["contacts_leaves_per_query"], res["contacts_nodes_per_query"] = st.leaves_visited / n, st.nodes_visited / n
    res["contacts_bytes_floor"] = n * (1 + 12 + 12 + 16 + 4 + 16 * 60 + 4)
    res["contacts_over_shapes"] = ms / res["shapes_1m_ms"]
    ms = timed(lambda: sq.depenetrate(kind, ext, p, rot, 0.05, 1e-4, 0.5, 4), reps)
    st = sq.stats()
    res["depenetrate_1m_ms"] = ms
    res["depenetrate_per_s"] = n / (ms * 1e-3)
    res["depenetrate_leaves_per_query"], res["depenetrate_nodes_per_query"] = st.leaves_visited / n, st.nodes_visited / n
    res["depenetrate_bytes_floor"] = n * (1 + 12 + 12 + 16 + 24)
    res["depenetrate_over_shapes"] = ms / res["shapes_1m_ms"]
    small = ext * 0.25
    crec = 60
    for name, md in (("short", short), ("long", long)):
        ms = timed(lambda: sq.cast_shapes(kind, small, o, rot, d, md), reps)
        st = sq.stats()
        res[f"cast_shapes_{name}_ms"] = ms
        res[f"cast_shapes_{name}_casts_per_s"] = n / (ms * 1e-3)
        res[f"cast_shapes_{name}_leaves_per_cast"], res[f"cast_shapes_{name}_nodes_per_cast"] = st.leaves_visited / n, st.nodes_visited / n
        res[f"cast_shapes_{name}_bytes_floor"] = n * (1 + 12 + 12 + 16 + 12 + 4 + crec)
    ms = timed(lambda: sq.shape_hits(kind[:nk], small[:nk], o[:nk], rot[:nk], d[:nk], 16, long[:nk]), reps)
    res["shape_hits_k16_64k_ms"] = ms
    res["shape_hits_k16_64k_casts_per_s"] = nk / (ms * 1e-3)
    res["shape_hits_k16_leaves_per_cast"] = sq.stats().leaves_visited / nk
    res["shape_hits_k16_bytes_floor"] = nk * (1 + 12 + 12 + 16 + 12 + 4 + 16 * crec + 4)
    # move and slide: a crowd of nc characters (the small cast shapes at the rays' origins, 4 m/s along the rays' directions, a step of 0.1 s)
    nc = 262144
    ck, che, cp, cr = kind[:nc].contiguous(), small[:nc].contiguous(), o[:nc].contiguous(), rot[:nc].contiguous()
    cv = (d[:nc] * 4.0).contiguous()
    mcfg = dict(delta_time=0.1, skin_width=0.01, max_depenetration_error=1e-4, penetration_rejection_threshold=0.5, depenetration_iterations=4)
    rounds = 4
    nv = 1_000_000
    pn = torch.nn.functional.normalize(torch.randn(nv, 4, 3, device=dev, generator=g), dim=2)
    pc = torch.randint(0, 5, (nv,), device=dev, generator=g, dtype=torch.int32)
    pv = torch.randn(nv, 3, device=dev, generator=g)
    ms = timed(lambda: sq.project_velocities(pv, pn, pc), reps)
    res["project_velocities_1m_ms"] = ms
    res["project_velocities_per_s"] = nv / (ms * 1e-3)
    res["project_velocities_bytes_floor"] = nv * (12 + 48 + 4 + 12)
    skin = torch.full((nc,), 0.01, device=dev)
    ms = timed(lambda: sq.cast_moves(ck, che, cp, cr, cv * 0.1, skin), reps)
    st = sq.stats()
    res["cast_moves_256k_ms"] = ms
    res["cast_moves_per_s"] = nc / (ms * 1e-3)
    res["cast_moves_leaves_per_move"], res["cast_moves_nodes_per_move"] = st.leaves_visited / nc, st.nodes_visited / nc
    ms = timed(lambda: sq.cast_shapes(ck, che, cp, cr, d[:nc].contiguous(), torch.full((nc,), 0.4, device=dev)), reps)
    res["cast_shapes_same_256k_ms"] = ms
    res["cast_moves_over_cast_shapes"] = res["cast_moves_256k_ms"] / ms
    slides = []
    ms = timed(lambda: slides.append(sq.move_and_slide(ck, che, cp, cr, cv, **mcfg, move_and_slide_iterations=rounds, hit_cap=0)[0]), reps)
    st = sq.stats()
    res["move_and_slide_256k_ms"] = ms
    res["move_and_slide_characters_per_s"] = nc / (ms * 1e-3)
    res["move_and_slide_leaves_per_character"], res["move_and_slide_nodes_per_character"] = st.leaves_visited / nc, st.nodes_visited / nc
    srec = slides[-1].cpu().numpy().reshape(-1).view(sq.slide_dtype)
    res["move_and_slide_live_share_per_round"] = [float((srec["iterations_run"] > r).mean()) for r in range(rounds)]
    res["move_and_slide_hits_per_character"] = float(srec["hit_count"].mean())
    # the same work through the entry points of the parent commit: two depenetrate calls, then per round one cast_shapes and one shape_contacts
    # call (cap AVN_SPATIAL_MAX_HITS, prediction 2 * skin_width) on the same characters, every character in every round
    md4 = torch.full((nc,), 0.4, device=dev)
    dn = d[:nc].contiguous()
    pred2 = torch.full((nc,), 0.02, device=dev)

    def composed():
        sq.depenetrate(ck, che, cp, cr, 0.01, 1e-4, 0.5, 4, skip_sensors=True)
        for _ in range(rounds):
            sq.cast_shapes(ck, che, cp, cr, dn, md4)
            sq.shape_contacts(ck, che, cp, cr, pred2, 64, skip_sensors=True)
        sq.depenetrate(ck, che, cp, cr, 0.01, 1e-4, 0.5, 4, skip_sensors=True)
    ms = timed(composed, reps)
    res["composed_parent_calls_256k_ms"] = ms
    res["move_and_slide_over_composed"] = res["move_and_slide_256k_ms"] / ms
    if "nocapsule" not in sys.argv[2:]:   # (an A/B run of a library from before the capsule: the legs above alone)
        capsule_legs(res, w2, sq, sc2, dev, p, o, d, rot, short, long, cv, nc, mcfg, rounds, reps)
    res["update_bytes_floor_per_collider"] = 4 * 16 + 16 + 8 + 4 * 16 + 2 * 16 + 2 * 2 * 16 + 8 + 12
    for k in [k for k in res if k.endswith("_bytes_floor")]:
        msk = k.replace("_bytes_floor", "_ms") if k.replace("_bytes_floor", "_ms") in res else None
        if msk:
            res[k.replace("_bytes_floor", "_hbm_fraction")] = res[k] / (res[msk] * 1e-3) / HBM
    casters_leg(res, w2, sq, sc2, reps)
    if "nocapsule" not in sys.argv[2:]:
        capsule_colliders_leg(res, sc2, w2, reps, dev)
    del sq, w2
    w4 = world(scenes.sparse_mixed(1_000_000), 0)
    sq4 = SpatialQuery(w4)

    def upd4():
        sq4.update(); w4.synchronize()
    res["update_cfg4_ms"] = timed(upd4, reps)
    res["update_cfg4_colliders"] = w4.n_colliders
    res["update_cfg2_hbm_fraction"] = res["update_bytes_floor_per_collider"] * C / (res["update_cfg2_ms"] * 1e-3) / HBM
    print(json.dumps(res))


if __name__ == "__main__":
    main()
