#!/usr/bin/env python3
"""What swept CCD (include/avian_mi355x_ccd.h) costs on cfg2's settled device closed loop (50 x 40 x 50 unit cubes on a ground).

usage: python tools/time_swept_ccd.py MODE [repeats]
  nolist          no SweptCcd list: `repeats` windows of 100 steps without a synchronisation in between, after 100 settling steps.  Run it with
                  AVN_LIB_PATH=<the parent commit's library> AVN_AB_OLDER_LIBRARY=1 for the other side of a same-box A/B: this tree adds no
                  launch, event or allocation without a list, so the two must sit within the spread of their own repeats.
  all             every body listed (the ground has no SolverBody and is skipped on the device): the same windows.
  bullets         1 000 balls (r = 0.1, AVN_COLLIDER_SWEPT_CCD, SpeculativeMargin 0) parked over the pile from the start, listed, and fired
                  down at 300 units / s after the settling steps: per step the wall time, swept_ccd_ms and the number of entries with a hit.
  bullets_nolist  the same scene and shots without the list (what the steps cost when the bullets tunnel into the pile instead).
  bullets_nl      the same 1 000 bullets, spinning at (20, 0, 35) rad / s and listed with SweepMode::NonLinear (avn_swept_ccd_non_linear_set on):
                  per step also nonlinear_tested, rounds_max and exhausted of avn_swept_ccd_stats_get.
  capsules        the same shots with 1 000 capsule bullets (AVN_SHAPE_CAPSULE, r = 0.1, h = 0.3, upright) and avn_swept_ccd_capsules_set on,
                  SweepMode::Linear: the figures of `bullets`.
  capsules_nl     the capsule bullets spinning at (20, 0, 35) rad / s, SweepMode::NonLinear: the figures of `bullets_nl`.
  ab OLDER [repeats]
                  a same-box A/B of `nolist` and `bullets` (1 000 Linear bullets) against an older build of the library (the parent commit's
                  libavian_mi355x.so): child processes, alternating older / this tree, `repeats` runs a side, the side that goes first alternating too.  Per leg one summary line: the
                  older library's min .. max over its repeats, this tree's, and whether this tree's median lies inside the older one's range.
One JSON line per run."""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import avian_amd
from avian_amd import _ffi as F, scenes

SETTLE, WINDOW, N_BULLETS = 100, 100, 1000


def tables(with_bullets, capsules=False):
    sc = scenes.box_stack(50, 40, 50)
    bodies, cols = sc.body_kwargs(), sc.collider_kwargs()
    n = sc.n
    bullets = np.zeros(0, np.uint32)
    if with_bullets:
        k = N_BULLETS
        side = int(np.ceil(np.sqrt(k)))
        gx, gz = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
        pos = np.stack([(gx.ravel()[:k] - (side - 1) * 0.5) * 1.5, np.full(k, 40 * 0.99 + 6.0), (gz.ravel()[:k] - (side - 1) * 0.5) * 1.5], axis=1)
        ident = np.tile([0.0, 0, 0, 1], (k, 1))
        add = dict(position=pos, rotation=ident, linear_velocity=np.zeros((k, 3)), angular_velocity=np.zeros((k, 3)), inv_mass=np.full(k, 1 / 0.004),
                   inv_inertia_local=np.tile([1 / 1.6e-5, 0, 0, 1 / 1.6e-5, 0, 1 / 1.6e-5], (k, 1)), rb_type=np.zeros(k, np.uint8))
        bodies = {key: np.concatenate([np.asarray(v), add[key]]) for key, v in bodies.items()}
        bodies["gravity_scale"] = np.concatenate([np.ones(n), np.zeros(k)])   # parked until they are fired
        he = np.zeros((k, 3)); he[:, 0] = 0.1
        if capsules:
            he[:, 1] = 0.3
        cols = dict(entity_index=np.arange(n + k, dtype=np.uint32), body=np.arange(n + k, dtype=np.int32),
                    shape=np.concatenate([cols["shape"], np.full(k, F.SHAPE_CAPSULE if capsules else F.SHAPE_BALL, np.uint8)]),
                    half_extents=np.concatenate([cols["half_extents"], he]), collider_flags=np.concatenate([np.zeros(n, np.uint8), np.full(k, F.COLLIDER_SWEPT_CCD, np.uint8)]),
                    speculative_margin=np.concatenate([np.full(n, -1.0), np.zeros(k)]))
        bullets = np.arange(n, n + k, dtype=np.uint32)
    return bodies, cols, n, bullets


def leg_metrics(mode, out):
    """What one run of a leg is judged by."""
    if mode == "nolist":
        return dict(ms_per_step=out["median"])
    steps = out["steps"]
    return dict(device_step_ms=float(np.median([r["device_step_ms"] for r in steps])), swept_ccd_ms=float(np.median([r["swept_ccd_ms"] for r in steps])),
                first_step_swept_ccd_ms=steps[0]["swept_ccd_ms"])


def ab(older, repeats):
    here = os.path.abspath(__file__)
    for mode in ("nolist", "bullets"):
        runs = {"older": [], "this": []}
        for rep in range(repeats):
            for side in (("older", "this") if rep % 2 == 0 else ("this", "older")):   # alternating, and the side that goes first alternates too
                env = dict(os.environ)
                env.pop("AVN_LIB_PATH", None); env.pop("AVN_AB_OLDER_LIBRARY", None)
                if side == "older":
                    env.update(AVN_LIB_PATH=os.path.abspath(older), AVN_AB_OLDER_LIBRARY="1")
                r = subprocess.run([sys.executable, here, mode, "5"], env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    print(json.dumps(dict(mode=mode, side=side, error=r.stderr[-400:])), flush=True)
                    sys.exit(1)
                out = json.loads(r.stdout.strip().splitlines()[-1])
                runs[side].append(leg_metrics(mode, out))
                print(json.dumps(dict(ab=mode, side=side, library=out["library"], **{k: round(v, 4) for k, v in runs[side][-1].items()})), flush=True)
        for key in runs["this"][0]:
            o, t = [r[key] for r in runs["older"]], [r[key] for r in runs["this"]]
            med = float(np.median(t))
            print(json.dumps(dict(ab=mode, metric=key, older_min=round(min(o), 4), older_median=round(float(np.median(o)), 4), older_max=round(max(o), 4),
                                  this_min=round(min(t), 4), this_median=round(med, 4), this_max=round(max(t), 4), this_median_inside_older_range=bool(min(o) <= med <= max(o)),
                                  difference_of_medians=round(med - float(np.median(o)), 4))), flush=True)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "nolist"
    if mode == "ab":
        return ab(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    capsules = mode.startswith("capsules")
    with_bullets = mode.startswith("bullets") or capsules
    non_linear = mode in ("bullets_nl", "capsules_nl")
    lib = avian_amd.load_library()
    bodies, cols, n, bullets = tables(with_bullets, capsules)
    w = F.World(lib, F.default_config(32, substeps=4))
    w.bodies_upload(**bodies); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
    w.pipeline_enable()
    ccd = None
    if mode in ("all", "bullets", "bullets_nl", "capsules", "capsules_nl"):
        from avian_amd.swept_ccd import SWEEP_LINEAR, SWEEP_NON_LINEAR, SweptCcd
        ccd = SweptCcd(w, non_linear=non_linear, capsules=capsules)
        ccd.upload(bullets if with_bullets else np.arange(n, dtype=np.uint32), mode=SWEEP_NON_LINEAR if non_linear else SWEEP_LINEAR)
    for _ in range(SETTLE):
        w.step()
    w.synchronize()
    out = dict(mode=mode, library=os.path.relpath(lib.path), bodies=len(bodies["inv_mass"]), listed=0 if ccd is None else ccd.count)
    if not with_bullets:
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(WINDOW):
                w.step()
            w.synchronize()
            ms.append((time.perf_counter() - t0) / WINDOW * 1e3)
        out.update(window_steps=WINDOW, ms_per_step=[round(x, 4) for x in ms], median=round(float(np.median(ms)), 4), spread=round(max(ms) - min(ms), 4))
        if ccd is not None:
            rec = ccd.results()
            out.update(swept_ccd_ms=round(w.diagnostics().swept_ccd_ms, 4), tested=int(rec["tested"].sum()), hits=int((rec["hit_body"] >= 0).sum()))
    else:
        state = w.bodies_download()
        kw = dict(bodies)
        for key in ("position", "rotation", "linear_velocity", "angular_velocity"):
            kw[key] = state[key].astype(np.float64)
        kw["linear_velocity"][bullets] = [0.0, -300.0, 0.0]
        if non_linear:
            kw["angular_velocity"][bullets] = [20.0, 0.0, 35.0]
        w.bodies_upload(**kw)
        rows = []
        for s in range(repeats * 2):
            t0 = time.perf_counter(); w.step(); w.synchronize(); wall = (time.perf_counter() - t0) * 1e3
            row = dict(step=s, wall_ms=round(wall, 3), device_step_ms=round(w.timers().step_ms, 3))
            if ccd is not None:
                rec = ccd.results()
                row.update(swept_ccd_ms=round(w.diagnostics().swept_ccd_ms, 4), tested=int(rec["tested"].sum()), hits=int((rec["hit_body"] >= 0).sum()))
                if non_linear:
                    row.update(ccd.stats())
            rows.append(row)
        out.update(steps=rows, lowest_bullet_y=round(float(w.bodies_download()["position"][bullets, 1].min()), 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
