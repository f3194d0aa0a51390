#!/usr/bin/env python3
"""The rounds SweepMode::NonLinear's conservative advancement (include/avian_mi355x_ccd.h, N3) takes: runs the numpy reference with a cap of
4096 over the fixed random set of tests/test_swept_ccd_nonlinear_cpu.py (20 000 Ball / Cuboid pairs, float64) and writes the histogram,
split by hit or miss, with the percentile CCD_NL_ROUNDS is chosen from.  CPU only.

--capsules: the capsule set of tests/swept_ccd_capsule_rounds.py instead (20 000 pairs with at least one Capsule collider, the five role / kind
combinations in equal parts), through its batched form of tests/swept_ccd_capsule_reference.py: the rounds under a cap of 4096, the pairs that
run out of the shipped CCD_NL_ROUNDS, and the Newton rounds of the Linear casts of the same pairs.  The cap is not chosen from this set.

usage: python tools/swept_ccd_nonlinear_rounds.py [jobs] > profiles/swept_ccd_nonlinear_rounds.txt
       python tools/swept_ccd_nonlinear_rounds.py --capsules > profiles/swept_ccd_capsule_rounds.txt"""
import os
import sys
from multiprocessing import Pool

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import swept_ccd_nonlinear_reference as NL          # noqa: E402
import test_swept_ccd_nonlinear_cpu as T            # noqa: E402


def run(p):
    res, _, rounds = T.run_rounds_pair(p, T.ROUNDS_MEASURE_CAP)
    return p["kind"], res, rounds


def capsules():
    import swept_ccd_capsule_reference as CAPR     # noqa: E402
    import swept_ccd_capsule_rounds as R           # noqa: E402
    pairs = R.rounds_set()
    n = len(pairs)
    res, _, rounds = R.batch_advance(pairs, R.ROUNDS_MEASURE_CAP)
    res64, _, _ = R.batch_advance(pairs, CAPR.CCD_NL_ROUNDS)
    newton = R.batch_newton_rounds(pairs)
    kind = np.array([p["kind"] for p in pairs])
    combo = np.array([p["combo"] for p in pairs])
    srt = np.sort(rounds)
    pct = lambda q: int(srt[int(np.ceil(q * n)) - 1])
    cap = CAPR.CCD_NL_ROUNDS
    over = int((res64 == CAPR.EXHAUSTED).sum())
    names = {CAPR.HIT: "hit", CAPR.MISSED: "miss", CAPR.EXHAUSTED: "exhausted"}
    print(f"# numpy reference (float64, batched), cap {R.ROUNDS_MEASURE_CAP}, seed {R.ROUNDS_SEED}, {n} pairs with a Capsule collider, dt = 1/60, contact_tolerance {R.TOL}")
    print("# outcomes: " + ", ".join(f"{names[k]} {int((res == k).sum())}" for k in names))
    print(f"# rounds: median {int(np.median(rounds))}, 99th percentile {pct(0.99)}, 99.9th percentile {pct(0.999)}, maximum {int(rounds.max())}")
    print(f"# under the shipped CCD_NL_ROUNDS = {cap} (not changed by this set): exhausted {over} ({100.0 * over / n:.3f} %)")
    print(f"# Linear casts of the same pairs (step 3): Newton rounds maximum {int(newton.max())}, casts that end on SP_CAPSULE_ROUNDS = {CAPR.SP_CAPSULE_ROUNDS}: "
          f"{int((newton == CAPR.SP_CAPSULE_ROUNDS).sum())}")
    for k, name in enumerate(("general", "graze", "pure spin", "pure translation")):
        r = rounds[kind == k]
        print(f"# {name}: maximum {int(r.max())}, more than {cap} rounds: {int((r > cap).sum())}")
    for k, name in enumerate(("cuboid - capsule", "ball - capsule", "capsule - ball", "capsule - cuboid", "capsule - capsule")):
        r = rounds[combo == k]
        print(f"# {name} (collider 1 - collider 2): median {int(np.median(r))}, maximum {int(r.max())}, more than {cap} rounds: {int((r > cap).sum())}, "
              f"Newton rounds maximum {int(newton[combo == k].max())}")
    print("# rounds      hit     miss")
    edges = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 512, 1024, 2048, 4096]
    lo = 1
    for hi in edges:
        sel = (rounds >= lo) & (rounds <= hi)
        label = f"{lo}" if lo == hi else f"{lo}-{hi}"
        print(f"{label:>9} {int((sel & (res == CAPR.HIT)).sum()):8d} {int((sel & (res == CAPR.MISSED)).sum()):8d}")
        lo = hi + 1
    print(f"exhausted at {R.ROUNDS_MEASURE_CAP}: {int((res == CAPR.EXHAUSTED).sum())}")


def main():
    if "--capsules" in sys.argv[1:]:
        return capsules()
    jobs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    pairs = T.rounds_set()
    with Pool(jobs) as pool:
        out = pool.map(run, pairs, chunksize=100)
    rounds = np.array([r for _, _, r in out])
    res = np.array([r for _, r, _ in out])
    kind = np.array([k for k, _, _ in out])
    n = len(out)
    srt = np.sort(rounds)
    p999 = int(srt[int(np.ceil(0.999 * n)) - 1])
    cap = 1
    while cap < p999:
        cap *= 2
    names = {NL.HIT: "hit", NL.MISSED: "miss", NL.EXHAUSTED: "exhausted"}
    print(f"# numpy reference (float64), cap {T.ROUNDS_MEASURE_CAP}, seed {T.ROUNDS_SEED}, {n} pairs, dt = 1/60, contact_tolerance {T.TOL}")
    print(f"# outcomes: " + ", ".join(f"{names[k]} {int((res == k).sum())}" for k in names))
    print(f"# rounds: median {int(np.median(rounds))}, 99th percentile {int(srt[int(np.ceil(0.99 * n)) - 1])}, 99.9th percentile {p999}, maximum {int(rounds.max())}")
    print(f"# CCD_NL_ROUNDS = {cap} (the smallest power of two >= the 99.9th percentile); pairs that need more than {cap} rounds: {int((rounds > cap).sum())} "
          f"({100.0 * (rounds > cap).sum() / n:.3f} %)")
    for k, name in enumerate(("general", "graze", "pure spin", "pure translation")):
        r = rounds[kind == k]
        print(f"# {name}: maximum {int(r.max())}, more than {cap} rounds: {int((r > cap).sum())}")
    print("# rounds      hit     miss")
    edges = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 512, 1024, 2048, 4096]
    lo = 1
    for hi in edges:
        sel = (rounds >= lo) & (rounds <= hi)
        label = f"{lo}" if lo == hi else f"{lo}-{hi}"
        print(f"{label:>9} {int((sel & (res == NL.HIT)).sum()):8d} {int((sel & (res == NL.MISSED)).sum()):8d}")
        lo = hi + 1
    print(f"exhausted at {T.ROUNDS_MEASURE_CAP}: {int((res == NL.EXHAUSTED).sum())}")


if __name__ == "__main__":
    main()
