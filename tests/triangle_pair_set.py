"""The pair set of the triangle collider's tests, built once per scalar and shared (with the reference's answer) by the host sanitizer test and the GPU
batch-query test: `random_pairs(rng, k1, k2, 800)` for the six COMBOS of test_triangle_collider_cpu with the two flag columns replaced by uniform random
values 0..7, plus `constructed_pairs()`, plus 400 triangle-free rows over kinds 0, 1 and 3.  Also the file format of tests/triangle_pair_main.cpp."""
import functools

import numpy as np

import triangle_collider_reference as TR
from test_triangle_collider_cpu import COMBOS, constructed_pairs, random_pairs

CUB, BALL, CAP, TRI = TR.SHAPE_CUBOID, TR.SHAPE_BALL, TR.SHAPE_CAPSULE, TR.SHAPE_TRIANGLE
ROWS_PER_COMBO = 800
TRIANGLE_FREE_ROWS = 400
SEED = 20261021
COLUMNS = ("shape1", "he1", "pos1", "rot1", "shape2", "he2", "pos2", "rot2", "prediction", "vertices1", "vertices2", "flags1", "flags2")
OUTPUTS = ("point_count", "normal", "anchor1", "anchor2", "penetration", "feature_id1", "feature_id2")


def concat(batches, dt):
    """A list of 13-column batches -> one dict of arrays in the scalar `dt`."""
    cols = [np.concatenate([np.asarray(b[k]) for b in batches]) for k in range(13)]
    out = {}
    for name, c in zip(COLUMNS, cols):
        out[name] = c.astype(np.uint8) if name.startswith(("shape", "flags")) else np.ascontiguousarray(c.astype(dt))
    return out


def random_flag_pairs(rng, k1, k2, n):
    b = list(random_pairs(rng, k1, k2, n))
    b[11] = rng.integers(0, 8, n).astype(np.uint8)
    b[12] = rng.integers(0, 8, n).astype(np.uint8)
    return tuple(b)


def triangle_free_pairs(rng, n):
    kinds = [(a, b) for a in (CUB, BALL, CAP) for b in (CUB, BALL, CAP)]
    sizes = [n // len(kinds) + (1 if k < n % len(kinds) else 0) for k in range(len(kinds))]
    return [random_pairs(rng, a, b, m) for (a, b), m in zip(kinds, sizes)]


def reference(p, dt, flags1=None, flags2=None):
    return TR.manifolds(p["shape1"], p["he1"], p["pos1"], p["rot1"], p["shape2"], p["he2"], p["pos2"], p["rot2"], p["prediction"], p["vertices1"], p["vertices2"],
                        p["flags1"] if flags1 is None else flags1, p["flags2"] if flags2 is None else flags2, dt)


@functools.lru_cache(maxsize=None)
def pair_set(bits):
    """(pairs, reference manifolds, reference manifolds with every flag 7, slices per combination) -- computed once per scalar; read-only for the tests."""
    dt = np.float32 if bits == 32 else np.float64
    rng = np.random.default_rng(SEED)
    batches, spans, at = [], {}, 0
    for k1, k2 in COMBOS:
        batches.append(random_flag_pairs(rng, k1, k2, ROWS_PER_COMBO))
        spans[(k1, k2)] = slice(at, at + ROWS_PER_COMBO); at += ROWS_PER_COMBO
    batches.append(constructed_pairs())
    at += len(batches[-1][0])
    free = triangle_free_pairs(rng, TRIANGLE_FREE_ROWS)
    batches += free
    spans["free"] = slice(at, at + TRIANGLE_FREE_ROWS)
    p = concat(batches, dt)
    ref = reference(p, dt)
    n = len(p["shape1"])
    ref7 = reference(p, dt, np.full(n, 7, np.uint8), np.full(n, 7, np.uint8))
    for a in list(p.values()) + list(ref.values()) + list(ref7.values()):
        a.setflags(write=False)
    return p, ref, ref7, spans


def coverage(p, ref, ref7, spans):
    """The coverage conditions of the pair set, counted on the REFERENCE's output: {label: (count, required)}."""
    pc = ref["point_count"].astype(int)
    out = {}
    for k1, k2 in COMBOS:
        s = spans[(k1, k2)]
        other = k2 if k1 == TRI else k1
        label = f"{k1}-{k2}"
        if other == CAP:
            out[label + " two-point capsule manifolds"] = (int((pc[s] == 2).sum()), 20)
        if other == CUB:
            out[label + " cuboid manifolds with 5 or more points"] = (int((pc[s] >= 5).sum()), 15)
        changed = (pc[s] != ref7["point_count"][s]) | (ref["normal"][s] != ref7["normal"][s]).any(axis=1)
        out[label + " rows the flags change"] = (int(changed.sum()), 50)
    cub = np.concatenate([np.arange(n_)[spans[c]] for n_ in [len(pc)] for c in COMBOS if CUB in c])
    out["cuboid manifolds with 6 or more points"] = (int((pc[cub] >= 6).sum()), 3)
    return out


def write_pairs(path, p, bits):
    """The input file of tests/triangle_pair_main.cpp."""
    dt = np.float32 if bits == 32 else np.float64
    n = len(p["shape1"])
    with open(path, "wb") as f:
        f.write(np.array([bits, n], np.int32).tobytes())
        for name in ("shape1", "shape2", "flags1", "flags2"):
            f.write(np.ascontiguousarray(p[name], np.uint8).tobytes())
        for name, k in (("he1", 3), ("pos1", 3), ("rot1", 4), ("he2", 3), ("pos2", 3), ("rot2", 4), ("prediction", 1), ("vertices1", 9), ("vertices2", 9)):
            a = np.ascontiguousarray(p[name], dt)
            assert a.size == k * n, name
            f.write(a.tobytes())


def read_manifolds(path, n, bits):
    """The output file of tests/triangle_pair_main.cpp, in the layout of World.contact_manifolds."""
    dt = np.float32 if bits == 32 else np.float64
    Q = TR.MAX_POINTS
    raw = open(path, "rb").read()
    at = 0

    def take(count, t):
        nonlocal at
        a = np.frombuffer(raw, t, count, at); at += a.nbytes
        return a
    out = dict(point_count=take(n, np.uint8), normal=take(3 * n, dt).reshape(n, 3), anchor1=take(3 * Q * n, dt).reshape(n, Q, 3), anchor2=take(3 * Q * n, dt).reshape(n, Q, 3),
               point=take(3 * Q * n, dt).reshape(n, Q, 3), penetration=take(Q * n, dt).reshape(n, Q), feature_id1=take(Q * n, np.uint32).reshape(n, Q),
               feature_id2=take(Q * n, np.uint32).reshape(n, Q))
    assert at == len(raw), "the output file has the expected size"
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
