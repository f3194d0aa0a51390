"""Two numpy (float64, no GPU) statements about the broad phase, and the scenes built to reach each of its interchangeable paths.

`reference_pairs` says WHAT collect_collision_pairs must return (reference collision/broad_phase.rs:214-475): the new interval order is a stable sort of
the previous order by aabb.min.x (-0 == +0, intervals with a non-finite AABB dropped); the pairs are, for every interval i of that order and every later
interval j whose min.x does not exceed i's max.x, the (i, j) whose y and z extents also meet (closed intervals: touching counts) and that pass the pair
filters -- i-major, j ascending.  It knows nothing of HOW the device gets there: no long / short split, no cull bounds, no quarters, no chunks.  Two routes
compute it: "sweep" enumerates the x-overlaps in row blocks of bounded memory; "grid" (for walls, where every x overlaps and the x-overlaps are n^2 / 2)
hashes the boxes into a y/z grid, tests the 3 x 3 neighbourhoods on all three axes and sorts what it finds into the same sequence.

`dispatch_model` restates the rule of k_sweep_ranges (which intervals are "long", in how many chunks).  It is used to BUILD scenes that sit on either side of
a threshold and to say what avn_broad_phase_stats::long_chunks must read; it never decides whether a pair list is right."""
from __future__ import annotations

import numpy as np

from helpers import F

# k_broadphase.hip (dispatch_model and the scene builders only)
SW_CAP, SW_LONG_MIN, SW_LCHUNK, SW_HIT_RECORDS = 65536, 256, 512, 15
SS_MAX, SM_TILE = 8192, 2048
TOL = 0.005   # NarrowPhaseConfig::contact_tolerance of default_config: every ColliderAabb is grown by it


# ---------------------------------------------------------------------------------------------------------------------------------------------
# what the result must be
def sorted_order(mn, mx, order_before):
    """The interval order after update_aabb_intervals + the stable sort: collider indices."""
    order_before = np.asarray(order_before, np.int64)
    finite = np.isfinite(mn[order_before]).all(axis=1) & np.isfinite(mx[order_before]).all(axis=1)
    kept = order_before[finite]
    key = mn[kept, 0].astype(np.float64) + 0.0   # (-0.0 + 0.0 is +0.0; argsort compares them equal anyway)
    return kept[np.argsort(key, kind="stable")]


def _expand(first, count):
    """rows, offset-in-row for `count[r]` entries per row r (row ids start at `first`)."""
    rows = np.repeat(np.arange(first, first + len(count)), count)
    start = np.cumsum(count) - count
    return rows, np.arange(len(rows)) - np.repeat(start, count)


def _route_sweep(mn, mx, order, block):
    n = len(order)
    minx, maxx = mn[order, 0], mx[order, 0]
    end = np.maximum(np.searchsorted(minx, maxx, side="right"), np.arange(n) + 1)   # first j with min.x[j] > max.x[i]
    count = end - (np.arange(n) + 1)
    cum = np.concatenate([[0], np.cumsum(count)])
    a = 0
    while a < n:
        b = max(a + 1, int(np.searchsorted(cum, cum[a] + block, side="right")) - 1)   # rows [a, b): at most `block` candidates (or one row)
        rows, off = _expand(a, count[a:b])
        cols = rows + 1 + off
        ca, cb = order[rows], order[cols]
        hit = (mn[ca, 1] <= mx[cb, 1]) & (mx[ca, 1] >= mn[cb, 1]) & (mn[ca, 2] <= mx[cb, 2]) & (mx[ca, 2] >= mn[cb, 2])
        yield rows[hit], cols[hit]
        a = b


def _route_grid(mn, mx, order):
    n = len(order)
    lo, hi = mn[order], mx[order]
    cell = []
    for ax in (1, 2):   # cells at least as wide as the widest box: two boxes that meet have min corners in the same or in adjacent cells
        size = max(float((hi[:, ax] - lo[:, ax]).max()), 1e-300)
        c = np.floor(lo[:, ax] / size).astype(np.int64)
        cell.append(c - c.min() + 1)
    width = int(cell[1].max()) + 2
    code = cell[0] * width + cell[1]
    by_cell = np.argsort(code, kind="stable")
    codes = code[by_cell]
    found = []
    for dy in (-1, 0, 1):
        for dz in (-1, 0, 1):
            want = code + dy * width + dz
            first = np.searchsorted(codes, want, side="left")
            count = np.searchsorted(codes, want, side="right") - first
            rows, off = _expand(0, count)
            cols = by_cell[np.repeat(first, count) + off]
            later = cols > rows
            rows, cols = rows[later], cols[later]
            hit = np.ones(len(rows), bool)
            for ax in range(3):
                hit &= (lo[rows, ax] <= hi[cols, ax]) & (hi[rows, ax] >= lo[cols, ax])
            found.append(rows[hit] * n + cols[hit])
    key = np.sort(np.concatenate(found))
    yield key // n, key % n


def pair_keys(c1, c2):
    c1 = np.asarray(c1, np.uint64); c2 = np.asarray(c2, np.uint64)
    return (np.minimum(c1, c2) << np.uint64(32)) | np.maximum(c1, c2)


def reference_pairs(mn, mx, order_before, inactive, body, memberships=None, filters=None, existing=None, route="auto", block=1 << 22):
    """-> (pairs [m, 2] collider indices in emission order, interval order after the frame).  `inactive`: the collider's body is static or sleeping;
    `existing`: uint64 PairKeys of ContactGraph::pair_set (pair_keys()); memberships / filters: CollisionLayers."""
    mn = np.asarray(mn, np.float64); mx = np.asarray(mx, np.float64)
    order = sorted_order(mn, mx, order_before)
    inactive = np.asarray(inactive, bool); body = np.asarray(body)
    if route == "auto":
        n = len(order)
        end = np.maximum(np.searchsorted(mn[order, 0], mx[order, 0], side="right"), np.arange(n) + 1)
        route = "grid" if int((end - np.arange(n) - 1).sum()) > (1 << 24) else "sweep"
    gen = _route_sweep(mn, mx, order, block) if route == "sweep" else _route_grid(mn, mx, order)
    out = []
    for rows, cols in gen:
        ca, cb = order[rows], order[cols]
        ok = ~(inactive[ca] & inactive[cb]) & (body[ca] != body[cb])
        if memberships is not None:
            ok &= ((memberships[ca] & filters[cb]) != 0) & ((memberships[cb] & filters[ca]) != 0)
        if existing is not None and len(existing):
            ok &= ~np.isin(pair_keys(ca, cb), existing)
        out.append(np.stack([ca[ok], cb[ok]], axis=1))
    return (np.concatenate(out) if out else np.zeros((0, 2), np.int64)), order


# ---------------------------------------------------------------------------------------------------------------------------------------------
# how the device splits the work (k_sweep_ranges)
def dispatch_model(mn_x, mx_x, order):
    """`order`: the SORTED interval order.  Per interval its candidate count, the mean of the other lanes of its 64-interval wave (integer division by 63,
    absent lanes of a ragged last wave count as 0), whether it is long (absolute rule | relative rule) and its chunks of SW_LCHUNK."""
    order = np.asarray(order, np.int64)
    n = len(order)
    minx, maxx = np.asarray(mn_x, np.float64)[order], np.asarray(mx_x, np.float64)[order]
    end = np.maximum(np.searchsorted(minx, maxx, side="right"), np.arange(n) + 1)
    length = end - (np.arange(n) + 1)
    waves = np.concatenate([length, np.zeros((-n) % 64, np.int64)]).reshape(-1, 64)
    others = ((waves.sum(axis=1, keepdims=True) - waves) // 63).ravel()[:n]
    absolute = length > SW_CAP
    relative = (length > SW_LONG_MIN) & (length > 4 * others)
    long = absolute | relative
    chunks = np.where(long, (length + SW_LCHUNK - 1) // SW_LCHUNK, 0)
    return dict(length=length, others=others, absolute=absolute, relative=relative, long=long, chunks=chunks,
                n_long=int(long.sum()), long_chunks=int(chunks.sum()), max_chunks=int(chunks.max()) if n else 0)


def sort_form(n, bits):
    """avn_broad_phase_stats::sort_form of a sort that runs over n intervals."""
    if n == 0:
        return F.SORT_FORM_NONE
    if bits == 32:
        return F.SORT_FORM_ONE_WORKGROUP if n <= SS_MAX else F.SORT_FORM_TILES_MERGE if n <= SM_TILE * 128 else F.SORT_FORM_RADIX_SCAN
    return F.SORT_FORM_FUSED_RADIX if n <= 1024 * 128 else F.SORT_FORM_RADIX_SCAN


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes: axis-aligned cuboids at rest, one body per collider, entity index == collider index
def world_tables(pos, he, static=None):
    pos = np.asarray(pos, np.float64); he = np.asarray(he, np.float64)
    n = len(pos)
    static = np.zeros(n, bool) if static is None else np.asarray(static, bool)
    inv_i = np.tile([6.0, 0, 0, 6.0, 0, 6.0], (n, 1)); inv_i[static] = 0.0
    bodies = dict(position=pos.copy(), rotation=np.tile([0, 0, 0, 1.0], (n, 1)), linear_velocity=np.zeros((n, 3)), angular_velocity=np.zeros((n, 3)),
                  inv_mass=np.where(static, 0.0, 1.0), inv_inertia_local=inv_i, rb_type=np.where(static, F.RB_STATIC, F.RB_DYNAMIC).astype(np.uint8))
    colliders = dict(entity_index=np.arange(n, dtype=np.uint32), body=np.arange(n, dtype=np.int32), shape=np.zeros(n, np.uint8), half_extents=he.copy(),
                     speculative_margin=np.zeros(n))   # (0: the ColliderAabb is the resting box grown by the contact tolerance, not a swept one)
    return bodies, colliders, static


def strip(N, dx, hx, planks, period=7):
    """N small boxes at x = k dx, y = (k mod period) / 4 (extent 0.11: rows do not meet, box k meets box k + period when their x extents do), every 5th static.
    planks = [(plank_at, L)]: a static plank sorted just before box `plank_at` (min.x half a step before that box's) whose max.x lies half a step past the
    min.x of follower L: exactly L x-overlapping candidates.  It spans rows 0 .. period - 2, so the last row's boxes are candidates it does not pair with.
    Planks are uploaded AFTER the boxes (collider N, N + 1, ...): the first frame's sort has work to do."""
    k = np.arange(N)
    pos = np.stack([k * dx, (k % period) * 0.25, np.zeros(N)], axis=1)
    he = np.tile([hx, 0.05, 0.05], (N, 1))
    static = (k % 5) == 0
    for plank_at, L in planks:
        assert 0 < plank_at and plank_at + L <= N
        lo = (plank_at * dx - hx - TOL) - dx / 2
        hi = ((plank_at + L - 1) * dx - hx - TOL) + dx / 2
        top = (period - 2) * 0.25
        pos = np.vstack([pos, [[(lo + hi) / 2, top / 2, 0.0]]])
        he = np.vstack([he, [[(hi - lo) / 2 - TOL, top / 2 + 0.01, 0.05]]])
        static = np.append(static, True)
    return pos, he, static


def wall(n, row, shift_every=7, x_step=2.0 ** -20):
    """n unit boxes on a sparse y/z grid (pitch 3, `row` boxes per row) whose x extents all overlap, in ascending x (collider k at x = k x_step);
    every `shift_every`-th box is moved 2.2 up, onto the box one row above it."""
    k = np.arange(n)
    pos = np.stack([k * x_step, (k // row) * 3.0, (k % row) * 3.0], axis=1)
    pos[::shift_every, 1] += 2.2
    return pos, np.full((n, 3), 0.5), np.zeros(n, bool)


def old_wall():
    """The 9 600-box wall test_long_interval_chunk_overflow_grows_and_retries used until SW_CAP went from 8 192 to 65 536."""
    ny, nz = 120, 80
    n = ny * nz
    yy, zz = np.meshgrid(np.arange(ny) * 3.0, np.arange(nz) * 3.0, indexing="ij")
    pos = np.stack([np.random.default_rng(7).uniform(-0.2, 0.2, n), yy.ravel(), zz.ravel()], axis=1)
    pos[::7, 1] += 2.2
    return pos, np.full((n, 3), 0.5), np.zeros(n, bool)


def emit_tiles():
    """Boxes at x = k (extent 1.01: box k's only x-overlapping candidate is k + 1), so a 64-interval tile's pairs all lie in quarter 0 of its workgroup.
    Tiles 0 .. 40: boxes 0 .. t of tile t share a row (t touching neighbour pairs), the rest alternate between two rows that do not meet: the count pass
    finds 0 .. 40 pairs, on both sides of SW_HIT_RECORDS.  Tile 41 / 42: lane 0 is wide and tall, it alone owns 15 / 16 pairs.  Tile 43: 16 lanes own one each.
    -> pos, he, static, pairs per tile."""
    tiles = 44
    n = 64 * tiles
    k = np.arange(n)
    lane, tile = k % 64, k // 64
    pos = np.stack([k * 1.0, 2.0 + 2.0 * (lane % 2), np.zeros(n)], axis=1)
    he = np.full((n, 3), 0.5)
    chain = (tile <= 40) & (lane <= tile)
    pos[chain, 1] = 0.0
    for t, w in ((41, 15), (42, 16)):   # min.x as every box, max.x reaching over w followers; y over both rows
        k0 = 64 * t
        pos[k0] = [k0 + (w - 1) / 2.0, 3.0, 0.0]
        he[k0] = [0.5 + (w - 1) / 2.0, 1.0, 0.5]
        pos[k0 - 1, 1] = 20.0   # (the last box of the tile before it keeps out of its way)
    k0 = 64 * 43
    pos[k0:k0 + 32, 1] = np.repeat(np.arange(16) * 2.0 + 8.0, 2)   # lanes (2 m, 2 m + 1) share row m
    per_tile = list(range(41)) + [15, 16, 16]
    return pos, he, np.zeros(n, bool), per_tile


SORT_PATTERNS = ("random", "equal", "runs", "one_byte")


def sort_keys(pattern, n, bits, seed=0):
    """n min.x values, ascending, exact in the world's scalar type (returned as float64)."""
    rng = np.random.default_rng(seed)
    ft, it = (np.float32, np.uint32) if bits == 32 else (np.float64, np.uint64)
    tiny = float(np.finfo(ft).tiny)
    if pattern == "random":   # ~4 copies of each value; negatives, both zeros, denormals
        pool = rng.normal(scale=50.0, size=n // 4).astype(ft)
        pool[:8] = np.array([0.0, -0.0, tiny / 4, -tiny / 4, tiny / 1024, -tiny / 2, tiny, -tiny], ft)
        keys = pool[rng.integers(0, len(pool), n)]
        keys[:32] = np.tile(pool[:8], 4)
    elif pattern == "equal":  # ... but one, uploaded last: the sort has to run, and the equal keys must come out in upload order
        keys = np.full(n, 1.5, ft)
        keys[0] = 0.25
    elif pattern == "runs":   # distinct keys, but the 100 around every multiple of SM_TILE -- counted from either end: the first frame sorts the
        keys = np.arange(n).astype(ft)   # descending upload order, later frames the ascending one -- are equal
        for b in sorted(set(range(SM_TILE, n, SM_TILE)) | {n - 1 - b for b in range(SM_TILE, n, SM_TILE)}):
            keys[max(0, b - 50):min(n, b + 50)] = ft(b)
    else:                     # one byte of the bit pattern varies (byte 1: the second radix pass alone orders them)
        base = np.array([1.0], ft).view(it)[0]
        keys = (base | (rng.integers(0, 256, n).astype(it) << it(8))).view(ft)
    keys = keys.astype(np.float64)
    return keys[np.argsort(keys + 0.0, kind="stable")]


def sort_scene(pattern, n, bits, seed=0):
    """Boxes of zero x extent whose min.x IS the key (contact_tolerance 0 in the world's config), uploaded in DESCENDING key order -- the merge of sorted
    tiles then searches every tile for every element.  y/z: `equal` spreads the boxes over a 91 x 91 grid in which neighbours meet; the other patterns
    deal them onto 8 x 8 cells, so that boxes of equal key often meet."""
    keys = sort_keys(pattern, n, bits, seed)[::-1]
    k = np.arange(n)
    g = 91 if pattern == "equal" else 8
    h = np.random.default_rng(seed + 1).permutation(n) if pattern != "equal" else k
    pos = np.stack([keys, (h % g) * 0.9, ((h // g) % g) * 0.9], axis=1)
    he = np.tile([0.0, 0.5, 0.5], (n, 1))
    return pos, he, np.zeros(n, bool)


def jitter_keys(pos, seed=0):
    """Frame 3 of the sort sequence: one box in 20 takes the key of another box, one in 20 swaps keys with its upload neighbour."""
    rng = np.random.default_rng(seed + 2)
    n = len(pos)
    x = pos[:, 0].copy()
    far = rng.choice(n, n // 20, replace=False)
    x[far] = pos[rng.integers(0, n, len(far)), 0]
    near = rng.choice(n - 1, n // 20, replace=False)
    x[near], x[near + 1] = x[near + 1].copy(), x[near].copy()
    out = pos.copy(); out[:, 0] = x
    return out


def pairs_array(p):
    """avn_pair records -> [m, 2] collider indices."""
    return np.stack([p["collider1"].astype(np.int64), p["collider2"].astype(np.int64)], axis=1)


def collect(w, bodies=None, colliders=None):
    """One frame on world `w`: (re-)upload what is given, UPDATE_AABB, COLLECT_COLLISION_PAIRS -> (aabb min, aabb max, interval order, pairs)."""
    if bodies is not None:
        w.bodies_upload(**bodies)
    if colliders is not None:
        w.colliders_upload(**colliders)
        w.existing_pairs_upload(np.zeros(0, np.uint64))
    w.run_system("UPDATE_AABB"); w.run_system("COLLECT_COLLISION_PAIRS")
    mn, mx, order = w.aabbs_download()
    return mn, mx, order.astype(np.int64), w.pairs_get()
