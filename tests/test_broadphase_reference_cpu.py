"""CPU: tests/broadphase_reference.py against the CPU oracle, on the scenes the GPU path tests use (tests/test_gpu_broadphase_paths.py).

reference_pairs is an independent numpy statement of collect_collision_pairs; here it must give the oracle's interval order and pair SEQUENCE on every scene
builder, up to 11 k colliders, by both of its routes.  dispatch_model is pinned on the two scenes whose path had drifted from what their tests said: the old
9 600-box wall (no long interval at all since SW_CAP became 65 536) and box_stack(30, 6, 60) (one long interval, 22 chunks, by the RELATIVE rule)."""
import numpy as np
import pytest

import broadphase_reference as R
from avian_amd import scenes
from helpers import F, oracle_lib


def oracle_frame(w, bodies=None, colliders=None):
    mn, mx, order, p = R.collect(w, bodies, colliders)
    return mn.astype(np.float64), mx.astype(np.float64), order, p


def check_scene(bits, pos, he, static, route="auto", **cfg):
    bodies, colliders, static = R.world_tables(pos, he, static)
    w = F.World(oracle_lib(), F.default_config(bits, **cfg))
    mn, mx, order, p = oracle_frame(w, bodies, colliders)
    n = len(pos)
    want, want_order = R.reference_pairs(mn, mx, np.arange(n), static, np.arange(n), route=route)
    assert np.array_equal(order, want_order), "interval order"
    assert np.array_equal(R.pairs_array(p), want), "pair sequence"
    return mn, mx, order, want


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("hx,plank_at,L", [(0.05, 64, 256), (0.05, 64, 257), (1.25, 128, 320), (1.25, 128, 321), (1.25, 191, 324), (1.25, 191, 325)])
def test_strip_matches_oracle_and_flips_where_the_issue_says(bits, hx, plank_at, L):
    pos, he, static = R.strip(1000, 1 / 32, hx, [(plank_at, L)])
    mn, mx, order, want = check_scene(bits, pos, he, static)
    assert len(want) > L // 2
    m = R.dispatch_model(mn[:, 0], mx[:, 0], order)
    at = int(np.flatnonzero(order == 1000)[0])
    assert at == plank_at and m["length"][at] == L, "the plank is sorted just before box plank_at and has exactly L candidates"
    others = {0.05: 3, 1.25: 81 if plank_at % 64 == 63 else 80}[hx]
    assert m["others"][at] == others
    assert m["n_long"] == (1 if L > max(256, 4 * others) else 0) and m["long_chunks"] == (-(-L // 512) if m["n_long"] else 0)


def test_more_than_64_chunks_scene_matches_oracle():
    pos, he, static = R.strip(33100, 1 / 32, 0.05, [(70, 32769), (200, 1025)])
    mn, mx, order, want = check_scene(32, pos, he, static)
    m = R.dispatch_model(mn[:, 0], mx[:, 0], order)
    assert sorted(m["chunks"][m["long"]].tolist()) == [3, 65] and len(want) > 20000


@pytest.mark.parametrize("bits", [32, 64])
def test_emit_tiles_match_oracle(bits):
    pos, he, static, per_tile = R.emit_tiles()
    mn, mx, order, want = check_scene(bits, pos, he, static)
    assert np.array_equal(order, np.arange(len(pos))), "tile-aligned: the sorted order is the upload order"
    assert np.bincount(want[:, 0] // 64, minlength=len(per_tile)).tolist() == per_tile
    assert np.all(want[:, 1] // 64 == want[:, 0] // 64), "no pair leaves its tile: every one lies in quarter 0 of its workgroup"
    owners = np.bincount(want[:, 0], minlength=len(pos))
    assert owners[64 * 41] == 15 and owners[64 * 42] == 16 and np.array_equal(owners[64 * 43:64 * 43 + 32], np.tile([1, 0], 16))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("pattern", R.SORT_PATTERNS)
def test_sort_scenes_match_oracle_over_three_frames(bits, pattern):
    n = 4 * R.SM_TILE + 1
    pos, he, static = R.sort_scene(pattern, n, bits)
    bodies, colliders, static = R.world_tables(pos, he, static)
    w = F.World(oracle_lib(), F.default_config(bits, contact_tolerance=0.0))
    order, seen, total = np.arange(n), np.zeros(0, np.uint64), 0
    for frame in range(3):
        if frame == 2:
            bodies["position"] = R.jitter_keys(pos)
        mn, mx, got_order, p = oracle_frame(w, bodies if frame != 1 else None, colliders if frame == 0 else None)
        if frame == 0:
            assert np.array_equal(mn[:, 0], pos[:, 0]), "min.x is the key, bit for bit"
        want, order = R.reference_pairs(mn, mx, order, static, np.arange(n), existing=seen)
        assert np.array_equal(got_order, order), f"frame {frame}: interval order"
        assert np.array_equal(R.pairs_array(p), want), f"frame {frame}: pair sequence"
        assert (len(want) > 500) if frame == 0 else (len(want) == 0) if frame == 1 else True
        seen = np.concatenate([seen, R.pair_keys(want[:, 0], want[:, 1])])
        total += len(want)
        if pattern == "equal" and frame < 2:
            assert np.array_equal(order, np.concatenate([[n - 1], np.arange(n - 1)])), "equal keys: the upload order survives behind the one smaller key"


def test_wall_route_equals_sweep_route_and_oracle_on_the_old_wall():
    pos, he, static = R.old_wall()
    mn, mx, order, want = check_scene(32, pos, he, static, route="sweep")
    grid, grid_order = R.reference_pairs(mn, mx, np.arange(len(pos)), static, np.arange(len(pos)), route="grid")
    assert np.array_equal(grid, want) and np.array_equal(grid_order, order) and len(want) > 500
    # the finding: this scene was written to overflow the chunk list when SW_CAP was 8 192.  Now no interval of it is long.
    m = R.dispatch_model(mn[:, 0], mx[:, 0], order)
    assert m["length"].max() == 9599 and m["n_long"] == 0 and m["long_chunks"] == 0


def test_box_stack_long_interval_is_one_relative_interval_of_22_chunks():
    sc = scenes.box_stack(30, 6, 60)
    w = F.World(oracle_lib(), F.default_config(32))
    mn, mx, order, p = oracle_frame(w, sc.body_kwargs(), sc.collider_kwargs())
    static = np.asarray(sc.rb_type) == F.RB_STATIC
    want, want_order = R.reference_pairs(mn, mx, np.arange(sc.n), static, np.arange(sc.n))
    assert np.array_equal(order, want_order) and np.array_equal(R.pairs_array(p), want)
    m = R.dispatch_model(mn[:, 0], mx[:, 0], order)
    assert m["n_long"] == 1 and m["long_chunks"] == 22 and not m["absolute"].any()


def test_absolute_rule_wall_is_what_the_gpu_test_claims():
    """The 65 601-box wall is compared with the grid route alone on the GPU (the oracle needs seconds for it): here the scene's claims, from closed-form AABBs."""
    n = 65601
    pos, he, static = R.wall(n, 257)
    mn, mx = pos - he - R.TOL, pos + he + R.TOL
    m = R.dispatch_model(mn[:, 0], mx[:, 0], np.arange(n))
    assert m["absolute"].sum() == 64 and m["absolute"][:64].all() and not m["relative"].any()
    assert set(m["chunks"][:64].tolist()) == {129} and m["long_chunks"] == 64 * 129
    want, order = R.reference_pairs(mn, mx, np.arange(n), static, np.arange(n), route="grid")
    assert np.array_equal(order, np.arange(n)) and len(want) > 9000
    # a small wall: both routes
    pos, he, static = R.wall(3000, 53)
    mn, mx = pos - he - R.TOL, pos + he + R.TOL
    a, _ = R.reference_pairs(mn, mx, np.arange(3000), static, np.arange(3000), route="grid")
    b, _ = R.reference_pairs(mn, mx, np.arange(3000), static, np.arange(3000), route="sweep")
    assert np.array_equal(a, b) and len(a) > 400


def test_reference_filters_layers_and_inactive_pairs_like_the_oracle():
    """CollisionLayers, static-static and an existing pair set, on a random cloud (the strip scenes use none of the layer bits)."""
    rng = np.random.default_rng(3)
    n = 1500
    pos = rng.uniform(0, 12, (n, 3)); he = rng.uniform(0.2, 0.6, (n, 3)); static = rng.random(n) < 0.3
    pos[7, 0] = np.nan; pos[8, 2] = np.inf
    bodies, colliders, static = R.world_tables(pos, he, static)
    colliders["memberships"] = rng.integers(1, 8, n).astype(np.uint32)
    colliders["filters"] = np.where(rng.random(n) < 0.3, rng.integers(0, 8, n), 0xFFFFFFFF).astype(np.uint32)
    w = F.World(oracle_lib(), F.default_config(64))
    mn, mx, order, p = oracle_frame(w, bodies, colliders)
    want, want_order = R.reference_pairs(mn, mx, np.arange(n), static, np.arange(n), colliders["memberships"], colliders["filters"])
    assert np.array_equal(order, want_order) and len(order) == n - 2
    assert np.array_equal(R.pairs_array(p), want) and len(want) > 1000
