"""GPU: the frozen-manifold step runs its broad phase on a second stream, and where the solver beside it is much longer than the chain
(world/broad_phase.hpp: sweep_count_pad) k_sweep's count pass is bounded to two resident workgroups per CU by an LDS reservation
(k_broadphase.hip: sweep_footprint_pad).  The bound is placement only: the pair list of such a step, order included, equals the CPU
oracle's COLLECT_COLLISION_PAIRS on the same colliders, in f32 and f64 --
  - seeded random unit boxes in a volume sized for ~6 overlaps each, uploaded in ascending min.x, n = 1, 63, 64, 65, 129 (the 64-interval tile's edges);
  - n = 64 * (CU count * 2) + 65: more tiles than workgroups can be resident under the bound;
  - a ground slab spanning everything (the long-interval path, by the RELATIVE rule of k_sweep_ranges: 1 500 candidates in 3 chunks, 288 in 1 chunk
    on the lattice -- the absolute rule, SW_CAP = 65 536 candidates, is tests/test_gpu_broadphase_paths.py's) and a NaN pose (dropped intervals);
  - a frozen box stack over four steps with an upload that makes the third step find new pairs (the emit pass): pair count, pairs, bodies, impulses.
The release build takes the bound only by its work rule, which these small scenes do not meet, so the bounded launches run on the `make measure`
build with AVN_SWEEP_BOUND_MIN_WORK=0 (the bound wherever the chain overlaps) and AVN_SWEEP_WG_PER_CU = 2 (the default), 1 (a workgroup's LDS above
64 KiB) and 0 (unbounded); the release build runs every case as well.

tests/test_gpu_frozen_replay_forms.py, which the round's plan named, does not exist: it was to cover the form kept for starting the broad phase
earlier in graph replay, and none of the three candidates was kept -- eager and replayed steps run the code they ran before."""
import numpy as np
import pytest

from avian_amd import scenes
from helpers import F, hip_lib, hip_measure_lib, oracle_lib

pytestmark = pytest.mark.gpu

SWEEP_WG_PER_CU = 2   # World::SWEEP_WG_PER_CU (world/broad_phase.hpp)


def bounded(monkeypatch, resident):
    """The measure build with the bound wherever the chain overlaps, `resident` workgroups per CU."""
    monkeypatch.setenv("AVN_SWEEP_BOUND_MIN_WORK", "0")
    monkeypatch.setenv("AVN_SWEEP_WG_PER_CU", str(resident))
    return hip_measure_lib()


def random_boxes(n, seed, slab=False):
    """n unit boxes at seeded random positions in a cube sized for ~6 overlaps each (two unit boxes overlap inside a volume of 8), in ascending
    min.x so that the oracle's insertion sort is linear.  Body 0 is static: the first box, or a slab under and around everything."""
    rng = np.random.default_rng(seed)
    side = max(1.0, (8.0 * n / 6.0) ** (1.0 / 3.0))
    c = rng.uniform(0.0, side, size=(n, 3))
    c = c[np.argsort(c[:, 0], kind="stable")]
    if slab:
        return scenes._assemble(c, (0.5, 0.5, 0.5), (side * 0.5, -1.0, side * 0.5), (side + 2.0, 1.0, side + 2.0))
    return scenes._assemble(c[1:], (0.5, 0.5, 0.5), c[0], (0.5, 0.5, 0.5))


def collect_pairs(lib, bits, sc, in_step):
    """Every pair of the scene is new: found by the step's own broad phase (count pass on the second stream) or by the stand-alone system."""
    w = F.World(lib, F.default_config(bits, substeps=1))
    w.bodies_upload(**sc.body_kwargs())
    w.colliders_upload(**sc.collider_kwargs())
    w.existing_pairs_upload(np.zeros(0, np.uint64))
    if in_step:
        w.step()
        w.synchronize()
    else:
        w.run_system("UPDATE_AABB")
        w.run_system("COLLECT_COLLISION_PAIRS")
    return w.pairs_get()


def check_against_oracle(monkeypatch, bits, sc, min_pairs, residents=(SWEEP_WG_PER_CU, 1, 0)):
    want = collect_pairs(oracle_lib(), bits, sc, in_step=False)
    assert len(want) >= min_pairs
    assert np.array_equal(collect_pairs(hip_lib(), bits, sc, in_step=True), want), "release build, in a step"
    for r in residents:
        assert np.array_equal(collect_pairs(bounded(monkeypatch, r), bits, sc, in_step=True), want), f"bounded to {r} per CU, in a step"
    return want


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_random_boxes_around_the_tile_edges(bits, n, monkeypatch):
    want = check_against_oracle(monkeypatch, bits, random_boxes(n, seed=100 + n), min_pairs=0 if n == 1 else n)
    assert (len(want) == 0) == (n == 1)


@pytest.mark.parametrize("bits", [32, 64])
def test_more_tiles_than_resident_workgroups(bits, monkeypatch):
    import torch
    cap = torch.cuda.get_device_properties(0).multi_processor_count * SWEEP_WG_PER_CU   # workgroups resident at once under the bound
    n = 64 * cap + 65
    check_against_oracle(monkeypatch, bits, random_boxes(n, seed=7), min_pairs=2 * n, residents=(SWEEP_WG_PER_CU, 1))


def nan_pose(sc):
    sc.position = np.array(sc.position, dtype=np.float64, copy=True)
    sc.position[sc.n // 2, 1] = np.nan
    return sc


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["slab", "nan_pose", "lattice_slab"])
def test_long_intervals_and_dropped_intervals(bits, name, monkeypatch):
    if name == "lattice_slab":
        sc = scenes.box_stack(9, 4, 8)    # equal min.x over whole lattice layers, ground 800 wide
    else:
        sc = random_boxes(1500, seed=11, slab=True)
        if name == "nan_pose":
            sc = nan_pose(sc)
    check_against_oracle(monkeypatch, bits, sc, min_pairs=500)


def frozen_world(lib, bits, sc, substeps=2):
    """As bench.py's setup_world: the pair list of one broad phase, synthetic face manifolds for it, coloured and uploaded."""
    w = F.World(lib, F.default_config(bits, substeps=substeps))
    w.bodies_upload(**sc.body_kwargs())
    w.colliders_upload(**sc.collider_kwargs())
    w.existing_pairs_upload(np.zeros(0, np.uint64))
    w.run_system("UPDATE_AABB")
    w.run_system("COLLECT_COLLISION_PAIRS")
    pairs = w.pairs_get()
    mf = scenes.axis_aligned_manifolds(sc, np.stack([pairs["body1"], pairs["body2"]], axis=1))
    offs, perm = scenes.color_manifolds(hip_lib(), mf, sc.rb_type)
    scenes.upload_manifolds(w, scenes.permute_manifolds(mf, perm), offs, sc.friction, sc.restitution)
    return w


def moved_top_box(sc):
    """The scene's bodies with one box of the top layer moved one lattice cell sideways (onto its neighbour: new pairs for the next broad phase)."""
    kw = dict(sc.body_kwargs())
    pos = np.array(kw["position"], dtype=np.float64, copy=True)
    dyn = np.flatnonzero(np.asarray(sc.inv_mass) > 0)
    top = dyn[pos[dyn, 1] == pos[dyn, 1].max()]
    xs = np.unique(pos[top, 0])
    pos[top[0], 0] += xs[1] - xs[0]
    kw["position"] = pos
    return kw


def run_frozen(lib, bits, sc):
    w = frozen_world(lib, bits, sc)
    out = []
    for s in range(4):
        if s == 2:
            w.bodies_upload(**moved_top_box(sc))
        w.step()
        w.synchronize()
        out.append((w.timers().pair_count, w.pairs_get(), w.bodies_download(), w.impulses_download()))
    return out


def assert_same(a, b, what):
    for s, ((na, pa, ba, ia), (nb, pb, bb, ib)) in enumerate(zip(a, b)):
        assert na == nb, f"{what}: step {s}: pair_count {na} != {nb}"
        assert np.array_equal(pa, pb), f"{what}: step {s}: pair lists differ"
        for k in ba:
            assert np.array_equal(ba[k], bb[k], equal_nan=True), f"{what}: step {s}: bodies.{k} differs"
        for k in ia:
            assert np.array_equal(ia[k], ib[k], equal_nan=True), f"{what}: step {s}: impulses.{k} differs"


@pytest.mark.parametrize("bits", [32, 64])
def test_frozen_steps_do_not_depend_on_the_sweep_bound(bits, monkeypatch):
    sc = scenes.box_stack(6, 5, 6)
    ref = run_frozen(oracle_lib(), bits, sc)
    assert ref[2][0] > 0 and len(ref[2][1]) == ref[2][0], "the moved box must give the third step new pairs"
    assert ref[0][0] == 0 and ref[3][0] == 0
    assert_same(ref, run_frozen(hip_lib(), bits, sc), "release build against the oracle")
    for r in (SWEEP_WG_PER_CU, 1, 4, 0):
        assert_same(ref, run_frozen(bounded(monkeypatch, r), bits, sc), f"bounded to {r} per CU against the oracle")


def test_the_reservation_is_the_two_per_cu_split_on_mi355x(monkeypatch, capfd):
    # 160 KiB of LDS per CU: 163 840 / 3 rounded up to 2 KiB plus 2 KiB = 57 344 B per workgroup, of which k_sweep's count pass holds 22 544 B statically.
    # (World init fails if the runtime's own occupancy for that size is not two per CU: sweep_footprint_pad.)
    monkeypatch.setenv("AVN_HOST_TRACE", "1")
    F.World(hip_measure_lib(), F.default_config(32, substeps=1))
    assert "2 resident workgroups per CU asked, 34800 bytes of LDS reserved" in capfd.readouterr().err
