"""GPU: Capsule colliders on the device (include/avian_mi355x.h "capsule colliders") against the numpy restatement of their definitions
(tests/capsule_collider_reference.py): the pair manifolds and the AABB bit for bit, and the closed loop against the ORACLE world that holds the
same capsules as AVN_SHAPE_HOST answered by that restatement -- the oracle has no capsule kind, the reference is not derived from the device code."""
import numpy as np
import pytest

import capsule_collider_reference as CC
from avian_amd import scenes
from helpers import F, hip_lib, oracle_lib
from host_shape_helpers import assert_same_closed_loop_step
from test_capsule_collider_cpu import CAP, COMBOS, SCENE, STEPS, RowKinds, constructed_pairs, hosted_world, random_pairs

pytestmark = pytest.mark.gpu


def native_world(lib, bits, scene_kw=SCENE, sleeping=False):
    """The capsule_drop scene with its capsules as AVN_SHAPE_CAPSULE colliders."""
    sc = scenes.capsule_drop(**scene_kw)
    w = F.World(lib, F.default_config(bits, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**sc.collider_kwargs())
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction, restitution=0.0)
    w.pipeline_enable()
    if sleeping:
        w.sleeping_enable()
    return w, sc


# ---- 1. pairs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_pair_manifolds_equal_the_reference_bit_for_bit(bits):
    dt = np.float32 if bits == 32 else np.float64
    rng = np.random.default_rng(40 + bits)
    batches = [random_pairs(rng, k1, k2, 800) for k1, k2 in COMBOS] + [random_pairs(rng, CAP, CAP, 400), constructed_pairs()]
    batch = tuple(np.concatenate([b[i] for b in batches]) for i in range(9))
    batch = tuple(x.astype(np.uint8) if i in (0, 4) else x.astype(dt) for i, x in enumerate(batch))
    w = F.World(hip_lib(), F.default_config(bits))
    got = w.contact_manifolds(*batch)
    ref = CC.manifolds(*batch, dt)
    assert len(batch[0]) > 4000 and (ref["point_count"] == 2).sum() > 100 and (ref["point_count"] == 1).sum() > 1000
    for k in ("point_count", "normal", "anchor1", "anchor2", "penetration", "feature_id1", "feature_id2"):
        if not np.array_equal(got[k], ref[k], equal_nan=True):
            bad = np.nonzero((got[k] != ref[k]).reshape(len(got[k]), -1).any(1))[0]
            raise AssertionError(f"{k}: {len(bad)} pairs differ, first {bad[0]} (kinds {batch[0][bad[0]]}, {batch[4][bad[0]]}): device {got[k][bad[0]]} reference {ref[k][bad[0]]}")


def test_kinds_two_and_four_stay_bad_arguments():
    w = F.World(hip_lib(), F.default_config(32))
    one = lambda k1, k2: w.contact_manifolds([k1], [[0.3, 0.4, 0.3]], [[0, 0, 0]], [[0, 0, 0, 1]], [k2], [[0.3, 0.4, 0.3]], [[0.5, 0, 0]], [[0, 0, 0, 1]], 0.1)
    for k1, k2 in ((2, 0), (0, 2), (4, 3), (3, 4), (3, 2)):
        with pytest.raises(F.AvnError) as e:
            one(k1, k2)
        assert e.value.status == 1   # AVN_ERR_BAD_ARG
    assert one(3, 0)["point_count"][0] == 2   # (a capsule standing next to a box face: the two ends of its clipped segment)


# ---- 2. AABB -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_collider_aabbs_equal_the_reference_boxes(bits):
    """After one UPDATE_AABB the native capsules' ColliderAabb equals the box of the world that holds them as host shapes answered by the reference
    (reference box of the start pose, merged with the end pose's under a positive speculative margin, grown by the same margins).  Half of the
    colliders have speculative margin 0 (the plain box), and there are child capsules with a ColliderTransform."""
    rng = np.random.default_rng(bits)
    sc = scenes.capsule_drop(40, seed=1, n_boxes=4, n_balls=4)
    n = sc.n
    cols = sc.collider_kwargs()
    cols["speculative_margin"] = np.where(np.arange(n) % 2 == 0, 0.0, -1.0)     # (-1: the world's default, which is positive)
    cols["collision_margin"] = np.where(np.arange(n) % 3 == 0, 0.02, 0.0)
    child = (np.arange(n) % 5 == 1).astype(np.uint8)
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    tr = rng.uniform(-0.3, 0.3, (n, 3))
    host = CC.CapsuleHost(cols["entity_index"], sc.shape, sc.half_extents)
    boxes = []
    for hosted in (False, True):
        w = F.World(hip_lib(), F.default_config(bits, substeps=4))
        w.bodies_upload(**sc.body_kwargs())
        w.colliders_upload(**dict(cols, shape=np.where(sc.shape == CAP, F.SHAPE_HOST, sc.shape).astype(np.uint8) if hosted else sc.shape))
        w.collider_transforms_upload(is_child=child, translation=tr, rotation=q)
        if hosted:
            w.host_shapes_set(host.aabb, host.manifolds)
        w.existing_pairs_upload(np.zeros(0, np.uint64))
        w.run_system("UPDATE_AABB")
        w.synchronize()
        assert not w.host_shape_errors()
        boxes.append(w.aabbs_download())
    (mna, mxa, _), (mnb, mxb, _) = boxes
    caps = sc.shape == CAP
    assert caps.sum() == 40 and (child.astype(bool) & caps).sum() >= 4
    assert np.array_equal(mna, mnb) and np.array_equal(mxa, mxb)
    assert np.isfinite(mna[caps]).all() and ((mxa - mna)[caps] > 0.49).all()


# ---- 3. closed loop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_closed_loop_equals_the_oracle_that_hosts_the_capsules(bits):
    """World A: HIP, native AVN_SHAPE_CAPSULE.  World B: the oracle, the capsules AVN_SHAPE_HOST answered by the reference.  World C: HIP, hosted through
    the same callbacks.  Bodies, new pairs, colour lists, contact rows and ColliderAabb are equal every step (tests/test_capsule_collider_cpu.py asserts
    that these steps of this scene meet every pair kind).  Without the feature kind 3 is a box: A != B at the first contact."""
    a, _ = native_world(hip_lib(), bits)
    b, hb, _ = hosted_world(oracle_lib(), bits)
    c, hc, _ = hosted_world(hip_lib(), bits)
    for step in range(STEPS):
        a.step(); b.step(); c.step()
        assert_same_closed_loop_step(a, b, step)
        assert_same_closed_loop_step(a, c, step)
    assert hb.kinds == hc.kinds and sum(v for (k, n), v in hb.kinds.items() if n == 2) >= 20 and hb.manifold_queries > 1000


# ---- 4. scale-free sanity ------------------------------------------------------------------------------------------------------------------
def test_two_hundred_native_capsules_come_to_rest_and_warm_start():
    w, sc = native_world(hip_lib(), 32, dict(n=200, seed=5, n_boxes=0, n_balls=0, spacing=1.4, layers=1))
    kinds = RowKinds(sc)
    for _ in range(240):
        w.step()
        kinds.after_step(w)
    assert not w.host_shape_errors() and w.host_shape_stats().host_colliders == 0
    b = w.bodies_download()
    y = b["position"][1:, 1]
    r = 0.25
    print("capsule heights: min", y.min(), "median", np.median(y), "max", y.max())
    assert np.isfinite(b["position"]).all()
    assert (y > r - 0.03).all(), "no capsule sank into the ground"
    assert (y < r + 0.45).all(), "every capsule lies on the ground or leans on a neighbour"
    assert np.median(y) < r + 0.05
    share, touching = kinds.warm_start_share(w)
    print("warm-started share of touching capsule rows:", share, "of", touching)
    assert touching > 150 and share >= 0.9, "feature ids carry the impulses of resting capsules from step to step"


# ---- 5. neighbours -------------------------------------------------------------------------------------------------------------------------
def test_a_capsule_free_world_is_untouched_by_a_capsule_world_next_to_it():
    """The capsule path is selected per world: boxes stepped alone == the same boxes stepped while a capsule world steps in the same process."""
    def boxes():
        sc = scenes.box_stack(5, 4, 5)
        w = F.World(hip_lib(), F.default_config(32, substeps=4))
        w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**sc.collider_kwargs())
        w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
        w.pipeline_enable()
        return w
    alone, beside = boxes(), boxes()
    for _ in range(20):
        alone.step()
    caps, _ = native_world(hip_lib(), 32)
    for step in range(20):
        caps.step(); beside.step(); caps.step()
    x, y = alone.bodies_download(), beside.bodies_download()
    for k in x:
        assert np.array_equal(x[k], y[k]), f"bodies.{k}"
    (oa, ha), (ob, hb) = alone.pipeline_handles(), beside.pipeline_handles()
    assert np.array_equal(oa, ob) and np.array_equal(ha, hb)
    ids = np.sort(ha)
    ra, rb = alone.contacts_download(ids), beside.contacts_download(ids)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), f"contact rows.{k}"
    assert float(np.abs(caps.bodies_download()["linear_velocity"]).max()) > 0.1


def test_spatial_queries_treat_capsule_colliders_as_host_shapes():
    from avian_amd.spatial_query import SpatialQuery
    w, sc = native_world(hip_lib(), 32)
    for _ in range(3):
        w.step()
    w.synchronize()
    sq = SpatialQuery(w)
    sq.update()
    rng = np.random.default_rng(9)
    o = rng.uniform([-2, 0.2, -2], [2, 4, 2], (256, 3)); d = rng.normal(size=(256, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d)
    assert e.value.status == 6   # AVN_ERR_STATE
    got = sq.cast_rays(o, d, skip_host_shapes=True)
    caps = np.nonzero(sc.shape == CAP)[0]
    hit = got["collider"][got["collider"] != 0xFFFFFFFF]
    assert len(hit) > 50 and not np.isin(hit, caps).any(), "capsule colliders are never candidates"
    assert sq.stats().host_skipped == len(caps) == 24


def test_sleeping_capsules_and_a_wake_equal_the_hosted_oracle():
    kw = dict(n=8, seed=2, n_boxes=2, n_balls=1)
    a, _ = native_world(hip_lib(), 32, kw, sleeping=True)
    b, _, _ = hosted_world(oracle_lib(), 32, kw, sleeping=True)
    slept = woke = 0
    for step in range(400):
        if slept and not woke and step % 10 == 0:
            body = int(np.nonzero(a.sleeping_state()["sleeping"])[0][0])
            a.wake_bodies([body]); b.wake_bodies([body])
            woke = step
        a.step(); b.step()
        slept = max(slept, int(a.sleeping_state()["sleeping"].sum()))
        if woke and step > woke + 20:
            break
    assert slept > 0 and woke, "the capsules must have fallen asleep and one must have been woken"
    assert not b.host_shape_errors()
    x, y = a.bodies_download(), b.bodies_download()
    for k in x:
        assert np.array_equal(x[k], y[k]), f"bodies.{k}"
    sa, sb = a.sleeping_state(), b.sleeping_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), f"sleeping state.{k}"
