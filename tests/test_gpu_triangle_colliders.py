"""GPU: Triangle colliders on the device (include/avian_mi355x_trimesh.h) against the numpy restatement of their definitions
(tests/triangle_collider_reference.py): the pair manifolds and the AABB bit for bit, the closed loop against the ORACLE world that holds the same faces as
AVN_SHAPE_HOST answered by that restatement (the oracle has no triangle kind; the reference is not derived from the device code) and against the HIP world
that hosts them the same way.  Every comparison is at tolerance 0: the definitions fix the operation order."""
import numpy as np
import pytest

import triangle_collider_reference as TR
import triangle_pair_set as PS
from avian_amd import scenes
from helpers import F, hip_lib, oracle_lib
from hook_helpers import Hooks, assert_same_hooked_step, hooked_world
from host_shape_helpers import assert_same_closed_loop_step
from test_triangle_collider_cpu import BALL, CAP, CUB, SCENE, STEPS, TRI, bumps, lowest_points

pytestmark = pytest.mark.gpu
BAD_ARG, STATE = 1, 6


def mesh_world(lib, bits, mode, scene_kw=None, sleeping=False, sc=None):
    """The trimesh_drop scene.  mode "native": HIP, AVN_SHAPE_TRIANGLE + AVN_SHAPE_CAPSULE colliders; "hosted": HIP, the faces AVN_SHAPE_HOST answered by
    TriangleHost (capsules native); "oracle": the faces and the capsules AVN_SHAPE_HOST answered by MeshHost."""
    sc = sc if sc is not None else scenes.trimesh_drop(**(scene_kw or SCENE), height_fn=bumps)
    cols = sc.collider_kwargs(native_triangles=True) if mode == "native" else sc.collider_kwargs(host_capsules=mode == "oracle")
    w = F.World(lib, F.default_config(bits, substeps=4))
    w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**cols)
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=sc.friction, restitution=0.0)
    host = None
    if mode != "native":
        host = (TR.MeshHost if mode == "oracle" else TR.TriangleHost)(cols["entity_index"], sc.col_shape, sc.col_half_extents, sc.vertices, sc.edge_flags)
        w.host_shapes_set(host.aabb, host.manifolds)
    w.pipeline_enable()
    if sleeping:
        w.sleeping_enable()
    return w, host, sc


# ---- 1. pairs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_pair_manifolds_equal_the_reference_bit_for_bit(bits):
    p, ref, ref7, spans = PS.pair_set(bits)
    for label, (got, need) in PS.coverage(p, ref, ref7, spans).items():
        print(f"{label}: {got} (at least {need})")
        assert got >= need, label
    w = F.World(hip_lib(), F.default_config(bits))
    args = [p[k] for k in ("shape1", "he1", "pos1", "rot1", "shape2", "he2", "pos2", "rot2", "prediction")]
    got = w.triangle_manifolds(*args, vertices1=p["vertices1"], vertices2=p["vertices2"], edge_flags1=p["flags1"], edge_flags2=p["flags2"])
    tri = (p["shape1"] == TRI) | (p["shape2"] == TRI)
    free = spans["free"]
    assert not tri[free].any() and tri.sum() == len(tri) - PS.TRIANGLE_FREE_ROWS
    plain = w.contact_manifolds(*[a[free] for a in args])
    assert (plain["point_count"] > 0).sum() > 50
    for k in PS.OUTPUTS:
        want = ref[k].copy()
        want[free] = plain[k]   # (the triangle-free rows: what World.contact_manifolds answers; the reference leaves them empty)
        if not np.array_equal(got[k], want, equal_nan=True):
            bad = np.nonzero((got[k] != want).reshape(len(want), -1).any(1))[0]
            raise AssertionError(f"{k}: {len(bad)} pairs differ, first {bad[0]} (kinds {p['shape1'][bad[0]]}, {p['shape2'][bad[0]]}): device {got[k][bad[0]]} reference {want[bad[0]]}")


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_kinds_the_batch_queries_refuse():
    w = F.World(hip_lib(), F.default_config(32))
    tri9 = [[0, 0, 0, 0, 0, 1, 1, 0, 0]]
    one = lambda fn, k1, k2, **kw: fn([k1], [[0.3, 0.4, 0.3]], [[0, 0.2, 0]], [[0, 0, 0, 1]], [k2], [[0.3, 0.4, 0.3]], [[0.2, 0, 0.2]], [[0, 0, 0, 1]], 0.1, **kw)
    for k1, k2 in ((4, 0), (0, 4), (4, 3)):
        with pytest.raises(F.AvnError) as e:
            one(w.contact_manifolds, k1, k2)
        assert e.value.status == BAD_ARG
    for k1, k2 in ((2, 4), (4, 2), (5, 0), (0, 5), (4, 5)):
        with pytest.raises(F.AvnError) as e:
            one(w.triangle_manifolds, k1, k2, vertices1=tri9, vertices2=tri9)
        assert e.value.status == BAD_ARG
    assert one(w.triangle_manifolds, 1, 4, vertices2=tri9)["point_count"][0] == 1   # (a ball of radius 0.3 at height 0.2 over the face)
    assert one(w.triangle_manifolds, 4, 4, vertices1=tri9, vertices2=tri9)["point_count"][0] == 0   # (two triangles: no manifold)


def test_the_table_upload_refuses_bad_tables_and_keeps_the_previous_one():
    sc = scenes.trimesh_drop(n_boxes=2, n_balls=2, n_capsules=2, nx=2, nz=2)
    w = F.World(hip_lib(), F.default_config(32, substeps=4))
    w.bodies_upload(**sc.body_kwargs())
    cols = sc.collider_kwargs(native_triangles=True)
    tri = cols.pop("triangles")
    import ctypes as C
    # (the binding refuses kind 4 without a table: call the C entry point itself)
    keep = [np.ascontiguousarray(cols["entity_index"], np.uint32), np.ascontiguousarray(cols["body"], np.int32), np.ascontiguousarray(cols["shape"], np.uint8),
            np.ascontiguousarray(cols["half_extents"], np.float32)]
    s = F.avn_colliders(len(keep[0]), *[a.ctypes.data_as(C.c_void_p) for a in keep], None, None, None, None, None)
    w._check(w.lib.fn("colliders_upload")(w.handle, C.byref(s)))
    w.n_colliders = len(keep[0])
    w.existing_pairs_upload(np.zeros(0, np.uint64))
    w.pipeline_enable()
    with pytest.raises(F.AvnError) as e:   # kind-4 colliders and no table
        w.step()
    assert e.value.status == STATE and "TRIANGLE" in str(e.value)
    with pytest.raises(F.AvnError) as e:
        w.run_system("UPDATE_AABB")
    assert e.value.status == STATE
    w.collider_triangles_upload(**tri)
    w.step()
    before = w.aabbs_download()
    c = w.n_colliders
    v = np.asarray(tri["vertices"], np.float32).reshape(c, 9)

    def refused(vertices=v, edge_flags=tri["edge_flags"], count=c, struct_size=C.sizeof(F.avn_collider_triangles)):
        a, f = np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(edge_flags, np.uint8)
        t = F.avn_collider_triangles(struct_size, count, a.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p))
        return w.lib.dll.avn_collider_triangles_upload(w.handle, C.byref(t))
    nan = v.copy(); nan[1, 4] = np.nan
    flat = v.copy(); flat[2, 6:9] = flat[2, 0:3] + 2.0 * (flat[2, 3:6] - flat[2, 0:3])   # c on the line through a and b: zero area
    eight = np.asarray(tri["edge_flags"]).copy(); eight[0] = 8
    nf = sc.n_faces

    def table_still_in_force():
        """One more step; the faces sit on the static body, so their boxes are what they were under the good table."""
        w.step()
        mn, mx, _ = w.aabbs_download()
        assert np.array_equal(before[0][:nf], mn[:nf]) and np.array_equal(before[1][:nf], mx[:nf]) and ((mx - mn)[:nf].max(axis=1) > 0.9).all()
        assert np.isfinite(w.bodies_download()["position"]).all()
    for bad in (dict(vertices=nan), dict(vertices=flat), dict(edge_flags=eight),
                dict(vertices=np.concatenate([v, v[:1]]), edge_flags=np.concatenate([eight * 0 + 7, [7]]), count=c + 1),
                dict(struct_size=C.sizeof(F.avn_collider_triangles) + 8)):
        assert refused(**bad) == BAD_ARG
        table_still_in_force()   # after EACH refusal on its own
    nan_elsewhere = v.copy(); nan_elsewhere[c - 1] = np.nan   # (a collider that is no triangle: its entry is not read)
    assert refused(vertices=nan_elsewhere) == 0
    table_still_in_force()


# ---- 3. AABB -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_collider_aabbs_equal_the_reference_boxes(bits):
    """After one UPDATE_AABB the native triangles' ColliderAabb equals the box of the HIP world that holds them as host shapes answered by TriangleHost.  Body 0
    has a rotated pose off the origin, half of the colliders have speculative margin 0 (the plain box), every third a collision margin, and some faces are
    child colliders with a ColliderTransform."""
    rng = np.random.default_rng(bits)
    sc = scenes.trimesh_drop(4, 4, 4, nx=4, nz=4)
    q0 = np.array([0.2, -0.4, 0.1, 0.88]); sc.rotation[0] = q0 / np.linalg.norm(q0); sc.position[0] = [0.3, -0.2, 0.5]
    c = len(sc.col_shape)
    extra = dict(speculative_margin=np.where(np.arange(c) % 2 == 0, 0.0, -1.0), collision_margin=np.where(np.arange(c) % 3 == 0, 0.02, 0.0))
    child = (np.arange(c) % 5 == 1).astype(np.uint8)
    q = rng.normal(size=(c, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    tr = rng.uniform(-0.3, 0.3, (c, 3))
    boxes = []
    for native in (True, False):
        cols = dict(sc.collider_kwargs(native_triangles=native), **extra)
        w = F.World(hip_lib(), F.default_config(bits, substeps=4))
        w.bodies_upload(**sc.body_kwargs())
        w.colliders_upload(**cols)
        w.collider_transforms_upload(is_child=child, translation=tr, rotation=q)
        if not native:
            host = TR.TriangleHost(cols["entity_index"], sc.col_shape, sc.col_half_extents, sc.vertices, sc.edge_flags)
            w.host_shapes_set(host.aabb, host.manifolds)
        w.existing_pairs_upload(np.zeros(0, np.uint64))
        w.run_system("UPDATE_AABB")
        w.synchronize()
        assert not w.host_shape_errors()
        boxes.append(w.aabbs_download())
    (mna, mxa, _), (mnb, mxb, _) = boxes
    tris = sc.col_shape == TRI
    assert tris.sum() == 32 and (child.astype(bool) & tris).sum() >= 4
    assert np.array_equal(mna, mnb) and np.array_equal(mxa, mxb)
    assert np.isfinite(mna[tris]).all() and ((mxa - mna)[tris].max(axis=1) > 0.9).all()


# ---- 4. closed loop ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_closed_loop_equals_the_oracle_and_the_hip_world_that_host_the_faces(bits):
    """World A: HIP, native AVN_SHAPE_TRIANGLE and AVN_SHAPE_CAPSULE.  World B: the oracle, faces and capsules AVN_SHAPE_HOST answered by the references.  World C:
    HIP, the faces hosted through TriangleHost.  Bodies, new pairs, colour lists, contact rows and ColliderAabb are equal every step
    (tests/test_triangle_collider_cpu.py asserts that these steps of this scene meet every pair kind at least 20 times).  Without the feature A cannot be built."""
    a, _, _ = mesh_world(hip_lib(), bits, "native")
    b, hb, _ = mesh_world(oracle_lib(), bits, "oracle")
    c, hc, _ = mesh_world(hip_lib(), bits, "hosted")
    for step in range(STEPS):
        a.step(); b.step(); c.step()
        assert_same_closed_loop_step(a, b, step)
        assert_same_closed_loop_step(a, c, step)
    assert hb.kinds == hc.kinds and hb.manifold_queries > 1000
    assert a.host_shape_stats().host_colliders == 0


# ---- 5. rest -------------------------------------------------------------------------------------------------------------------------------
def test_the_native_mesh_scene_comes_to_rest():
    """The bounds of test_oracle_hosted_mesh_scene_covers_every_pair_kind_and_comes_to_rest, on the native world."""
    w, _, sc = mesh_world(hip_lib(), 32, "native")
    for _ in range(300):
        w.step()
    b = w.bodies_download()
    assert np.isfinite(b["position"]).all()
    low = lowest_points(sc, b)
    depth = sc.surface_height(low[:, 0], low[:, 2]) - low[:, 1]
    print("deepest lowest point under the surface:", depth.max(), " fastest body:", np.abs(b["linear_velocity"]).max())
    assert (np.abs(low[:, [0, 2]]) < 4.0).all(), "every body is still over the mesh"
    assert (depth <= 0.03).all(), "no body sank into the ground"
    assert (depth >= -0.45).all() and np.median(depth) > -0.05, "every body lies on the ground or leans on a neighbour"
    speed = np.linalg.norm(b["linear_velocity"][1:], axis=1)
    assert speed.max() < 2.0 and np.median(speed[sc.shape[1:] == CUB]) < 0.05, "nothing was thrown about; the cuboids stand still"


# ---- 6. neighbours -------------------------------------------------------------------------------------------------------------------------
def test_a_triangle_free_world_is_untouched_by_a_mesh_world_next_to_it():
    """The triangle path is selected per world: boxes stepped alone == the same boxes stepped while a mesh world steps in the same process."""
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
    mesh, _, _ = mesh_world(hip_lib(), 32, "native")
    for step in range(20):
        mesh.step(); beside.step(); mesh.step()
    x, y = alone.bodies_download(), beside.bodies_download()
    for k in x:
        assert np.array_equal(x[k], y[k]), f"bodies.{k}"
    (oa, ha), (ob, hb) = alone.pipeline_handles(), beside.pipeline_handles()
    assert np.array_equal(oa, ob) and np.array_equal(ha, hb)
    ids = np.sort(ha)
    ra, rb = alone.contacts_download(ids), beside.contacts_download(ids)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), f"contact rows.{k}"
    assert float(np.abs(mesh.bodies_download()["linear_velocity"]).max()) > 0.1


def test_spatial_queries_treat_triangle_colliders_as_host_shapes():
    """The state error names the kind; under AVN_SPATIAL_SKIP_HOST_SHAPES the queries answer what the world without the faces answers."""
    from avian_amd.spatial_query import SpatialQuery
    kw = dict(n_boxes=6, n_balls=6, n_capsules=0, nx=4, nz=4, seed=4)
    w, _, sc = mesh_world(hip_lib(), 32, "native", kw)
    nf = sc.n_faces
    bare = F.World(hip_lib(), F.default_config(32, substeps=4))   # the same bodies, the faces gone (body 0 keeps no collider)
    bare.bodies_upload(**sc.body_kwargs())
    cols = sc.collider_kwargs()
    bare.colliders_upload(**{k: v[nf:] for k, v in cols.items()})
    bare.existing_pairs_upload(np.zeros(0, np.uint64))
    sq, sqb = SpatialQuery(w), SpatialQuery(bare)
    sq.update(); sqb.update()
    rng = np.random.default_rng(9)
    o = rng.uniform([-2, 0.2, -2], [2, 3, 2], (256, 3)); d = rng.normal(size=(256, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    with pytest.raises(F.AvnError) as e:
        sq.cast_rays(o, d)
    assert e.value.status == STATE and "AVN_SHAPE_TRIANGLE" in str(e.value)
    got, want = sq.cast_rays(o, d, skip_host_shapes=True), sqb.cast_rays(o, d)
    hit = got["collider"] != 0xFFFFFFFF
    assert hit.sum() > 10 and (got["collider"][hit] >= nf).all(), "triangle colliders are never candidates"
    assert np.array_equal(got["entity"], want["entity"]) and np.array_equal(got["distance"], want["distance"]) and np.array_equal(got["normal"], want["normal"])
    assert sq.stats().host_skipped == nf == 32


def test_swept_ccd_tests_no_triangle_pair():
    """A declared deviation: swept CCD skips a pair with a triangle on either side, as it skips host shapes."""
    from avian_amd.swept_ccd import SweptCcd
    sc = scenes.trimesh_drop(n_boxes=0, n_balls=1, n_capsules=0, nx=2, nz=2, drop_height=0.3)
    sc.linear_velocity[1] = [0.0, -30.0, 0.0]
    w, _, _ = mesh_world(hip_lib(), 32, "native", sc=sc)
    ccd = SweptCcd(w)
    ccd.upload([1])
    pairs = 0
    for _ in range(4):
        w.step()
        r = ccd.results()
        assert len(r) == 1 and r["tested"][0] == 0 and r["hit_collider"][0] == 0xFFFFFFFF
        pairs += len(w.pairs_get())
    assert pairs > 0, "the ball's box did meet faces: there were triangle pairs the pass could have tested"


# ---- 7. hooks ------------------------------------------------------------------------------------------------------------------------------
def test_hooks_see_triangle_pairs_like_any_other_pair():
    """The modify_contacts conveyor of tests/test_gpu_collision_hooks.py on a mesh scene: HIP native == the oracle hosted, bit for bit, and the records shown to
    the hook are equal."""
    sc = scenes.trimesh_drop(2, 2, 2, nx=2, nz=2)
    c = len(sc.col_shape)
    flagged = np.random.default_rng(2).random(c) < 0.5
    flagged[: sc.n_faces: 2] = True   # (every other face: resting contacts on the mesh go through the hook)
    hd, ho = Hooks(), Hooks()
    dev = hooked_world(hip_lib(), 32, sc.body_kwargs(), sc.collider_kwargs(native_triangles=True), flagged, hd, friction=sc.friction)
    cols = sc.collider_kwargs(host_capsules=True)
    ref = hooked_world(oracle_lib(), 32, sc.body_kwargs(), cols, flagged, ho, friction=sc.friction)
    host = TR.MeshHost(cols["entity_index"], sc.col_shape, sc.col_half_extents, sc.vertices, sc.edge_flags)
    ref.host_shapes_set(host.aabb, host.manifolds)
    dev.pipeline_enable(); ref.pipeline_enable()
    for step in range(30):
        dev.step(); ref.step()
        assert_same_hooked_step(dev, ref, step)
    assert hd.filter_log == ho.filter_log and hd.modify_log == ho.modify_log
    dt = F.hook_contact_dtype(32)
    faces = sum(int(np.frombuffer(raw, dt)[0]["collider1"]) < sc.n_faces or int(np.frombuffer(raw, dt)[0]["collider2"]) < sc.n_faces for raw in hd.modify_log)
    assert faces > 0 and len(hd.modify_log) > 0, "pairs with a triangle collider must have reached the hook"


# ---- 8. sleeping ---------------------------------------------------------------------------------------------------------------------------
def test_sleeping_on_the_mesh_and_a_wake_equal_the_hosted_oracle():
    a, _, _ = mesh_world(hip_lib(), 32, "native", sleeping=True)
    b, _, _ = mesh_world(oracle_lib(), 32, "oracle", sleeping=True)
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
    assert slept > 0 and woke, "bodies must have fallen asleep on the mesh and one must have been woken"
    assert not b.host_shape_errors()
    x, y = a.bodies_download(), b.bodies_download()
    for k in x:
        assert np.array_equal(x[k], y[k]), f"bodies.{k}"
    sa, sb = a.sleeping_state(), b.sleeping_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), f"sleeping state.{k}"
