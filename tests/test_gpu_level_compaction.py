"""GPU: level compaction of host-uploaded manifolds (world/manifolds.hpp, k_levels.hip).  avn_manifolds_upload regroups colours 0..22 into the
levels of the per-body order the colouring fixes, so the solver launches once per LEVEL.  Every body still sees its manifolds in the same sequence, so every
result must equal, bit for bit,
  * the CPU oracle, which solves colour by colour, and
  * the `make measure` build with AVN_NO_LEVEL_COMPACTION set (colour launches, as before the change),
with rows of impulses_download / constraints_download in UPLOAD order.  Which path ran is read from avn_level_compaction_stats; the level sizes it reports are
checked against numpy_levels below, a restatement of the rule that shares nothing with the library.  The rank pass works on tiles of 256 manifolds."""
import functools
import os

import numpy as np
import pytest

from helpers import F, assert_same, hip_lib, hip_measure_lib, oracle_lib, random_world   # (first: puts the repository on sys.path)
import level2_helpers as L2
from avian_amd import scenes

pytestmark = pytest.mark.gpu

OVF = F.COLOR_OVERFLOW_INDEX   # 23
TILE = 256


def numpy_levels(offs, body1, body2, has_sb):
    """level(m) = max over m's ordering bodies of next[body]; next[body] = level(m) + 1; colours 0..22 in order.  A body orders unless some colour 0..22
    holds two of its manifolds.  Returns (level per manifold of colours 0..22, level sizes [23], populated colours, ordering mask)."""
    offs = np.asarray(offs, np.int64)
    n, nb = int(offs[OVF]), len(has_sb)
    colour = np.searchsorted(offs[1:OVF + 1], np.arange(n), side="right")
    seen = np.zeros((nb, OVF), np.int64)
    b1n, b2n = np.asarray(body1[:n], np.int64), np.asarray(body2[:n], np.int64)
    np.add.at(seen, (b1n, colour), 1)
    np.add.at(seen, (b2n[b2n != b1n], colour[b2n != b1n]), 1)   # (a manifold of a body with itself names it once, as in k_level_masks)
    orders = ~(seen > 1).any(axis=1)   # (from the lists alone: body state, has_sb included, plays no part)
    nxt = np.zeros(nb, np.int64)
    level = np.zeros(n, np.int64)
    for c in range(OVF):
        a, b = np.asarray(body1[offs[c]:offs[c + 1]], np.int64), np.asarray(body2[offs[c]:offs[c + 1]], np.int64)
        lv = np.maximum(np.where(orders[a], nxt[a], 0), np.where(orders[b], nxt[b], 0))
        level[offs[c]:offs[c + 1]] = lv
        nxt[a[orders[a]]] = lv[orders[a]] + 1
        nxt[b[orders[b]]] = lv[orders[b]] + 1
    return level, np.bincount(level, minlength=OVF)[:OVF], int((np.diff(offs[:OVF + 1]) > 0).sum()), orders


def has_solver_body(bodies):
    n = len(bodies["rb_type"])
    fl = np.asarray(bodies.get("body_flags", np.zeros(n, np.uint8)))
    return (np.asarray(bodies["rb_type"]) != F.RB_STATIC) & ((fl & (F.BODY_SLEEPING | F.BODY_DISABLED)) == 0)


def world(lib, bits, bodies, use_graph=1, substeps=2, switched_off=False):
    """switched_off: on the measure build, with AVN_NO_LEVEL_COMPACTION read when the world is created"""
    if switched_off:
        os.environ["AVN_NO_LEVEL_COMPACTION"] = "1"
    try:
        w = F.World(lib, F.default_config(bits, substeps=substeps, use_graph=use_graph))
    finally:
        os.environ.pop("AVN_NO_LEVEL_COMPACTION", None)
    w.bodies_upload(**bodies)
    return w


def upload(w, case):
    scenes.upload_manifolds(w, case["mf"], case["offs"], case["friction"], case["restitution"], case.get("warm_n"), case.get("warm_t"))


def state(w):
    w.synchronize()
    return {"bodies": w.bodies_download(), "impulses": w.impulses_download(), "constraints": w.constraints_download()}


def same(a, b, what):
    for part in a:
        for k in a[part]:
            assert_same(a[part][k], b[part][k], f"{what}: {part}.{k}")


def run(lib, bits, case, steps, use_graph=1, switched_off=False):
    w = world(lib, bits, case["bodies"], use_graph, switched_off=switched_off)
    upload(w, case)
    for _ in range(steps):
        w.step()
    return w, state(w)


def sizes(st):
    return np.array(list(st.sizes), np.int64)


def check_readout(w, case, compacted=True):
    """the read-out against the numpy rule; returns it"""
    st = w.level_compaction_stats()
    mf, offs = case["mf"], np.asarray(case["offs"], np.int64)
    level, want, populated, _ = numpy_levels(offs, mf["body1"], mf["body2"], has_solver_body(case["bodies"]))
    print("level compaction read-out: state", st.state, "colours", st.colours, "levels", st.levels, "max degree", st.max_degree, "moved", st.moved, "sizes", sizes(st)[:st.levels + 1],
          "numpy", want[:int((want > 0).sum()) + 1])
    assert st.colours == populated
    assert int(sizes(st).sum()) == int(offs[OVF]), "the overflow range must start where it was uploaded"
    assert (st.overflow_first, st.overflow_count) == (int(offs[OVF]), int(offs[OVF + 1] - offs[OVF])), "the overflow range's offsets, after the upload as before it"
    if compacted:
        assert st.state == F.LEVELS_COMPACTED and st.why_off == F.LEVELS_WHY_NONE
        assert np.array_equal(sizes(st), want) and st.levels == int((want > 0).sum())
        assert st.max_degree <= st.levels < st.colours
    return st


# ---- 1. box_stack_1k, frozen: 15 colours become 14 levels ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box_stack_1k():
    sc = scenes.box_stack(10, 10, 10)
    o = F.World(oracle_lib(), F.default_config(32, substeps=4))   # the pair list in the broad phase's emission order (the oracle's: no device needed)
    o.bodies_upload(**sc.body_kwargs()); o.colliders_upload(**sc.collider_kwargs()); o.existing_pairs_upload(np.zeros(0, np.uint64))
    o.run_system("UPDATE_AABB"); o.run_system("COLLECT_COLLISION_PAIRS")
    pairs = o.pairs_get()
    rng = np.random.default_rng(5)
    sc.linear_velocity[1:] += rng.normal(scale=0.3, size=(sc.n - 1, 3))   # not a resting lattice: impulses differ everywhere
    sc.angular_velocity[1:] += rng.normal(scale=0.2, size=(sc.n - 1, 3))
    mf = scenes.axis_aligned_manifolds(sc, np.stack([pairs["body1"], pairs["body2"]], axis=1))
    offs, perm = scenes.color_manifolds(oracle_lib(), mf, sc.rb_type)
    return dict(bodies=sc.body_kwargs(), mf=scenes.permute_manifolds(mf, perm), offs=offs, friction=sc.friction, restitution=sc.restitution)


@functools.lru_cache(maxsize=None)
def box_stack_1k_references(bits):
    case = box_stack_1k()
    return run(oracle_lib(), bits, case, 3)[1], run(hip_measure_lib(), bits, case, 3, switched_off=True)


@pytest.mark.parametrize("use_graph", [0, 1], ids=["eager", "replayed"])
@pytest.mark.parametrize("bits", [32, 64])
def test_box_stack_1k(bits, use_graph):
    case = box_stack_1k()
    assert len(case["mf"]["body1"]) == 6040
    w, got = run(hip_lib(), bits, case, 3, use_graph)
    st = check_readout(w, case)
    assert (st.colours, st.levels) == (15, 14) and st.moved == 1
    f = w.solver_forms()
    assert f.island_blocks == 0, "one island of a thousand bodies: the device-wide path"
    assert [x for x in f.colour_form if x] == [F.COLOUR_FORM_OCT if bits == 32 else F.COLOUR_FORM_LANE] * 14, "one launch per level: oct in f32 (every level is small), lane in f64"
    ms, launches = w.profile_system("SOLVE_CONTACTS_BIAS", 1)
    print("SOLVE_CONTACTS_BIAS launches:", launches)
    assert launches == 14
    oracle, (w_off, off) = box_stack_1k_references(bits)
    so = w_off.level_compaction_stats()
    assert so.state == F.LEVELS_OFF and so.why_off == F.LEVELS_WHY_SWITCH and so.levels == 15
    assert w_off.profile_system("SOLVE_CONTACTS_BIAS", 1)[1] == 15
    same(got, oracle, f"box_stack_1k f{bits} vs the oracle")
    same(got, off, f"box_stack_1k f{bits} vs colour launches")


# ---- hand-made sets: bodies from random_world, manifolds between chosen bodies in chosen colours -----------------------------------------------------------------------
def make_case(seed, n_bodies, colours, n_static=1, n_kinematic=0, overflow=(), point_counts=None, odd=False):
    """colours: {colour: [(body1, body2), ...]} (colour-major upload order = dict order by colour); overflow: pairs of the overflow list"""
    wd = random_world(seed, n_bodies=n_bodies, n_manifolds=1, n_static=n_static, n_kinematic=n_kinematic, with_odd_features=odd)
    rng = np.random.default_rng(seed + 1000)
    offs = np.zeros(F.GRAPH_COLOR_COUNT + 1, np.uint32)
    pairs = []
    for c in range(OVF):
        pairs += list(colours.get(c, []))
        offs[c + 1] = len(pairs)
    pairs += list(overflow)
    offs[OVF + 1] = len(pairs)
    m = len(pairs)
    p = np.array(pairs, np.int32).reshape(m, 2)
    normal = rng.normal(size=(m, 3)); normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-9)
    mf = dict(body1=p[:, 0].copy(), body2=p[:, 1].copy(), normal=normal,
              point_count=(np.arange(m) % 5 if point_counts == "cycle" else rng.integers(1, 5, m)).astype(np.uint8),
              anchor1=rng.normal(scale=0.7, size=(m, 4, 3)), anchor2=rng.normal(scale=0.7, size=(m, 4, 3)),
              penetration=rng.normal(scale=0.05, size=(m, 4)), normal_speed=rng.normal(scale=2.0, size=(m, 4)))
    return dict(bodies=wd["bodies"], mf=mf, offs=offs, friction=rng.uniform(0.05, 1.2, m), restitution=np.where(rng.random(m) < 0.5, 0.0, rng.uniform(0.1, 0.9, m)),
                warm_n=np.abs(rng.normal(scale=0.3, size=(m, 4))), warm_t=rng.normal(scale=0.1, size=(m, 4, 2)))


def judge(case, bits=32, steps=2, compacted=True, use_graph=1):
    w, got = run(hip_lib(), bits, case, steps, use_graph)
    st = check_readout(w, case, compacted)
    if bits == 32 and len(case["mf"]["body1"]):   # (f32, no joints, small islands: these sets never reach the level LAUNCHES -- tests/test_gpu_solver_forms.py runs them there)
        assert w.solver_forms().island_blocks > 0 and not any(w.solver_forms().colour_form), "the hand-made f32 sets solve through the island blocks"
    same(got, run(oracle_lib(), bits, case, steps)[1], "vs the oracle")
    same(got, run(hip_measure_lib(), bits, case, steps, switched_off=True)[1], "vs colour launches (rows in upload order)")
    return w, st


# ---- 2. a wastefully coloured set --------------------------------------------------------------------------------------------------------------------------------------
def columns_case():
    """body 0: the static ground; column A = bodies 1..64, column B = 65..128, a lone box 129; colours 0, 5 | 11 (ground) | 17, 22: valid, and sparse"""
    a, b = np.arange(1, 65), np.arange(65, 129)
    colours = {0: [(a[k], a[k + 1]) for k in range(0, 63, 2)], 5: [(a[k], a[k + 1]) for k in range(1, 63, 2)],
               11: [(0, a[0]), (b[0], 0), (0, 129)],
               17: [(b[k], b[k + 1]) for k in range(0, 63, 2)], 22: [(b[k], b[k + 1]) for k in range(1, 63, 2)]}
    return make_case(21, 130, colours)


@pytest.mark.parametrize("bits", [32, 64])
def test_sparse_colours_collapse(bits):
    case = columns_case()
    w, st = judge(case, bits)
    assert st.colours == 5 and 2 <= st.levels <= 3 and st.moved == 1
    level, _, _, orders = numpy_levels(case["offs"], case["mf"]["body1"], case["mf"]["body2"], has_solver_body(case["bodies"]))
    ground = np.flatnonzero((case["mf"]["body1"] == 0) | (case["mf"]["body2"] == 0))
    assert not orders[0] and len(ground) == 3 and len(set(level[ground])) < 3, "manifolds of the ground share a level"


# ---- 3. mixed content ----------------------------------------------------------------------------------------------------------------------------------------------------
def mixed_case():
    wd = random_world(7, n_bodies=160, n_manifolds=420, n_static=3, n_kinematic=3, hub_degree=30, with_odd_features=True)
    mf = dict(wd["manifolds"])
    m = len(mf["body1"])
    mf["point_count"] = (np.arange(m) % 5).astype(np.uint8)   # 0..4
    rb = np.asarray(wd["bodies"]["rb_type"])
    offs, perm = scenes.color_manifolds(oracle_lib(), mf, rb)
    return dict(bodies=wd["bodies"], mf=scenes.permute_manifolds(mf, perm), offs=offs, friction=wd["friction"][perm], restitution=wd["restitution"][perm],
                warm_n=wd["warm_n"][perm], warm_t=wd["warm_t"][perm])


def test_mixed_content():
    case = mixed_case()
    mf, offs, bodies = case["mf"], np.asarray(case["offs"], np.int64), case["bodies"]
    sb = has_solver_body(bodies)
    level, _, _, orders = numpy_levels(offs, mf["body1"], mf["body2"], sb)
    n = int(offs[OVF])
    colour = np.searchsorted(offs[1:OVF + 1], np.arange(n), side="right")
    # what the set must contain for this test to mean anything
    assert offs[OVF + 1] > offs[OVF], "a populated overflow list"
    coloured_bodies = set(mf["body1"][:n]) | set(mf["body2"][:n])
    assert coloured_bodies & (set(mf["body1"][n:]) | set(mf["body2"][n:])), "overflow bodies also appear in colours"
    twice = [b for b in np.flatnonzero(~sb) if max(np.bincount(colour[(mf["body1"][:n] == b) | (mf["body2"][:n] == b)], minlength=1)) >= 2]
    assert twice, "a body without a SolverBody named by two manifolds of one colour"
    kin = np.flatnonzero((np.asarray(bodies["rb_type"]) == F.RB_KINEMATIC) & sb)
    assert any(orders[k] and ((mf["body1"][:n] == k) | (mf["body2"][:n] == k)).sum() >= 2 for k in kin), "a kinematic body that orders"
    assert set(np.unique(mf["point_count"])) == {0, 1, 2, 3, 4}
    judge(case, 32)
    judge(case, 64, use_graph=0)


# ---- 4. sizes around the rank pass's tile; M = 0, M = 1; the early out ------------------------------------------------------------------------------------------------------
def tile_case(n0, n1, j, n2):
    """colour 0: n0 manifolds on body pairs of their own; colour 3: n1, the first j on colour 0's pairs (level 1), the others on fresh pairs (level 0);
    colour 7: n2 on fresh pairs (level 0).  Three colours, at most two on one body: two levels of n0 + n1 - j + n2 and j manifolds."""
    pair = lambda i: (1 + 2 * i, 2 + 2 * i)
    colours = {0: [pair(i) for i in range(n0)], 3: [pair(i) for i in range(j)] + [pair(n0 + i) for i in range(n1 - j)], 7: [pair(n0 + n1 + i) for i in range(n2)]}
    return make_case(31, 1 + 2 * (n0 + n1 + n2), colours)


@pytest.mark.parametrize("n0,n1,j,n2", [(300, 300, 1, 40), (300, 300, TILE - 1, 40), (300, 300, TILE, 40), (300, 300, TILE + 1, 40),
                                        (100, 100, 1, TILE - 200), (100, 100, 1, TILE + 1 - 200), (100, 100, 1, TILE + 2 - 200), (1, 2, 1, 1)])
def test_level_populations_at_tile_edges(n0, n1, j, n2):
    case = tile_case(n0, n1, j, n2)
    w, st = judge(case, 32, steps=1)
    assert list(sizes(st)[:3]) == [n0 + n1 - j + n2, j, 0] and st.max_degree == 2 and st.colours == 3


def test_early_out_and_tiny_sets():
    # two colours and a body in both: as many launches as the deepest body needs -- left as uploaded
    pair = lambda i: (1 + 2 * i, 2 + 2 * i)
    case = make_case(41, 1200, {2: [pair(i) for i in range(300)], 9: [pair(i) for i in range(5)] + [pair(300 + i) for i in range(295)]})
    w, st = judge(case, 32, steps=1, compacted=False)
    assert st.state == F.LEVELS_EARLY_OUT and st.max_degree == st.colours == st.levels == 2 and st.moved == 0
    assert np.array_equal(sizes(st), np.diff(np.asarray(case["offs"], np.int64))[:OVF]), "offsets as uploaded"
    one = make_case(42, 5, {4: [(1, 2)]})
    w, st = judge(one, 32, steps=1, compacted=False)
    assert st.state == F.LEVELS_EARLY_OUT and st.colours == st.levels == 1
    none = make_case(43, 5, {})
    w, st = judge(none, 32, steps=1, compacted=False)
    assert st.state == F.LEVELS_OFF and st.why_off == F.LEVELS_WHY_EMPTY and st.levels == 0


# ---- 5. re-upload sequences against fresh worlds -------------------------------------------------------------------------------------------------------------------------
def sequence(lib, bits, script, switched_off=False):
    """script: a list of cases (all over the same bodies).  Every case is uploaded -- behind a fresh bodies_upload, so that a fresh world is comparable -- and stepped."""
    w = world(lib, bits, script[0]["bodies"], switched_off=switched_off)
    out = []
    for k, case in enumerate(script):
        if k:
            w.bodies_upload(**case["bodies"])
        upload(w, case)
        w.step()
        out.append((state(w), w.level_compaction_stats().state if lib is not oracle_lib() else None))
    return out


@pytest.mark.parametrize("bits", [32, 64])
def test_reupload_sequences(bits):
    a = columns_case()
    pair = lambda i: (1 + 2 * i, 2 + 2 * i)
    b = make_case(51, 130, {1: [pair(i) for i in range(40)], 6: [pair(i) for i in range(10)] + [pair(40 + i) for i in range(20)], 20: [(0, 129), (0, 128)]}, overflow=[(1, 3), (3, 5)])
    early = make_case(52, 130, {2: [pair(i) for i in range(30)], 9: [pair(i) for i in range(30)]})
    for c in (b, early):
        c["bodies"] = a["bodies"]
    for script, states in (([a, b], [F.LEVELS_COMPACTED, F.LEVELS_COMPACTED]), ([a, early, a], [F.LEVELS_COMPACTED, F.LEVELS_EARLY_OUT, F.LEVELS_COMPACTED])):
        got = sequence(hip_lib(), bits, script)
        assert [s for _, s in got] == states
        off = sequence(hip_measure_lib(), bits, script, switched_off=True)
        ora = sequence(oracle_lib(), bits, script)
        for k, case in enumerate(script):
            same(got[k][0], run(hip_lib(), bits, case, 1)[1], f"upload {k}: the sequence left stale state (vs a fresh world)")
            same(got[k][0], off[k][0], f"upload {k} vs colour launches")
            same(got[k][0], ora[k][0], f"upload {k} vs the oracle")
    # bodies_upload between manifolds_upload and the step: the levels come from the lists alone
    w = world(hip_lib(), bits, a["bodies"])
    upload(w, a)
    w.bodies_upload(**a["bodies"])
    w.step()
    assert w.level_compaction_stats().state == F.LEVELS_COMPACTED
    same(state(w), run(hip_lib(), bits, a, 1)[1], "bodies_upload behind manifolds_upload")


# ---- 6. no silent disabling: the closed loop and level-2 worlds report it off and compute what colour launches compute ---------------------------------------------------------
def test_closed_loop_reports_off():
    sc = scenes.box_stack(4, 4, 4)
    out = []
    for lib in (hip_lib(), oracle_lib()):
        w = F.World(lib, F.default_config(32, substeps=4))
        w.bodies_upload(**sc.body_kwargs()); w.colliders_upload(**sc.collider_kwargs())
        w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
        w.pipeline_enable()
        for _ in range(3):
            w.step()
        w.synchronize()
        out.append((w, w.bodies_download()))
    st = out[0][0].level_compaction_stats()
    assert st.state == F.LEVELS_OFF and st.why_off == F.LEVELS_WHY_CLOSED_LOOP and st.moved == 0
    for k in out[0][1]:
        assert_same(out[0][1][k], out[1][1][k], f"closed loop bodies.{k}")


@pytest.mark.parametrize("world_size,bits", [(1, 32), (2, 32), (2, 64)])
def test_level2_worlds_stay_in_colour_order(world_size, bits):
    """the upload compacts, the halo plan that follows puts the set back into colour order: ranks exchange colour by colour"""
    lib = hip_lib()
    sc, pm, offs, restitution = L2.global_problem(lib, 6, 5, 6)
    single = L2.make_single(lib, bits, sc, pm, offs, restitution, 2)
    assert single.level_compaction_stats().state == F.LEVELS_COMPACTED
    plan, worlds = L2.make_split(lib, bits, sc, pm, offs, restitution, 2, world_size)
    for w in worlds:
        st = w.level_compaction_stats()
        assert st.state == F.LEVELS_OFF and st.why_off == F.LEVELS_WHY_LEVEL2
    os.environ["AVN_NO_LEVEL_COMPACTION"] = "1"
    try:
        off = L2.make_single(hip_measure_lib(), bits, sc, pm, offs, restitution, 2)
    finally:
        os.environ.pop("AVN_NO_LEVEL_COMPACTION", None)
    for _ in range(2):
        single.step(); off.step()
        L2.step_split_in_process(plan, worlds, 2, restitution)
    L2.compare_with_single(single, plan, worlds)
    L2.compare_with_single(off, plan, worlds)


@pytest.mark.parametrize("bits", [32, 64])
def test_put_back_after_steps(bits):
    """a world that becomes a level-2 rank AFTER it has stepped: every manifold-indexed array goes back to upload order, warm-start impulses included"""
    case = columns_case()
    ws = [world(hip_lib(), bits, case["bodies"]), world(hip_measure_lib(), bits, case["bodies"], switched_off=True)]
    for w in ws:
        upload(w, case)
        w.step()
        w.halo_plan_upload([], [], [], [], [])
        st = w.level_compaction_stats()
        assert st.state == F.LEVELS_OFF and st.levels == st.colours == 5
    same(state(ws[0]), state(ws[1]), "right after the put-back")
    for w in ws:
        w.step(); w.step()
    same(state(ws[0]), state(ws[1]), "two steps after the put-back")
    upload(ws[0], case)
    assert ws[0].level_compaction_stats().why_off == F.LEVELS_WHY_LEVEL2, "a level-2 world is not compacted again"
