"""GPU: the impulses have one home, and c_pa is written once per upload.

avn_step on host-uploaded manifolds leaves the step's impulses in the constraint rows (c_pd) and does not copy them into the manifolds' warm-start records (mp_w); the
next step's k_prepare_contact_constraints reads them there, and whoever else wants them -- a download, an upload, the level permutation, a single system, the closed
loop -- gets k_store_contact_impulses first (World::materialize_impulses).  Bit 31 of m_meta says that a manifold's c_pa rows are current, and a lane that finds it
set does not write them again.

Every script below runs on three worlds: the CPU oracle, the device world under test, and a TWIN device world that calls impulses_download after every step and so
stores after every step, as the library did before.  After a script the bodies, impulses_download and constraints_download of the three are equal bit for bit; inside a
script only constraints_download is compared (it reads c_pa .. c_pd as they are and materialises nothing).  No tolerance appears anywhere.

Sets: box_stack(3, 3, 3) and (4, 4, 4) with their lattice manifolds -- f64 takes the colour launches, f32 the island blocks -- and the smallest set of
tests/test_gpu_solver_forms.py in the lane form of the f32 colour launches; the form each world ran in is asserted through avn_solver_forms_get.  Every set has point
counts cycling 0..4 (unused slots behind the count), manifolds with friction 0 (no tangent bit) and warm-start impulses in every slot."""
import functools

import numpy as np
import pytest

import solver_forms_helpers as H
from avian_amd import scenes
from helpers import F, hip_lib, hip_measure_lib, oracle_lib
from test_gpu_level_compaction import columns_case, same, state
from test_gpu_solver_forms import oct_case

pytestmark = pytest.mark.gpu

LANE_ENV = {"AVN_ISLAND_BLOCKS": 0, "AVN_NO_LEVEL_COMPACTION": 1, "AVN_NO_OCT": 1}
SUBSTEPS = 2


# ---- sets -------------------------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_case(n):
    """box_stack(n, n, n), the pairs in the broad phase's emission order (the oracle's), face manifolds between neighbours; then point counts 0..4 in turn, friction 0 on
    every third manifold and a warm-start impulse in every slot, used or not"""
    sc = scenes.box_stack(n, n, n)
    o = F.World(oracle_lib(), F.default_config(32, substeps=SUBSTEPS))
    o.bodies_upload(**sc.body_kwargs()); o.colliders_upload(**sc.collider_kwargs()); o.existing_pairs_upload(np.zeros(0, np.uint64))
    o.run_system("UPDATE_AABB"); o.run_system("COLLECT_COLLISION_PAIRS")
    pairs = o.pairs_get()
    o.close()
    rng = np.random.default_rng(40 + n)
    sc.linear_velocity[1:] += rng.normal(scale=0.3, size=(sc.n - 1, 3))
    sc.angular_velocity[1:] += rng.normal(scale=0.2, size=(sc.n - 1, 3))
    mf = scenes.axis_aligned_manifolds(sc, np.stack([pairs["body1"], pairs["body2"]], axis=1))
    offs, perm = scenes.color_manifolds(oracle_lib(), mf, sc.rb_type)
    mf = scenes.permute_manifolds(mf, perm)
    m = len(mf["body1"])
    mf["point_count"] = (np.arange(m) % 5).astype(np.uint8)
    friction = np.where(np.arange(m) % 3 == 1, 0.0, rng.uniform(0.2, 0.9, m))
    case = dict(bodies=sc.body_kwargs(), colliders=sc.collider_kwargs(), mf=mf, offs=offs, friction=friction, restitution=np.zeros(m),
                warm_n=np.abs(rng.normal(scale=0.3, size=(m, 4))), warm_t=rng.normal(scale=0.1, size=(m, 4, 2)))
    assert set(mf["point_count"]) == {0, 1, 2, 3, 4} and (friction == 0).any() and (friction > 0).any()
    return case


@functools.lru_cache(maxsize=None)
def lane_case():
    case = dict(oct_case(1))
    fr = np.array(case["friction"], copy=True); fr[1::3] = 0.0
    case["friction"] = fr
    assert set(case["mf"]["point_count"]) == {0, 1, 2, 3, 4}
    return case


# (name, set, scalar bits, library of the device worlds, switches, the form the device worlds must report)
CASES = {
    "lattice3_f64_colours": (lambda: lattice_case(3), 64, hip_lib, None, "colours"),
    "lattice3_f32_islands": (lambda: lattice_case(3), 32, hip_lib, None, "islands"),
    "lattice4_f64_colours": (lambda: lattice_case(4), 64, hip_lib, None, "colours"),
    "lattice4_f32_islands": (lambda: lattice_case(4), 32, hip_lib, None, "islands"),
    "lane_f32": (lane_case, 32, hip_measure_lib, LANE_ENV, "lane"),
}


def assert_form(w, form, what):
    f = w.solver_forms()
    launched = [x for x in f.colour_form if x != F.FORM_NONE]
    if form == "islands":
        assert f.island_blocks > 0 and not launched, f"{what}: expected the island blocks, got colour forms {launched}"
    elif form == "colours":
        assert f.island_blocks == 0 and launched, f"{what}: expected colour launches"
    else:
        assert f.island_blocks == 0 and launched and set(launched) == {F.COLOUR_FORM_LANE}, f"{what}: expected lane-form colour launches, got {launched}"


def other_values(case, seed):
    """the same pairs in the same colours with other anchors, penetrations, speeds and warm-start impulses"""
    rng = np.random.default_rng(seed)
    out = dict(case)
    mf = dict(case["mf"])
    m = len(mf["body1"])
    mf["anchor1"] = mf["anchor1"] + rng.normal(scale=0.05, size=(m, 4, 3))
    mf["anchor2"] = mf["anchor2"] + rng.normal(scale=0.05, size=(m, 4, 3))
    mf["penetration"] = mf["penetration"] + rng.normal(scale=0.02, size=(m, 4))
    mf["point_count"] = ((np.arange(m) + 2) % 5).astype(np.uint8)
    out["mf"] = mf
    out["warm_n"] = np.abs(rng.normal(scale=0.2, size=(m, 4)))
    out["warm_t"] = rng.normal(scale=0.07, size=(m, 4, 2))
    return out


def with_flags(w, case, disabled):
    """the world's bodies as they are now with the set's own flags, the bodies `disabled` flagged RigidBodyDisabled in addition"""
    kw = dict(case["bodies"]); kw.update(w.bodies_download())
    n = len(np.asarray(kw["inv_mass"]).reshape(-1))
    fl = np.array(kw["body_flags"], np.uint8, copy=True) if kw.get("body_flags") is not None else np.zeros(n, np.uint8)
    fl[disabled] |= F.BODY_DISABLED
    kw["body_flags"] = fl
    return kw


def some_manifold_bodies(case):
    """a few dynamic bodies that manifolds with used points name on either side"""
    mf = case["mf"]
    rb = np.asarray(case["bodies"]["rb_type"])
    used = mf["point_count"] > 0
    named = np.concatenate([mf["body1"][used], mf["body2"][used]])
    named = np.unique(named[rb[named] == F.RB_DYNAMIC])
    assert len(named) >= 3
    return named[::max(1, len(named) // 3)][:3]


# ---- scripts: lists of ("step", k) | ("do", fn(world, case)[, "closed loop"]) | ("constraints",) | ("bodies",) | ("state",) ------------------------------------------------------------------------------
def upload(w, case):
    scenes.upload_manifolds(w, case["mf"], case["offs"], case["friction"], case["restitution"], case["warm_n"], case["warm_t"])


def script_steps_then_download(case):
    return [("step", 1), ("constraints",), ("step", 2), ("constraints",), ("state",)]


def script_download_in_the_middle(case):
    return [("step", 2), ("state",), ("step", 2), ("state",)]


def script_bodies_inactive_then_active(case):
    off = some_manifold_bodies(case)
    return [("step", 2),
            ("do", lambda w, c: w.bodies_upload(**with_flags(w, c, off))), ("step", 1), ("constraints",),   # constraint -> skipped: the slots are flushed into mp_w
            ("do", lambda w, c: w.bodies_upload(**with_flags(w, c, []))), ("step", 1), ("constraints",),    # skipped -> generating: warm start from mp_w
            ("step", 1), ("state",)]


def script_skipped_at_the_first_step(case):
    off = some_manifold_bodies(case)
    return [("do", lambda w, c: w.bodies_upload(**with_flags(w, c, off))), ("step", 1), ("constraints",),   # these manifolds write no c_pa at step 1 ...
            ("do", lambda w, c: w.bodies_upload(**with_flags(w, c, []))), ("step", 1), ("constraints",),    # ... and write it at step 2
            ("step", 1), ("state",)]


def script_upload_again(case):
    second = other_values(case, 7)
    return [("step", 2), ("do", lambda w, c: upload(w, second)), ("step", 1), ("constraints",), ("step", 2), ("state",),
            ("do", lambda w, c: upload(w, c)), ("step", 1), ("state",)]


def script_put_back(case):
    return [("step", 2), ("do", lambda w, c: w.halo_plan_upload([], [], [], [], [])), ("constraints",), ("step", 2), ("constraints",), ("state",)]


def script_single_systems(case):
    def systems(w, c):
        for s in ("PREPARE_CONTACT_CONSTRAINTS", "WARM_START", "SOLVE_CONTACTS_BIAS", "SOLVE_CONTACTS_RELAX", "STORE_CONTACT_IMPULSES"):
            w.run_system(s)
    return [("step", 2), ("do", lambda w, c: w.profile_system("SOLVE_CONTACTS_BIAS", 2)), ("step", 2), ("do", systems), ("step", 2), ("state",)]


def script_pipeline_enable(case):
    def enable(w, c):
        w.colliders_upload(**c["colliders"]); w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
        w.pipeline_enable()
    return [("step", 2), ("do", enable, "closed loop"), ("step", 2), ("bodies",)]


SCRIPTS = {
    "steps_then_one_download": script_steps_then_download,
    "download_in_the_middle": script_download_in_the_middle,
    "bodies_inactive_then_active": script_bodies_inactive_then_active,
    "skipped_at_the_first_step": script_skipped_at_the_first_step,
    "upload_again_with_other_values": script_upload_again,
    "put_back_into_upload_order": script_put_back,
    "single_systems_between_steps": script_single_systems,
    "pipeline_enable": script_pipeline_enable,
}


def new_world(lib, bits, case, use_graph, env=None, match_contacts=1):
    with H.switches(**(env or {})):
        w = F.World(lib, F.default_config(bits, substeps=SUBSTEPS, use_graph=use_graph, match_contacts=match_contacts))
    w.bodies_upload(**case["bodies"])
    upload(w, case)
    return w


def run_three(case, bits, lib, env, form, script, use_graph, match_contacts, what):
    worlds = {"oracle": new_world(oracle_lib(), bits, case, 0, None, match_contacts),
              "lazy": new_world(lib(), bits, case, use_graph, env, match_contacts),
              "twin": new_world(lib(), bits, case, use_graph, env, match_contacts)}
    array_mode = True
    n = 0
    for op in script:
        if op[0] == "step":
            for _ in range(op[1]):
                for name, w in worlds.items():
                    w.step()
                    if name == "twin" and array_mode:
                        w.impulses_download()   # the twin's impulses are in mp_w after every step
                n += 1
            if array_mode:
                for name in ("lazy", "twin"):
                    assert_form(worlds[name], form, f"{what}, {name}, step {n}")
        elif op[0] == "do":
            for w in worlds.values():
                op[1](w, case)
            array_mode = array_mode and len(op) == 2   # (a third entry: the operation leaves the host-manifold mode)
        elif op[0] == "constraints":
            got = {name: {"constraints": w.constraints_download()} for name, w in worlds.items()}
            same(got["lazy"], got["oracle"], f"{what}: constraints after step {n}, vs the oracle")
            same(got["lazy"], got["twin"], f"{what}: constraints after step {n}, vs the twin that stores every step")
        elif op[0] == "bodies":
            got = {name: {"bodies": (w.synchronize(), w.bodies_download())[1]} for name, w in worlds.items()}
            same(got["lazy"], got["oracle"], f"{what}: bodies after step {n}, vs the oracle")
            same(got["lazy"], got["twin"], f"{what}: bodies after step {n}, vs the twin")
        else:
            got = {name: state(w) for name, w in worlds.items()}
            same(got["lazy"], got["oracle"], f"{what}: after step {n}, vs the oracle")
            same(got["lazy"], got["twin"], f"{what}: after step {n}, vs the twin that stores every step")
            assert float(np.abs(got["lazy"]["impulses"]["normal_impulse"]).max()) > 0.0
    for w in worlds.values():
        w.close()


def params():
    out = []
    for ci, cname in enumerate(CASES):
        for si, sname in enumerate(SCRIPTS):
            if sname == "pipeline_enable" and not cname.startswith("lattice3"):
                continue   # (the closed loop needs colliders: the lattice sets have them, and one size is enough for a change of mode)
            if sname == "put_back_into_upload_order" and cname == "lane_f32":
                continue   # (its switches keep the set in colour order: nothing to put back -- columns below covers f32)
            for use_graph in (0, 1):
                if (ci + si + use_graph) % 2 and sname not in ("steps_then_one_download", "bodies_inactive_then_active"):
                    continue   # (the two scripts every other one builds on run replayed AND eager on every set; the others alternate)
                out.append(pytest.param(cname, sname, use_graph, 1, id=f"{cname}-{sname}-{'replayed' if use_graph else 'eager'}"))
    for cname in ("lattice3_f64_colours", "lattice4_f32_islands", "lane_f32"):
        for sname in ("bodies_inactive_then_active", "upload_again_with_other_values"):
            out.append(pytest.param(cname, sname, 1, 0, id=f"{cname}-{sname}-replayed-match_contacts_off"))
    return out


@pytest.mark.parametrize("cname,sname,use_graph,match_contacts", params())
def test_lazy_world_equals_oracle_and_storing_twin(cname, sname, use_graph, match_contacts):
    make, bits, lib, env, form = CASES[cname]
    case = make()
    run_three(case, bits, lib, env, form, SCRIPTS[sname](case), use_graph, match_contacts, f"{cname}, {sname}, use_graph {use_graph}, match_contacts {match_contacts}")


# ---- the level permutation has moved rows: columns_case is compacted (5 colours -> fewer levels) -------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("sname", ["steps_then_one_download", "upload_again_with_other_values", "put_back_into_upload_order", "bodies_inactive_then_active"])
def test_compacted_set(sname, bits):
    case = dict(columns_case())
    m = len(case["mf"]["body1"])
    mf = dict(case["mf"]); mf["point_count"] = (np.arange(m) % 5).astype(np.uint8); case["mf"] = mf
    fr = np.array(case["friction"], copy=True); fr[1::3] = 0.0; case["friction"] = fr
    probe = new_world(hip_lib(), bits, case, 1)
    st = probe.level_compaction_stats()
    probe.close()
    assert st.state == F.LEVELS_COMPACTED and st.moved > 0, "the upload must have moved rows"
    run_three(case, bits, hip_lib, None, "islands" if bits == 32 else "colours", SCRIPTS[sname](case), 1, 1, f"columns f{bits}, {sname}")


# ---- the copy really did not run ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["lattice4_f64_colours", "lattice4_f32_islands", "lane_f32"])
def test_a_lazy_step_launches_one_kernel_less(cname):
    """the same set and steps on the measure build with AVN_EAGER_STORE (k_store_contact_impulses after every step, as before) and without; the release build counts as the
    lazy measure build does.  A step that follows a download is lazy again, and the download's own store is no launch of a step."""
    make, bits, _, env, form = CASES[cname]
    case = make()
    counts = {}
    for name, lib, e in (("eager", hip_measure_lib(), dict(env or {}, AVN_EAGER_STORE=1)), ("lazy", hip_measure_lib(), env), ("release", hip_lib(), None)):
        w = new_world(lib, bits, case, 1, e)
        per_step = []
        for k in range(4):
            w.step(); w.synchronize()
            per_step.append(w.timers().kernel_launches)
            if k == 1:
                w.impulses_download()
        counts[name] = per_step
        if name != "release" or env is None:
            assert_form(w, form, f"{cname}, {name}")
        w.close()
    print(cname, "kernel launches per step:", counts)
    assert all(c > 0 for c in counts["eager"])
    assert counts["lazy"] == [c - 1 for c in counts["eager"]], counts
    if env is None:
        assert counts["release"] == counts["lazy"], counts
