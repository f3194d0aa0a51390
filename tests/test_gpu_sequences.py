"""GPU: re-upload sequences on the HIP backend (tests/sequence_helpers.py).  A real host re-sends manifolds every step, re-uploads bodies when it spawns or
teleports, swaps joint sets and changes avn_config between steps; whether that works depends on the hand-kept cache flags of World<T> and on the captured substep
graph, and a wrong flag raises no error -- it replays a stale schedule.  Every checkpoint of every script is compared bit for bit with
  * the oracle driven through the same script (the oracle shares none of the caches), and
  * a FRESH HIP world built from the sequenced world's bodies just before the step plus the latest upload of every other table: sequenced != fresh means the
    sequence left stale state, fresh != oracle means a kernel is wrong.
That every upload of every script changes bits (so that ignoring it is visible) is checked on the CPU: tests/test_sequences_cpu.py.

f64: the scripts whose mutation changes launch parameters, buffer addresses or schedules that depend on the scalar size run in f64 too (body buffers, joint
schedule in LDS, config); for the pure manifold re-orderings and the restitution gate the f64 run would repeat the same host decisions on the same integer tables and
add only oracle time -- colour_blocks_exchanged, permuted_inside_colours, overflow_reversed, restitution_toggled and local_accelerations run in f32 only."""
import numpy as np
import pytest

import sequence_helpers as S
from helpers import hip_lib, hip_measure_lib, oracle_lib
from test_gpu_graph import compare_step

pytestmark = pytest.mark.gpu

# script -> (the cache flags and captured state it is aimed at, scalar sizes)
HOST = {
    # graph_valid through set_color_offsets (colour ranges are captured kernel arguments), grid_blocks, incidence_dirty, slots_dirty
    "colour_blocks_exchanged": (32,),
    # incidence_dirty, slots_dirty (body-sorted slot order), groups_dirty; the captured graph must read the new rows from unchanged pointers
    "permuted_inside_colours": (32,),
    # ovf_csr_dirty (per-body CSR of the overflow colour), sched_overflow / level schedule, graph_valid when the captured level sizes change
    "overflow_reversed": (32,),
    # any_restitution: the graph captured without the restitution pass must be re-captured when a set brings restitution, and again when it leaves
    "restitution_toggled": (32,),
    # h_body_has_sb, joint_schedule_dirty, incidence_dirty, bodies_prepared_early with manifolds and joints untouched
    "body_membership": (32, 64),
    # cap_bodies growth: every body buffer moves under the captured graph (graph_valid via `moved`), the drop rules of a shrinking upload, lacc dropped
    "bodies_grow_shrink": (32, 64),
    # joint_schedule_dirty, any_damped (the damping pass in / out of the captured graph), the joint schedule in LDS, n_joints == 0
    "joint_sets": (32, 64),
    # graph_valid on substeps / solver_iterations / use_graph, params re-derived from gravity and dt
    "config_changes": (32, 64),
    # dw.lacc_l / lacc_a: same pointers, new contents (the graph must read them); cleared = pointers dropped (graph_valid)
    "local_accelerations": (32,),
}
assert set(HOST) == set(S.HOST_SCRIPTS)

_oracle_runs = {}


def oracle_checkpoints(name, bits):
    """the oracle through the script, once per (script, scalar size): use_graph is no input of the oracle"""
    if (name, bits) not in _oracle_runs:
        _oracle_runs[(name, bits)] = S.run_script(oracle_lib(), bits, S.host_script(name), 0)
    return _oracle_runs[(name, bits)]


def judge(name, bits, use_graph, lib, probe=None):
    got = S.run_script(lib, bits, S.host_script(name), use_graph, twin=True, probe=probe)
    want = oracle_checkpoints(name, bits)
    assert len(got) == len(want) >= 3
    for k, (g, o) in enumerate(zip(got, want)):
        what = f"{name} f{bits} use_graph={use_graph} checkpoint {k}"
        S.assert_twin(g, what + ": the sequence left stale state (sequenced device world vs fresh device world)")
        S.assert_equal_downloads(o["seq"], g["seq"], what + ": the device world equals its fresh twin but not the oracle (a kernel is wrong)")
    return got


def overflow_levels(m, bodies):
    """levels of the overflow list, restated: in list order, level = 1 + the highest level so far on either body that has a SolverBody"""
    offs = np.asarray(m["offs"]).astype(np.int64)
    fl = np.asarray(bodies.get("body_flags", np.zeros(len(bodies["rb_type"]), np.uint8)))
    sb = (np.asarray(bodies["rb_type"]) != S.F.RB_STATIC) & ((fl & (S.F.BODY_SLEEPING | S.F.BODY_DISABLED)) == 0)
    last, top = {}, 0
    for i in range(offs[S.F.COLOR_OVERFLOW_INDEX], offs[S.F.COLOR_OVERFLOW_INDEX + 1]):
        keys = [int(b) for b in (m["mf"]["body1"][i], m["mf"]["body2"][i]) if sb[b]]
        lv = 1 + max([last.get(b, 0) for b in keys], default=0)
        for b in keys:
            last[b] = lv
        top = max(top, lv)
    return top


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("name,bits", [(n, b) for n in sorted(HOST) for b in HOST[n]])
def test_host_manifold_sequence(name, bits, use_graph):
    judge(name, bits, use_graph, hip_lib())


@pytest.mark.parametrize("use_graph", [0, 1])
def test_overflow_reversed_in_the_per_level_form(use_graph, monkeypatch):
    """the same script with the overflow colour above AVN_OVERFLOW_LEVEL_THRESHOLD (measure build): one launch per level, the level sizes are launch parameters
    (sched_overflow.gorder / glevel_offsets, graph_valid when they change)"""
    monkeypatch.setenv("AVN_OVERFLOW_LEVEL_THRESHOLD", "16")
    monkeypatch.setenv("AVN_ISLAND_BLOCKS", "0")   # (f32, no joints, 260 bodies: without it the island blocks solve the set and no overflow launch of either form is ever made)
    got = judge("overflow_reversed", 32, use_graph, hip_measure_lib(), probe=lambda w: w.solver_forms())
    script = S.host_script("overflow_reversed")
    sets = [op.args for op in script if op.kind == "manifolds"]
    bodies = [op.args for op in script if op.kind == "bodies"][0]
    want = [overflow_levels(m, bodies) for m in sets]
    print("overflow levels per upload:", want, "read out:", [(g["probe"].overflow_form, g["probe"].overflow_levels, g["probe"].island_blocks) for g in got])
    assert len(set(want)) > 1 or want[0] > 1, "the reversed list must have a schedule of its own"
    for g, levels in zip(got, want):
        f = g["probe"]
        assert f.island_blocks == 0 and f.overflow_form == S.F.OVERFLOW_FORM_LEVEL and f.overflow_levels == levels and f.overflow_components == 0


# ---- the closed loop: the contact table lives on the device, so the reference is the oracle in lock step after EVERY step (test_gpu_graph.compare_step: colour lists
#      with order, new ids, status changes, counters, bodies).  script -> the cached state it is aimed at
CLOSED = {
    # col_mat rows read by the narrow phase of live pairs; any_restitution / materials_restitution (the restitution pass enters the captured graph)
    "materials_changed": None,
    # tf_any and the collider-local poses in the AABB and narrow-phase launches (other kernel instantiations), sp_valid
    "transforms_changed_then_cleared": None,
    # slot_entity / entity_slot / ent2slot re-used for the same entities, the interval table and pair set kept across the upload
    "half_extents_changed": None,
    # bodies_prepared_early, slot_clear_pending, incidence_dirty, joint_schedule_dirty with live contact rows; islands_dirty / isl_labels_step_valid
    "body_teleported_onto_the_pile": None,
    # slp_on, slp_world_asleep / slp_world_idle, h_body_has_sb from the island manager, pipe_handles_dirty after the wake-all of the switch-off
    "sleeping_on_off_on": None,
    # pipeline_device_reset: pgm_* mirrors, contact_keys_live, use_handles, graph_valid, the pair set rebuilt from the host's keys
    "restart": None,
}
assert set(CLOSED) == set(S.CLOSED_SCRIPTS)


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_loop_sequence(name, bits, use_graph):
    def after_step(s, worlds):
        compare_step(s, worlds[1], worlds[0])
    out, wh = S.run_closed([hip_lib(), oracle_lib()], bits, use_graph, S.CLOSED_SCRIPTS[name], S.closed_scene(), after_step=after_step)
    assert wh.pipeline_stats().manifolds > 10 and any(not np.array_equal(out[0][k], out[-1][k]) for k in out[0])


@pytest.mark.parametrize("use_graph", [0, 1])
def test_restarted_closed_loop_equals_a_fresh_world(use_graph):
    """avn_pipeline_enable(0) -> uploads -> (1) starts from an empty contact table: the restarted world == a NEW device world given the same uploads (no row, id,
    colour mask or warm-start impulse of the first run survives).  The oracle's half: tests/test_sequences_cpu.py."""
    hip, scene = hip_lib(), S.closed_scene()
    w = S.closed_world(hip, 32, use_graph, scene)
    for _ in range(12): w.step()
    kw = dict(scene["bodies"]); kw.update(w.bodies_download())
    S.op_restart(w, scene)
    tw = S.closed_world(hip, 32, use_graph, dict(bodies=kw, colliders=scene["colliders"]))
    for s in range(8):
        w.step(); tw.step()
        compare_step(s, tw, w)
