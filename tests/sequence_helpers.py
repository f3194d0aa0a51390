"""Re-upload sequences: scripts of uploads, config changes and steps driven through one F.World, judged at every checkpoint against (1) the oracle driven
through the same script, (2) a FRESH world of the same library built from the sequenced world's state just before the checkpoint's step, and (3) -- on the CPU --
the oracle with each mutating operation skipped, which must then differ (a mutation that changes nothing cannot reveal a stale cache).

A script is a list of Op.  The scripts of the host-manifold path are built here (HOST_SCRIPTS) so that the CPU tier (tests/test_sequences_cpu.py) validates exactly
what the GPU tier (tests/test_gpu_sequences.py) runs."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from avian_amd import scenes
from helpers import F, oracle_lib, random_joints, random_world

STATE_KEYS = ("position", "rotation", "linear_velocity", "angular_velocity")


@dataclass
class Op:
    kind: str                       # bodies | manifolds | joints | config | lacc | step
    args: Dict = field(default_factory=dict)
    checkpoint: bool = False        # (steps only) download everything after it and judge it
    note: str = ""

    @property
    def mutates(self) -> bool:
        return self.kind != "step"


def bodies(kw, note=""): return Op("bodies", dict(kw), note=note)
def manifolds(m, note=""): return Op("manifolds", dict(m), note=note)
def joints(kw, note=""): return Op("joints", dict(kw), note=note)
def config(note="", **kw): return Op("config", kw, note=note)
def lacc(linear=None, angular=None, note=""): return Op("lacc", dict(linear=linear, angular=angular), note=note)
def step(checkpoint=True): return Op("step", checkpoint=checkpoint)


def empty_joints():
    z3 = np.zeros((0, 3))
    return dict(joint_type=np.zeros(0, np.uint8), body1=np.zeros(0, np.int32), body2=np.zeros(0, np.int32), local_anchor1=z3, local_anchor2=z3, compliance=z3)


class Tables:
    """the most recent upload of every table: what a fresh twin is built from"""
    def __init__(self):
        self.bodies = self.manifolds = self.joints = self.lacc = None
        self.stepped_since_manifolds = False


def make_cfg(bits, use_graph, cfg_kw):
    kw = dict(substeps=3, use_graph=use_graph)
    kw.update(cfg_kw)
    return F.default_config(bits, **kw)


def upload_manifold_set(w, m, warm=None):
    wn, wt = warm if warm is not None else (m["warm_n"], m["warm_t"])
    scenes.upload_manifolds(w, m["mf"], m["offs"], m["friction"], m["restitution"], warm_n=wn, warm_t=wt)


def apply(w, op, bits, use_graph, tab, cfg_kw):
    if op.kind == "bodies":
        w.bodies_upload(**op.args); tab.bodies = op.args
        if tab.lacc is not None and len(op.args["inv_mass"]) != tab.n_lacc: tab.lacc = None   # (header: another body count drops the local accelerations)
    elif op.kind == "manifolds":
        upload_manifold_set(w, op.args); tab.manifolds = op.args; tab.stepped_since_manifolds = False
    elif op.kind == "joints":
        w.joints_upload(**op.args); tab.joints = op.args
    elif op.kind == "config":
        cfg_kw.update(op.args); w.config_set(make_cfg(bits, use_graph, cfg_kw))
    elif op.kind == "lacc":
        if op.args["linear"] is None and op.args["angular"] is None:
            w.local_accelerations_upload(); tab.lacc = None
        else:
            w.local_accelerations_upload(op.args["linear"], op.args["angular"]); tab.lacc = op.args; tab.n_lacc = len(op.args["linear"])
    elif op.kind == "step":
        w.step(); w.synchronize(); tab.stepped_since_manifolds = True
    else:
        raise ValueError(op.kind)


def downloads(w):
    out = {"bodies": w.bodies_download(), "solver_bodies": w.solver_bodies_download()}
    if w.n_manifolds:
        out["impulses"] = w.impulses_download(); out["constraints"] = w.constraints_download()
    if w.n_joints:
        out["joints"] = w.joints_download()
    return out


def fresh_twin_step(lib, bits, use_graph, w, tab, cfg_kw):
    """A new world holding the sequenced world's bodies as they are NOW plus the most recent upload of every other table (the manifolds with the impulses the
    sequenced world would warm-start from), stepped once."""
    tw = F.World(lib, make_cfg(bits, use_graph, cfg_kw))
    kw = dict(tab.bodies); kw.update(w.bodies_download())
    tw.bodies_upload(**kw)
    if tab.manifolds is not None:
        warm = None
        if tab.stepped_since_manifolds and w.n_manifolds:
            imp = w.impulses_download()
            warm = (imp["warm_start_normal_impulse"], imp["warm_start_tangent_impulse"])
        upload_manifold_set(tw, tab.manifolds, warm)
    if tab.joints is not None:
        tw.joints_upload(**tab.joints)
    if tab.lacc is not None:
        tw.local_accelerations_upload(tab.lacc["linear"], tab.lacc["angular"])
    tw.step(); tw.synchronize()
    out = downloads(tw)
    tw.close()
    return out


def run_script(lib, bits, script: List[Op], use_graph, twin=False, skip: Optional[int] = None, until_checkpoint: Optional[int] = None, base_cfg=None, probe=None):
    """Executes `script` on a new world of `lib`; returns one dict per checkpoint: {"seq": downloads of the sequenced world, "twin": downloads of the fresh twin
    (twin=True) or None}.  skip: the index of ONE operation to leave out (the mutation control); until_checkpoint: stop after that many checkpoints;
    probe: called with the sequenced world at every checkpoint, its result kept under "probe" (read-outs such as avn_solver_forms)."""
    cfg_kw = dict(base_cfg or {})
    w = F.World(lib, make_cfg(bits, use_graph, cfg_kw))
    tab = Tables()
    out = []
    for i, op in enumerate(script):
        if i == skip:
            continue
        tw = None
        if op.kind == "step" and op.checkpoint and twin:
            tw = fresh_twin_step(lib, bits, use_graph, w, tab, cfg_kw)
        apply(w, op, bits, use_graph, tab, cfg_kw)
        if op.kind == "step" and op.checkpoint:
            out.append({"seq": downloads(w), "twin": tw, "twin_rows": enabled_rows(tab), "probe": probe(w) if probe else None})
            if until_checkpoint is not None and len(out) >= until_checkpoint:
                break
    w.close()
    return out


def enabled_rows(tab):
    """manifolds whose bodies are both enabled.  A manifold on a RigidBodyDisabled body generates no constraint and its normal_impulse record keeps the value of the
    last step that did: state of the sequenced world that no upload carries, so the fresh twin is no reference for that record (the oracle still is)."""
    if tab.manifolds is None or tab.bodies.get("body_flags") is None:
        return None
    off = (np.asarray(tab.bodies["body_flags"]) & F.BODY_DISABLED) != 0
    return ~(off[tab.manifolds["mf"]["body1"]] | off[tab.manifolds["mf"]["body2"]])


def assert_twin(c, what):
    """the sequenced world against its fresh twin: "the sequence left stale state" when this fails while the twin equals the oracle"""
    seq, tw = c["seq"], c["twin"]
    if c["twin_rows"] is not None and "impulses" in seq:
        seq = dict(seq); tw = dict(tw)
        seq["impulses"] = dict(seq["impulses"]); tw["impulses"] = dict(tw["impulses"])
        for d in (seq, tw):
            d["impulses"]["normal_impulse"] = d["impulses"]["normal_impulse"][c["twin_rows"]]
    assert_equal_downloads(seq, tw, what)


def same(a, b):
    """bit for bit, NaN == NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


def assert_equal_downloads(a, b, what):
    assert a.keys() == b.keys(), f"{what}: tables {sorted(a)} vs {sorted(b)}"
    for t in a:
        for k in a[t]:
            if not same(a[t][k], b[t][k]):
                x, y = np.asarray(a[t][k]), np.asarray(b[t][k])
                bad = ~((x == y) | ((x != x) & (y != y))) if x.shape == y.shape else None
                where = tuple(np.argwhere(bad)[0]) if bad is not None else None
                raise AssertionError(f"{what}: {t}.{k} differs" + (f" in {int(bad.sum())} of {bad.size}; first at {where}: {x[where]!r} vs {y[where]!r}" if bad is not None else f": shapes {x.shape} vs {y.shape}"))


def bodies_differ(a, b):
    return any(not same(a["bodies"][k], b["bodies"][k]) for k in STATE_KEYS)


def mutation_controls(lib, bits, script, base_cfg=None):
    """For every mutating operation: the oracle with that ONE operation skipped must differ in the bodies at the next checkpoint (an upload that the world then
    refuses for want of the skipped table differs too).  Returns the operations that changed nothing."""
    full = run_script(lib, bits, script, 0, base_cfg=base_cfg)
    idle = []
    for i, op in enumerate(script):
        if not op.mutates:
            continue
        k = sum(1 for o in script[:i] if o.kind == "step" and o.checkpoint)   # checkpoints in front of the operation
        if k >= len(full):
            idle.append((i, op.kind, op.note, "no checkpoint behind it")); continue
        try:
            got = run_script(lib, bits, script, 0, skip=i, until_checkpoint=k + 1, base_cfg=base_cfg)
        except F.AvnError:
            continue
        if len(got) <= k or not bodies_differ(full[k]["seq"], got[k]["seq"]):
            idle.append((i, op.kind, op.note, "the next checkpoint's bodies are bit-identical without it"))
    return full, idle


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------------------------
def colored(wd, keep=None, restitution=None):
    """the manifolds `keep` of a random_world, coloured (persistent greedy, in manifold order) and colour-major: the arguments of one manifolds upload"""
    keep = np.arange(len(wd["manifolds"]["body1"])) if keep is None else np.asarray(keep)
    mf = {k: np.asarray(v)[keep] for k, v in wd["manifolds"].items()}
    offs, perm = scenes.color_manifolds(oracle_lib(), mf, np.asarray(wd["bodies"]["rb_type"]))
    rest = wd["restitution"][keep][perm] if restitution is None else np.full(len(keep), float(restitution))
    return dict(mf=scenes.permute_manifolds(mf, perm), offs=np.asarray(offs).copy(), friction=wd["friction"][keep][perm], restitution=rest,
                warm_n=wd["warm_n"][keep][perm], warm_t=wd["warm_t"][keep][perm])


def reordered(m, perm, offs=None):
    perm = np.asarray(perm)
    return dict(mf={k: np.asarray(v)[perm] for k, v in m["mf"].items()}, offs=np.asarray(m["offs"] if offs is None else offs).copy(),
                friction=m["friction"][perm], restitution=m["restitution"][perm], warm_n=m["warm_n"][perm], warm_t=m["warm_t"][perm])


def hub_world(seed=31):
    """260 bodies, 500 random manifolds and a hub with 70 neighbours: the overflow colour holds about 50 manifolds"""
    return random_world(seed=seed, n_bodies=260, n_manifolds=500, hub_degree=70, with_odd_features=False)


def blocks_exchanged(m):
    """two colour blocks of different sizes exchanged (the colouring stays valid: a colour's manifolds share no body wherever the colour sits)"""
    offs = np.asarray(m["offs"]).astype(np.int64)
    size = np.diff(offs[:F.COLOR_OVERFLOW_INDEX + 1])
    used = np.flatnonzero(size > 0)
    a, b = int(used[0]), int(used[-1])
    assert a != b and size[a] != size[b], "the exchange must change the captured colour ranges"
    order = list(range(F.COLOR_OVERFLOW_INDEX)); order[a], order[b] = b, a
    perm = np.concatenate([np.arange(offs[c], offs[c + 1]) for c in order] + [np.arange(offs[F.COLOR_OVERFLOW_INDEX], offs[-1])])
    new = offs.copy(); new[1:F.COLOR_OVERFLOW_INDEX + 1] = np.cumsum(size[order])
    out = reordered(m, perm, new.astype(np.uint32))
    assert not np.array_equal(out["offs"], m["offs"]) and out["offs"][-1] == m["offs"][-1]
    return out


def permuted_inside_colours(m, seed=5):
    """every colour's manifolds shuffled (other bodies per slot), and other point counts on a fifth of them"""
    rng = np.random.default_rng(seed)
    offs = np.asarray(m["offs"]).astype(np.int64)
    perm = np.concatenate([offs[c] + rng.permutation(offs[c + 1] - offs[c]) for c in range(F.COLOR_OVERFLOW_INDEX)] + [np.arange(offs[F.COLOR_OVERFLOW_INDEX], offs[-1])])
    out = reordered(m, perm)
    pc = out["mf"]["point_count"].copy()
    pick = rng.random(len(pc)) < 0.2
    pc[pick] = (pc[pick] % 4) + 1
    out["mf"]["point_count"] = pc
    assert not np.array_equal(out["mf"]["body1"], m["mf"]["body1"]) and not np.array_equal(pc, m["mf"]["point_count"][perm])
    return out


def overflow_reversed(m):
    offs = np.asarray(m["offs"]).astype(np.int64)
    o0, o1 = offs[F.COLOR_OVERFLOW_INDEX], offs[F.COLOR_OVERFLOW_INDEX + 1]
    assert o1 - o0 > 16, "the overflow colour must be populated (and above the per-level threshold of the measure run)"
    return reordered(m, np.concatenate([np.arange(o0), np.arange(o1 - 1, o0 - 1, -1)]))


def three_uploads(wd, first, second):
    return [bodies(wd["bodies"]), manifolds(first, "first set"), step(), manifolds(second, "changed set"), step(), manifolds(first, "first set again"), step()]


def script_colour_blocks():
    wd = hub_world(); m = colored(wd)
    return three_uploads(wd, m, blocks_exchanged(m))


def script_permuted_colours():
    wd = hub_world(32); m = colored(wd)
    return three_uploads(wd, m, permuted_inside_colours(m))


def script_overflow_reversed():
    wd = hub_world(33); m = colored(wd)
    return three_uploads(wd, m, overflow_reversed(m))


def script_restitution_toggle():
    wd = hub_world(34)
    wd["manifolds"]["normal_speed"] = -np.abs(wd["manifolds"]["normal_speed"]) - 1.5   # (approaching faster than the restitution threshold: the pass has work)
    m0, m3 = colored(wd, restitution=0.0), colored(wd, restitution=0.3)
    return three_uploads(wd, m0, m3)


def some_joints(seed, n_bodies, n_joints=60, damped=True):
    j = random_joints(np.random.default_rng(seed), n_bodies, n_joints, with_damping=damped)
    assert set(j["joint_type"].tolist()) == {0, 1, 2, 3, 4}
    return j


def script_body_membership():
    """the same count, other SolverBody membership: one dynamic body static, one DISABLED, one kinematic -- then back; manifolds and joints untouched"""
    wd = hub_world(35); m = colored(wd); j = some_joints(1, 260)
    b0 = dict(wd["bodies"]); b0["body_flags"] = np.zeros(260, np.uint8)
    used = np.intersect1d(np.concatenate([m["mf"]["body1"], m["mf"]["body2"]]), np.concatenate([j["body1"], j["body2"]]))
    used = used[np.asarray(b0["rb_type"])[used] == F.RB_DYNAMIC]
    a, c = int(used[0]), int(used[1])
    # (the disabled body has manifolds but no joint: prepare_xpbd_joint skips a joint on a RigidBodyDisabled body and the joint keeps the anchors of the last step
    #  that prepared it -- component state no upload carries, which a fresh twin cannot hold)
    free = np.setdiff1d(np.concatenate([m["mf"]["body1"], m["mf"]["body2"]]), np.concatenate([j["body1"], j["body2"]]))
    b = int(free[np.asarray(b0["rb_type"])[free] == F.RB_DYNAMIC][0])
    b1 = {k: np.array(v, copy=True) for k, v in b0.items()}
    b1["rb_type"][a] = F.RB_STATIC; b1["inv_mass"][a] = 0.0; b1["inv_inertia_local"][a] = 0.0; b1["linear_velocity"][a] = 0.0; b1["angular_velocity"][a] = 0.0
    b1["body_flags"][b] = F.BODY_DISABLED
    b1["rb_type"][c] = F.RB_KINEMATIC
    return [bodies(b0), manifolds(m), joints(j), step(), bodies(b1, "static / disabled / kinematic"), step(), bodies(b0, "dynamic again"), step()]


def script_bodies_grow_shrink():
    """260 -> 400 bodies (past cap_bodies: every body buffer moves) with manifolds on the new bodies, then back to 260 (the drop rules) and the first manifolds again"""
    wd = random_world(seed=36, n_bodies=400, n_manifolds=800, hub_degree=110, with_odd_features=False)
    small = {k: np.asarray(v)[:260] for k, v in wd["bodies"].items()}
    inside = np.flatnonzero((wd["manifolds"]["body1"] < 260) & (wd["manifolds"]["body2"] < 260))
    wsmall = dict(wd); wsmall["bodies"] = small
    m_small, m_big = colored(wsmall, inside), colored(wd)
    assert m_small["offs"][24] - m_small["offs"][23] > 0 and (m_big["mf"]["body1"] >= 260).any()
    return [bodies(small), manifolds(m_small), step(), bodies(wd["bodies"], "grown"), manifolds(m_big, "with the new bodies"), step(),
            bodies(small, "shrunk"), manifolds(m_small, "the first set again"), step()]


def script_joint_sets():
    wd = hub_world(37); m = colored(wd)
    j1, j2 = some_joints(2, 260, damped=True), some_joints(3, 260, damped=False)
    return [bodies(wd["bodies"]), manifolds(m), joints(j1, "J1 damped"), step(), joints(j2, "J2 undamped"), step(), joints(empty_joints(), "none"), step(),
            joints(j1, "J1 damped again"), step()]


def script_config_changes():
    wd = hub_world(38); m = colored(wd); j = some_joints(4, 260)
    return [bodies(wd["bodies"]), manifolds(m), joints(j), step(), config("5 substeps", substeps=5), step(), config("3 substeps, 2 iterations", substeps=3, solver_iterations=2), step(),
            config("gravity and dt", gravity=(0.5, -3.0, 1.0), dt_ns=int(round(1e9 / 120))), step(),
            # (use_graph changes no bit by design, so each flip rides on a change that does: the mutation control holds for the operation as a whole)
            config("direct launches, 4 substeps", use_graph=0, substeps=4), step(), config("graph replay, 3 substeps, one iteration", use_graph=1, substeps=3, solver_iterations=1), step()]


def script_local_accelerations():
    wd = hub_world(39); m = colored(wd)
    rng = np.random.default_rng(9)
    a1, a2 = (rng.normal(scale=3.0, size=(260, 3)), rng.normal(scale=3.0, size=(260, 3))), (rng.normal(scale=3.0, size=(260, 3)), rng.normal(scale=3.0, size=(260, 3)))
    return [bodies(wd["bodies"]), manifolds(m), lacc(*a1, note="values"), step(), lacc(*a2, note="other values"), step(), lacc(note="cleared"), step(), lacc(*a1, note="values again"), step()]


HOST_SCRIPTS = {
    "colour_blocks_exchanged": script_colour_blocks,
    "permuted_inside_colours": script_permuted_colours,
    "overflow_reversed": script_overflow_reversed,
    "restitution_toggled": script_restitution_toggle,
    "body_membership": script_body_membership,
    "bodies_grow_shrink": script_bodies_grow_shrink,
    "joint_sets": script_joint_sets,
    "config_changes": script_config_changes,
    "local_accelerations": script_local_accelerations,
}
_built = {}


def host_script(name):
    """built once per process: the scripts are read-only inputs shared by every test that runs them"""
    if name not in _built:
        _built[name] = HOST_SCRIPTS[name]()
    return _built[name]


# ---- the closed loop (avn_pipeline_enable(1)): the contact table persists on the device, so the reference is the oracle in lock step (and the mutation control) ------
# A closed-loop script is a list of ("step", n) and ("op", name, fn) entries; fn(world, scene) applies ONE host action to one world from that world's own state.
def closed_scene(seed=21, n=80):
    from pipeline_scenes import dropped_boxes
    b, c = dropped_boxes(seed=seed, n=n)
    return dict(bodies=b, colliders=c)


def closed_world(lib, bits, use_graph, scene, substeps=4):
    w = F.World(lib, F.default_config(bits, substeps=substeps, use_graph=use_graph))
    w.bodies_upload(**scene["bodies"]); w.colliders_upload(**scene["colliders"])
    w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.6, restitution=0.0)
    w.pipeline_enable()
    return w


def op_materials(w, sc): w.collider_materials_upload(friction=0.05, restitution=0.6)


def op_transforms(w, sc):
    n = len(sc["colliders"]["body"])
    rng = np.random.default_rng(4)
    child = (np.arange(n) % 3 == 1).astype(np.uint8); child[0] = 0
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w.collider_transforms_upload(child, rng.uniform(-0.3, 0.3, (n, 3)), q)


def op_transforms_cleared(w, sc): w.collider_transforms_upload()


def op_half_extents(w, sc):
    c = dict(sc["colliders"]); he = np.array(c["half_extents"], copy=True); he[1:] *= 0.8; c["half_extents"] = he
    w.colliders_upload(**c); w.collider_materials_upload(friction=0.6, restitution=0.0)


def op_teleport(w, sc):
    """the last body goes above the middle of the pile, falling"""
    kw = dict(sc["bodies"]); st = w.bodies_download()
    for k in STATE_KEYS: kw[k] = np.array(st[k], copy=True)
    mid = kw["position"][1:-1].mean(axis=0)
    kw["position"][-1] = [mid[0], kw["position"][1:-1, 1].max() + 0.8, mid[2]]; kw["linear_velocity"][-1] = [0.0, -4.0, 0.0]
    w.bodies_upload(**kw)


def op_sleeping_on(w, sc): w.sleeping_enable(True, time_to_sleep=0.05, linear_threshold=3.0, angular_threshold=3.0)
def op_sleeping_off(w, sc):
    """off (every island is woken first) -- and on again is refused once the loop holds pairs (both backends: AVN_ERR_STATE, nothing changes)"""
    w.sleeping_enable(False)
    try:
        op_sleeping_on(w, sc)
    except F.AvnError as e:
        assert e.status == 6, e
    else:
        raise AssertionError("avn_sleeping_enable inside a running closed loop must be refused")


def op_restart(w, sc):
    """avn_pipeline_enable(0) -> every table again with the bodies where they are -> avn_pipeline_enable(1): the contact table starts empty"""
    kw = dict(sc["bodies"]); kw.update(w.bodies_download())
    w.pipeline_enable(False)
    w.bodies_upload(**kw); w.colliders_upload(**sc["colliders"]); w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.6, restitution=0.0)
    w.pipeline_enable()


CLOSED_SCRIPTS = {
    "materials_changed": [("step", 14), ("op", "other materials", op_materials), ("step", 8)],
    "transforms_changed_then_cleared": [("step", 10), ("op", "child transforms", op_transforms), ("step", 8), ("op", "cleared", op_transforms_cleared), ("step", 8)],
    "half_extents_changed": [("step", 12), ("op", "smaller colliders", op_half_extents), ("step", 10)],
    "body_teleported_onto_the_pile": [("step", 12), ("op", "teleport", op_teleport), ("step", 14)],
    # (avn_sleeping_enable(on) is only accepted before the first pair exists: on at the start, off in the running loop, and the refused second on)
    "sleeping_on_off_on": [("op", "sleeping on", op_sleeping_on), ("step", 16), ("op", "sleeping off, on again refused", op_sleeping_off), ("step", 8)],
    "restart": [("step", 12), ("op", "restart", op_restart), ("step", 8)],
}


def run_closed(libs, bits, use_graph, script, scene, skip=None, after_step=None, stop_after_block=None):
    """one world per library in lock step; after_step(s, worlds) after every step.  Returns the first world's bodies after every block of steps."""
    worlds = [closed_world(l, bits, use_graph, scene) for l in libs]
    out, s = [], 0
    for i, e in enumerate(script):
        if e[0] == "op":
            if i != skip:
                for w in worlds: e[2](w, scene)
            continue
        for _ in range(e[1]):
            for w in worlds: w.step()
            if after_step is not None: after_step(s, worlds)
            s += 1
        out.append(worlds[0].bodies_download())
        if stop_after_block is not None and len(out) >= stop_after_block:
            break
    for w in worlds[1:]: w.close()
    return out, worlds[0]


def closed_mutation_controls(lib, bits, script, scene):
    full, w = run_closed([lib], bits, 0, script, scene); w.close()
    idle = []
    for i, e in enumerate(script):
        if e[0] != "op":
            continue
        k = sum(1 for x in script[:i] if x[0] == "step")   # the block of steps behind the operation
        got, w = run_closed([lib], bits, 0, script, scene, skip=i, stop_after_block=k + 1); w.close()
        if all(same(full[k][key], got[k][key]) for key in STATE_KEYS):
            idle.append((i, e[1]))
    return idle
