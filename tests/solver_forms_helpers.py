"""Helpers of tests/test_gpu_solver_forms.py: worlds created under `make measure` switches, the handle mode driven by hand (contact_pairs_add, contacts_upload,
manifold_handles_upload -- host bookkeeping, not the closed loop), and HostRule: a restatement, in plain Python, of how the host picks a colour's kernel and grid
and of when it must capture the substep graph again.  HostRule shares nothing with the library: the tests compare avn_solver_forms with it."""
import contextlib
import os

import numpy as np

from helpers import F, assert_same

NC = F.COLOR_OVERFLOW_INDEX   # 23 launch ranges in front of the overflow list
ENTITY0 = 1000                # collider entity of body b = ENTITY0 + b
OCT_ON, OCT_OFF = 12288, 20480


@contextlib.contextmanager
def switches(**env):
    """AVN_* switches are read when a world is created, by the measure build only"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_world(lib, bits, bodies, use_graph, env=None, substeps=2):
    with switches(**(env or {})):
        w = F.World(lib, F.default_config(bits, substeps=substeps, use_graph=use_graph))
    w.bodies_upload(**bodies)
    return w


def forms_of(f):
    return list(f.colour_form), list(f.colour_grid_blocks), list(f.restitution_colour_form)


def color_grid_blocks(count):
    """workgroups of the lane form for `count` manifolds: 64 per workgroup, rounded up to a multiple of 8 (one per XCD)"""
    return (((count + 63) // 64 + 7) // 8) * 8


class HostRule:
    """Per launch range c of colours 0..22, from the range's size alone:
      grid:  kept while need <= grid <= 4 * need + 64 (need = color_grid_blocks(cnt), 0 for an empty range); else grid = color_grid_blocks(cnt + cnt / 4 + 64), 0 when empty
      form:  oct (f32 only) while cnt != 0 and cnt <= (OCT_OFF if it was oct else OCT_ON); else lane
    and the substep graph is captured again by the next step when a grid or a form changed, when the number of manifolds changed, when the world changes between
    host manifolds and handles, and -- host manifolds only, whose ranges are captured kernel arguments -- when any offset changed."""

    def __init__(self, f32, handles, oct_on=OCT_ON, oct_off=OCT_OFF, oct_enabled=True):
        self.oct_ok, self.handles, self.on, self.off = f32 and oct_enabled, handles, oct_on, oct_off
        self.grid, self.oct, self.offs, self.captures = [0] * NC, [False] * NC, None, 0

    def upload(self, offs):
        """returns (colour_form, colour_grid_blocks, captures after the step that follows) as avn_solver_forms must report them"""
        offs = [int(x) for x in offs]
        invalid = self.offs is None or offs[-1] != self.offs[-1] or (not self.handles and offs != self.offs)
        self.offs = offs
        why = ["first capture"] if invalid else []
        for c in range(NC):
            cnt = offs[c + 1] - offs[c]
            need = color_grid_blocks(cnt) if cnt else 0
            if need > self.grid[c] or self.grid[c] > 4 * need + 64:
                why.append(f"colour {c}: grid {self.grid[c]} {'outgrown' if need > self.grid[c] else 'shrunk'} (need {need})")
                self.grid[c] = color_grid_blocks(cnt + cnt // 4 + 64) if cnt else 0
                invalid = True
            now = self.oct_ok and cnt != 0 and cnt <= (self.off if self.oct[c] else self.on)
            if now != self.oct[c]:
                why.append(f"colour {c}: {'lane -> oct' if now else 'oct -> lane'} at {cnt}")
                self.oct[c] = now
                invalid = True
        self.captures += invalid
        # host manifolds: a captured range is exact and an empty one is not launched; handles: a grid kept for an emptied range still launches (idle lanes)
        launched = [self.grid[c] != 0 and (self.handles or offs[c + 1] > offs[c]) for c in range(NC)]
        form = [(F.COLOUR_FORM_OCT if self.oct[c] else F.COLOUR_FORM_LANE) if launched[c] else F.FORM_NONE for c in range(NC)]
        return form, [self.grid[c] if launched[c] else 0 for c in range(NC)], self.captures, why


# ---- handle mode by hand ------------------------------------------------------------------------------------------------------------------------------------------------
def colliders_for(n_bodies):
    return dict(entity_index=np.arange(n_bodies, dtype=np.uint32) + ENTITY0, body=np.arange(n_bodies, dtype=np.int32), shape=np.zeros(n_bodies, np.uint8),
                half_extents=np.full((n_bodies, 3), 0.5))


def rows_of(case):
    """the ContactGraph rows of a make_case set, in the layout of contacts_download"""
    mf = case["mf"]
    m = len(mf["body1"])
    return dict(flags=np.full(m, F.CP_TOUCHING | F.CP_GENERATE_CONSTRAINTS, np.uint32), point_count=mf["point_count"], normal=mf["normal"], friction=case["friction"],
                restitution=case["restitution"], anchor1=mf["anchor1"], anchor2=mf["anchor2"], penetration=mf["penetration"], normal_speed=mf["normal_speed"],
                warm_start_normal_impulse=case["warm_n"], warm_start_tangent_impulse=case["warm_t"], normal_impulse=np.zeros((m, 4)),
                feature_id1=np.zeros((m, 4), np.uint32), feature_id2=np.zeros((m, 4), np.uint32))


def contact_ids(case, seed=77):
    """contact id of manifold i: a permutation, so that handle -> row is no identity"""
    return np.random.default_rng(seed).permutation(len(case["mf"]["body1"])).astype(np.uint32)


def handle_world(lib, bits, case, use_graph, ids, env=None, bodies=None, rows=None):
    """a world that holds every manifold of `case` as a contact row (ids[i] = row of manifold i); no handle list yet"""
    w = make_world(lib, bits, bodies or case["bodies"], use_graph, env)
    mf = case["mf"]
    w.colliders_upload(**colliders_for(len(case["bodies"]["rb_type"])))
    w.existing_pairs_upload(np.zeros(0, np.uint64))
    w.collider_materials_upload(friction=0.5, restitution=0.3)   # (handle mode: the restitution pass runs when a material has restitution; the rows carry their own values)
    w.contact_pairs_add(ids, mf["body1"].astype(np.uint32) + ENTITY0, mf["body2"].astype(np.uint32) + ENTITY0, np.full(len(ids), F.PAIR_GENERATE_CONSTRAINTS, np.uint32))
    w.contacts_upload(ids, rows if rows is not None else rows_of(case))
    return w


def handle_state(w, ids):
    w.synchronize()
    return {"bodies": w.bodies_download(), "impulses": w.impulses_download(), "constraints": w.constraints_download(), "rows": w.contacts_download(np.sort(ids))}


def same(a, b, what):
    for part in a:
        for k in a[part]:
            assert_same(a[part][k], b[part][k], f"{what}: {part}.{k}")


def run_handle_script(lib, bits, case, ids, lists, use_graph=1, env=None, twin=False):
    """lists: per step (offsets[25], manifold indices in list order).  One world; before every step the handle lists are sent again.  twin: a FRESH world of the same
    library and switches is built before every step from the sequenced world's bodies and contact rows as they are at that moment, given the same lists and stepped
    once.  Returns per step (state, twin state or None, avn_solver_forms)."""
    w = handle_world(lib, bits, case, use_graph, ids, env)
    out = []
    for offs, order in lists:
        tw = None
        if twin:
            w.synchronize()
            bodies = dict(case["bodies"]); bodies.update(w.bodies_download())
            t = handle_world(lib, bits, case, use_graph, ids, env, bodies=bodies, rows=w.contacts_download(ids))
            t.manifold_handles_upload(offs, ids[order])
            t.run_system("SOLVER")
            tw = handle_state(t, ids)
            t.close()
        w.manifold_handles_upload(offs, ids[order])
        w.run_system("SOLVER")
        out.append((handle_state(w, ids), tw, w.solver_forms()))
    w.close()
    return out
