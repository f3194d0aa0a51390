"""Shared by tests/test_dshard_cpu.py and tests/test_gpu_dshard.py: the DEVICE closed loop sharded by islands (avn_dshard_*) against the single world."""
import numpy as np

from avian_amd import shard
from helpers import F


def make_worlds(lib, bits, bodies, colliders, owner, n_ranks, substeps=4):
    """the single world and one world per rank: every world holds every body; rank r simulates the bodies with owner == r"""
    def one():
        w = F.World(lib, F.default_config(bits, substeps=substeps))
        w.bodies_upload(**bodies); w.colliders_upload(**colliders); w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
        w.pipeline_enable()
        return w
    ref = one()
    ranks = []
    for r in range(n_ranks):
        w = one()
        w.dshard_enable(n_ranks, r, owner)
        ranks.append(w)
    return ref, ranks


def compare(step, ref, ranks, owner, rows=False):
    """every rank: the replicated colour lists WITH ORDER, the new pairs and their ids, the counters; the bodies it simulates; and -- the exchange -- every body"""
    off, handles = ref.pipeline_handles()
    pr, ir = ref.pairs_get(), ref.pipeline_new_pair_ids()
    edge_owner = ref.__dict__.setdefault("_edge_owner", {})   # ContactId -> the rank of its non-static body, kept up to date EVERY step (ids are reused)
    for p, i in zip(pr, ir):
        o1, o2 = owner[p["body1"]], owner[p["body2"]]
        edge_owner[int(i)] = int(o1 if o1 >= 0 else o2)
    sr = ref.pipeline_stats()
    br = ref.bodies_download()
    total = 0
    for r, w in enumerate(ranks):
        o2, h2 = w.pipeline_handles()
        assert np.array_equal(off, o2) and np.array_equal(handles, h2), f"step {step}: rank {r}'s replicated colour lists differ from the single world's (content or order)"
        assert np.array_equal(pr, w.pairs_get()) and np.array_equal(ir, w.pipeline_new_pair_ids()), f"step {step}: rank {r}: new pairs / ContactIds differ"
        s = w.pipeline_stats()
        for f in ("pairs_added", "pairs_removed", "manifolds_pushed", "manifolds_popped", "last_status_changes", "active_pairs"):
            assert getattr(s, f) == getattr(sr, f), f"step {step}: rank {r}: pipeline_stats.{f} {getattr(s, f)} != {getattr(sr, f)}"
        b = w.bodies_download()
        for k in br:
            assert np.array_equal(br[k], b[k]), f"step {step}: rank {r}: bodies.{k} differ from the single world's (own bodies: the solver; the others: the exchange)"
        d = w.dshard_stats()
        assert d.global_manifolds == len(handles) and d.own_bodies == int((owner == r).sum())
        total += d.own_manifolds
        if rows and len(handles):
            ids = np.unique(handles)
            mine = np.array([edge_owner.get(int(i)) == r for i in ids])
            ro, rw = ref.contacts_download(ids[mine]), w.contacts_download(ids[mine])
            for k in ro:
                assert np.array_equal(ro[k], rw[k]), f"step {step}: rank {r}: contact rows {k} of its own pairs differ"
    assert total == len(handles), f"step {step}: the ranks' shares of the colour lists do not add up to the single world's ({total} vs {len(handles)})"


def run(lib, bits, bodies, colliders, owner, n_ranks, steps, substeps=4, rows_every=0):
    ref, ranks = make_worlds(lib, bits, bodies, colliders, owner, n_ranks, substeps)
    for s in range(steps):
        ref.step()
        shard.dshard_step_in_process(ranks)
        compare(s, ref, ranks, owner, rows=bool(rows_every) and s % rows_every == rows_every - 1)
    return ref, ranks


ERR_STATE = 6   # AVN_ERR_STATE


def with_state(bodies, state, body=None, dv=None):
    """the upload arrays `bodies` holding a downloaded state, one body's linear velocity changed by dv"""
    out = dict(bodies)
    for k in ("position", "rotation", "linear_velocity", "angular_velocity"):
        out[k] = np.array(state[k], copy=True)
    if body is not None:
        out["linear_velocity"][body] += np.asarray(dv, out["linear_velocity"].dtype)
    return out


def assert_solver_bodies_are_the_ranks_own(step, ranks, owner):
    """a rank holds a SolverBody for exactly the bodies it simulates (avn_solver_bodies_download: flags bit 31 = the body has none).  The lists, ids and bodies alone do
    not show a rank that simulates everybody's bodies: its share of the colour lists is cut by the owner table, and the exchange overwrites the foreign bodies every step."""
    for r, w in enumerate(ranks):
        has = (w.solver_bodies_download()["flags"] & 0x80000000) == 0
        assert np.array_equal(has, owner == r), f"step {step}: rank {r} holds SolverBodies for bodies {np.flatnonzero(has & (owner != r))[:8]} it does not simulate"


def reupload_case(lib, bits, bodies, colliders, owner, n_ranks, body, dv, also=(), control=None, before=20, after=10):
    """avn_bodies_upload between sharded steps (a host that teleports or kicks a body): every rank and the single world upload the downloaded state with one velocity
    changed.  The ranks must go on equal to the single world (compare: lists, ids, counters, every body, shares that add up) and must still own only their share.
    also: unsharded worlds of other libraries given the same edit, bodies compared bit for bit; control: an unsharded world that uploads the state WITHOUT the
    change -- it must differ afterwards, or the edit would not matter."""
    ref, ranks = make_worlds(lib, bits, bodies, colliders, owner, n_ranks)
    extra = list(also) + ([control] if control is not None else [])
    for s in range(before):
        ref.step()
        for w in extra: w.step()
        shard.dshard_step_in_process(ranks)
        compare(s, ref, ranks, owner)
    assert_solver_bodies_are_the_ranks_own(before - 1, ranks, owner)
    share = [w.dshard_stats().own_manifolds for w in ranks]
    total = ranks[0].dshard_stats().global_manifolds
    assert total > 20 and all(0 < x < total for x in share), "every rank must hold a proper share of the manifolds before the upload"
    state = ref.bodies_download()
    edited = with_state(bodies, state, body, dv)
    for w in [ref] + ranks + list(also):
        w.bodies_upload(**edited)
    if control is not None:
        control.bodies_upload(**with_state(bodies, state))
    for s in range(before, before + after):
        ref.step()
        for w in extra: w.step()
        shard.dshard_step_in_process(ranks)
        compare(s, ref, ranks, owner, rows=(s == before + after - 1))
        br = ref.bodies_download()
        for w in also:
            for k, v in w.bodies_download().items():
                assert np.array_equal(br[k], v), f"step {s}: bodies.{k} differ from the unsharded world of the other library"
        assert_solver_bodies_are_the_ranks_own(s, ranks, owner)
        d = [w.dshard_stats() for w in ranks]
        assert all(0 < x.own_manifolds < x.global_manifolds and x.own_bodies == int((owner == r).sum()) for r, x in enumerate(d)), \
            f"step {s}: a rank no longer owns only its share: {[(x.own_manifolds, x.global_manifolds) for x in d]}"
    if control is not None:
        a, b = ref.bodies_download(), control.bodies_download()
        assert any(not np.array_equal(a[k], b[k]) for k in a), "the edited velocity changed no bit: the script cannot see a dropped upload"
    return ref, ranks


def refusals_case(lib, bits, bodies, colliders, owner, n_ranks, enable_is_refused, steps=12, after=6):
    """Inside the sharded loop: another body count is refused with AVN_ERR_STATE (the owner table is per body), and -- on the product -- so is avn_dshard_enable once a
    step has created a pair.  Neither changes anything: the loop goes on equal to the single world."""
    import pytest
    ref, ranks = make_worlds(lib, bits, bodies, colliders, owner, n_ranks)
    for s in range(steps):
        ref.step(); shard.dshard_step_in_process(ranks); compare(s, ref, ranks, owner)
    assert ref.pipeline_stats().pairs_added > 0
    state = ref.bodies_download()
    same = with_state(bodies, state)
    grown = {k: np.concatenate([np.asarray(v), np.asarray(v)[-1:]]) for k, v in same.items()}
    grown["position"][-1, 0] += 100.0
    shrunk = {k: np.asarray(v)[:-1] for k, v in same.items()}
    for w in ranks:
        for other in (grown, shrunk):
            with pytest.raises(F.AvnError) as e:
                w.bodies_upload(**other)
            assert e.value.status == ERR_STATE, e.value
        if enable_is_refused:
            with pytest.raises(F.AvnError) as e:
                w.dshard_enable(n_ranks, w.dshard_stats().rank, owner)
            assert e.value.status == ERR_STATE, e.value
    for s in range(steps, steps + after):
        ref.step(); shard.dshard_step_in_process(ranks); compare(s, ref, ranks, owner)
