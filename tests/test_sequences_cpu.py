"""CPU: every re-upload script of tests/sequence_helpers.py on the oracle -- the sequenced world against a FRESH oracle world at every checkpoint (the oracle's own
re-upload behaviour: it must hold no stale state either), and the mutation control: with any ONE upload / config change skipped the next checkpoint's bodies differ,
so each script can see a cache that ignores that operation.  This validates the scripts tests/test_gpu_sequences.py runs on the device."""
import pytest

import sequence_helpers as S
from helpers import oracle_lib


@pytest.mark.parametrize("name", sorted(S.HOST_SCRIPTS))
def test_oracle_sequence_equals_fresh_worlds_and_every_mutation_matters(name):
    lib = oracle_lib()
    script = S.host_script(name)
    n_check = sum(1 for o in script if o.kind == "step" and o.checkpoint)
    for bits in (32, 64):
        got = S.run_script(lib, bits, script, 0, twin=True)
        assert len(got) == n_check >= 3
        for k, c in enumerate(got):
            S.assert_twin(c, f"{name} f{bits} checkpoint {k}: sequenced oracle vs fresh oracle")
        assert any(S.bodies_differ(got[0]["seq"], c["seq"]) for c in got[1:])
    full, idle = S.mutation_controls(lib, 32, script)
    assert not idle, f"{name}: operations that change nothing: {idle}"


@pytest.mark.parametrize("name", sorted(S.CLOSED_SCRIPTS))
def test_closed_loop_script_mutations_matter(name):
    """the closed-loop scripts on the oracle: every host action changes the bodies of the steps behind it"""
    idle = S.closed_mutation_controls(oracle_lib(), 32, S.CLOSED_SCRIPTS[name], S.closed_scene())
    assert not idle, f"{name}: operations that change nothing: {idle}"


def test_restart_of_the_closed_loop_equals_a_fresh_world():
    """avn_pipeline_enable(0) -> uploads -> (1) empties the contact table (header: avn_pipeline_enable): the restarted oracle world == a new world given the same
    uploads, for the steps behind the restart"""
    import numpy as np
    from helpers import F
    lib, scene = oracle_lib(), S.closed_scene()
    w = S.closed_world(lib, 32, 0, scene)
    for _ in range(12): w.step()
    kw = dict(scene["bodies"]); kw.update(w.bodies_download())
    S.op_restart(w, scene)
    tw = S.closed_world(lib, 32, 0, dict(bodies=kw, colliders=scene["colliders"]))
    for s in range(8):
        w.step(); tw.step()
        a, b = w.bodies_download(), tw.bodies_download()
        assert all(np.array_equal(a[k], b[k]) for k in a), s
        assert np.array_equal(w.pipeline_handles()[1], tw.pipeline_handles()[1]), s
