"""GPU: the load schedule of k_color_pass's biased solve and relax pass (lane form; k_contacts.hip lane_pass).

The two passes issue their loads themselves -- headers and body indices, then the body gathers, then the point records -- take their arguments from a narrow block
(SolveArgs) and leave early on a point count of zero BEFORE the point records are loaded; the arithmetic is the solve's, untouched.  So every case here is a bitwise
comparison with the CPU oracle of the bodies, impulses_download and constraints_download after two steps of two substeps, on sets that reach the lane form's launches
(measure build, island blocks / level compaction / eight-lane form switched off; asserted through avn_solver_forms_get) and sit on the schedule's edges:
  * the first colour holds 1, 63, 64, 65, 511, 512 or 513 manifolds: a partial wave, the one-wave workgroup's edge, and the grid of eight workgroups (one per XCD eighth
    of k_color_pass's block mapping) and one manifold more;
  * point counts cycle 0..4, so lanes with nothing to solve sit inside live waves -- their rows, and bodies that ONLY such manifolds name, are part of the comparison: a
    lane that has nothing to solve writes nothing; one set has a whole wave of them;
  * a static body on side 1 of one manifold and on side 2 of another, a kinematic body, bodies without a SolverBody (odd flags);
  * friction zero on every third manifold (no tangent part: the c_pc records are loaded and never read), restitution on half (the restitution pass keeps the wide arguments);
  * warm-start impulses in every slot, or none;
  * ranges from the kernel arguments (host-uploaded set) and from device memory (handle mode), eager and replayed, f32 and f64.
No tolerance appears anywhere."""
import functools

import numpy as np
import pytest

import solver_forms_helpers as H
from helpers import F, hip_measure_lib, oracle_lib
from test_gpu_level_compaction import has_solver_body, make_case, state, upload

pytestmark = pytest.mark.gpu

LANE_ENV = {"AVN_ISLAND_BLOCKS": 0, "AVN_NO_LEVEL_COMPACTION": 1, "AVN_NO_OCT": 1}
SIZES = [1, 63, 64, 65, 511, 512, 513]
STEPS = 2
CA, CB, CC = 0, 4, 9


@functools.lru_cache(maxsize=None)
def schedule_case(n, idle_wave=False, warm=True):
    """bodies: 0 static, 1 and 2 kinematic, the others dynamic with odd flags mixed in.  Colour CA: n manifolds on body pairs of their own (3 + 2 i, 4 + 2 i).  Colour CB: five
    manifolds -- one on body 3, one with the static body on side 1, one with it on side 2 (both with points to solve).  Colour CC: 70 manifolds that share bodies with CA's pairs
    as far as those reach, one of them on a kinematic body.  Body 3 is in all three colours."""
    fresh = iter(range(3 + 2 * n, 10 ** 9))
    a = [(3 + 2 * i, 4 + 2 * i) for i in range(n)]
    b = [(3, next(fresh))] + [(next(fresh), next(fresh)) for _ in range(4)]
    live = [j for j in range(1, 5) if (n + j) % 5 != 0]   # (point counts cycle with the manifold's index: CB's manifolds are n .. n + 4)
    b[live[0]] = (0, b[live[0]][1]); b[live[1]] = (b[live[1]][0], 0)
    c = [(next(fresh), 3 if k == 0 else 4 + 2 * k) if k < n else (next(fresh), next(fresh)) for k in range(70)]
    c[-2] = (1, c[-2][1])
    case = make_case(300 + n, next(fresh), {CA: a, CB: b, CC: c}, n_static=1, n_kinematic=2, point_counts="cycle", odd=True)
    mf = dict(case["mf"]); m = len(mf["body1"])
    assert m == n + 75 and list(np.diff(np.asarray(case["offs"], np.int64))[[CA, CB, CC]]) == [n, 5, 70]
    if idle_wave:
        pc = np.array(mf["point_count"], copy=True); pc[64:128] = 0; mf["point_count"] = pc; case["mf"] = mf
    fr = np.array(case["friction"], copy=True); fr[1::3] = 0.0; case["friction"] = fr
    if not warm:
        case["warm_n"] = np.zeros((m, 4)); case["warm_t"] = np.zeros((m, 4, 2))
    # what the set is meant to hold
    pc, b1, b2 = np.asarray(mf["point_count"]), np.asarray(mf["body1"]), np.asarray(mf["body2"])
    sb = has_solver_body(case["bodies"])
    assert case["bodies"]["rb_type"][0] == F.RB_STATIC and not sb[0]
    assert ((b1 == 0) & (pc > 0)).any() and ((b2 == 0) & (pc > 0)).any(), "the static body on either side of a manifold that is solved"
    for col in (a, b, c):   # a valid colouring: a body with a SolverBody is in at most one manifold of a colour
        named = np.array(col).reshape(-1)
        assert len(set(named[sb[named]])) == len(named[sb[named]])
    assert set(np.unique(pc)) == {0, 1, 2, 3, 4} and (fr[pc > 0] == 0).any() and (fr[pc > 0] > 0).any()
    if n >= 63:
        solved = set(b1[pc > 0]) | set(b2[pc > 0])
        idle_only = (set(b1[pc == 0]) | set(b2[pc == 0])) - solved
        assert any(sb[i] for i in idle_only), "bodies that only manifolds without points name"
    if idle_wave:
        assert n >= 128 and not pc[64:128].any() and pc[:64].any() and pc[128:192].any()
    return case


def assert_lane(f, ranges_from, what):
    launched = [x for x in f.colour_form if x != F.FORM_NONE]
    assert f.island_blocks == 0 and len(launched) == 3 and set(launched) == {F.COLOUR_FORM_LANE}, f"{what}: expected three lane-form colour launches, got {list(f.colour_form)}"
    assert [f.colour_form[c] for c in (CA, CB, CC)] == [F.COLOUR_FORM_LANE] * 3 and f.colour_ranges_from == ranges_from and f.overflow_form == F.FORM_NONE, what


def run_arguments(lib, bits, case, use_graph, env=None):
    w = H.make_world(lib, bits, case["bodies"], use_graph, env)
    upload(w, case)
    for _ in range(STEPS):
        w.step()
    got, forms = state(w), w.solver_forms()
    w.close()
    return got, forms


@functools.lru_cache(maxsize=None)
def oracle_arguments(n, bits, idle_wave=False, warm=True):
    return run_arguments(oracle_lib(), bits, schedule_case(n, idle_wave, warm), 0)[0]


def lists_of(case):
    return [(np.asarray(case["offs"], np.uint32), np.arange(len(case["mf"]["body1"])))] * STEPS


@functools.lru_cache(maxsize=None)
def oracle_handles(n, bits):
    case = schedule_case(n)
    return H.run_handle_script(oracle_lib(), bits, case, H.contact_ids(case), lists_of(case), 0)


def check_arguments(n, bits, use_graph, idle_wave=False, warm=True):
    what = f"n = {n}, f{bits}, {'replayed' if use_graph else 'eager'}, ranges from the arguments" + (", a whole wave without points" if idle_wave else "") + ("" if warm else ", no warm start")
    got, forms = run_arguments(hip_measure_lib(), bits, schedule_case(n, idle_wave, warm), use_graph, LANE_ENV)
    assert_lane(forms, F.RANGES_FROM_ARGUMENTS, what)
    assert forms.graph_replays == (STEPS if use_graph else 0), what
    H.same(got, oracle_arguments(n, bits, idle_wave, warm), what + ": vs the oracle")
    assert float(np.abs(got["impulses"]["normal_impulse"]).max()) > 0.0


@pytest.mark.parametrize("use_graph", [1, 0], ids=["replayed", "eager"])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", SIZES)
def test_lane_form_ranges_from_arguments(n, bits, use_graph):
    check_arguments(n, bits, use_graph)


@pytest.mark.parametrize("use_graph", [1, 0], ids=["replayed", "eager"])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", SIZES)
def test_lane_form_ranges_from_device_memory(n, bits, use_graph):
    case = schedule_case(n)
    what = f"n = {n}, f{bits}, {'replayed' if use_graph else 'eager'}, handle mode"
    got = H.run_handle_script(hip_measure_lib(), bits, case, H.contact_ids(case), lists_of(case), use_graph, LANE_ENV)
    want = oracle_handles(n, bits)
    for k in range(STEPS):
        assert_lane(got[k][2], F.RANGES_FROM_DEVICE, f"{what}, step {k}")
        H.same(got[k][0], want[k][0], f"{what}, step {k}: vs the oracle")
    assert float(np.abs(got[-1][0]["impulses"]["normal_impulse"]).max()) > 0.0


@pytest.mark.parametrize("use_graph", [1, 0], ids=["replayed", "eager"])
@pytest.mark.parametrize("bits", [32, 64])
def test_a_whole_wave_with_nothing_to_solve(bits, use_graph):
    check_arguments(513, bits, use_graph, idle_wave=True)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [65, 513])
def test_without_warm_start_impulses(n, bits):
    check_arguments(n, bits, 1, warm=False)
