"""GPU: every form of the contact solve, each proven to have run.  The host picks a kernel per launch range and for the overflow list from thresholds with
hysteresis, grids kept with slack and hand-kept flags (world/contacts.hpp set_color_offsets, world/systems.hpp); every choice is "bit-identical either way" and
a wrong one raises no error.  avn_solver_forms_get reports what the last enqueued or captured substep loop contained, so every test here
  1. asserts the read-out -- which form ran, on which grid, how often the graph was captured -- against HostRule (tests/solver_forms_helpers.py), a restatement of
     the host's rule that shares nothing with the library, and then
  2. compares bodies, impulses_download and constraints_download bit for bit with the CPU oracle and with the same set solved in the OTHER form.
No tolerance appears anywhere.  Sets come from make_case of tests/test_gpu_level_compaction.py: point counts cycling 0..4, a static, kinematic and odd-flag bodies,
restitution on half the rows, warm-start impulses.  Two steps of two substeps, replayed and eager.  Switches (AVN_*) exist in the `make measure` build only."""
import functools

import numpy as np
import pytest

import solver_forms_helpers as H
from helpers import F, hip_lib, hip_measure_lib, oracle_lib
from test_gpu_level_compaction import columns_case, has_solver_body, make_case, state, tile_case, upload

pytestmark = pytest.mark.gpu

NC = H.NC
LANE, OCT, NONE = F.COLOUR_FORM_LANE, F.COLOUR_FORM_OCT, F.FORM_NONE
NO_ISLANDS = {"AVN_ISLAND_BLOCKS": 0}
STEPS = 2
CA, CB, CC = 0, 4, 9   # the three colours of the oct sets


def names(forms):
    return "".join(".lo"[f] for f in forms)


def check_colours(f, rule_out, use_graph, what, ranges_from):
    """the read-out of colours 0..22 against HostRule; the restitution pass always takes the lane form"""
    form, grid, captures, why = rule_out
    got_form, got_grid, got_rest = H.forms_of(f)
    print(f"{what}: forms {names(got_form)} expected {names(form)} | restitution {names(got_rest)} | grids {[g for g in got_grid if g]} expected {[g for g in grid if g]} | "
          f"captures {f.graph_captures} expected {captures if use_graph else 0} replays {f.graph_replays} | {'; '.join(why) or 'no capture'}")
    assert got_form == form, f"{what}: colour forms {names(got_form)}, expected {names(form)} (. none, l lane, o oct)"
    assert got_grid == grid, f"{what}: captured grids {got_grid}, expected {grid}"
    assert got_rest == [LANE if x != NONE else NONE for x in form], f"{what}: the restitution pass has a lane form only: {names(got_rest)}"
    assert f.colour_ranges_from == (ranges_from if any(form) else NONE), what
    assert f.graph_captures == (captures if use_graph else 0), f"{what}: {f.graph_captures} graph captures, expected {captures if use_graph else 0}"
    assert f.island_blocks == 0 and f.island_cache_records == 0 and f.warm_start_form == F.WARM_START_FORM_LANE and f.overflow_form == NONE, what


# ---- a. oct against lane at the oct kernel's edges ------------------------------------------------------------------------------------------------------------------------
# k_color_pass_oct: 8 manifolds per wave (tile), the colour's tiles split in eighths over the XCDs (per = ceil(tiles / 8) tiles per XCD; workgroup b serves tile
# (b % 8) * per + b / 8 and leaves when b / 8 >= per), a manifold past the end leaves with its eight lanes.  k_color_pass: 64 manifolds per workgroup, grids in
# multiples of 8.  n = 1, 7: a partial tile; 8, 9: one tile and one manifold more; 63, 64, 65: exactly 8 tiles (per = 1) and the lane form's workgroup edge; 72:
# 9 tiles (per = 2, most rows idle); 511, 512, 513: the lane form's grid of 8 workgroups and one more.
OCT_SIZES = [1, 7, 8, 9, 63, 64, 65, 72, 511, 512, 513]


@functools.lru_cache(maxsize=None)
def oct_case(n):
    """bodies: 0 static, 1 and 2 kinematic, the others dynamic (odd flags mixed in).  Colour CA: n manifolds on body pairs of their own (3 + 2 i, 4 + 2 i).  Colour CB: 5 and
    colour CC: 70 manifolds that share bodies with colour CA's pairs as far as those reach, with the ground and the kinematic bodies, and are otherwise on fresh bodies.
    Body 3 is in all three colours, so the level compaction of the release build finds nothing to regroup and colour = launch range in every run."""
    fresh = iter(range(3 + 2 * n, 10 ** 9))
    a = [(3 + 2 * i, 4 + 2 * i) for i in range(n)]
    b = [(3 + 2 * k, next(fresh)) if k < n else (next(fresh), next(fresh)) for k in range(5)]
    c = [(next(fresh), 3 + 2 * k if k == 0 else 4 + 2 * k) if k < n else (next(fresh), next(fresh)) for k in range(70)]
    b[4] = (0, b[4][1]) if n <= 4 else b[4]          # the ground (as many manifolds as it likes) ...
    c[-1] = (c[-1][0], 0); c[-2] = (1, c[-2][1]); b[3] = (b[3][0], 2) if n <= 3 else (next(fresh), 2)   # ... and each kinematic body once
    case = make_case(100 + n, next(fresh), {CA: a, CB: b, CC: c}, n_static=1, n_kinematic=2, point_counts="cycle", odd=True)
    sizes = np.diff(np.asarray(case["offs"], np.int64))
    assert (sizes[CA], sizes[CB], sizes[CC]) == (n, 5, 70) and sizes.sum() == n + 75
    sb = has_solver_body(case["bodies"])
    for col in (a, b, c):   # a valid colouring: a body with a SolverBody is in at most one manifold of a colour
        named = np.array(col).reshape(-1)
        assert len(set(named[sb[named]])) == len(named[sb[named]])
    assert set(np.unique(case["mf"]["point_count"])) == ({0, 1, 2, 3, 4} if n + 75 >= 5 else set())
    return case


def run_host(lib, bits, case, use_graph, env=None):
    w = H.make_world(lib, bits, case["bodies"], use_graph, env)
    upload(w, case)
    for _ in range(STEPS):
        w.step()
    return w, state(w)


@functools.lru_cache(maxsize=None)
def oct_oracle(n, bits):
    return run_host(oracle_lib(), bits, oct_case(n), 0)[1]


@pytest.mark.parametrize("use_graph", [1, 0], ids=["replayed", "eager"])
@pytest.mark.parametrize("n", OCT_SIZES)
def test_oct_against_lane_at_the_oct_kernels_edges(n, use_graph):
    case = oct_case(n)
    off = dict(NO_ISLANDS, AVN_NO_LEVEL_COMPACTION=1)
    runs = {"oct": (hip_measure_lib(), 32, off, True), "lane": (hip_measure_lib(), 32, dict(off, AVN_NO_OCT=1), False), "f64": (hip_lib(), 64, None, False)}
    got = {}
    for name, (lib, bits, env, oct_enabled) in runs.items():
        w, got[name] = run_host(lib, bits, case, use_graph, env)
        want = H.HostRule(bits == 32, handles=False, oct_enabled=oct_enabled).upload(case["offs"])
        assert [want[0][c] for c in (CA, CB, CC)] == [OCT if name == "oct" else LANE] * 3 and sum(x != NONE for x in want[0]) == 3
        check_colours(w.solver_forms(), want, use_graph, f"n = {n}, {name}", F.RANGES_FROM_ARGUMENTS)
        assert w.solver_forms().graph_replays == (STEPS if use_graph else 0)
        lv = w.level_compaction_stats()
        assert lv.state == (F.LEVELS_EARLY_OUT if name == "f64" else F.LEVELS_OFF), "colour = launch range"
        w.close()
    H.same(got["oct"], oct_oracle(n, 32), f"n = {n}: oct form vs the oracle")
    H.same(got["lane"], oct_oracle(n, 32), f"n = {n}: lane form vs the oracle")
    H.same(got["oct"], got["lane"], f"n = {n}: oct form vs lane form")
    H.same(got["f64"], oct_oracle(n, 64), f"n = {n}: f64 (lane form) vs the f64 oracle")


# ---- b. the same sets in handle mode: the kernels read the ranges from device memory -------------------------------------------------------------------------------------
def colour_major(case):
    return np.asarray(case["offs"], np.uint32), np.arange(len(case["mf"]["body1"]))


@pytest.mark.parametrize("n", [7, 65, 513])
def test_oct_against_lane_in_handle_mode(n):
    case = oct_case(n)
    ids = H.contact_ids(case)
    lists = [colour_major(case)] * STEPS
    oracle = {bits: H.run_handle_script(oracle_lib(), bits, case, ids, lists, 0) for bits in (32, 64)}
    for use_graph in (1, 0):
        runs = {"oct": (hip_measure_lib(), 32, NO_ISLANDS, True), "lane": (hip_measure_lib(), 32, dict(NO_ISLANDS, AVN_NO_OCT=1), False), "f64": (hip_lib(), 64, None, False)}
        got = {}
        for name, (lib, bits, env, oct_enabled) in runs.items():
            got[name] = H.run_handle_script(lib, bits, case, ids, lists, use_graph, env)
            rule = H.HostRule(bits == 32, handles=True, oct_enabled=oct_enabled)
            for k in range(STEPS):
                check_colours(got[name][k][2], rule.upload(lists[k][0]), use_graph, f"handles, n = {n}, {name}, use_graph = {use_graph}, step {k}", F.RANGES_FROM_DEVICE)
        for k in range(STEPS):
            H.same(got["oct"][k][0], oracle[32][k][0], f"handles, n = {n}, step {k}: oct form vs the oracle")
            H.same(got["lane"][k][0], oracle[32][k][0], f"handles, n = {n}, step {k}: lane form vs the oracle")
            H.same(got["oct"][k][0], got["lane"][k][0], f"handles, n = {n}, step {k}: oct form vs lane form")
            H.same(got["f64"][k][0], oracle[64][k][0], f"handles, n = {n}, step {k}: f64 vs the f64 oracle")


# ---- c, d. state that carries from one upload to the next under a captured graph: the hysteresis band and the grid slack ----------------------------------------------------
RESERVOIR = 15


def sized_case(seed, n_max, extra):
    """n_max manifolds on body pairs of their own that a step puts into colour CA (the first `size` of them) or into colour RESERVOIR (the others), so that the number
    of manifolds -- which alone would make the host capture again -- stays the same from step to step; `extra` more manifolds on pairs of their own live in
    RESERVOIR, which keeps that colour on one side of every threshold of the script; colours CB and CC as in oct_case."""
    fresh = iter(range(3 + 2 * (n_max + extra), 10 ** 9))
    a = [(3 + 2 * i, 4 + 2 * i) for i in range(n_max + extra)]
    b = [(3 + 2 * k, next(fresh)) for k in range(5)]
    c = [(next(fresh), 3 if k == 0 else 4 + 2 * k) for k in range(70)]
    c[-1] = (c[-1][0], 0); c[-2] = (1, c[-2][1]); b[3] = (next(fresh), 2)
    case = make_case(seed, next(fresh), {CA: a, CB: b, CC: c}, n_static=1, n_kinematic=2, point_counts="cycle", odd=True)
    m = n_max + extra

    def lists(size):
        offs = np.zeros(F.GRAPH_COLOR_COUNT + 1, np.uint32)
        counts = {CA: size, CB: 5, CC: 70, RESERVOIR: m - size}
        for col in range(F.GRAPH_COLOR_COUNT):
            offs[col + 1] = offs[col] + counts.get(col, 0)
        order = np.concatenate([np.arange(size), m + np.arange(5), m + 5 + np.arange(70), np.arange(size, m)])   # colour order: CA < CB < CC < RESERVOIR
        assert CA < CB < CC < RESERVOIR and offs[-1] == m + 75 == len(order)
        return offs, order
    return case, lists


def judge_sized_script(case, lists, sizes, env, rule, expect):
    """expect: per step (form of colour CA, captures); the rule must agree with it before anything runs on the device"""
    ids = H.contact_ids(case)
    script = [lists(s) for s in sizes]
    want = [rule.upload(offs) for offs, _ in script]
    for s, (form, grid, captures, why) in zip(sizes, want):
        print(f"HostRule: colour {CA} holds {s}: form {names(form)[CA]}, grid {grid[CA]}, reservoir {names(form)[RESERVOIR]} grid {grid[RESERVOIR]}, captures so far {captures}: {'; '.join(why) or 'no capture'}")
    assert [(w[0][CA], w[2]) for w in want] == expect, "the sizes of the script do not take the branches they are meant to"
    got = H.run_handle_script(hip_measure_lib(), 32, case, ids, script, 1, env, twin=True)
    oracle = H.run_handle_script(oracle_lib(), 32, case, ids, script, 0)
    for k, s in enumerate(sizes):
        what = f"step {k + 1} (colour {CA} holds {s})"
        check_colours(got[k][2], want[k], 1, what, F.RANGES_FROM_DEVICE)
        assert got[k][2].graph_replays == k + 1
        H.same(got[k][0], oracle[k][0], what + ": vs the oracle through the same script")
        H.same(got[k][0], got[k][1], what + ": the sequence left stale state (vs a fresh world built at this step)")


def test_hysteresis_band_of_the_oct_form():
    """thresholds 40 / 80 (AVN_OCT_ON / AVN_OCT_OFF).  At 60 the form is the one the colour had: the fresh world of step 2 runs lane where the sequenced one runs oct, the
    fresh world of step 4 oct where the sequenced one runs lane.  The graph is captured at the start and with every flip, and never inside the band.  The reservoir
    (100 .. 170 manifolds) stays lane throughout; every grid is 8 workgroups throughout."""
    case, lists = sized_case(61, 100, 100)
    env = dict(NO_ISLANDS, AVN_OCT_ON=40, AVN_OCT_OFF=80)
    judge_sized_script(case, lists, [30, 60, 100, 60, 30], env, H.HostRule(True, handles=True, oct_on=40, oct_off=80),
                       [(OCT, 1), (OCT, 1), (LANE, 2), (LANE, 2), (OCT, 3)])
    fresh = H.HostRule(True, handles=True, oct_on=40, oct_off=80).upload(lists(60)[0])
    assert fresh[0][CA] == LANE, "a fresh world at 60 has the other history"


def test_grid_slack_of_a_colour():
    """grid = color_grid_blocks(cnt + cnt / 4 + 64), captured again when need > grid or grid > 4 * need + 64.  Grids come in multiples of 8 workgroups = 512
    manifolds, so a colour of 100 is outgrown only above 512 manifolds (the issue's 200 still fits: 600 here), and a grid is shed only above 4 * 8 + 64 = 96 workgroups
    (5000 -> 104).  100 -> 120: inside the grid, no capture; -> 600: outgrown; -> 5000: outgrown; -> 100: 104 > 96, shrunk.  The reservoir (2000 .. 6900) keeps its
    first grid (136: never outgrown, 136 <= 4 * 32 + 64) and every colour stays under the oct threshold of 12 288."""
    case, lists = sized_case(62, 5000, 2000)
    judge_sized_script(case, lists, [100, 120, 600, 5000, 100], NO_ISLANDS, H.HostRule(True, handles=True), [(OCT, 1), (OCT, 1), (OCT, 2), (OCT, 3), (OCT, 4)])


# ---- e. level launches in f32: the hand-made sets of the level-compaction tests, kept off the island blocks -------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [1, 0], ids=["replayed", "eager"])
@pytest.mark.parametrize("which", ["columns", "tile_255", "tile_257"])
def test_level_launches_in_f32(which, use_graph):
    case = columns_case() if which == "columns" else tile_case(300, 300, 255 if which == "tile_255" else 257, 40)
    w, got = run_host(hip_measure_lib(), 32, case, use_graph, NO_ISLANDS)
    lv, f = w.level_compaction_stats(), w.solver_forms()
    assert lv.state == F.LEVELS_COMPACTED and 2 <= lv.levels < lv.colours
    level_offs = np.concatenate([[0], np.cumsum(list(lv.sizes)), [lv.overflow_first + lv.overflow_count]])   # the ranges the solver runs: levels, then the (empty) overflow list
    want = H.HostRule(True, handles=False).upload(level_offs)
    assert want[0] == [OCT] * lv.levels + [NONE] * (NC - lv.levels), "one launch range per level"
    check_colours(f, want, use_graph, f"{which}: level launches", F.RANGES_FROM_ARGUMENTS)
    d, default = run_host(hip_lib(), 32, case, use_graph)
    fd = d.solver_forms()
    assert fd.island_blocks > 0 and fd.warm_start_form == F.WARM_START_FORM_COLOURS and not any(fd.colour_form) and fd.graph_captures == 0, "the default world takes the island blocks"
    n_bodies, m = len(case["bodies"]["rb_type"]), len(case["mf"]["body1"])
    if 6 * n_bodies + 20 * (m + 1) <= 4088:   # (bodies and constraint records of the whole set fit one block's LDS, so they fit however the islands are packed)
        assert which == "columns" and fd.island_cache_records == 1
    if fd.island_blocks * 204 < m:            # (20 records per manifold in 4088: a block of the CACHE variant holds at most 204)
        assert fd.island_cache_records == 0
    H.same(got, run_host(oracle_lib(), 32, case, 0)[1], f"{which}: level launches vs the oracle")
    H.same(got, default, f"{which}: level launches vs island blocks")


def test_read_out_rejects_a_wrong_struct_size():
    w = H.make_world(hip_lib(), 32, oct_case(7)["bodies"], 1)
    f = w.solver_forms()
    assert not any(f.colour_form) and f.graph_captures == f.graph_replays == 0, "nothing enqueued yet"
    bad = F.avn_solver_forms(4)
    assert hip_lib().dll.avn_solver_forms_get(w.handle, F.C.byref(bad)) == 1   # AVN_ERR_BAD_ARG
