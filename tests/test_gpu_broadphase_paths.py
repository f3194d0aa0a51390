"""GPU: every interchangeable path of the broad phase (avian_amd/csrc/k_broadphase.hip), each PROVED to have run.

The paths are order-exact, so a pair list equal to the oracle's says nothing about which of them produced it: a scene that no longer reaches the path it was
written for keeps passing.  Every case here therefore asserts three things: the HIP interval order and pair sequence are those of reference_pairs (an independent
numpy statement, tests/broadphase_reference.py), they are the oracle's as well (wherever the oracle's cost allows), and avn_broad_phase_stats -- what the host
read back from the count pass -- reports the path the case claims: the chunks requested for long intervals (dispatch_model, the numpy restatement of
k_sweep_ranges), a repeated count pass, the form of the sort.  All comparisons are exact."""
import numpy as np
import pytest

import broadphase_reference as R
from helpers import F, assert_same, hip_lib, hip_measure_lib, oracle_lib

pytestmark = pytest.mark.gpu


def expected_unsorted(mn, mx, order_before):
    """k_interval_keys: the previous order is no longer ascending in this frame's keys (a non-finite AABB sorts last)."""
    ob = np.asarray(order_before, np.int64)
    finite = np.isfinite(mn[ob]).all(axis=1) & np.isfinite(mx[ob]).all(axis=1)
    key = np.where(finite, mn[ob, 0].astype(np.float64), np.inf)
    return int(np.any(key[:-1] > key[1:]))


def check_frame(bits, wh, wo, order_before, static, seen=None, bodies=None, colliders=None, route="auto"):
    """One frame on the HIP world (and on the oracle, when given): order and pairs against reference_pairs and the oracle, the path-independent stats.
    -> (aabb min, aabb max, order after, pairs [m, 2], stats)"""
    mn, mx, order, p = R.collect(wh, bodies, colliders)
    want, want_order = R.reference_pairs(mn, mx, order_before, static, np.arange(len(static)), existing=seen, route=route)
    assert np.array_equal(order, want_order), "interval order differs from reference_pairs"
    got = R.pairs_array(p)
    assert got.shape == want.shape and np.array_equal(got, want), f"pair sequence differs from reference_pairs ({len(got)} vs {len(want)} pairs)"
    assert np.array_equal(p["body1"], p["collider1"].astype(np.int32)) and np.array_equal(p["body2"], p["collider2"].astype(np.int32))
    assert np.all(p["flags"] == F.PAIR_GENERATE_CONSTRAINTS) and np.all(p["reserved"] == 0)
    if wo is not None:
        mo, xo, oo, po = R.collect(wo, bodies, colliders)
        assert_same(mo, mn, "aabb.min vs oracle"); assert_same(xo, mx, "aabb.max vs oracle")
        assert np.array_equal(oo, order), "interval order differs from the oracle"
        assert np.array_equal(po, p), "pair records differ from the oracle"
    st = wh.broad_phase_stats()
    unsorted = expected_unsorted(mn, mx, order_before)
    assert (st.intervals, st.dropped, st.pairs) == (len(order_before), len(order_before) - len(order), len(want))
    assert st.unsorted == unsorted and st.sort_form == (R.sort_form(len(order_before), bits) if unsorted else F.SORT_FORM_NONE)
    return mn, mx, order, want, st


def worlds(bits, oracle=True, lib=None, **cfg):
    return F.World(lib or hip_lib(), F.default_config(bits, **cfg)), (F.World(oracle_lib(), F.default_config(bits, **cfg)) if oracle else None)


def strip_case(bits, N, hx, planks, oracle=True, lib=None, nan_at=None):
    pos, he, static = R.strip(N, 1 / 32, hx, planks)
    if nan_at is not None:
        pos[nan_at, 1] = np.nan
    bodies, colliders, static = R.world_tables(pos, he, static)
    wh, wo = worlds(bits, oracle, lib)
    n = len(pos)
    mn, mx, order, want, st = check_frame(bits, wh, wo, np.arange(n), static, bodies=bodies, colliders=colliders)
    strip_case.static = static
    return wh, wo, mn, mx, order, want, st, R.dispatch_model(mn[:, 0], mx[:, 0], order)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the relative rule: len > 256 && len > 4 * others, others = (wave sum - len) / 63
RELATIVE = [   # hx, plank_at, L, others, long -- plank_at is the plank's position in the sorted order (lane = plank_at % 64)
    (0.05, 64, 256, 3, False), (0.05, 64, 257, 3, True),          # lane 0, at SW_LONG_MIN (4 * others = 12 is far below)
    (1.25, 128, 320, 80, False), (1.25, 128, 321, 80, True),      # lane 0, at 4 * others
    (1.25, 191, 324, 81, False), (1.25, 191, 325, 81, True),      # lane 63: the 63 boxes before it all count the plank among their candidates
    (0.05, 970, 30, None, False),                                 # in the ragged last wave (41 of 64 lanes): fewer than 64 followers exist, never long
]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("hx,plank_at,L,others,long", RELATIVE)
def test_relative_rule_at_its_thresholds(bits, hx, plank_at, L, others, long):
    wh, wo, mn, mx, order, want, st, m = strip_case(bits, 1000, hx, [(plank_at, L)])
    at = int(np.flatnonzero(order == 1000)[0])
    assert at == plank_at and m["length"][at] == L, "the scene: the plank sits at plank_at with exactly L candidates"
    assert others is None or m["others"][at] == others
    assert m["n_long"] == int(long) and not m["absolute"].any()
    assert st.long_chunks == m["long_chunks"] == (-(-L // 512) if long else 0) and st.long_retries == 0
    assert (want[:, 0] == 1000).sum() > L // 3, "the plank pairs with many of its candidates (not the last row's, not the static boxes)"


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("L", [257, 511, 512, 513, 1025])
def test_long_interval_chunk_edges(bits, L):
    """k_sweep_long walks a chunk 256 candidates at a time: a second iteration holding one candidate (257), a full chunk less one, a full chunk, a last
    chunk of one (513, 1025)."""
    wh, wo, mn, mx, order, want, st, m = strip_case(bits, 1200, 0.05, [(64, L)])
    assert m["n_long"] == 1 and m["length"][64] == L
    assert st.long_chunks == m["long_chunks"] == -(-L // 512) and st.long_retries == 0


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("planks,chunks", [([(70, 32769)], [65]), ([(70, 32769), (200, 1025)], [3, 65])])
def test_interval_of_more_than_64_chunks(bits, planks, chunks):
    """k_long_finish scans an interval's chunk counts 64 per round and carries the total: 65 chunks need the second round and the carry; with a second long
    interval in the scene the items of the two are claimed in whatever order their lanes reach the atomic."""
    wh, wo, mn, mx, order, want, st, m = strip_case(bits, 33100, 0.05, planks)
    assert sorted(m["chunks"][m["long"]].tolist()) == chunks and m["max_chunks"] == 65
    assert st.long_chunks == m["long_chunks"] == sum(chunks) and st.long_retries == 0
    assert (want[:, 0] == 33100).sum() > 20000


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_absolute_rule_a_whole_wave_of_long_intervals(bits):
    """len > SW_CAP: 65 601 boxes whose x extents all overlap, in ascending x.  Interval i has 65 600 - i candidates: exactly the first 64 -- one whole wave of
    k_sweep_ranges -- exceed 65 536, with 129 chunks each; none is long by the relative rule (its neighbours are as long as it is).  The reference is the
    grid route of reference_pairs alone: the oracle's sweep of this wall takes seconds (tests/test_broadphase_reference_cpu.py holds the two routes and the
    oracle to each other on smaller walls)."""
    n = 65601
    pos, he, static = R.wall(n, 257)
    bodies, colliders, static = R.world_tables(pos, he, static)
    wh, _ = worlds(bits, oracle=False)
    mn, mx, order, want, st = check_frame(bits, wh, None, np.arange(n), static, bodies=bodies, colliders=colliders, route="grid")
    m = R.dispatch_model(mn[:, 0], mx[:, 0], order)
    assert m["absolute"].sum() == 64 and m["absolute"][:64].all() and not m["relative"].any() and set(m["chunks"][:64].tolist()) == {129}
    assert st.long_chunks == m["long_chunks"] == 64 * 129 and st.long_retries == 0 and st.unsorted == 0
    assert len(want) > 9000 and (want[:, 0] < 64).sum() >= 9, "the long wave owns pairs of its own"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# grow and retry: more chunks requested than the chunk list holds
RETRY_PLANKS = [(100, 2500), (2400, 2500)]   # 5 chunks each


def retry_world(bits, monkeypatch, cap="8"):
    """AVN_SWEEP_LONG_CAP is read by the `make measure` build when a world first sizes its collider arrays: set it before that upload."""
    if cap is not None:
        monkeypatch.setenv("AVN_SWEEP_LONG_CAP", cap)
    return hip_measure_lib()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("nan_at", [None, 300])
def test_chunk_overflow_grows_and_repeats_the_count_pass(bits, nan_at, monkeypatch):
    """10 chunks against a list of 8: k_sweep_ranges raises the overflow flag and writes no item, collect_finish grows the list and runs the count pass again.
    With a NaN pose among the first plank's candidates the repeated pass drops it again (2 499 candidates: still 5 chunks)."""
    wh, wo, mn, mx, order, want, st, m = strip_case(bits, 5000, 0.05, RETRY_PLANKS, lib=retry_world(bits, monkeypatch), nan_at=nan_at)
    assert m["chunks"][m["long"]].tolist() == [5, 5]
    assert st.long_chunks == 10 and st.long_retries == 1 and st.dropped == (0 if nan_at is None else 1)
    assert (want[:, 0] >= 5000).sum() > 3000
    # the list has grown: the next collect of this world needs no second pass
    mn, mx, order, want, st = check_frame(bits, wh, wo, order, strip_case.static, seen=R.pair_keys(want[:, 0], want[:, 1]))
    assert len(want) == 0 and st.long_chunks == 10 and st.long_retries == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_chunk_overflow_without_the_small_list_needs_no_retry(bits):
    wh, wo, mn, mx, order, want, st, m = strip_case(bits, 5000, 0.05, RETRY_PLANKS, lib=hip_measure_lib())
    assert st.long_chunks == m["long_chunks"] == 10 and st.long_retries == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_chunk_overflow_in_a_second_frame_with_a_pair_set(bits, monkeypatch):
    """Frame 1: the second plank is far away (5 chunks fit the list of 8, the first plank's pairs enter the pair set).  Frame 2: it moves into place: 10 chunks,
    the list grows, and BOTH count passes filter against a non-empty pair set: only the second plank's pairs are new."""
    pos, he, static = R.strip(5000, 1 / 32, 0.05, RETRY_PLANKS)
    home = pos[5001].copy()
    pos[5001, 0] += 10000.0
    bodies, colliders, static = R.world_tables(pos, he, static)
    wh, wo = worlds(bits, lib=retry_world(bits, monkeypatch))
    mn, mx, order, want, st = check_frame(bits, wh, wo, np.arange(5002), static, bodies=bodies, colliders=colliders)
    assert st.long_chunks == 5 and st.long_retries == 0 and (want[:, 0] == 5000).sum() > 1500 and not (want == 5001).any()
    bodies["position"][5001] = home
    seen = R.pair_keys(want[:, 0], want[:, 1])
    mn, mx, order, want, st = check_frame(bits, wh, wo, order, static, seen=seen, bodies=bodies)
    assert st.long_chunks == 10 and st.long_retries == 1 and st.unsorted == 1
    assert len(want) > 1500 and np.all((want == 5001).any(axis=1)), "every new pair has the plank that moved in on one side"


@pytest.mark.parametrize("bits", [32, 64])
def test_chunk_overflow_in_the_device_closed_loop(bits, monkeypatch):
    """The same retry inside a step of the device closed loop (world/pipeline_device.hpp), held to the oracle's closed loop as
    test_library_pipeline_hip_matches_oracle_and_python_driver holds it: colour lists and body state, bit for bit, for 3 steps."""
    pos, he, static = R.strip(5000, 1 / 32, 0.05, RETRY_PLANKS)
    bodies, colliders, static = R.world_tables(pos, he, static)
    ws = []
    for lib in (oracle_lib(), retry_world(bits, monkeypatch)):
        w = F.World(lib, F.default_config(bits, substeps=2))
        w.bodies_upload(**bodies); w.colliders_upload(**colliders)
        w.existing_pairs_upload(np.zeros(0, np.uint64)); w.collider_materials_upload(friction=0.5)
        w.pipeline_enable()
        ws.append(w)
    wo, wh = ws
    for s in range(3):
        wo.step(); wh.step()
        st = wh.broad_phase_stats()
        assert (st.intervals, st.long_chunks, st.long_retries) == (5002, 10, 1 if s == 0 else 0), f"step {s}"
        oo, oh = wo.pipeline_handles(), wh.pipeline_handles()
        assert np.array_equal(oo[0], oh[0]) and np.array_equal(oo[1], oh[1]), f"step {s}: colour lists"
        bo, bh = wo.bodies_download(), wh.bodies_download()
        for k in bo:
            assert np.array_equal(bo[k], bh[k]), f"step {s}: bodies.{k}"
        if s == 0:
            assert st.pairs > 3000 and st.unsorted == 1
    so, sh = wo.pipeline_stats(), wh.pipeline_stats()
    assert so.pairs_added == sh.pairs_added > 3000 and so.manifolds == sh.manifolds > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_emit_from_records_and_by_a_second_sweep(bits):
    """The emit pass writes a wave quarter's pairs from the count pass's (lane, j) records when it found at most SW_HIT_RECORDS = 15, and sweeps again otherwise.
    41 tiles whose quarter 0 finds 0 .. 40 pairs (every other quarter none), a tile whose lane 0 owns 15 / 16 pairs (the rank of a record among those of its
    lane), a tile in which 16 lanes own one each."""
    pos, he, static, per_tile = R.emit_tiles()
    n = len(pos)
    bodies, colliders, static = R.world_tables(pos, he, static)
    wh, wo = worlds(bits)
    mn, mx, order, want, st = check_frame(bits, wh, wo, np.arange(n), static, bodies=bodies, colliders=colliders)
    assert np.array_equal(order, np.arange(n)) and st.unsorted == 0
    assert np.bincount(want[:, 0] // 64, minlength=len(per_tile)).tolist() == per_tile and np.all(want[:, 1] // 64 == want[:, 0] // 64)
    assert min(per_tile) == 0 and R.SW_HIT_RECORDS in per_tile and R.SW_HIT_RECORDS + 1 in per_tile
    assert st.pairs == sum(per_tile) and st.long_chunks == 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("pattern", R.SORT_PATTERNS)
@pytest.mark.parametrize("n", sorted({8191, 8192, 8193, 4 * 2048 + 1, 10241}))
def test_sort_forms_at_their_size_edges(bits, pattern, n):
    """f32 keys: one workgroup up to 8 192 intervals, sorted tiles of 2 048 + a merge from 8 193 (a last tile of one element at 4 x 2 048 + 1 and 5 x 2 048 + 1);
    f64 keys: fused radix passes.  Frame 1 arrives in DESCENDING key order (every element of the merge searches every tile), frame 2 is unchanged (the sort
    does not run, the order stays), frame 3 follows a small jitter (the merge's common case).  Form 4 (radix passes + scan) needs more than 262 144 f32 /
    131 072 f64 intervals, out of reach of a quick test: tests/test_gpu_configs.py::test_cfg4_one_million_sparse_mixed_pairs_bit_exact takes 10^6 f32 keys
    in random order through it against the oracle, and test_sort_radix_scan_form_just_above_its_threshold below holds it to reference_pairs.  (f32 keys never
    take form 3: above 262 144 intervals a radix pass has more than the 128 tiles the fused form allows.)"""
    pos, he, static = R.sort_scene(pattern, n, bits)
    bodies, colliders, static = R.world_tables(pos, he, static)
    wh, wo = worlds(bits, contact_tolerance=0.0)
    form = {32: F.SORT_FORM_ONE_WORKGROUP if n <= 8192 else F.SORT_FORM_TILES_MERGE, 64: F.SORT_FORM_FUSED_RADIX}[bits]
    order, seen = np.arange(n), np.zeros(0, np.uint64)
    for frame in range(3):
        if frame == 2:
            bodies["position"] = R.jitter_keys(pos)
        mn, mx, new_order, want, st = check_frame(bits, wh, wo, order, static, seen=seen, bodies=bodies if frame != 1 else None, colliders=colliders if frame == 0 else None)
        if frame == 0:
            assert_same(mn[:, 0].astype(np.float64), pos[:, 0], "min.x is the key")
            assert st.unsorted == 1 and st.sort_form == form and len(want) > 500
            if pattern == "equal":
                assert np.array_equal(new_order, np.concatenate([[n - 1], np.arange(n - 1)])), "equal keys keep their upload order"
        elif frame == 1:
            assert st.unsorted == 0 and st.sort_form == F.SORT_FORM_NONE and np.array_equal(new_order, order) and len(want) == 0
        elif pattern != "equal":
            assert st.unsorted == 1 and st.sort_form == form and not np.array_equal(new_order, order)
        order = new_order
        seen = np.concatenate([seen, R.pair_keys(want[:, 0], want[:, 1])])


@pytest.mark.parametrize("bits,n", [(32, 2048 * 128 + 1), (64, 1024 * 128 + 1)])
def test_sort_radix_scan_form_just_above_its_threshold(bits, n):
    """One interval more than tiles + merge (f32) / the fused radix passes (f64) take: 8-bit radix passes with a scanned histogram (257 / 129 tiles of 1 024).
    A descending first frame of random keys with repeats, then an unchanged one.  reference_pairs only: the oracle's insertion sort is quadratic in a
    descending frame.  (cfg5's half a million f64 colliders in tests/test_gpu_configs.py are uploaded in ascending x: their sort never runs.)"""
    pos, he, static = R.sort_scene("random", n, bits)
    bodies, colliders, static = R.world_tables(pos, he, static)
    wh, _ = worlds(bits, oracle=False, contact_tolerance=0.0)
    mn, mx, order, want, st = check_frame(bits, wh, None, np.arange(n), static, bodies=bodies, colliders=colliders)
    assert st.unsorted == 1 and st.sort_form == F.SORT_FORM_RADIX_SCAN and len(want) > 10000
    seen = R.pair_keys(want[:, 0], want[:, 1])
    mn, mx, order2, want, st = check_frame(bits, wh, None, order, static, seen=seen)
    assert st.unsorted == 0 and st.sort_form == F.SORT_FORM_NONE and np.array_equal(order2, order) and len(want) == 0


def test_stats_argument_checks_and_empty_world():
    wh = F.World(hip_lib(), F.default_config(32))
    st = wh.broad_phase_stats()
    assert (st.intervals, st.pairs, st.sort_form, st.long_chunks, st.long_retries) == (0, 0, 0, 0, 0)
    bad = F.avn_broad_phase_stats(4)
    assert hip_lib().dll.avn_broad_phase_stats_get(wh.handle, F.C.byref(bad)) == 1   # AVN_ERR_BAD_ARG
