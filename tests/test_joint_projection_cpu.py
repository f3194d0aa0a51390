"""CPU: the oracle's XPBD joints -- prepare, the five solves, velocity projection, joint damping, joint forces -- against the
independent reference of tests/joint_projection_reference.py, system by system through the C ABI.  tests/test_gpu_joint_projection.py applies the same
check (joint_projection_scenes.check) to the HIP library.

Truth = the reference in the next wider type (float64 for f32 worlds, longdouble for f64 worlds) on the world's own inputs of every system.
Noise = the reference in the world's type on the same inputs: its largest difference to the truth, per compared field and scene.
Bound = 16 x that noise per field and scene: it pays for another association order, for the polynomial sin / cos / asin of avn_math.h (stated <= 2 ulp)
and for comparing one maximum with another.  It is not tuned on the oracle or the kernels.

Measured (oracle; the HIP library's records are bit-identical): the worst ratio of any field is 2.4 in f32 and 4.8 in f64.
"""
import numpy as np
import pytest

import joint_projection_reference as R
import joint_projection_scenes as P
from helpers import F

LONGDOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < 1e-18


def bits_or_skip(bits):
    if bits == 64 and not LONGDOUBLE_IS_WIDER:
        pytest.skip("np.longdouble is no wider than float64 here: there is no truth for an f64 world")
    return bits


recorded = P.oracle_record


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("with_damping", [True, False])
def test_formula_scene_within_the_reference_noise(bits, with_damping):
    scene = P.formula_scene(with_damping)
    P.check(recorded(scene, bits_or_skip(bits)), scene, bits, "oracle")


def test_formula_scene_holds_every_case():
    """Each item of the variation list occurs, read off the scene's arrays and off what the float64 truth saw in the first substep."""
    scene = P.formula_scene(True)
    tr = recorded(scene, 32)
    _, report = P.evaluate(tr, scene, 32)
    first = report[0]
    J, B, meta = scene["joints"], scene["bodies"], scene["meta"]
    jt, fl = J["joint_type"], J["limit_flags"]
    sb = tr["substeps"][0]["before"]
    has = (sb["flags"] & R.NO_SOLVER_BODY) == 0
    assert len(jt) == 201 and all((jt == t).sum() >= 40 for t in range(5))

    def seen(j, tag, lo, hi):
        """Where the truth found limit `tag` of joint j: None when the limit was not evaluated."""
        if tag + "_phi" not in first[j]: return None
        phi = first[j][tag + "_phi"]
        return "equal" if lo == hi else ("below" if phi < lo else ("above" if phi > hi else "inside"))

    for t, tag, need, lo, hi in ((F.JOINT_REVOLUTE, "l1", F.JOINT_HAS_LIMIT1, "limit_min", "limit_max"), (F.JOINT_SPHERICAL, "l1", F.JOINT_HAS_LIMIT1, "limit_min", "limit_max"),
                                (F.JOINT_SPHERICAL, "l2", F.JOINT_HAS_LIMIT2, "limit2_min", "limit2_max")):
        js = [j for j in range(len(jt)) if jt[j] == t and meta[j]["variant"] != "body1_disabled"]   # (an unprepared joint has no angle)
        found = {seen(j, tag, J[lo][j], J[hi][j]) for j in js if fl[j] & need}
        assert {"inside", "below", "above", "equal"} <= found, (t, tag, found)
        assert any(not (fl[j] & need) for j in js), (t, tag, "limit absent")
        for j in js:   # the angles are known by construction: where nothing moves (both bodies static) the truth must measure exactly what was built
            if meta[j]["variant"] == "both_static" and tag + "_phi" in first[j]:
                built = meta[j]["angle1" if tag == "l1" else "angle2"]   # (a revolute joint's hinge axes are misaligned by up to 0.15 rad: asin sees sin(angle) * cos(that))
                assert abs(first[j][tag + "_phi"] - built) < (0.03 if t == F.JOINT_REVOLUTE else 1e-5), (j, built, first[j])
        angles = np.degrees(np.abs([first[j][tag + "_phi"] for j in js if tag + "_phi" in first[j]]))
        assert (angles < 85).any() and ((angles > 95) & (angles < 170)).any(), (t, tag, "acute and obtuse angles")
    # prismatic slider and distance limits: the position along the axis / the distance against [min, max]
    for t, key in ((F.JOINT_PRISMATIC, "along"), (F.JOINT_DISTANCE, "distance")):
        js = [j for j in range(len(jt)) if jt[j] == t and meta[j]["variant"] != "body1_disabled" and (fl[j] & F.JOINT_HAS_LIMIT1 or t == F.JOINT_DISTANCE)]
        where = {("equal" if J["limit_min"][j] == J["limit_max"][j] else "below" if first[j][key] < J["limit_min"][j] else "above" if first[j][key] > J["limit_max"][j] else "inside")
                 for j in js if key in first[j]}
        assert {"inside", "below", "above", "equal"} <= where, (t, where)
    assert any(jt[j] == F.JOINT_PRISMATIC and not fl[j] & F.JOINT_HAS_LIMIT1 for j in range(len(jt)))
    # both sides of the twist switch, with a twist limit that is evaluated
    swing = np.degrees(np.arccos([first[j]["swing_cos"] for j in first if "swing_cos" in first[j]]))
    assert (swing < 110).any() and ((swing > 130) & (swing < 170)).any()
    right = first[200]
    assert right["l1_phi"] == np.pi / 2 and right["l1_cos"] == 0.0, "the deterministic case: a limit angle of exactly 90 degrees"
    for t in range(5):
        js = np.flatnonzero(jt == t)
        for lane in range(3):   # compliance 0 and non-zero in each lane, three different values
            assert (J["compliance"][js, lane] == 0).any() and (J["compliance"][js, lane] == P.COMPLIANCE[lane]).any()
        d1, d2 = sb["dominance"][J["body1"][js]].astype(int), sb["dominance"][J["body2"][js]].astype(int)
        both = has[J["body1"][js]] & has[J["body2"][js]]
        assert (both & (d1 > d2)).any() and (both & (d1 < d2)).any() and (both & (d1 == d2) & (d1 != 0)).any(), "dominance +, -, and equal but non-zero"
        v = [meta[j]["variant"] for j in js]
        assert all(x in v for x in P.BODY_VARIANTS)
        st1 = (B["rb_type"][J["body1"][js]] == F.RB_STATIC) & ~has[J["body1"][js]]
        st2 = ~has[J["body2"][js]]
        assert (st1 & ~st2).any() and (st1 & st2).any(), "body 1 static, and both bodies without a SolverBody"
        assert (B["rb_type"][J["body2"][js]] == F.RB_KINEMATIC).any() and ((B["body_flags"][J["body1"][js]] & F.BODY_DISABLED) != 0).any()
        lock1, lock2 = B["locked_axes"][J["body1"][js]], B["locked_axes"][J["body2"][js]]
        assert (lock2 == 0b100000).any() and (lock1 == 0b110000).any() and (lock1 & 0b000111).any() and (lock2 & 0b000111).any(), "one and two locked translation axes, locked rotation axes"
        h = 1.0 / 120.0
        for k in ("damping_linear", "damping_angular"):
            assert (J[k][js] * h < 1).any() and (J[k][js] * h > 1).any()
    dyn = B["rb_type"] == F.RB_DYNAMIC
    inertia = B["inv_inertia_local"][dyn][:-2]   # (but for the deterministic right-angle pair, which is isotropic)
    assert (np.abs(inertia[:, [1, 2, 4]]).max(axis=1) > 1e-2).all(), "anisotropic inertia with off-diagonal terms, in randomly rotated frames"
    axes = {tuple(a) for a in J["axis"]}
    assert all(tuple(float(c) for c in p) in axes for p in P.AXIS_PRESETS) and any(np.signbit(a[2]) and a[2] == 0 for a in J["axis"])
    assert sum(1 for a in J["axis"] if 0.05 <= abs(a[2]) < 1) >= 40, "random unit axes with |z| >= 0.05"
    assert "damping_linear" not in P.formula_scene(False)["joints"], "damping absent: the second scene of test_formula_scene_within_the_reference_noise"
    assert P.SUBSTEPS == 2 and np.abs(tr["substeps"][1]["before"]["delta_rotation"][has][:, :3]).max() > 1e-3, "the second substep starts from turned bodies"


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_a_wrong_reference_is_noticed(mutation):
    """Negative controls: with a deliberate error in the reference the oracle must leave the tolerance on the formula scene -- the scene can tell the
    two apart, so an oracle (or kernel) with that error would have failed above."""
    scene = P.formula_scene(True)
    result, _ = P.evaluate(recorded(scene, 32), scene, 32, mutation=mutation)
    over = {f: err / noise for f, (err, noise) in result.items() if err > P.FACTOR * noise}
    print(mutation, {f: f"{r:.3g}" for f, r in over.items()})
    assert over, f"{mutation}: the oracle stays within {P.FACTOR:.0f} x noise of a reference with this error: the scenes are too weak"


def test_chain_lengths_straddle_the_lds_ceiling():
    """The chains of the mixed scene come from the staging formula of the level schedule (world/joints.hpp: fill_joint_recs), nb = nj + 1."""
    assert P.straddling_chain_lengths(32) == (212, 213) and P.straddling_chain_lengths(64) == (106, 107)
    for bits in (32, 64):
        fit, over = P.straddling_chain_lengths(bits)
        assert P.lds_bytes(fit + 1, fit, bits) <= 65536 < P.lds_bytes(over + 1, over, bits)


def test_schedule_scenes_have_the_shapes_they_are_for():
    """The level structure each scene asks of the schedule, from the serial order alone (joint_projection_scenes.level_shape)."""
    assert P.level_shape(P.comb_scene()) == [[130, 130]], "one component, two levels of 130 joints: two full 64-lane rounds and a tail of 2"
    for bits in (32, 64):
        fit, over = P.straddling_chain_lengths(bits)
        shape = P.level_shape(P.mixed_scene(bits))
        assert [sum(w) for w in shape] == [over, fit] + [1] * 21 and len(shape) == 23, "both chains, twenty single joints, the static pair"
        assert [sum(w) for w in P.level_shape(P.chains_scene(bits))] == [over, fit]
    assert P.level_shape(P.hub_scene(False)) == [[1] * 70], "a dynamic hub: 70 levels of one joint"
    assert P.level_shape(P.hub_scene(True)) == [[1]] * 70, "a hub without a SolverBody: 70 components of one joint"
    for case in P.SCHEDULE_CASES:
        J = P.schedule_case(case, 32)["joints"]
        assert set(J["joint_type"]) == {0, 1, 2, 3, 4} and "damping_linear" in J and "damping_angular" in J, "all five types, damping on"


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("case", P.SCHEDULE_CASES)
def test_schedule_scenes_within_the_reference_noise(case, bits):
    scene = P.schedule_case(case, bits_or_skip(bits))
    P.check(recorded(scene, bits), scene, bits, "oracle")
