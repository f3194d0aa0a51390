"""GPU: the HIP library's XPBD joints against the independent reference (tests/joint_projection_reference.py) with the check of
tests/test_joint_projection_cpu.py -- truth in the next wider type, at most 16 x the reference's own noise per field and scene -- and the shape edges of
the level schedule (world/joints.hpp, k_joint_schedule / k_joint_schedule_lds) bit for bit against the oracle:

  comb         one component, two levels of 130 joints: the 64-lane stride runs twice and then with a tail of 2
  chains       a chain just under and one just over the 64 KiB LDS ceiling of fill_joint_recs, alone
  mixed        a chain just under and one just over the 64 KiB LDS ceiling of fill_joint_recs (212 / 213 joints in f32, 106 / 107 in f64), twenty single-joint
               components and a joint between two static bodies in one launch: staged components next to comp_bodies = 0xFFFFFFFF ones
  hub_dynamic  70 joints on one dynamic body: 70 levels of one joint
  hub_static   the same star on a body without a SolverBody: 70 one-joint components, nothing staged

All five joint types are mixed in every case and damping is on.  Each case is recorded system by system (PREPARE_JOINTS, then per substep XPBD_SOLVE,
XPBD_VELOCITY_PROJECTION, JOINT_DAMPING, then the joint forces) and through two whole steps; the record must equal the oracle's bit for bit, and the record of
the `make measure` build with AVN_NO_JOINT_LDS=1 (the global-memory walk) must equal both."""
import numpy as np
import pytest

import joint_projection_scenes as P
from helpers import hip_lib, hip_measure_lib

pytestmark = pytest.mark.gpu

LONGDOUBLE_IS_WIDER = np.finfo(np.longdouble).eps < 1e-18


def tolerance_check(tr, scene, bits):
    if bits == 64 and not LONGDOUBLE_IS_WIDER:
        pytest.skip("np.longdouble is no wider than float64 here: there is no truth for an f64 world")
    P.check(tr, scene, bits, "hip")


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("with_damping", [True, False])
def test_hip_formula_scene_within_the_reference_noise(bits, with_damping):
    scene = P.formula_scene(with_damping)
    tr = P.record(hip_lib(), bits, scene, whole_steps=2)
    P.assert_same_bits(tr, P.oracle_record(scene, bits), "hip vs oracle")
    tolerance_check(tr, scene, bits)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("case", P.SCHEDULE_CASES)
def test_hip_schedule_edges(case, bits, monkeypatch):
    scene = P.schedule_case(case, bits)
    tr = P.record(hip_lib(), bits, scene, whole_steps=2)
    P.assert_same_bits(tr, P.oracle_record(scene, bits), f"{case}: hip vs oracle")
    monkeypatch.setenv("AVN_NO_JOINT_LDS", "1")   # read by the measure build when the world is created
    P.assert_same_bits(P.record(hip_measure_lib(), bits, scene, whole_steps=2), tr, f"{case}: global-memory walk vs LDS walk")
    tolerance_check(tr, scene, bits)
