"""Golden vectors from REAL Avian -- the route from "parity partial" to "parity green" (VERDICT r5, next-round item 4).

integration/rust/avian_fixtures is a headless avian3d binary that dumps, per step, body state as bit patterns, the broad phase's new pairs in emission order, every
GraphColor's manifold_handles in order, ContactPoint impulses and island ids, for cfg1, Large Pyramid (base 20), Many Pyramids (3 x 3 x base 5), a scene with one joint
of each of the five types and a sleeping scene.  It cannot be built in the image this repository was written in (no Rust toolchain, no network).  On a machine that
has cargo:   cd integration/rust/avian_fixtures && cargo run --release -- /tmp/avf && python tools/avian_fixtures_to_npz.py /tmp/avf   and commit tests/golden/avian/.

What runs here:
  * with tests/golden/avian/<scene>.npz present: the ORACLE (CPU) and, under -m gpu, the HIP path are stepped from the fixture's initial frame and held to it --
    pair sequences, colour lists and island ids bit-exact, bodies within the N1 tolerance -- for the first steps, then for as long as the
    trajectories stay together; ABSENT fixtures are reported loudly (skip reason + warning), never silently;
  * always: every avian3d / bevy name the generator uses is checked against the reference's source, as recorded in tests/golden/reference_facts.json
    (tests/reference_facts.py; the check tests/test_rust_layer_cpu.py does for the shim);
  * always: the whole consumer side is exercised on fixtures written IN THE GENERATOR'S FORMAT from the oracle itself -- converter, reader, world construction,
    replay -- which the oracle must reproduce with tolerance 0 (CPU) and the HIP path too (-m gpu)."""
import os
import re
import warnings

import numpy as np
import pytest

import avian_fixture_format as AF
import reference_facts as R
from avian_amd import scenes
from helpers import hip_lib, oracle_lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "avian")
GEN = os.path.join(REPO, "integration", "rust", "avian_fixtures", "src", "main.rs")
SCENES = ["cfg1", "large_pyramid", "many_pyramids", "joints", "sleeping"]
EXACT_STEPS = 3                                        # integer structures and bodies are ASSERTED for this many steps ...
def body_tol(step): return 2e-6 * 4.0 ** (step - 1)   # ... within N1's one-step 1e-7..1e-6 (libm sin/cos, FMA, SIMD quaternion product), growing as a pile amplifies it


def fixture_path(scene):
    return os.path.join(GOLDEN, scene + ".npz")


def absent(scene):
    msg = (f"ABSENT: tests/golden/avian/{scene}.npz -- no Avian golden vectors for '{scene}': parity with the reference stays UNPINNED for this scene "
           f"(generate them with integration/rust/avian_fixtures on a machine that has cargo, convert with tools/avian_fixtures_to_npz.py)")
    warnings.warn(msg)
    pytest.skip(msg)


@pytest.mark.parametrize("scene", SCENES)
def test_oracle_matches_avian_fixture(scene):
    if not os.path.exists(fixture_path(scene)): absent(scene)
    fx = AF.load(fixture_path(scene))
    r = AF.replay(oracle_lib(), fx, steps=60, body_tol=body_tol, exact_steps=EXACT_STEPS)
    assert r["steps_held"] >= EXACT_STEPS, r


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_hip_matches_avian_fixture(scene):
    if not os.path.exists(fixture_path(scene)): absent(scene)
    fx = AF.load(fixture_path(scene))
    r = AF.replay(hip_lib(), fx, steps=60, body_tol=body_tol, exact_steps=EXACT_STEPS)
    assert r["steps_held"] >= EXACT_STEPS, r


# ---- the generator only names things the reference has ---------------------------------------------------------------------------------------------------------
def test_every_avian_name_the_generator_uses_exists_in_the_reference():
    src, ref = open(GEN).read(), R.ALL_RS   # (the reference's answers: tests/reference_facts.py)
    # (1) module paths of the `use avian3d::{...}` block
    for path in ("collision::contact_types::ContactId", "dynamics::solver::constraint_graph::ConstraintGraph", "dynamics::solver::islands::BodyIslandNode", "math::Scalar", "math::Vector"):
        *mods, name = path.split("::")
        assert R.search(ref, r"pub (struct|type|enum) " + name + r"\b"), f"avian3d::{path}: no such public item"
        f = "/".join(["src", *mods[:-1], mods[-1] + ".rs"]); d = "/".join(["src", *mods, "mod.rs"])
        assert R.exists(f) or R.exists(d), f"avian3d::{'::'.join(mods)}: no such module"
    # (2) types, resources and components taken from the prelude: each must be a public item of the reference
    types = ["PhysicsPlugins", "RigidBody", "Collider", "Position", "Rotation", "LinearVelocity", "AngularVelocity", "SleepTimer", "Sleeping", "ComputedMass", "ComputedAngularInertia",
             "ComputedCenterOfMass", "Friction", "Restitution", "Gravity", "SubstepCount", "PhysicsSchedule", "PhysicsStepSystems", "ContactGraph", "ContactPair", "DistanceJoint", "FixedJoint",
             "RevoluteJoint", "SphericalJoint", "PrismaticJoint", "JointCollisionDisabled", "WakeBody"]
    for t in types:
        assert re.search(r"\b" + t + r"\b", src), f"the generator no longer uses {t}: drop it from this list"
        assert R.search(ref, r"pub (struct|enum|type) " + t + r"\b"), f"{t}: not a public item of the reference"
    # (3) methods and fields, each with the item that owns it
    members = {"fn cuboid": "Collider::cuboid", "fn shape": "Collider::shape", "fn inverse": "ComputedMass::inverse", "fn island_id": "IslandNode::island_id", "fn iter_active": "ContactGraph::iter_active",
               "fn iter_sleeping": "ContactGraph::iter_sleeping", "fn with_local_anchor2": "joints", "fn with_limits": "DistanceJoint / PrismaticJoint", "fn with_hinge_axis": "RevoluteJoint",
               "fn with_slider_axis": "PrismaticJoint", "pub manifold_handles": "GraphColor", "pub colors": "ConstraintGraph", "pub contact_id": "ContactPair / ContactManifoldHandle",
               "pub manifold_index": "ContactManifoldHandle", "pub manifolds": "ContactPair", "pub points": "ContactManifold", "pub normal_impulse": "ContactPoint", "pub warm_start_normal_impulse": "ContactPoint",
               "pub warm_start_tangent_impulse": "ContactPoint", "pub feature_id1": "ContactPoint", "pub penetration": "ContactPoint", "pub normal": "ContactManifold", "pub dynamic_coefficient": "Friction",
               "pub coefficient": "Restitution", "pub collider1": "ContactPair", "pub flags": "ContactPair"}
    for decl, owner in members.items():
        name = decl.split()[-1]
        assert re.search(r"\b" + name + r"\b", src), f"the generator no longer uses {name}"
        assert R.search(ref, r"pub (const )?" + decl.replace("pub ", "").replace("fn ", r"fn ") + r"\b"), f"{owner}: `{decl}` is not public in the reference"
    # (4) the scenes are the reference's: the bench constants the generator restates
    bench = "benches/src/dim3/large_pyramid.rs"
    assert R.contains(bench, "(2.0 * i as f32 + 1.0) * shift * 0.99") and "(2.0 * i as f32 + 1.0) * shift * 0.99" in src
    many = "benches/src/dim3/many_pyramids.rs"
    assert R.contains(many, "j as f32 * (base_width + 2.0 * h) + h") and "j as f32 * (base_width + 2.0 * h) + h" in src
    cargo = open(os.path.join(REPO, "integration", "rust", "avian_fixtures", "Cargo.toml")).read()
    for feat in ("3d", "f32", "parry-f32", "parallel", "simd"):   # benches/Cargo.toml:25-31
        assert f'"{feat}"' in cargo and R.contains("benches/Cargo.toml", f'"{feat}"')


# ---- the consumer side, end to end, on fixtures the oracle wrote in the generator's format ---------------------------------------------------------------
def oracle_fixture(tmp_path, name, sc, substeps, frames):
    avf = os.path.join(tmp_path, name + ".avf"); npz = os.path.join(tmp_path, name + ".npz")
    AF.write_fixture_from_library(oracle_lib(), sc, avf, substeps, frames)
    AF.avf_to_npz(avf, npz)
    return AF.load(npz)


def test_consumer_reproduces_oracle_made_fixtures_exactly(tmp_path):
    """stack of 4 x 4 x 4 on a slab, 25 steps: contacts form, the overflow colour fills, ids are reused; tolerance 0 throughout"""
    fx = oracle_fixture(str(tmp_path), "stack", scenes.box_stack(4, 4, 4), 4, 26)
    assert fx.n == 65 and fx.frame0 == 0 and fx.substeps == 4
    assert sum(len(c) for c in fx.colours(10)) > 100 and len(fx.ragged("pair", 1, 3)) > 100 and len(fx.ragged("impl", 10, AF.IMPL_W)) > 100
    r = AF.replay(oracle_lib(), fx, steps=25, body_tol=lambda k: 0.0, exact_steps=25)
    assert r == {"steps_held": 25, "worst_body_difference": 0.0}


def test_consumer_notices_a_wrong_fixture(tmp_path):
    """negative control: one flipped mantissa bit in one body of one frame, one swapped pair of handles -- the replay must fail at that step"""
    fx = oracle_fixture(str(tmp_path), "stack", scenes.box_stack(3, 3, 3), 4, 8)
    fx.a["body"][3, 5, 1] ^= 1
    with pytest.raises(AssertionError, match="step 3: bodies differ"):
        AF.replay(oracle_lib(), fx, steps=7, body_tol=lambda k: 0.0, exact_steps=7)
    fx.a["body"][3, 5, 1] ^= 1
    o = fx.a["colr_off"]; flat = fx.a["colr"]; lo = int(o[4])
    k = next(i for i in range(lo, int(o[5])) if flat[i] >= 2 and i + 3 < int(o[5]))   # a colour with at least two handles: swap the first two ids
    flat[k + 1], flat[k + 3] = flat[k + 3], flat[k + 1]
    with pytest.raises(AssertionError, match="step 4: a GraphColor's manifold_handles differ"):
        AF.replay(oracle_lib(), fx, steps=7, body_tol=lambda k: 0.0, exact_steps=7)


@pytest.mark.gpu
def test_hip_reproduces_oracle_made_fixtures_exactly(tmp_path):
    fx = oracle_fixture(str(tmp_path), "stack", scenes.box_stack(5, 4, 5), 4, 31)
    r = AF.replay(hip_lib(), fx, steps=30, body_tol=lambda k: 0.0, exact_steps=30)
    assert r == {"steps_held": 30, "worst_body_difference": 0.0}


def test_absent_fixtures_are_listed():
    """not a skip: the list of missing golden files is part of every CPU run's output"""
    missing = [s for s in SCENES if not os.path.exists(fixture_path(s))]
    if missing:
        warnings.warn("Avian golden vectors ABSENT for: " + ", ".join(missing) + " -- SURVEY.md section 8 row (c) stays 'parity unpinned' beyond rows a3-a9 until they are generated")
