/*
 * avian_mi355x_ccd.h — swept continuous collision detection (the SweptCcd component, dynamics/ccd/mod.rs) inside the device closed loop.
 *
 * Mirrors `solve_swept_ccd` (ccd/mod.rs:523-687), the system of PhysicsStepSystems::Solver that the reference schedules after
 * SolverSystems::PostSubstep and before SolverSystems::Restitution (ccd/mod.rs:257-261): per SweptCcd body it finds the first time of impact
 * against the colliders whose AABBs its own collider's AABB intersects and moves both bodies back to that time, so that a fast body stops
 * at a thin wall instead of passing through it.  SweepMode::Linear and, behind avn_swept_ccd_non_linear_set, SweepMode::NonLinear (Avian's
 * default, which also follows the bodies' rotation) are built, for Ball / Cuboid colliders and, behind avn_swept_ccd_capsules_set, Capsule
 * colliders (AVN_SHAPE_CAPSULE, both modes); the pass runs on the world's
 * stream between the substep loop and the restitution pass of avn_step / AVN_SYS_SOLVER, and nothing is read back.  A world without a list
 * launches, stamps and allocates nothing for it.
 *
 * Conventions are those of avian_mi355x.h.  These entry points are plain `avn_swept_ccd_*` functions of libavian_mi355x.so; they are not part
 * of the AVN_FN list of the main header.
 *
 * THE DEFINITION (the kernels of k_ccd.hip and tests/swept_ccd_reference.py follow it; parry's iterative time-of-impact search cannot be
 * restated bit for bit, so the pair test is the closed-form shape cast of avian_mi355x_spatial.h: parity with parry is UNPINNED, as there).
 * The list is in the order of Avian's Query<Entity, With<SweptCcd>>.  dt = the step's delta in the world's scalar (what the narrow phase
 * uses).  For entry i with body b1:
 *  1. skipped when b1 has no SolverBody (static, disabled, or asleep with sleeping enabled) or no collider of its own.  Its own collider c1
 *     is the lowest collider slot attached to b1 without an avn_collider_transforms_upload entry (the reference reads the Collider on the
 *     body's entity).
 *  2. candidates: the live contact rows (one per AABB-overlapping pair) with c1 in either slot; c2 is the other slot, b2 its body.  A row is
 *     not tested when c2 is a child collider (the reference would cast it at the body's pose, `TODO: Support child colliders`: a declared
 *     deviation); when either collider is AVN_SHAPE_HOST or AVN_SHAPE_TRIANGLE (avian_mi355x_trimesh.h) (declared deviations: the pass has no geometry for them), or AVN_SHAPE_CAPSULE
 *     unless avn_swept_ccd_capsules_set is on ("capsule colliders" below); when include_dynamic == 0 and b2 is dynamic, awake or
 *     asleep; when |w1 - w2|^2 < angular_threshold^2 and |v1 - v2|^2 < linear_threshold^2 (the thresholds cast to the world's scalar, then
 *     squared; v2, w2 = b2's SolverBody velocities, 0 when it has none).  Sensors ARE tested: the reference does not filter them.
 *  3. time of impact: the "shape cast" of avian_mi355x_spatial.h with the collider = c1 at b1's step-start Position / Rotation, the cast
 *     shape = c2 at b2's step-start pose, d = v2 - v1 (not normalised: the cast's distance is time) and max_distance = dt.
 *  4. t == 0 (overlapping or touching at the start; parry's stop_at_penetration = false) goes through the ORIGIN-PENETRATION RULE of
 *     avn_spatial_cast_moves: the pair's shape contact at prediction 0 (the cast shape as shape 1), n = -manifold.normal (from c1 towards
 *     c2).  A contact with d.x n.x + d.y n.y + d.z n.z >= 0: the pair answers nothing.  Otherwise the reference's "small ball" fallback: a
 *     Ball of radius default_speculative_margin (* length_unit) at b2's step-start position, cast along d against c1 with max_distance = dt.
 *     With an unbounded margin (>= FLT_MAX, the default) the fallback is not evaluated and answers nothing: in exact arithmetic that ball
 *     contains c1 for the whole motion.
 *  5. a candidate counts iff 0 < t < dt, both strict.  The entry's hit is the smallest t; among equal times the edge that comes first in
 *     the reference's `neighbors` order: the rows with c1 in slot 1 by descending insertion stamp, then those with c1 in slot 2 by
 *     descending stamp (the reference narrows max_time_of_impact as it goes and compares with strict <).
 *  6. apply, in list order, with t' = t * 1.0001: delta_position(b1) = t' v1; delta_rotation(b1) = from_scaled_axis(w1 t') *
 *     delta_rotation(b1) in integrate_positions' arithmetic (the product with the FULL step's delta_rotation is the reference's behaviour);
 *     the same two writes to b2 with its own v2, w2 when b2 has a SolverBody.  When several entries write one body the result is what the
 *     serial loop leaves: the last delta_position, the delta_rotations multiplied in list order.  Velocities are never changed.
 *
 * SweepMode::NonLinear (`NonlinearRigidMotion` + parry's cast_shapes_nonlinear in the reference; iterative there too, so it is DEFINED here
 * and parity with parry stays UNPINNED; k_ccd.hip and tests/swept_ccd_nonlinear_reference.py follow it at tolerance 0).  Steps 1, 2, 5 and 6
 * hold unchanged; steps 3 and 4 of a NonLinear pair are N1 - N4.  Every operation is in the world's scalar, without fused multiply-adds,
 * with avn_math.h's dot / cross / length / qrot / qmul / from_scaled_axis in the association written here.
 *  N0. the pair's mode: NonLinear iff the entry's mode is AVN_SWEEP_NON_LINEAR or b2 is itself in the list with AVN_SWEEP_NON_LINEAR
 *      (`body2.ccd.is_none_or(..)`, ccd/mod.rs:621-627).  This goes by BODY: a listed b2 whose colliders are all children counts.
 *  N1. the motion of body k (k = 1, 2) with step-start pos_k, rot_k, local centre of mass com_k and SolverBody v_k, w_k (0 without one):
 *      c0_k = pos_k + qrot(rot_k, com_k);  q_k(t) = qmul(from_scaled_axis(w_k * t), rot_k) (not renormalised);
 *      p_k(t) = (c0_k + t * v_k) - qrot(q_k(t), com_k).  Every round evaluates from the step-start pose; nothing is accumulated.
 *  N2. the gap g and a unit axis n (world, from collider 1 towards 2) at the poses (p_1, q_1), (p_2, q_2), the rotations used as they are:
 *      ball - ball: dv = p_2 - p_1, dist = length(dv), g = dist - (r_1 + r_2), n = dv / dist, or (0, 1, 0) when !(dist > 0).
 *      ball - cuboid: l = qrot(conj(q_c), p_b - p_c), df = l - clamp(l, -he, he), dist = length(df).  dist > 0: g = dist - r, nl = df / dist.
 *        Otherwise (the centre is inside) g = -r and nl = the unit axis i of the smallest he_i - |l_i| (the lowest i among equals) with the
 *        sign of l_i.  n = qrot(q_c, nl) when the cuboid is collider 1, its negation when the ball is.
 *      cuboid - cuboid: pos12 = iso_inv_mul((q_1, p_1), (q_2, p_2)), pos21 = iso_inverse(pos12); sep1 = sat_normal_oneway(he1, he2, pos12),
 *        sep2 = sat_normal_oneway(he2, he1, pos21), sep3 = sat_edge_twoway(he1, he2, pos12) (avn_narrow.h, nalgebra's arithmetic); the narrow
 *        phase's choice: (g, nl) = (sep2, iso_vec(pos12, -d2)) when sep2 > sep1 and sep2 > sep3, else (sep3, d3) when sep3 > sep1, else
 *        (sep1, d1); n = na_qrot(q_1, nl).  g is a lower bound of the distance that is positive exactly when the boxes are disjoint, which is
 *        all conservative advancement needs.
 *  N3. conservative advancement.  d = v_2 - v_1; R_k = length(com_k) + rho_k with rho = r (ball) or length(half_extents) (cuboid);
 *      tol = contact_tolerance * length_unit, the project's own number for "touching".  t = 0; at most CCD_NL_ROUNDS (64) rounds of:
 *        evaluate (g, n) at t.  g <= tol: a hit at t.
 *        B = (-dot(d, n) + length(cross(w_1, n)) * R_1) + length(cross(w_2, n)) * R_2: no faster can the separation along the fixed axis n
 *        shrink, and that separation is a lower bound of the distance.  !(B > 0): a miss.
 *        tn = t + g / B.  tn > dt: a miss.  !(tn > t): a hit at t (no progress).  Otherwise t = tn.
 *      Out of rounds: the pair answers NOTHING and counts in avn_swept_ccd_stats::exhausted (the advancement converges from the left: "the
 *      last t standing" of a pair that never touches would freeze its bodies in time every step).  A hit with 0 < t < dt is a candidate of
 *      step 5.  With contact_tolerance == 0 only g <= 0 or no progress ends in a hit.  Resting bodies sit within tol, answer t == 0 and go
 *      through N4 instead of being rewound every step.
 *  N4. t == 0 (a hit in the first round): step 4 as it stands, the contact at prediction 0 at the step-start poses and the leaving test with
 *      d; the small-ball fallback is the loop N3 with shape 2 = Ball(default_speculative_margin * length_unit) at body 2's origin riding body
 *      2's motion, rho_2 = that radius.  With an unbounded margin it is not evaluated and answers nothing.
 * `tested` counts NonLinear pair tests too.  A list without a NonLinear entry launches exactly the kernels of a Linear-only library and leaves
 * the same bytes, whatever the switch says.
 *
 * CAPSULE COLLIDERS (avn_swept_ccd_capsules_set; DEFINED like the rest, parity with parry UNPINNED; k_ccd.hip's _cap kernels and
 * tests/swept_ccd_capsule_reference.py follow it at tolerance 0).  With the switch off a pair with a capsule on either side is skipped, as it
 * always was.  With it on the pair is tested, in both modes; steps 1, 2, 5 and 6 and N0, N1 and N3 stand as written.  A capsule's
 * half_extents are (r, h, .): parry's Capsule::new_y, the core segment (0, -h, 0) .. (0, +h, 0) of its frame swept by a ball of radius r.
 *  Step 3 is unchanged: the shape cast of avian_mi355x_spatial.h, which defines the capsule cases ("capsule query shapes", "queries against
 *     capsule colliders"), round cap included (at most 32 Newton evaluations, the last t standing).  By role: c1 a Ball or a Cuboid and c2 a
 *     capsule: the capsule query's cast against that collider; c1 a capsule and c2 a Ball or a Cuboid: that query shape's cast against the
 *     capsule collider; both capsules: the capsule query's cast against the capsule collider (Newton's iteration on the two cores).
 *  Step 4 / N4: the contact at prediction 0 is the narrow phase's capsule manifold (avian_mi355x.h, "capsule colliders") with the cast shape as
 *     shape 1.  The small ball against a capsule c1 is the Ball query's cast against the capsule collider in Linear mode, the advancement N3
 *     with the capsule - ball gap below in NonLinear mode; against a Ball / Cuboid c1 (the capsule is c2) it is what it always was.
 *  N2 for a pair with a capsule: the exact distance of the cores minus the radii, so the bound B of N3 is valid as written with
 *     rho(capsule) = h + r (that sum, in this order).  Arithmetic as in N2 above; `core` of a capsule in its own frame: A = (0, -h, 0),
 *     u = (0, h * 2, 0); of a capsule at the relative pose (q, t): hv = na_qrot(q, (0, h, 0)), A = t - hv, u = hv * 2.
 *      capsule - ball: l = qrot(conj(q_c), p_b - p_c); s = clamp(na_dot(l - A, u) / na_dot(u, u), 0, 1) (0 when na_dot(u, u) == 0);
 *        pc = A + u * s; df = l - pc; dist = length(df); g = dist - (r_c + r_b); nl = df / dist; n = qrot(q_c, nl) when the capsule is
 *        collider 1, its negation when the ball is.
 *      capsule - capsule: pos12 = iso_inv_mul((q_1, p_1), (q_2, p_2)); collider 1's core in its own frame as segment 1, collider 2's at pos12 as
 *        segment 2; (d2, p1, p2) = the segment - segment distance of the spatial queries (six candidate pairs evaluated in full, the first
 *        smallest wins); dist = sqrt(d2); g = dist - (r_1 + r_2); nl = (p2 - p1) / dist; n = na_qrot(q_1, nl).
 *      capsule - cuboid: pos = iso_inv_mul((q_x, p_x), (q_c, p_c)) (the capsule in the cuboid's frame), its core at pos; (f, ps, pb) = the
 *        segment - box routine of the spatial queries (ps on the core, pb = clamp(ps, -he, he)); dist = sqrt(f); g = dist - r;
 *        nl = (ps - pb) / dist (box towards capsule); n = qrot(q_x, nl) when the cuboid is collider 1, its negation otherwise.
 *      !(dist > 0) in any arm (a core point on the other core, in the ball's centre or in the box): g is as computed, minus the radius or
 *        radii, and n = (0, 1, 0).  With tol >= 0 the round ends in a hit before n is used.
 * A world whose collider table holds no capsule launches exactly the kernels it launches with the switch off and leaves the same bytes.
 * NOT covered: shapes other than Ball / Cuboid / Capsule, child and host-shape colliders as targets, parity with parry's searches,
 * level-2 / sharded worlds, the host-bookkeeping closed loop, 2D, Rust declarations.
 */
#ifndef AVIAN_MI355X_CCD_H
#define AVIAN_MI355X_CCD_H

#include "avian_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AVN_SWEEP_LINEAR = 0, AVN_SWEEP_NON_LINEAR = 1 };   /* SweepMode */
#define AVN_SWEPT_CCD_MISS 0xFFFFFFFFu                      /* hit_collider of an entry without a hit (= AVN_SPATIAL_MISS) */

/* the world's SweptCcd components; host pointers (configuration, not per-step data) */
typedef struct avn_swept_ccd {
    uint32_t struct_size;             /* sizeof(avn_swept_ccd) */
    uint32_t count;                   /* n; 0 clears the list */
    const uint32_t* body;             /* [n] body-table index; each body at most once */
    const uint32_t* mode;             /* [n] AVN_SWEEP_LINEAR; AVN_SWEEP_NON_LINEAR only after avn_swept_ccd_non_linear_set(w, 1) */
    const uint32_t* include_dynamic;  /* [n] 0: dynamic bodies are not tested */
    const double* linear_threshold;   /* [n] */
    const double* angular_threshold;  /* [n] */
} avn_swept_ccd;

/* what the pass left per entry.  16 / 24 bytes, every byte written. */
typedef struct avn_swept_ccd_result_f32 {
    float toi;              /* the time of impact the bodies were moved back to (before the factor 1.0001); 0: no hit */
    uint32_t hit_collider;  /* entity_index of the collider that was hit | AVN_SWEPT_CCD_MISS */
    int32_t hit_body;       /* its body | -1 */
    uint32_t tested;        /* pair casts that ran (step 3; the fallback's cast is not counted) */
} avn_swept_ccd_result_f32;
typedef struct avn_swept_ccd_result_f64 {
    double toi;
    uint32_t hit_collider;
    int32_t hit_body;
    uint32_t tested;
    uint32_t reserved;      /* always written as 0 */
} avn_swept_ccd_result_f64;

typedef struct avn_swept_ccd_results_out {
    void* results;          /* avn_swept_ccd_result_fNN [capacity], list order; NULL is legal (count only) */
    uint32_t capacity;
    uint32_t count;         /* out: entries of the last pass; 0 if no pass has run since the list was uploaded */
} avn_swept_ccd_results_out;

/* what the last pass did under SweepMode::NonLinear; the counters live on the device and nothing is read back during a step */
typedef struct avn_swept_ccd_stats {
    uint32_t struct_size;       /* in: sizeof(avn_swept_ccd_stats) */
    uint32_t nonlinear_tested;  /* pair tests that ran under N1 - N3 (the fallback of N4 is not counted, as in `tested`) */
    uint32_t rounds_max;        /* the most rounds one advancement took (the fallback's included) */
    uint32_t exhausted;         /* advancements that ran out of CCD_NL_ROUNDS rounds and answered nothing */
} avn_swept_ccd_stats;

/* Replaces the world's list (NULL or count 0 clears it).  AVN_ERR_BAD_ARG, with the previous list left in force: a mode other than
 * AVN_SWEEP_LINEAR (with the switch below on: other than the two modes), a body index outside the body table, a body named twice, a null array.  AVN_ERR_STATE: level-2 (halo plan) and
 * avn_dshard worlds.  avn_bodies_upload with another body count and avn_despawn clear the list: its indices are stale.
 * With a non-empty list avn_step and AVN_SYS_SOLVER return AVN_ERR_STATE, before doing anything, unless the world is in device closed-loop
 * mode (avn_pipeline_enable(w, 1)): the pass reads the contact table that mode keeps. */
AVN_API avn_status avn_swept_ccd_upload(avn_world* w, const avn_swept_ccd* list);
/* The records of the last step's pass (waits for it).  More entries than `capacity`: AVN_ERR_CAPACITY with `count` set. */
AVN_API avn_status avn_swept_ccd_results_get(avn_world* w, avn_swept_ccd_results_out* out);
/* Whether avn_swept_ccd_upload accepts AVN_SWEEP_NON_LINEAR, per entry.  Sticky; off in a new world, where the upload refuses the mode as it
 * always has.  Turning it off while the list in force holds a NonLinear entry: AVN_ERR_STATE, the switch and the list unchanged. */
AVN_API avn_status avn_swept_ccd_non_linear_set(avn_world* w, uint32_t enabled);
/* Whether a pair with an AVN_SHAPE_CAPSULE collider on either side is tested ("capsule colliders" above), in both sweep modes.  Sticky; off in
 * a new world, where such a pair is skipped as it always was.  May be toggled between steps at any time: it strands no state and takes effect
 * from the next pass.  AVN_SHAPE_HOST and child colliders as targets stay declared deviations. */
AVN_API avn_status avn_swept_ccd_capsules_set(avn_world* w, uint32_t enabled);
/* The statistics of the last step's pass (waits for it); zeros if no pass has run since the list was uploaded. */
AVN_API avn_status avn_swept_ccd_stats_get(avn_world* w, avn_swept_ccd_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* AVIAN_MI355X_CCD_H */
