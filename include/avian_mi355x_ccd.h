/*
 * avian_mi355x_ccd.h — swept continuous collision detection (the SweptCcd component, dynamics/ccd/mod.rs) inside the device closed loop.
 *
 * Mirrors `solve_swept_ccd` (ccd/mod.rs:523-687), the system of PhysicsStepSystems::Solver that the reference schedules after
 * SolverSystems::PostSubstep and before SolverSystems::Restitution (ccd/mod.rs:257-261): per SweptCcd body it finds the first time of impact
 * against the colliders whose AABBs its own collider's AABB intersects and moves both bodies back to that time, so that a fast body stops
 * at a thin wall instead of passing through it.  Only SweepMode::Linear is built, for Ball / Cuboid colliders; the pass runs on the world's
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
 *     deviation); when either collider is AVN_SHAPE_HOST or AVN_SHAPE_CAPSULE (every kind above Ball is skipped: a declared deviation; capsule colliders have no cast here yet); when include_dynamic == 0 and b2 is dynamic, awake or
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
 * NOT covered: SweepMode::NonLinear (the upload refuses it), shapes other than Ball / Cuboid, child and host-shape colliders as targets,
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
    const uint32_t* mode;             /* [n] AVN_SWEEP_LINEAR (AVN_SWEEP_NON_LINEAR is refused) */
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

/* Replaces the world's list (NULL or count 0 clears it).  AVN_ERR_BAD_ARG, with the previous list left in force: a mode other than
 * AVN_SWEEP_LINEAR, a body index outside the body table, a body named twice, a null array.  AVN_ERR_STATE: level-2 (halo plan) and
 * avn_dshard worlds.  avn_bodies_upload with another body count and avn_despawn clear the list: its indices are stale.
 * With a non-empty list avn_step and AVN_SYS_SOLVER return AVN_ERR_STATE, before doing anything, unless the world is in device closed-loop
 * mode (avn_pipeline_enable(w, 1)): the pass reads the contact table that mode keeps. */
AVN_API avn_status avn_swept_ccd_upload(avn_world* w, const avn_swept_ccd* list);
/* The records of the last step's pass (waits for it).  More entries than `capacity`: AVN_ERR_CAPACITY with `count` set. */
AVN_API avn_status avn_swept_ccd_results_get(avn_world* w, avn_swept_ccd_results_out* out);

#ifdef __cplusplus
}
#endif

#endif /* AVIAN_MI355X_CCD_H */
