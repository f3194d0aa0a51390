/*
 * avian_mi355x_spatial.h — device spatial queries: ray casts, point and AABB intersections, point projection and shape intersections against
 * the colliders the world holds in HBM.  Of SpatialQueryPipeline's query families only the shape casts (cast_shape, shape_hits) are not here.
 *
 * Mirrors Avian's `SpatialQueryPlugin` (spatial_query/mod.rs:190-212), whose systems run in `PhysicsStepSystems::SpatialQuery` right after
 * `Sleeping` (schedule/mod.rs:98-105): `update_spatial_query_pipeline` rebuilds a BVH of every collider from `Position` / `Rotation`
 * (spatial_query/pipeline.rs:96-133), and the queries of `SpatialQueryPipeline` / the `raycast` system of `RayCaster` read it.
 * Here the structure is an LBVH built on the device from the poses the device holds (avn_spatial_update); the queries traverse it one lane
 * per query.  The BVH only culls: every answer comes from an exact per-collider test (below), so the result equals a brute-force pass
 * over all colliders with the same tests, bit for bit.
 *
 * Conventions are those of avian_mi355x.h (scalar type = the world's, vectors interleaved xyz, quaternions xyzw, every call returns
 * avn_status with a message in avn_last_error).  The calls are synchronous: they return once the outputs are written.  These entry
 * points are plain `avn_spatial_*` functions of libavian_mi355x.so; they are not part of the AVN_FN list of the main header.
 *
 * Exact per-collider tests (restatements of parry3d's published algorithms; parry's source is not vendored, so the parity of these
 * functions against parry is UNPINNED -- they are defined here and the device and the test suite's restatement agree bit for bit):
 *  - pose: collider_pose (child colliders through ColliderTransform), then the ray / point in the collider's local frame with the
 *    conjugate rotation (parry's Ray::inverse_transform_by): o_l = rot^-1 (o - pos), d_l = rot^-1 d.
 *  - cuboid: parry's local-AABB slab clip (Aabb::cast_local_ray_and_get_normal).  Per axis with d != 0: t_near / t_far of the two
 *    faces; the entry is the largest t_near (strict >, so at an edge or corner the first axis in x, y, z order gives the normal), the
 *    exit the smallest t_far (strict <).  An axis with d == 0 is a parallel slab: a miss when the origin lies outside it.  A miss when
 *    entry > exit or exit < 0.  Origin inside (entry < 0): solid -> distance 0, normal 0; not solid -> the exit distance and the exit
 *    face's normal.  Otherwise the entry distance and the entry face's outward normal.
 *  - ball: parry's ray_toi_with_ball with its discriminant in a well-conditioned form: a = |d|^2, b = o.d, c = |o|^2 - r^2; a miss when
 *    c > 0 && b > 0; delta = a (r^2 - |f|^2) with f = o - d (b / a), the offset of the ray's point nearest the centre; a miss when
 *    delta < 0; t = (-b - sqrt(delta)) / a; t <= 0 (inside): solid -> 0 with normal 0, else (-b + sqrt(delta)) / a.  The normal is
 *    (o + d t) / |o + d t| (0 when that is 0).  delta equals parry's b^2 - a c in exact arithmetic; parry's form rounds with an error of
 *    eps |o|^2 (far from the ball it accepts rays that miss by a whole radius), this one with eps |o| r, so the two decide differently only
 *    inside the band where parry's own rounding decides.
 *  - a hit counts when its distance is finite and <= max_distance (max_distance = +inf is legal); the local normal is rotated back to
 *    world space.
 *  - point containment: |p_l.i| <= he.i for a cuboid, |p_l|^2 <= r^2 for a ball.
 *  - AABB: the collider's exact shape AABB at the snapshot pose (the broad phase's shape_aabb, no margins) intersects the query box
 *    (min <= other.max && max >= other.min per axis).
 *  - point projection (SpatialQueryPipeline::project_point; parry's PointQuery::project_local_point of Ball and Cuboid plus the
 *    nearest-collider search of a composite shape).  p_l = rot^-1 (p - pos) as above.
 *      ball: d2 = |p_l|^2, inside = d2 <= r^2 (the containment predicate above).  solid && inside: the projection is the query point itself,
 *        bit for bit, at distance 0.  Otherwise proj_l = p_l * (r / sqrt(d2)); when d2 == 0 (a hollow ball asked at its centre, where
 *        every surface point is nearest) proj_l = (0, r, 0): THIS LIBRARY'S CHOICE, defined here.
 *      cuboid: inside = |p_l.i| <= he.i on all axes.  Outside: each component clamped to [-he.i, he.i].  Inside and solid: the query point
 *        itself, distance 0.  Inside and hollow: the axis with the smallest he.i - |p_l.i| (strict <: the first axis in x, y, z order
 *        wins a tie) has its component set to copysign(he.i, p_l.i).
 *      distance = sqrt(dot(diff, diff)), diff = p_l - proj_l (local frame); the world point is rot * proj_l + pos, rotated back as the ray
 *      normal is.  A projection needs a finite distance.  The answer of a query is the smallest (distance, collider index): with solid = 1
 *      a point inside several colliders answers the lowest-indexed one at distance 0, which is point_intersections' first collider.
 *  - shape intersection (SpatialQueryPipeline::shape_intersections; parry's intersection_test of Ball / Cuboid pairs).  Shape 1 is the
 *    query, shape 2 the collider: pos12 = iso_inv_mul(make_isometry(query position, query rotation), {collider rotation, collider
 *    position}) in nalgebra's arithmetic (avn_narrow.h).  Touching counts as intersecting.
 *      ball / ball: |pos12.t|^2 <= (r1 + r2)^2.
 *      ball query / cuboid collider: c = iso_inv_point(pos12, 0), the ball's centre in the cuboid's frame; intersecting when c is inside
 *        (the containment predicate) or |c - clamp(c)|^2 <= r^2.  Cuboid query / ball collider: the same with c = pos12.t.
 *      cuboid / cuboid: parry's intersection_test_cuboid_cuboid, in this order: sat_normal_oneway(he1, he2, pos12) > 0 -> disjoint;
 *        sat_normal_oneway(he2, he1, iso_inverse(pos12)) > 0 -> disjoint; sat_edge_twoway(he1, he2, pos12) > 0 -> disjoint (edge axes
 *        whose norm is <= eps are skipped); otherwise intersecting.  The three functions are the narrow phase's.
 *
 * Non-finite inputs (NaN or inf components):
 *  - a collider whose snapshot position, rotation or shape AABB is not finite is never a candidate (it keeps its collider index);
 *  - a query whose origin, direction, point or box corner is not finite answers a miss (ray queries, projection) or a count of 0, whatever
 *    the scene;
 *  - a query shape whose kind is neither AVN_SHAPE_CUBOID nor AVN_SHAPE_BALL, whose position, rotation, half extents (a ball: its radius) or
 *    AABB are not finite, or which has a negative half extent, answers a count of 0.  This is decided per query on the device;
 *  - a hit needs a finite distance.
 *  Answers to finite inputs do not depend on these rules.
 *
 * Accuracy: every answer is the exact test above in the world's scalar type.  tests/spatial_exact_geometry.py states the forward-error
 * bound the answers are held to against exact rational geometry (a few eps times the magnitudes of the ray, the pose, the shape and the
 * distance; for balls, plus the grazing term of the square root).
 *
 * Snapshot rules:
 *  - a query before any avn_spatial_update, or after avn_bodies_upload / avn_colliders_upload / avn_collider_transforms_upload /
 *    avn_despawn changed the tables without a new update, returns AVN_ERR_STATE.  Steps do not invalidate the snapshot: queries answer
 *    against the poses of the last update, as Avian's pipeline does between updates (SpatialQuery::update_pipeline).
 *  - AVN_SHAPE_HOST colliders have no device geometry: if the snapshot holds any, queries return AVN_ERR_STATE unless the query sets
 *    AVN_SPATIAL_SKIP_HOST_SHAPES; with the flag they are never candidates (avn_spatial_stats.host_skipped counts them).
 *  - sensors, sleeping and static bodies' colliders are all candidates, as in Avian's pipeline.
 *
 * Filter (SpatialQueryFilter::test, query_filter.rs:97-101): a collider is a candidate when memberships & mask != 0 and its
 * entity_index is not in the excluded list.  ONE excluded list is shared by every query of a call (a caster's own entity goes in it for
 * RayCaster::ignore_self); per-query exclusion lists are not supported.
 *
 * Ties: closest hit = smallest (distance, collider index); ray_hits = the max_hits nearest by (distance, collider index), sorted, plus
 * the true number of hits (Avian returns an arbitrary subset when truncated: nearest-k is a deterministic strengthening); point and AABB
 * intersections = ascending collider index, the first `cap`, plus the true count; shape intersections the same; a projection = the
 * smallest (distance, collider index).  A collider index is its slot in the last avn_colliders_upload.
 */
#ifndef AVIAN_MI355X_SPATIAL_H
#define AVIAN_MI355X_SPATIAL_H

#include "avian_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of a query */
enum {
    AVN_SPATIAL_DEVICE_POINTERS = 1,   /* every input and output array of the call (filter included) is a device pointer on the world's device;
                                          the caller's writes to them must be complete before the call */
    AVN_SPATIAL_SKIP_HOST_SHAPES = 2   /* AVN_SHAPE_HOST colliders are never candidates (else their presence is AVN_ERR_STATE) */
};
#define AVN_SPATIAL_MAX_HITS 64        /* largest max_hits of avn_spatial_ray_hits */
#define AVN_SPATIAL_MISS 0xFFFFFFFFu   /* collider index of a miss */

typedef struct avn_spatial_filter {
    const uint32_t* mask;      /* [n] LayerMask per query; NULL = LayerMask::ALL */
    const uint32_t* excluded;  /* [n_excluded] collider entity_index values excluded from every query of the call; NULL if n_excluded == 0 */
    uint32_t n_excluded;
} avn_spatial_filter;

typedef struct avn_spatial_rays {
    uint32_t count;              /* n */
    uint32_t flags;              /* AVN_SPATIAL_* */
    const void* origin;          /* [3n] */
    const void* direction;       /* [3n] unit (the caller normalises, as Dir3 does) */
    const void* max_distance;    /* [n] */
    const uint8_t* solid;        /* [n] 1: an origin inside a shape hits at distance 0 */
    avn_spatial_filter filter;
} avn_spatial_rays;

typedef struct avn_spatial_points {
    uint32_t count;
    uint32_t flags;
    const void* point;           /* [3n] */
    avn_spatial_filter filter;
} avn_spatial_points;

typedef struct avn_spatial_aabbs {
    uint32_t count;
    uint32_t flags;
    const void* min;             /* [3n] */
    const void* max;             /* [3n] */
    avn_spatial_filter filter;
} avn_spatial_aabbs;

typedef struct avn_spatial_solid_points {
    uint32_t count;
    uint32_t flags;
    const void* point;           /* [3n] */
    const uint8_t* solid;        /* [n] 1: a point inside a shape projects onto itself at distance 0; 0: onto the shape's boundary */
    avn_spatial_filter filter;
} avn_spatial_solid_points;

/* the query shapes of avn_spatial_shape_intersections (a later shape cast takes the same record) */
typedef struct avn_spatial_shapes {
    uint32_t count;
    uint32_t flags;
    const uint8_t* shape;        /* [n] AVN_SHAPE_CUBOID / AVN_SHAPE_BALL */
    const void* half_extents;    /* [3n] (ball: radius in x, as in the collider table) */
    const void* position;        /* [3n] */
    const void* rotation;        /* [4n] xyzw, unit (the caller normalises) */
    avn_spatial_filter filter;
} avn_spatial_shapes;

/* RayHitData (ray_caster.rs) with the collider's table index */
typedef struct avn_spatial_hit_f32 {
    uint32_t collider;   /* slot of the last avn_colliders_upload; AVN_SPATIAL_MISS = no hit (entity too; distance and normal 0) */
    uint32_t entity;     /* entity_index as uploaded */
    float distance;      /* time_of_impact */
    float normal[3];     /* world space */
} avn_spatial_hit_f32;
typedef struct avn_spatial_hit_f64 {
    uint32_t collider;
    uint32_t entity;
    double distance;
    double normal[3];
} avn_spatial_hit_f64;

/* PointProjection (spatial_query/pipeline.rs) with the collider's table index and the distance */
typedef struct avn_spatial_projection_f32 {
    uint32_t collider;   /* AVN_SPATIAL_MISS = no candidate (entity too; the rest 0) */
    uint32_t entity;
    uint32_t is_inside;  /* 0 / 1: the point lies inside the collider (whatever `solid` says) */
    float point[3];      /* world space */
    float distance;      /* |point - projection| as computed in the collider's frame */
} avn_spatial_projection_f32;
typedef struct avn_spatial_projection_f64 {
    uint32_t collider;
    uint32_t entity;
    uint32_t is_inside;
    uint32_t reserved;   /* always written as 0: every byte of a record is defined */
    double point[3];
    double distance;
} avn_spatial_projection_f64;

typedef struct avn_spatial_projections_out {
    void* projection;    /* avn_spatial_projection_fNN [n] */
} avn_spatial_projections_out;

typedef struct avn_spatial_hits_out {
    void* hits;          /* avn_spatial_hit_fNN [n] (cast_rays) or [n * max_hits] (ray_hits; unused slots are misses) */
    uint32_t* count;     /* [n] true number of hits (ray_hits); ignored by cast_rays */
} avn_spatial_hits_out;

typedef struct avn_spatial_ids_out {
    uint32_t* collider;  /* [n * cap] collider indices, ascending, AVN_SPATIAL_MISS past the count */
    uint32_t* count;     /* [n] true number of colliders */
} avn_spatial_ids_out;

typedef struct avn_spatial_stats {
    uint32_t colliders;        /* colliders in the snapshot */
    uint32_t nodes;            /* BVH nodes (2 * colliders - 1) */
    uint32_t host_skipped;     /* AVN_SHAPE_HOST colliders in the snapshot (never candidates) */
    uint32_t valid;            /* 1: the snapshot can be queried */
    uint64_t nodes_visited;    /* last query call: node boxes tested, all queries together */
    uint64_t leaves_visited;   /* last query call: exact per-collider tests run, all queries together */
} avn_spatial_stats;

/* update_spatial_query_pipeline / SpatialQueryPipeline::update (pipeline.rs:96-133): builds the LBVH from the poses the device holds when the
 * call runs, enqueued on the world's stream after any step work.  avn_step never calls it. */
AVN_API avn_status avn_spatial_update(avn_world* w);
/* SpatialQueryPipeline::cast_ray (pipeline.rs:162-231); RayCaster with max_hits = 1: per ray the closest hit within max_distance, or a miss */
AVN_API avn_status avn_spatial_cast_rays(avn_world* w, const avn_spatial_rays* rays, const avn_spatial_hits_out* out);
/* SpatialQueryPipeline::ray_hits (pipeline.rs:233-333); RayCaster / RayHits: per ray the max_hits nearest hits, sorted, plus the true count.
 * 1 <= max_hits <= AVN_SPATIAL_MAX_HITS, else AVN_ERR_BAD_ARG. */
AVN_API avn_status avn_spatial_ray_hits(avn_world* w, const avn_spatial_rays* rays, uint32_t max_hits, const avn_spatial_hits_out* out);
/* SpatialQueryPipeline::point_intersections (pipeline.rs:628-689): per point the colliders containing it */
AVN_API avn_status avn_spatial_point_intersections(avn_world* w, const avn_spatial_points* points, uint32_t cap, const avn_spatial_ids_out* out);
/* SpatialQueryPipeline::aabb_intersections_with_aabb (pipeline.rs:691-742): per box the colliders whose shape AABB intersects it */
AVN_API avn_status avn_spatial_aabb_intersections(avn_world* w, const avn_spatial_aabbs* boxes, uint32_t cap, const avn_spatial_ids_out* out);
/* SpatialQueryPipeline::project_point (pipeline.rs:570-615) per point: the nearest collider's projection, or a miss when there is no candidate */
AVN_API avn_status avn_spatial_project_points(avn_world* w, const avn_spatial_solid_points* points, const avn_spatial_projections_out* out);
/* SpatialQueryPipeline::shape_intersections (pipeline.rs:744-826): per query shape the colliders intersecting it.  cap = 0 is legal (counts only) */
AVN_API avn_status avn_spatial_shape_intersections(avn_world* w, const avn_spatial_shapes* shapes, uint32_t cap, const avn_spatial_ids_out* out);
/* snapshot sizes and the traversal counters of the last query call */
AVN_API avn_status avn_spatial_stats_get(avn_world* w, avn_spatial_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* AVIAN_MI355X_SPATIAL_H */
