/*
 * avian_mi355x_trimesh.h — the Triangle collider (parry's Triangle, Avian's Collider::triangle; a static triangle mesh is one such collider
 * per face) as a device kind of the HIP backend: its table in HBM, its AABB, its contact manifolds against a Ball, a Capsule or a Cuboid in
 * the narrow phase, the device closed loop and a batch query.
 *
 * Conventions are those of avian_mi355x.h.  These entry points are plain `avn_*` functions of libavian_mi355x.so; they are not part of the
 * AVN_FN list of the main header and the CPU oracle does not have them (there a triangle stays an AVN_SHAPE_HOST collider).
 *
 * THE DEFINITION (avian_amd/csrc/avn_triangle_pair.h and tests/triangle_collider_reference.py follow it operation for operation in the
 * world's scalar, every operation rounded once, no fused multiply-add; parry is not vendored and its triangle manifolds cannot be restated
 * bit for bit: parity with parry is UNPINNED, as for the capsule collider).
 *  The triangle (a, b, c), given in the collider's frame, is two-sided and has zero thickness.  Edge k is (ab, bc, ca)[k]; bit k of the edge
 *  flags says that edge k is a real edge (boundary or convex), a clear bit that it is interior (shared with a coplanar or concave neighbour:
 *  avian_amd/trimesh.py computes the flags from mesh adjacency).  N = cross(b - a, c - a) / |cross(b - a, c - a)| is the face normal.
 *  AABB: the component-wise min / max of position + qrot(rotation, v) over v = a, b, c (avn_math.h's qrot), at the collider's pose (a child
 *   collider's own pose); update_aabb merges the boxes of the start and the predicted end pose and grows them as for every other kind.
 *  INTERIOR-EDGE RULE: where the feature of the triangle that gives the contact direction is an edge whose flag is clear, or a vertex both of
 *   whose edges have their flags clear, the normal is N signed towards the other shape and depths are measured along it; the acceptance test
 *   stays on the true distance.
 *  Manifolds are computed in nalgebra's arithmetic (avn_narrow.h's na_* functions, make_isometry, pos12 = iso_inv_mul) and converted as
 *  contact_query::contact_manifolds converts every manifold (local normal of shape 1 -> world normal, anchor1 = qrot(rotation1, local point) +
 *  normal * dist / 2).  Both slot orders are defined: `flipped` = the triangle is shape 2, and then the local normal and point are the other
 *  shape's.
 *  triangle - ball: q = the closest point of the triangle to the centre (Ericson 5.1.5 in its order of tests; region = face, edge k or vertex
 *   k), d = centre - q, dist = |d|.  No manifold unless 0 < dist <= r + prediction.  n = d / dist, depth = dist - r; under the interior-edge
 *   rule n = +-N (towards the centre) and depth = dot(d, n) - r.  One point: q on the triangle (feature = the region), or n_ball * r on the
 *   ball with n_ball = -n in the ball's frame.
 *  triangle - capsule: the core A + s u (A = t - hv, u = 2 hv, hv = na_qrot(r, (0, h, 0)) in the triangle's frame).  If its ends lie
 *   strictly on both sides of the face's plane and the crossing point's closest feature is the face: one point, the end deeper along the side
 *   of the core's middle, depth = its plane distance - r.  Otherwise the closest pair among (end A, triangle), (end B, triangle) and (core,
 *   edge k) for k = 0, 1, 2 (the segment - segment routine of the capsule collider; strict <, the first smallest wins) gives dist, the
 *   triangle's feature and n as for the ball (the face and the interior-edge rule: +-N); accepted when 0 < dist <= r + prediction.  When the
 *   feature is the face and the core has a length, the core is clipped to the prism over the triangle; an interval lo < hi gives two points
 *   (feature ids vertex 0 / vertex 1 on the capsule) each within r + prediction of the plane; else the one closest pair.
 *  triangle - cuboid, in the cuboid's frame (SAT): the candidate axes are the three box faces, N, and the nine normalised cross products of a
 *   triangle edge with a box axis (skipped when shorter than eps |edge|); any separation > prediction: no manifold.  The direction is the
 *   candidate with the greatest separation (strict >, in that order) among N, the box faces that are ADMISSIBLE (the triangle's lowest
 *   feature along the face normal is the whole face, or a real -- not interior -- edge or vertex one of whose vertices lies over the box face,
 *   |x_j| <= he_j on the two other axes), and the edge axes of FLAGGED edges that are the triangle's lowest feature along them (the opposite
 *   vertex is not strictly lower).  Edge axis: one point, the closest points of the triangle's edge and the box's supporting edge.  Box face:
 *   the triangle clipped (Sutherland - Hodgman) to the face's four side planes, every corner within the prediction of the face's plane is a
 *   point.  N: the box's support face (cuboid_support_face) clipped to the three planes of the prism over the triangle, every corner within
 *   the prediction of the triangle's plane is a point.  The clipped polygon holds at most 8 corners: a corner that would be the ninth is
 *   dropped, in the clip's own order -- this cap is part of the definition.  A manifold holds only what lies over its reference feature: a
 *   pair within the prediction distance whose clipped polygon has no corner within it has no manifold.
 *  FEATURE IDS: PackedFeatureId's vertex / edge / face classes.  The triangle's: vertex k, edge k, face 0 for the ball and capsule cases and
 *   the edge case of the cuboid; a clipped corner is vertex k (an original vertex), edge (original edge | (plane + 1) << 2) (an original edge
 *   cut by a clip plane) or face 16 + 4 * plane_a + plane_b (the crossing of two clip planes).  The cuboid's: cuboid_support_face's numbering
 *   for faces, vertices and edges; a clipped corner of its support face carries (plane + 1) << 8 on the edge id or (1 + 3 * plane_a + plane_b)
 *   << 8 on the face id.  A ball's and a capsule's side: face 0 (the capsule's two clip points: vertex 0 / 1).
 *  TWO TRIANGLES: no manifold (not built: it cannot arise for meshes on static bodies).
 *
 * IN THE WORLD: avn_colliders_upload accepts shape = AVN_SHAPE_TRIANGLE (half_extents ignored) and counts such colliders; while that count
 * is not zero and no table has been uploaded (avn_collider_triangles_upload after EVERY avn_colliders_upload, which clears the table),
 * avn_step and the systems return AVN_ERR_STATE before doing anything.  With the table in force update_aabb, the narrow phase (host-driven and
 * device closed loop), collision hooks (which see triangle pairs like any other pair) and sleeping treat the collider like every other device
 * kind; a pair of a triangle and an AVN_SHAPE_HOST collider stays the host's.  A world without a triangle launches exactly the kernels it
 * launches without this header and leaves the same bytes.
 * SPATIAL QUERIES: by default the spatial queries, the casters and move-and-slide leave triangles out exactly as they leave AVN_SHAPE_HOST
 * colliders out (AVN_ERR_STATE unless AVN_SPATIAL_SKIP_HOST_SHAPES; avn_spatial_stats.host_skipped counts them).  avn_spatial_triangle_colliders_set
 * (avian_mi355x_spatial.h, "queries against triangle colliders") switches them in as candidates of every query, for the three query shapes.
 * DECLARED DEVIATION: swept CCD skips a pair with a triangle on either side, as it skips host shapes (avian_mi355x_ccd.h says the same).
 * NOT BUILT: CCD against triangles, a triangle as a query shape, triangle - triangle, the oracle backend, Rust declarations, level-2 (halo plan) and
 * avn_dshard worlds.  avn_query_manifolds (AVN_FN(contact_manifolds)) still answers kind 4 with AVN_ERR_BAD_ARG: its struct has nowhere to
 * put vertices; avn_triangle_manifolds below is the batch query for pairs that may hold a triangle.
 */
#ifndef AVIAN_MI355X_TRIMESH_H
#define AVIAN_MI355X_TRIMESH_H

#include "avian_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AVN_SHAPE_TRIANGLE = 4 };
#define AVN_TRIANGLE_ALL_EDGES 7   /* every edge is a real edge: a lone triangle */

/* the triangles of the collider table; host pointers */
typedef struct avn_collider_triangles {
    uint32_t struct_size;        /* sizeof(avn_collider_triangles) */
    uint32_t count;              /* C of the last avn_colliders_upload */
    const void* vertices;        /* [9C] a, b, c in the collider's frame, the world's scalar; read only where that collider's shape is AVN_SHAPE_TRIANGLE */
    const uint8_t* edge_flags;   /* [C] bit k: edge k of (ab, bc, ca) is a real edge; NULL = AVN_TRIANGLE_ALL_EDGES everywhere */
} avn_collider_triangles;

/* One entry per collider, after every avn_colliders_upload (which clears the table).  AVN_ERR_BAD_ARG, with nothing changed (the previous
 * table stays in force): a wrong struct_size or count, a null `vertices`, and for a collider of kind AVN_SHAPE_TRIANGLE a vertex that is not
 * finite, a flag above 7 or a degenerate triangle -- |cross(b - a, c - a)|^2, computed in the world's scalar, is not > 0.
 * AVN_ERR_STATE: level-2 (halo plan) and avn_dshard worlds, and a call before any avn_colliders_upload. */
AVN_API avn_status avn_collider_triangles_upload(avn_world* w, const avn_collider_triangles* t);

/* avn_shape_pairs plus the triangles of the rows that hold one */
typedef struct avn_triangle_pairs {
    uint32_t struct_size;        /* sizeof(avn_triangle_pairs) */
    uint32_t count;
    const uint8_t* shape1;       /* [n] AVN_SHAPE_CUBOID, AVN_SHAPE_BALL, AVN_SHAPE_CAPSULE or AVN_SHAPE_TRIANGLE */
    const void* half_extents1;   /* [3n] (ignored for a triangle) */
    const void* position1;       /* [3n] */
    const void* rotation1;       /* [4n] xyzw */
    const uint8_t* shape2;
    const void* half_extents2;
    const void* position2;
    const void* rotation2;
    const void* prediction_distance;   /* [n] */
    const void* vertices1;       /* [9n] read only where shape1 is a triangle; may be NULL if no shape1 is */
    const void* vertices2;       /* [9n] likewise for shape2 */
    const uint8_t* edge_flags1;  /* [n] NULL = AVN_TRIANGLE_ALL_EDGES */
    const uint8_t* edge_flags2;  /* [n] NULL = AVN_TRIANGLE_ALL_EDGES */
} avn_triangle_pairs;

/* The batch form of contact_query::contact_manifolds for pairs that may hold a triangle.  Rows without a triangle answer exactly what
 * AVN_FN(contact_manifolds) answers; a row with two triangles answers no manifold.  AVN_ERR_BAD_ARG: kind 2 (AVN_SHAPE_HOST), a kind above 4,
 * a flag above 7, a wrong struct_size, a null array that is needed. */
AVN_API avn_status avn_triangle_manifolds(avn_world* w, const avn_triangle_pairs* q, const avn_query_manifolds_out* out);

#ifdef __cplusplus
}
#endif

#endif /* AVIAN_MI355X_TRIMESH_H */
