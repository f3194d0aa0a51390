/*
 * avian_mi355x_spatial.h — device spatial queries: ray casts, point and AABB intersections, point projection, shape intersections and shape
 * casts against the colliders the world holds in HBM: every query family of SpatialQueryPipeline, for the shapes with device geometry (Ball,
 * Cuboid); plus the kinematic character controller (character_controller/move_and_slide.rs): shape contacts and depenetration
 * (MoveAndSlide::intersections / depenetrate), project_velocity, cast_move and the move_and_slide loop.
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
 *  - shape cast (SpatialQueryPipeline::cast_shape / shape_hits; parry's cast_shapes with target_distance = 0, compute_contact_on_penetration =
 *    false).  Parry casts these pairs with an iterative GJK ray cast (ball / ball excepted) whose iteration cannot be restated bit for bit, so
 *    the time of impact per pair is DEFINED HERE, in closed form, in the collider's frame (shape 1 = the collider, shape 2 = the cast shape):
 *      q = iso_inv_mul({collider rotation, collider position}, make_isometry(query position, query rotation)),  d_l = na_qrot(rot_c^-1, d).
 *      A local ball-ray test B(o, d, r) and slab clip S(o, d, h) are the ray tests above, solid: B: a, b, c as above, a miss when c > 0 &&
 *      b > 0, delta = a (r^2 - |f|^2), a miss when delta < 0, t = (-b - sqrt(delta)) / a, t <= 0 -> inside, t = 0.  S: entry = the largest
 *      t_near (strict >), exit = the smallest t_far, a miss when entry > exit or exit < 0, entry < 0 -> inside, t = 0.
 *      ball / ball: B(q.t, d_l, r_c + r_q).  n = (q.t + d_l t) / |q.t + d_l t| (0 when that is 0); point1 = rot_c (n r_c) + pos_c.
 *      ball and cuboid, in either role: the ray (o, dd) of the ball's centre against the cuboid rounded by the ball's radius r, in the
 *        cuboid's frame.  A ball cast at a cuboid collider: o = q.t, dd = d_l.  A cuboid cast at a ball collider (the ray reversed in the
 *        cuboid's, i.e. the query's, frame): o = iso_inv_point(q, 0), dd = -iso_inv_vec(q, d_l); the two sides of the record swap.  The
 *        rounded cuboid is the union of, in this order: the three boxes he + r e_i (S; i = x, y, z), and when r > 0 the twelve edge
 *        cylinders (edge direction k = x, y, z; a = k + 1, b = k + 2 mod 3; the edge through (sa he_a, sb he_b), e = 4 k + (sa > 0) + 2 (sb >
 *        0); B on the (a, b) components alone, left out when those components of dd are both 0, accepted when |o_k + dd_k t| <= he_k) and the eight corner spheres (bit 0 / 1 / 2 of
 *        the index = the sign of x / y / z; B).  The distance is the smallest entry over the primitives (strict <: the first in that order
 *        wins a tie) and the normal is that primitive's: the entry face's, (p_a, p_b) / |(p_a, p_b)| of the cylinder, p / |p| of the sphere.
 *        Every quadratic is B's nearest-point-offset form.  The cuboid's witness is (o + dd t) - n r, the ball's its centre - n_world r.
 *      cuboid / cuboid: a swept SAT over 15 axes in the collider's frame: e_0..e_2, u_j = q.r e_j (j = 0..2), then e_a x u_b normalised, b
 *        outer and a inner (sat_edge_twoway's order), skipped when its norm <= eps.  Per axis: s0 = axis . q.t, v = axis . d_l, R = sum
 *        |axis_i| he_c.i + sum |axis . u_j| he_q.j.  v != 0: t1 = (-R - s0) / v, t2 = (R - s0) / v, swapped when 1 / v < 0; the entry is the
 *        largest t1 (strict >, the first axis wins), the exit the smallest t2.  v == 0: a parallel slab, a miss when |s0| > R.  A miss when
 *        entry > exit or exit < 0; entry < 0: overlapping at the start.  The normal n is the winning axis oriented from the collider towards
 *        the query (-axis when 1 / v > 0).  Witnesses at the impact pose t' = q.t + d_l t.  A face axis of the collider: the query's support
 *        vertex s2 = q.r support(he_q, q.r^-1 (-n)) + t' (cuboid_support_point's sign rule) and its projection onto the face (component k set
 *        to n_k he_c.k).  A face axis of the query: s1 = support(he_c, n) and s1 - n ((s1 - t') . n + he_q.j).  An edge axis: the closest
 *        points of the lines s1 + lambda e_a and s2 + mu u_b (den = |u_b|^2 - (e_a . u_b)^2; when den <= eps the collider's point is the
 *        middle of its edge).  When faces or edges are parallel the contact is a segment or a polygon and such a witness can fall outside the
 *        other shape's face or edge (|coordinate| > half extent on a tangential axis, or den <= eps).  Then, with C(p) the clamp of p to the
 *        collider's cuboid and Q(p) the query cuboid's closest point to p (clamped in its frame at the impact pose), the witnesses are
 *        point1 = C(Q(C(p))) and point2 = Q(point1), p being the collider-side witness (for a face axis of the query: the point of that face
 *        nearest s1).  Each point then lies on its own shape; they coincide when the edges of the two faces are parallel (axis-aligned
 *        stacks), and otherwise wherever the clamps land in the overlap.
 *      all three: the shapes overlapping at the start answer distance 0 with points and normals 0 (the convention of a solid ray's normal);
 *      a hit needs a finite distance <= max_distance; normal1 = rot_c n, point1 / point2 in world space through rot_c and pos_c (a cuboid
 *      cast at a ball: through the query's isometry at pos_q + d t), normal2 = -normal1 with a zero component staying +0.
 *    NOT covered: target_distance != 0, compute_contact_on_penetration = true, predicates (cast_shape_predicate) other than cast_move's,
 *    casts against AVN_SHAPE_HOST colliders, Rust declarations.  (ignore_origin_penetration: avn_spatial_cast_moves, below.)
 *  - shape contacts (MoveAndSlide::intersections, character_controller/move_and_slide.rs:1032-1078).  Per query shape at its pose with a
 *    prediction distance p, collider c contributes ONE contact iff all of (a)-(d) hold, evaluated in this order:
 *      (a) c is a candidate and passes the filter (with AVN_SPATIAL_SKIP_SENSORS: and is not a sensor).
 *      (b) the AABB precondition (Avian's aabb_intersections_with_aabb(shape.aabb().grow(p)); part of the definition, not a culling step):
 *          [a, b] = shape_aabb of the query shape at its pose (the broad phase's shape_aabb, no margins), qmin = a - p, qmax = b + p per
 *          component; [mn, mx] = shape_aabb of the collider at its snapshot pose, computed from the snapshot's pose and half extents with the
 *          same function (not the padded leaf box); the boxes intersect: mn <= qmax && mx >= qmin per axis.
 *      (c) contact_query::contact_manifolds(query as shape 1, collider as shape 2, prediction p) returns a manifold: the narrow phase's own
 *          per-pair function (avn_contact_manifolds of avian_mi355x.h is its batch form), poses through make_isometry.
 *      (d) the manifold's deepest raw point exists: ContactManifold::find_deepest_contact, Rust's max_by over the raw points in emission
 *          order, where the LATER point wins a tie.  As a fold over the raw points (at most 16), best = the first point, then
 *          if (!(best.penetration > pt.penetration)) best = pt.
 *    The record: penetration = best.penetration; normal = -manifold.normal per component (from the collider towards the query shape, the
 *    direction MoveAndSlide::intersections hands to its callback); anchor1 = best.anchor1 (relative to the query shape's position);
 *    anchor2 = anchor1 + (query position - collider position); point = query position + anchor1.
 *    Per query the records come in ascending collider index, the first `cap`, plus the true count (Avian's order is its BVH's traversal
 *    order, which is arbitrary: ascending index is a deterministic strengthening).  Unused slots: both ids AVN_SPATIAL_MISS, the rest 0.
 *  - depenetration (MoveAndSlide::depenetrate = intersections with prediction skin_width, then depenetrate_intersections,
 *    move_and_slide.rs:982-1009).  With the contacts of the query in ascending collider index (at most AVN_SPATIAL_MAX_HITS of them; with
 *    more, `truncated` is 1 and the fixup comes from the first AVN_SPATIAL_MAX_HITS) and the configuration cast once to the world's scalar:
 *      fixup = 0;  repeat up to `iterations` times:  total_error = 0;  for each contact in order:  dist = penetration + skin_width;
 *      skipped when dist > penetration_rejection_threshold;  error = max(dist - (fixup.x n.x + fixup.y n.y + fixup.z n.z), 0) (a NaN
 *      difference gives 0);  total_error += error;  fixup += error * n (per component);  after the pass: stop when total_error <
 *      max_depenetration_error.  iterations_run counts the passes started.  Avian hands the normal over as a Dir, which is f32: in an f64
 *      world every component of n is rounded through float before use (the contact records keep the full-precision normal).  The caller
 *      applies PhysicsLengthUnit to max_depenetration_error and penetration_rejection_threshold.
 *    NOT covered: query shapes other than Ball / Cuboid / Capsule (cylinders, cones, hulls), contacts against AVN_SHAPE_HOST colliders, predicates, Rust declarations.
 *  - capsule query shapes (AVN_SHAPE_CAPSULE; parry's Capsule::new_y, the shape of Avian's character-controller examples).  A capsule is a
 *    QUERY shape here: every entry point that takes a query shape accepts it against Ball and Cuboid colliders, and against Capsule colliders
 *    once avn_spatial_capsule_colliders_set has switched them in ("queries against capsule colliders" below; by default a capsule COLLIDER --
 *    avian_mi355x.h "capsule colliders" -- is to these queries what a host shape is: AVN_ERR_STATE unless AVN_SPATIAL_SKIP_HOST_SHAPES is set, then
 *    never a candidate and counted in host_skipped).  half_extents = (r, h, .): x the radius (as a ball keeps its radius in x), y the half length of the segment (0, -h, 0) ..
 *    (0, +h, 0) of the shape's frame, z not read; Collider::capsule(radius, length) is r = radius, h = length / 2.  Valid: finite r and h,
 *    both >= 0 (h == 0 is a ball, r == 0 a segment, both 0 a point), the usual finite pose, and a finite AABB
 *      [a, b] = position -+ (|qrot(rotation, (0, h, 0))| + (r, r, r))   per component (qrot: the function collider_pose uses),
 *    which stands wherever a query shape's shape_aabb stands above (node tests, the AABB precondition (b) of a contact).  As for the shape
 *    casts the pair tests are DEFINED HERE with their operation order (no FMA contraction); parity with parry is UNPINNED.  All of them
 *    work in the collider's frame on the capsule's core, the segment A + s u, s in [0, 1]:
 *      q = iso_inv_mul({collider rotation, collider position}, make_isometry(query position, query rotation)), hv = na_qrot(q.r, (0, h, 0)),
 *      A = q.t - hv, u = 2 hv.  A ball collider's core is its centre (the origin) with radius r_c; a cuboid's core is the box, r_c = 0.
 *      dot is na_dot (left to right), clamp(p) the clamp of p to the box per component.
 *      P (segment - point c): uu = dot(u, u); s = dot(c - A, u) / uu clamped to [0, 1], 0 when uu == 0; d2 = |c - (A + u s)|^2.
 *      X (segment - box he, exact): f(s) = |x - clamp(x)|^2 at x = A + u s is convex and piecewise quadratic.  Breakpoints: per axis i = x, y, z
 *        and side -he_i then +he_i, b = (side - A_i) / u_i when u_i != 0 and 0 < b < 1, else 1; the six sorted ascending b_1..b_6, with b_0 = 0
 *        and b_7 = 1.  Candidates in this order: 0, 1, b_1..b_6, then for k = 0..6 the candidate of the interval [b_k, b_k+1]: mid = (b_k +
 *        b_k+1) / 2, m = A + u mid, sg_i = m_i > he_i ? 1 : m_i < -he_i ? -1 : 0 (the active faces); none active: mid; else den = the sum of
 *        u_i u_i and num = the sum of u_i (A_i - sg_i he_i) over the active axes in x, y, z order, the candidate is -num / den clamped to the
 *        interval when den > 0 and b_k otherwise.  Every candidate's f is evaluated in full; the first with the smallest f wins (strict <).
 *        X answers f, s, p_seg = A + u s and p_box = clamp(p_seg).
 *      intersection: P's d2 <= (r + r_c)^2 against a ball, X's f <= r * r against a cuboid (touching counts).
 *      cast against a ball collider: the ball's centre as a ray against the capsule of radius R = r + r_c in the capsule's frame, the ray
 *        reversed: o = iso_inv_point(q, 0), dd = -iso_inv_vec(q, d_l).  The capsule is, in this order, the cylinder about y (B on the (x, z)
 *        components alone, left out when those components of dd are both 0, accepted when |o_y + dd_y t| <= h) and the end spheres at (0, -h, 0)
 *        and (0, +h, 0) (B); the smallest entry wins (strict <) and gives the normal n_q ((p_x, 0, p_z) / |(p_x, p_z)| of the cylinder, p / |p|
 *        of a sphere).  normal1 = -rot_q n_q; point1 = pos_c + normal1 r_c; point2 = rot_q ((0, clamp(o_y + dd_y t, -h, h), 0) + n_q r) +
 *        (pos_q + d t).
 *      cast against a cuboid collider: there is no finite SAT for a rounded segment; the cast is Newton's iteration on the convex g(t) =
 *        sqrt(X(A + d_l t, u).f) - r from t = 0, at most 32 rounds.  A round: X at t, dist = sqrt(f), n = (p_seg - p_box) / dist (when
 *        dist is 0 the n of the round before stands, 0 in round 0).  dist <= r: overlap at the start in round 0, else a hit at t.  v = -dot(n, d_l); !(v > 0): a miss.  t' = t + (dist - r)
 *        / v; t' > max_distance: a miss; !(t' > t), or the 32nd round: a hit at t; else t = t'.  From the left of the root the iterates rise
 *        monotonically and do not pass it in exact arithmetic, so a hit under-estimates the distance, never over-estimates it.  normal1 =
 *        rot_c n; point1 = rot_c p_box + pos_c; point2 = rot_c (p_seg - n r) + pos_c.  Where the closest pair is not unique (a capsule side
 *        parallel to a face or an edge) the witness is the one X's candidate order picks: a deterministic strengthening.
 *      contact (the record of shape contacts, ONE point per collider, for a capsule query in place of (c) and (d); (a) and (b) unchanged):
 *        dist = sqrt(P.d2) or sqrt(X.f).  dist > 0: gap = (dist - r) - r_c; a contact iff !(gap > p); n = (p_seg - p_core) / dist,
 *        penetration = -gap, anchor1 = rot_c ((p_seg - n r) - q.t), anchor2 = rot_c (p_core + n r_c).  dist == 0 against a cuboid (the segment
 *        touches or crosses the box): the smallest overlap over the six axes of the Minkowski difference, e_0..e_2 then (u x e_i) / |u x e_i|
 *        (skipped when |u x e_i|^2 is not above eps^2 dot(u, u)), overlap = (sum |axis_i| he_i + |dot(axis, u / 2)|) - |dot(axis, A + u / 2)|,
 *        the first smallest wins; n = the axis signed towards the segment's midpoint, penetration = overlap + r, anchor1 from p_d - n r with
 *        p_d the segment's end deepest along -n (A on a tie), anchor2 from p_d projected onto the box's supporting plane of n.  dist == 0
 *        against a ball (its centre on the segment): no direction, no contact.  normal = rot_c n (from the collider towards the query), point
 *        = query position + anchor1.  cast_move's ORIGIN-PENETRATION RULE uses this contact at prediction 0 (point1 = collider position +
 *        anchor2); depenetration, project_velocity and the slide loop read records only and are unchanged.
 *    A capsule with h == 0 answers what the Ball query of radius r answers up to rounding (tests/test_spatial_capsule_cpu.py).
 *  - queries against capsule colliders (avn_spatial_capsule_colliders_set(w, 1); off by default, and then every answer is what it was before the
 *    switch existed).  With the switch on a capsule collider (r_c, h_c) = (half_extents.x, half_extents.y) is a candidate of every query: its leaf
 *    box is the capsule box [a, b] above at the collider's pose, padded like every other; host_skipped and the AVN_SPATIAL_SKIP_HOST_SHAPES rule
 *    are about AVN_SHAPE_HOST colliders alone.  The pair tests are DEFINED HERE with their operation order (no FMA contraction); parity with
 *    parry is UNPINNED.  The collider's core is the segment A_c + s u_c of its own frame, A_c = (0, -h_c, 0), u_c = (0, 2 h_c, 0); P, X, B and
 *    the cylinder-and-spheres ray are the ones of "capsule query shapes" above.
 *      S (segment - segment, A1 + s u1 against A2 + t u2, the clamped closest points; the capsule collider's manifold uses the same routine):
 *        w = A1 - A2; a = dot(u1, u1), e = dot(u2, u2), f = dot(u2, w), c = dot(u1, w), b = dot(u1, u2); clamp = to [0, 1].  a == 0 and e == 0:
 *        s = t = 0.  a == 0: s = 0, t = clamp(f / e).  e == 0: t = 0, s = clamp(-c / a).  Else den = a e - b b; s = 0 when !(den > 64 eps a e)
 *        (parallel axes), else clamp((b f - c e) / den); t = (b s + f) / e; t < 0: t = 0, s = clamp(-c / a); t > 1: t = 1, s = clamp((b - c) / a).
 *        p1 = A1 + u1 s, p2 = A2 + u2 t, d2 = |p2 - p1|^2.
 *      ray (in the collider's frame, o_l and d_l as for the other kinds): the entry is the cylinder-and-spheres ray with R = r_c.  An origin
 *        inside the winning primitive: solid answers distance 0 and a zero normal; not solid answers the EXIT, the largest (strict >) of, in
 *        this order, the cylinder's far root (-b + sqrt(delta)) / a on the (x, z) components (left out when those components of d_l are both 0
 *        or delta < 0, accepted when |o_y + d_y t| <= h_c) and the far roots of the spheres at (0, -h_c, 0) and (0, +h_c, 0) (delta = a (r_c^2 -
 *        |f|^2) with f = o - d (b / a), left out when delta < 0).  The normal is the outward surface normal of the winning primitive at the hit
 *        point ((p_x, 0, p_z) / |(p_x, p_z)| or p / |p|; a zero length: the zero normal), rotated by the collider's rotation.  max_distance
 *        and the finite-distance rule as for the other kinds.
 *      point intersection: P(A_c, u_c, point_l).d2 <= r_c^2.  AABB intersection: the capsule box against the query box.
 *      point projection: P gives the nearest core point p_c = A_c + u_c s and d2; is_inside = d2 <= r_c^2; the projection is the ball's about
 *        p_c: p_c + (0, r_c, 0) when d2 == 0, else p_c + (point_l - p_c) (r_c / sqrt(d2)); solid and the distance as for a ball.
 *      S' (the DISTANCE of two segments, for the queries): S's quotient cancels for nearly parallel axes and its parallel rule sets s = 0, which
 *        over-estimates the distance of converging or crossing cores; so six candidate (s, t) are evaluated in full, d2 = |p2 - p1|^2, and the first
 *        with the smallest d2 wins (strict <; a NaN never wins): S's own; the interior point in its well-conditioned form, with u2p = u2 - u1 (b / a)
 *        and wp = w - u1 (c / a): t = clamp(dot(wp, u2p) / dot(u2p, u2p)), s = clamp((b t - c) / a), t = clamp((b s + f) / e); and the four ends,
 *        (0, clamp(f / e)), (1, clamp((b + f) / e)), (clamp(-c / a), 0), (clamp((b - c) / a), 1).  The manifold of two capsules keeps S alone.
 *      shape intersection: a ball or a cuboid query: the capsule-query test above with the roles exchanged (the collider is the capsule, posed
 *        in the query's frame by iso_inv_mul(make_isometry(query), {collider rotation, collider position}); the query shape is the "collider"
 *        of that test).  A capsule query: S in the collider's frame with the collider's core as segment 1 and the query's (A, u of q above) as
 *        segment 2, the distance by S'; they intersect iff d2 <= (r + r_c)^2.
 *      shape cast (point1 / normal1 the collider's, point2 the query's at the impact pose; everything 0 when the shapes overlap at the start):
 *        a ball query (radius r): its centre q.t as a ray along d_l against the capsule of radius R = r_c + r in the collider's frame (the
 *          cylinder-and-spheres ray, not reversed), n its normal: normal1 = rot_c n; point1 = rot_c ((0, clamp(q.t_y + d_l_y t, -h_c, h_c), 0) +
 *          n r_c) + pos_c; point2 = (pos_q + d t) + (-normal1) r.
 *        a cuboid query: the Newton iteration of the capsule-query cast in the QUERY's frame: q' = iso_inv_mul(make_isometry(query), {collider
 *          rotation, collider position}), the collider's core (A, u of q', h_c) moves by d' = -iso_inv_vec(make_isometry(query), d) against the
 *          box he_q, radius r_c.  With R_q = make_isometry(query).r and c2 = pos_q + d t: normal1 = -(R_q n); point1 = R_q (p_seg - n r_c) + c2;
 *          point2 = R_q p_box + c2.
 *        a capsule query: the same iteration on g(t) = sqrt(S'(A_c, u_c, A + d_l t, u).d2) - (r + r_c) in the collider's frame, n = (p2 - p1) /
 *          dist: normal1 = rot_c n; point1 = rot_c (p1 + n r_c) + pos_c; point2 = rot_c (p2 - n r) + pos_c.
 *        The 32-round cap, the last t standing and "never an over-estimate" are those of the capsule-query cast.
 *      contacts (shape contacts, depenetration, cast_move's origin-penetration rule, move and slide): (a), (b) with the capsule box, then the
 *        narrow phase's capsule manifold of avian_mi355x.h "capsule colliders" with the query as shape 1 -- a ball or a cuboid query, and a
 *        capsule query against a capsule collider alike -- and (d)'s fold: the deepest point, the later point wins a tie.  A ball's centre on the
 *        collider's core, or two capsule cores that touch or cross, have no direction and give NO contact, as a ball's centre inside a cuboid gives
 *        none.  A cuboid query whose box the collider's core touches or crosses DOES get the manifold's six-axis contact -- the one place where an
 *        h_c == 0 capsule collider answers more than a Ball collider does (a Ball's centre inside a cuboid query: no contact).  A capsule query
 *        against Ball / Cuboid colliders keeps its own contact above.
 *    A capsule collider with h_c == 0 answers what a Ball collider of radius r_c answers up to rounding (tests/test_spatial_capsule_colliders_cpu.py).
 *    NOT covered: target_distance != 0, queries against AVN_SHAPE_HOST colliders.
 *  - queries against triangle colliders (avn_spatial_triangle_colliders_set(w, 1); off by default, and then every answer is what it was before the
 *    switch existed: a triangle collider -- avian_mi355x_trimesh.h -- is left out and counted like a host shape).  With the switch on a triangle
 *    collider is a candidate of every query, caster and move-and-slide call, for the three query shapes; host_skipped, the AVN_SPATIAL_SKIP_HOST_SHAPES
 *    rule and the state error stop counting and naming triangles.  The switch and avn_spatial_capsule_colliders_set are independent.  The collider is
 *    the triangle (a, b, c) of its table record in the collider's frame, two-sided and without interior; every test works in that frame (o_l, d_l, q as
 *    for the capsule collider).  The leaf reads the triangle from the WORLD's table at query time, not from a copy in the snapshot:
 *    avn_colliders_upload and avn_collider_triangles_upload both invalidate the snapshot, so no query reads a table newer than its snapshot.  The
 *    pair tests are DEFINED HERE with their operation order (no FMA contraction, dot = na_dot, cross = na_cross); parity with parry is UNPINNED.
 *    EDGE FLAGS matter only to the contacts; rays, projection, intersections and casts are pure geometry.  N = cross(b - a, c - a) / |.| (tri_unit_normal);
 *    C(p) = the closest point of the triangle to p by Ericson 5.1.5 in its order of tests with its region (the narrow phase's tri_closest_point).
 *      ray: den = dot(N, d_l); !(den != 0) (a parallel or coplanar ray, a zero direction, a NaN): a miss.  t = dot(N, a - o_l) / den; !(t >= 0): a
 *        miss (t == 0, the origin on the plane, is a hit).  Inside test, per edge k = 0, 1, 2 with v = v_k, v' = v_k+1: m = (v + v') * 0.5; o = o_l + d_l
 *        (dot(d_l, m - o_l) / dot(d_l, d_l)) (the ray's point nearest the edge's midpoint); s_k = dot(d_l, cross(v - o, v' - o)).  The ray is inside when
 *        no s_k is negative or no s_k is positive (a NaN is both).  m and the cross product are exactly symmetric / antisymmetric in (v, v'), so the two
 *        faces sharing an edge compute s_k of opposite sign bit for bit: a ray through a shared edge is never missed by both faces (both may hit; the
 *        traversal's tie rule, lower collider index, picks).  The normal is N turned against d_l (-N when den > 0) rotated by the collider's
 *        rotation; `solid` has no effect; hits from either side count; max_distance and the finite-distance rule as for the other kinds.
 *      point intersection: C(point_l) == point_l, component for component.  AABB intersection: the triangle's shape AABB (the min / max of the three
 *        posed vertices) against the query box.  The leaf box is that AABB padded like every kind's.
 *      point projection: C(point_l) carried back to the world; distance = |point_l - C(point_l)|; is_inside iff C(point_l) == point_l; `solid` has no effect.
 *      D (segment A + s u - triangle, squared distance with the closest points p_seg, p_tri; the narrow phase's triangle-capsule manifold uses the same
 *        candidates routine): B = A + u, da = dot(N, A - a), db = dot(N, B - a).  The ends strictly on opposite sides (da > 0 and db < 0, or the
 *        reverse) and X = A + u (da / (da - db)) with C(X) in the face region: 0, p_seg = X, p_tri = C(X).  Otherwise the first smallest (strict <) of
 *        five candidates: (A, C(A)), (B, C(B)), then for k = 0, 1, 2 the S of the segment against edge k (v_k, v_k+1 - v_k).
 *      shape intersection: a ball: |q.t - C(q.t)|^2 <= r^2.  A capsule: D(A, u of q).d2 <= r^2.  A cuboid: in the QUERY's frame (the vertices through
 *        iso_inv_mul(make_isometry(query), {collider rotation, collider position})) no axis of the 13 separates (separation > 0): e_0..e_2, N of the posed
 *        vertices, then edge_k x e_i / |.| with k outer and i inner, skipped when the norm is not above eps |edge_k|; per axis L the separation is
 *        max(min_k dot(L, v_k) - rb, -max_k dot(L, v_k) - rb), rb = (|L_x| he_x + |L_y| he_y) + |L_z| he_z (the narrow phase's tri_box_axis).
 *      shape cast (point1 / normal1 the collider's, point2 the query's at the impact pose; everything 0 when the shapes overlap at the start):
 *        a ball query: the Newton iteration of the capsule-query cast on g(t) = |c - C(c)| - r, c = q.t + d_l t, n = (c - C(c)) / dist: normal1 =
 *          rot_c n; point1 = rot_c C(c) + pos_c; point2 = rot_c (c - n r) + pos_c.
 *        a capsule query: the same iteration on g(t) = sqrt(D(A + d_l t, u).d2) - r, n = (p_seg - p_tri) / dist: normal1 = rot_c n; point1 = rot_c
 *          p_tri + pos_c; point2 = rot_c (p_seg - n r) + pos_c.  The 32-round cap, the last t standing and "never an over-estimate" are unchanged.
 *        a cuboid query: a swept SAT in the collider's frame over 13 axes in this order: N; u_0..u_2 (the query's face axes, iso_vec(q, e_b)); cross(edge_k,
 *          u_b) / |.| with b outer and k inner (edge_0 = b - a, edge_1 = c - b, edge_2 = a - c), skipped when the norm is not above eps.  Per axis:
 *          [lo, hi] = min / max of dot(axis, a), dot(axis, b), dot(axis, c); s0 = dot(axis, q.t), v = dot(axis, d_l), r2 = the sum of |dot(axis, u_i)|
 *          he_i; v != 0: t1 = ((lo - r2) - s0) / v, t2 = ((hi + r2) - s0) / v by inv = 1 / v, exchanged when inv < 0; the largest t1 (strict >) is the
 *          entry with its axis, oriented from the triangle towards the query (-axis, or +axis when inv < 0), the smallest t2 the exit; v == 0: a miss
 *          when s0 + r2 < lo or s0 - r2 > hi.  !(entry <= exit) or exit < 0: a miss; entry < 0: overlap at the start.  Witnesses by the entering axis,
 *          n its orientation, tp = q.t + d_l t, s2 = the query's support vertex along -n: N: p2 = s2, p1 = s2 - N dot(N, s2 - a), inside when C(p1) is
 *          in the face region.  u_b: p1 = the triangle's vertex of the largest dot(n, v) (the first), p2 = p1 - n (dot(p1 - tp, n) + he_b), inside when
 *          p1 lies within the query's face on the other two axes.  An edge pair: the closest points of the lines v_k + lambda edge_k and s2 + mu u_b
 *          (aa = |edge_k|^2, bc = dot(edge_k, u_b), cc = |u_b|^2, w = v_k - s2, dd = dot(edge_k, w), ee = dot(u_b, w), den = aa cc - bc bc, lambda = (bc ee -
 *          cc dd) / den, mu = (aa ee - bc dd) / den; den not above eps aa cc: p1 = the edge's middle and not inside), inside when 0 <= lambda <= 1 and p2 lies
 *          on the query's edge.  Not inside: p1 = C(p1), p2 = the box's closest point to p1 (clamp in the query's frame), p1 = C(p2), p2 = the box's closest
 *          point to p1.  normal1 = rot_c n; point1 = rot_c p1 + pos_c; point2 = rot_c p2 + pos_c.
 *      contacts (shape contacts, depenetration, cast_move's origin-penetration rule, move and slide): (a), (b) with the triangle's AABB, then the
 *        narrow phase's triangle manifold of avian_mi355x_trimesh.h with the query as shape 1 -- a ball, a cuboid or a capsule query alike -- the
 *        collider's triangle WITH ITS EDGE FLAGS as shape 2, and (d)'s fold: the deepest point, the later point wins a tie.  A character sliding over
 *        the interior edges of a flat mesh therefore gets the face normal there.
 *    NOT covered: swept CCD against triangles, a triangle as a query shape, triangle-triangle, target_distance != 0, level-2 and sharded worlds.
 *  - move and slide (MoveAndSlide::cast_move, project_velocity, move_and_slide; move_and_slide.rs:464-793, velocity_project.rs).  As above the
 *    definitions are written out here with their operation order (no FMA contraction); parity with glam / parry is UNPINNED.  Common rules:
 *      Sensors are never candidates (MoveAndSlide's collider query is Without<Sensor>; cast_move's predicate enforces it for the cast too).
 *      self_entity [n]: a collider whose entity_index equals the query's self_entity is not a candidate of that query (NULL or
 *        AVN_SPATIAL_MISS: none); the call's shared mask / excluded list still apply.
 *      A Dir is f32, in an f64 world too: it is normalised or rounded in float and widened where the reference calls adjust_precision.
 *        D(v) = Dir::new_and_length(v as f32): x, y, z = the components rounded to float; len = sqrt(x*x + y*y + z*z) in float, left to
 *        right; valid iff len is finite and > 0; the direction is (x / len, y / len, z / len), the length is len widened.
 *      Rust's a.max(b) is a > b ? a : b with the constant as b (a NaN gives the constant).  DOT_EPSILON = 0.005, MIN_DISTANCE = 1e-4, in the
 *        world's scalar.  dot(a, b) = a.x*b.x + a.y*b.y + a.z*b.z, cross(a, b) = (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y).
 *    project_velocity(v, normals) = -C(-v) per component (a fully blocked velocity comes out with -0.0 components), C = project_onto_conical_hull:
 *      x0 = -v, s = x0, cone = Origin; at most 10 rounds of: stop when dot(s, s) < DOT_EPSILON * DOT_EPSILON or there are no normals; the best
 *      normal is the LAST maximum of dot(n_k, s) under total_cmp (n_k widened; a fold from k = 0 that takes k whenever the best is not
 *      greater under the total order, where -0 < +0); stop when best_dot <= DOT_EPSILON; then with n the best normal
 *        Origin: d = dot(n, x0), s = x0 - d * n per component, cone = Ray(n).
 *        Ray(p): c = cross(n, p), d = dot(x0, c), s = d * c / dot(c, c) per component; cone = d > 0 ? Wedge(n, p) : Wedge(p, n).
 *        Wedge(n1, n2): c1 = cross(n1, n), q1 = dot(c1, c1), d1 = dot(x0, c1); c2 = cross(n, n2), q2 = dot(c2, c2), d2 = dot(x0, c2);
 *          d1 <= 0 && d2 <= 0: s = +0 and the iteration ends; else if d1 * |d1| * q2 > d2 * |d2| * q1: cone = Wedge(n1, n), s = d1 * c1 / q1;
 *          else cone = Wedge(n, n2), s = d2 * c2 / q2.
 *      A non-finite velocity, or a non-finite normal among the first normal_count, answers the input velocity unchanged.  A normal_count
 *      above `stride` is read as `stride`.
 *    cast_move(shape at position / rotation, movement, skin_width): (dir, dist) = D(movement), or ((1, 0, 0), 0) when that is not valid.  The
 *      cast is the shape cast above along dir (widened) with max_distance = dist over the candidates (not sensors, not self_entity), with
 *      Avian's ignore_origin_penetration = true as this ORIGIN-PENETRATION RULE: a collider whose pair test reports overlap at the start
 *      (distance 0 with normal1 = 0) takes the shape contact of the pair, steps (c) and (d) above at prediction 0 with the query as shape 1.
 *      With a contact, n = -manifold.normal (from the collider towards the query): when dir.x*n.x + dir.y*n.y + dir.z*n.z >= 0 (the
 *      character is on its way out) the collider is ignored by this cast; otherwise it is a hit at distance 0 with normal1 = n, point1 =
 *      collider position + anchor2, point2 = query position + anchor1 (the contact record's `point`).  Without a contact (e.g. a ball's
 *      centre inside a cuboid) it is a hit at distance 0 with points and normals 0.  The answer is the smallest (distance, collider index)
 *      over those and the ordinary hits; normal2 = -normal1 with a zero component staying +0.  Then
 *        distance = dist == 0 ? 0 : max(hit.distance - skin_width / max(dot(dir, -normal1), DOT_EPSILON), 0)   (the safe distance)
 *        collision_distance = dist: the reference stores the movement's length there, not the hit's distance; this library keeps that.
 *      A non-finite movement, a skin_width that is NaN, infinite or negative, or an invalid query shape answers a miss.
 *    move_and_slide, per character (move_and_slide.rs:475-608): position, velocity = the inputs, time_left = delta_time;
 *      position += depenetrate(position) (the depenetration above with AVN_SPATIAL_SKIP_SENSORS and self_entity; depenetration_iterations =
 *      0: a zero offset is added).  Then up to move_and_slide_iterations rounds: sweep = time_left * velocity per component; (dir, dist) =
 *      D(sweep), not valid: stop; dist < MIN_DISTANCE: stop; hit = cast_move(position, sweep, skin_width) (iterations_run counts these
 *      casts), a miss: position += sweep, stop.  point = hit.point2 + position (the position before the move: the reference adds them and so
 *      does this library); time_left -= time_left * (hit.distance / dist); position += dir * hit.distance per component.  planes = the
 *      configuration's, then hit.normal1 rounded to float (logged as kind 0; not deduplicated).  The shape contacts of the new position at
 *      prediction 2 * skin_width in ascending collider index (the first AVN_SPATIAL_MAX_HITS; more sets flag bit 0), each with its normal n
 *      rounded to float: the first existing plane e with (float dot(n, e)) widened >= plane_similarity_dot_threshold is replaced by n when
 *      dot(n, velocity) < dot(e, velocity) (both widened) and the contact is done; otherwise, while fewer than max_planes planes exist, it
 *      is logged (kind 1: the contact's own collider and entity -- the reference passes the sweep's entity: a stated strengthening -- its
 *      point, n, the sweep's distance and collision_distance) and pushed.  on_hit is taken as `true`; a full plane list does not stop the
 *      loop over the contacts (nor does the reference's).  velocity = project_velocity(velocity, planes).  After the rounds: position +=
 *      depenetrate(position).  A character whose query shape is invalid or whose position is not finite answers its input position and
 *      velocity with zero counts.  The hit log holds the first hit_cap records in call order; hit_count is the true number; unused slots
 *      are misses (collider and entity AVN_SPATIAL_MISS, the rest 0).
 *    NOT covered: on_hit callbacks that change position / velocity or return false, 2D, Rust declarations.
 *
 * Non-finite inputs (NaN or inf components):
 *  - a collider whose snapshot position, rotation or shape AABB is not finite is never a candidate (it keeps its collider index);
 *  - a query whose origin, direction, point or box corner is not finite answers a miss (ray queries, projection) or a count of 0, whatever
 *    the scene;
 *  - a query shape whose kind is none of AVN_SHAPE_CUBOID, AVN_SHAPE_BALL and AVN_SHAPE_CAPSULE (kind 2 is not a query shape), whose position,
 *    rotation, half extents (a ball: its radius; a capsule: r and h) or AABB are not finite, or which has a negative half extent, answers a count of 0 (a shape cast: a miss / count 0; so does a cast whose
 *    direction is not finite or whose max_distance is NaN; shape contacts: so does a prediction_distance that is NaN, infinite or
 *    negative; depenetration: a zero fixup with count 0).  This is decided per query on the device;
 *  - a hit needs a finite distance.
 *  Answers to finite inputs do not depend on these rules.
 *
 * Accuracy: every answer is the exact test above in the world's scalar type.  tests/spatial_exact_geometry.py states the forward-error
 * bound the answers are held to against exact rational geometry (a few eps times the magnitudes of the ray, the pose, the shape and the
 * distance; for balls, plus the grazing term of the square root); tests/spatial_cast_exact_geometry.py does the same for shape casts.
 *
 * Snapshot rules:
 *  - a query before any avn_spatial_update, or after avn_bodies_upload / avn_colliders_upload / avn_collider_transforms_upload /
 *    avn_despawn changed the tables without a new update, returns AVN_ERR_STATE.  Steps do not invalidate the snapshot: queries answer
 *    against the poses of the last update, as Avian's pipeline does between updates (SpatialQuery::update_pipeline).
 *  - AVN_SHAPE_HOST colliders have no device geometry: if the snapshot holds any, queries return AVN_ERR_STATE unless the query sets
 *    AVN_SPATIAL_SKIP_HOST_SHAPES; with the flag they are never candidates (avn_spatial_stats.host_skipped counts them).
 *  - sensors, sleeping and static bodies' colliders are all candidates, as in Avian's pipeline.  MoveAndSlide's collider query is
 *    Without<Sensor>: avn_spatial_shape_contacts and avn_spatial_depenetrate (and only they) accept AVN_SPATIAL_SKIP_SENSORS, with which a
 *    collider uploaded with AVN_COLLIDER_SENSOR is never a candidate.
 *
 * Filter (SpatialQueryFilter::test, query_filter.rs:97-101): a collider is a candidate when memberships & mask != 0 and its
 * entity_index is not in the excluded list.  ONE excluded list is shared by every query of a call (a caster's own entity goes in it for
 * RayCaster::ignore_self); per-query exclusion lists are not supported by the batched entry points.  The casters below carry their own
 * self_entity and excluded list per caster.
 *
 * Ties: closest hit = smallest (distance, collider index); ray_hits = the max_hits nearest by (distance, collider index), sorted, plus
 * the true number of hits (Avian returns an arbitrary subset when truncated: nearest-k is a deterministic strengthening); point and AABB
 * intersections = ascending collider index, the first `cap`, plus the true count; shape intersections the same; a projection = the
 * smallest (distance, collider index); cast_shapes = the smallest (distance, collider index); shape_hits = the max_hits nearest by (distance,
 * collider index), sorted, plus the true number of hits (Avian's shape_hits repeats cast_shape, excluding each hit entity in turn: the same
 * list in exact arithmetic, here with a deterministic tie rule).  A collider index is its slot in the last avn_colliders_upload.
 *
 * Casters (the RayCaster / ShapeCaster components, spatial_query/ray_caster.rs, shape_caster.rs, mod.rs:236-435): a caster is defined once
 * (avn_spatial_ray_casters_upload / avn_spatial_shape_casters_upload), anchored to nothing, to a body or to a collider, and every
 * avn_spatial_casters_run re-aims it from its anchor's pose and casts it; the hits stay on the device until a getter asks for them.
 *  - the run, on the world's stream, in Avian's order (caster positions, pipeline update, raycast, shapecast): (a) a new snapshot, as
 *    avn_spatial_update takes it; (b) every caster, disabled ones too, is re-aimed from the poses that snapshot was taken from: a body anchor
 *    from the body's position and rotation, a collider anchor from the snapshot's collider pose (collider_pose: a child collider through its
 *    ColliderTransform), a world anchor not at all (its global values are its local ones, bit for bit); (c) the enabled ones are cast.
 *    The run reads nothing back and does not wait for the device (the buffers of a world that grew are reallocated first, which does wait).
 *  - re-aiming (update_ray_caster_positions / update_shape_caster_positions, `Mul<Dir> for Rotation`, physics_transform/transform.rs:899-904),
 *    with (pos, rot) the anchor's pose, qrot and qmul the functions collider_pose uses, T the world's scalar:
 *      global_origin = pos + qrot(rot, origin)                       per component, the rotation first
 *      global_direction = (float) qrot(rot, (T) direction)           widened, rotated in T, each component rounded to float; NOT renormalised
 *                                                                    (Dir::new_unchecked); widened again where the cast consumes it
 *      global_shape_rotation = qmul(shape_rotation, rot)             the shape's rotation on the LEFT, as the reference writes it; NOT renormalised
 *    A non-finite anchor pose gives a non-finite query, which answers a miss without traversing (the rules above).
 *  - candidates of a caster: the snapshot's candidate flag, memberships & the caster's mask != 0, the entity not in the caster's own excluded
 *    list, entity != self_entity (RayCaster::ignore_self).  Sensors stay candidates.
 *  - answers, per caster with k = min(max_hits, hit_cap): k == 1: what avn_spatial_cast_rays / avn_spatial_cast_shapes answer, the smallest
 *    (distance, collider index), count 0 or 1.  k > 1: what avn_spatial_ray_hits / avn_spatial_shape_hits answer with max_hits = k: the nearest
 *    k, sorted, and the TRUE number of hits in count.  k == 0, or a disabled caster: count 0, no traversal.  Records are [count, hit_cap] in
 *    caster order; slots past the answer are misses (both ids AVN_SPATIAL_MISS, the rest 0).  Avian's ShapeCaster loop of casts that exclude
 *    each hit in turn gives the same list; its RayCaster keeps an arbitrary subset when truncated (nearest-k: the strengthening above).
 *    NOT covered: target_distance, compute_contact_on_penetration, ignore_origin_penetration of ShapeCaster (the cast is cast_shapes': an overlap at
 *    the start answers distance 0), caster shapes other than Ball / Cuboid / Capsule, ChildOf chains other than the two anchors, running the casters from
 *    avn_step, Rust declarations.
 *  - avn_despawn renumbers bodies and colliders: it drops every caster definition (a call rejected before it changed anything keeps them).  Other table uploads keep them; a run whose anchors no
 *    longer fit the tables is AVN_ERR_STATE.
 */
#ifndef AVIAN_MI355X_SPATIAL_H
#define AVIAN_MI355X_SPATIAL_H

#include "avian_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A capsule (the segment (0, -h, 0) .. (0, +h, 0) swept by a ball of radius r; half_extents = (r, h, .)): a query-shape kind of this header and, on the HIP
 * backend, a collider kind (avian_mi355x.h "capsule colliders": avn_colliders_upload, avn_contact_manifolds).  The spatial queries of this header answer
 * against capsule COLLIDERS once avn_spatial_capsule_colliders_set has switched them in; by default a snapshot treats them as host shapes.  The swept
 * CCD tests them behind avn_swept_ccd_capsules_set (avian_mi355x_ccd.h) and skips them by default. */
enum { AVN_SHAPE_CAPSULE = 3 };

/* flags of a query */
enum {
    AVN_SPATIAL_DEVICE_POINTERS = 1,   /* every input and output array of the call (filter included) is a device pointer on the world's device;
                                          the caller's writes to them must be complete before the call */
    AVN_SPATIAL_SKIP_HOST_SHAPES = 2,  /* AVN_SHAPE_HOST colliders are never candidates (else their presence is AVN_ERR_STATE) */
    AVN_SPATIAL_SKIP_SENSORS = 4       /* avn_spatial_shape_contacts / avn_spatial_depenetrate only: AVN_COLLIDER_SENSOR colliders are never
                                          candidates (MoveAndSlide's Without<Sensor>); the other queries ignore the flag
                                          (avn_spatial_cast_moves / avn_spatial_move_and_slide never see sensors, flag or not) */
};
#define AVN_SPATIAL_MAX_HITS 64        /* largest max_hits of avn_spatial_ray_hits / avn_spatial_shape_hits, largest cap of avn_spatial_shape_contacts */
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

/* the query shapes of avn_spatial_shape_intersections (avn_spatial_shape_casts carries the same fields) */
typedef struct avn_spatial_shapes {
    uint32_t count;
    uint32_t flags;
    const uint8_t* shape;        /* [n] AVN_SHAPE_CUBOID / AVN_SHAPE_BALL / AVN_SHAPE_CAPSULE */
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

/* the casts of avn_spatial_cast_shapes / avn_spatial_shape_hits: the fields of avn_spatial_shapes plus a direction and a range per cast */
typedef struct avn_spatial_shape_casts {
    uint32_t count;
    uint32_t flags;
    const uint8_t* shape;        /* [n] AVN_SHAPE_CUBOID / AVN_SHAPE_BALL / AVN_SHAPE_CAPSULE */
    const void* half_extents;    /* [3n] (ball: radius in x) */
    const void* position;        /* [3n] the shape's position at distance 0 */
    const void* rotation;        /* [4n] xyzw, unit (the caller normalises) */
    const void* direction;       /* [3n] unit (the caller normalises, as Dir3 does): distances are in units of |direction|, and the tree's
                                    padding is only guaranteed for |direction| = 1 */
    const void* max_distance;    /* [n] (+inf is legal) */
    avn_spatial_filter filter;
} avn_spatial_shape_casts;

/* ShapeHitData (shape_caster.rs) with the collider's table index.  Index 1 is the collider that was hit, index 2 the cast shape at the impact
 * pose; everything in world space.  60 / 112 bytes, no implicit padding: every byte of a record is written. */
typedef struct avn_spatial_shape_hit_f32 {
    uint32_t collider;   /* AVN_SPATIAL_MISS = no hit (entity too; the rest 0) */
    uint32_t entity;
    float distance;      /* the distance travelled along `direction` at the impact */
    float point1[3];     /* the witness on the collider */
    float point2[3];     /* the witness on the cast shape */
    float normal1[3];    /* the collider's outward normal at point1 */
    float normal2[3];    /* -normal1 (a zero component stays +0) */
} avn_spatial_shape_hit_f32;
typedef struct avn_spatial_shape_hit_f64 {
    uint32_t collider;
    uint32_t entity;
    double distance;
    double point1[3];
    double point2[3];
    double normal1[3];
    double normal2[3];
} avn_spatial_shape_hit_f64;

/* the queries of avn_spatial_shape_contacts: the fields of avn_spatial_shapes plus a prediction distance per query */
typedef struct avn_spatial_shape_contact_queries {
    uint32_t count;
    uint32_t flags;              /* AVN_SPATIAL_*, AVN_SPATIAL_SKIP_SENSORS included */
    const uint8_t* shape;        /* [n] AVN_SHAPE_CUBOID / AVN_SHAPE_BALL / AVN_SHAPE_CAPSULE */
    const void* half_extents;    /* [3n] (ball: radius in x) */
    const void* position;        /* [3n] */
    const void* rotation;        /* [4n] xyzw, unit (the caller normalises) */
    const void* prediction_distance;   /* [n] finite and >= 0 (else the query answers count 0) */
    avn_spatial_filter filter;
} avn_spatial_shape_contact_queries;

/* The deepest contact of the query shape with one collider (MoveAndSlide::intersections' callback arguments) with the collider's table index.
 * 60 / 120 bytes, no implicit padding: every byte of a record is written. */
typedef struct avn_spatial_shape_contact_f32 {
    uint32_t collider;   /* AVN_SPATIAL_MISS = an unused slot (entity too; the rest 0) */
    uint32_t entity;
    float penetration;   /* ContactPoint::penetration of the deepest point (negative: a gap within the prediction distance) */
    float normal[3];     /* -manifold.normal: from the collider towards the query shape, world space */
    float point[3];      /* query position + anchor1 */
    float anchor1[3];    /* relative to the query shape's position, world orientation */
    float anchor2[3];    /* relative to the collider's position */
} avn_spatial_shape_contact_f32;
typedef struct avn_spatial_shape_contact_f64 {
    uint32_t collider;
    uint32_t entity;
    double penetration;
    double normal[3];
    double point[3];
    double anchor1[3];
    double anchor2[3];
    uint32_t reserved[2];   /* always written as 0 */
} avn_spatial_shape_contact_f64;

typedef struct avn_spatial_shape_contacts_out {
    void* contacts;      /* avn_spatial_shape_contact_fNN [n * cap], ascending collider index per query; NULL is legal when cap == 0 */
    uint32_t* count;     /* [n] true number of contacts */
} avn_spatial_shape_contacts_out;

/* DepenetrationConfig (move_and_slide.rs); cast once to the world's scalar.  The caller applies PhysicsLengthUnit. */
typedef struct avn_spatial_depenetration_config {
    double skin_width;                        /* the prediction distance of the contacts, added to every penetration */
    double max_depenetration_error;           /* a pass whose total error is below this ends the iteration */
    double penetration_rejection_threshold;   /* contacts with penetration + skin_width above this are ignored */
    uint32_t iterations;                      /* depenetration_iterations; 0 answers zero vectors without traversing */
} avn_spatial_depenetration_config;

/* 24 / 40 bytes, every byte written */
typedef struct avn_spatial_depenetration_f32 {
    float fixup[3];            /* the offset to add to the query shape's position */
    uint32_t count;            /* true number of contacts of the query */
    uint32_t iterations_run;   /* passes started */
    uint32_t truncated;        /* 1: count > AVN_SPATIAL_MAX_HITS, the fixup comes from the first AVN_SPATIAL_MAX_HITS contacts */
} avn_spatial_depenetration_f32;
typedef struct avn_spatial_depenetration_f64 {
    double fixup[3];
    uint32_t count;
    uint32_t iterations_run;
    uint32_t truncated;
    uint32_t reserved;         /* always written as 0 */
} avn_spatial_depenetration_f64;

typedef struct avn_spatial_depenetrations_out {
    void* depenetration; /* avn_spatial_depenetration_fNN [n] */
} avn_spatial_depenetrations_out;

/* project_velocity (velocity_project.rs) per query: no snapshot is needed */
#define AVN_SPATIAL_MAX_PLANES 32
typedef struct avn_spatial_velocity_projections {
    uint32_t count;              /* n */
    uint32_t flags;              /* AVN_SPATIAL_DEVICE_POINTERS */
    uint32_t stride;             /* normals per query in `normals`, <= AVN_SPATIAL_MAX_PLANES */
    const void* velocity;        /* [3n] the world's scalar */
    const float* normals;        /* [n * stride * 3] unit (Dir is f32) */
    const uint32_t* normal_count;/* [n] each <= stride */
} avn_spatial_velocity_projections;
typedef struct avn_spatial_velocities_out {
    void* velocity;              /* [3n] */
} avn_spatial_velocities_out;

/* the moves of avn_spatial_cast_moves: the fields of avn_spatial_shapes plus a movement, a skin width and the character's own entity */
typedef struct avn_spatial_moves {
    uint32_t count;
    uint32_t flags;
    const uint8_t* shape;        /* [n] AVN_SHAPE_CUBOID / AVN_SHAPE_BALL / AVN_SHAPE_CAPSULE */
    const void* half_extents;    /* [3n] (ball: radius in x) */
    const void* position;        /* [3n] */
    const void* rotation;        /* [4n] xyzw, unit */
    const void* movement;        /* [3n] direction and length of the move */
    const void* skin_width;      /* [n] finite and >= 0 (else a miss) */
    const uint32_t* self_entity; /* [n] entity_index never hit by this query; NULL or AVN_SPATIAL_MISS = none */
    avn_spatial_filter filter;
} avn_spatial_moves;
/* MoveHitData with the collider's table index.  64 / 120 bytes, no implicit padding: every byte of a record is written. */
typedef struct avn_spatial_move_hit_f32 {
    uint32_t collider;   /* AVN_SPATIAL_MISS = no hit (entity too; the rest 0) */
    uint32_t entity;
    float distance;             /* the safe distance: the hit's distance pulled back by the skin width */
    float collision_distance;   /* the movement's length (the reference's field of that name) */
    float point1[3], point2[3], normal1[3], normal2[3];
} avn_spatial_move_hit_f32;
typedef struct avn_spatial_move_hit_f64 {
    uint32_t collider;
    uint32_t entity;
    double distance;
    double collision_distance;
    double point1[3], point2[3], normal1[3], normal2[3];
} avn_spatial_move_hit_f64;
typedef struct avn_spatial_move_hits_out {
    void* hits;          /* avn_spatial_move_hit_fNN [n] */
} avn_spatial_move_hits_out;

/* the characters of avn_spatial_move_and_slide */
typedef struct avn_spatial_characters {
    uint32_t count;
    uint32_t flags;
    const uint8_t* shape;
    const void* half_extents;    /* [3n] */
    const void* position;        /* [3n] */
    const void* rotation;        /* [4n] */
    const void* velocity;        /* [3n] */
    const uint32_t* self_entity; /* [n] or NULL */
    avn_spatial_filter filter;
} avn_spatial_characters;
/* MoveAndSlideConfig; the doubles are cast once to the world's scalar.  The caller applies PhysicsLengthUnit.  The struct and `planes` are host
 * memory whatever the flags say. */
typedef struct avn_spatial_move_and_slide_config {
    double delta_time;
    double skin_width;
    double max_depenetration_error;
    double penetration_rejection_threshold;
    double plane_similarity_dot_threshold;
    const float* planes;                  /* [3 * n_planes] initial planes of every character of the call; NULL if n_planes == 0 */
    uint32_t n_planes;                    /* <= AVN_SPATIAL_MAX_PLANES */
    uint32_t max_planes;                  /* <= AVN_SPATIAL_MAX_PLANES */
    uint32_t move_and_slide_iterations;   /* <= AVN_SPATIAL_MAX_SLIDE_ITERATIONS */
    uint32_t depenetration_iterations;
} avn_spatial_move_and_slide_config;
#define AVN_SPATIAL_MAX_SLIDE_ITERATIONS 16
#define AVN_SPATIAL_SLIDE_TRUNCATED 1u    /* flags bit 0: some contacts pass of the character exceeded AVN_SPATIAL_MAX_HITS records; the first were used */
/* MoveAndSlideOutput plus counters.  36 / 64 bytes, every byte written. */
typedef struct avn_spatial_slide_f32 {
    float position[3];
    float projected_velocity[3];
    uint32_t iterations_run;   /* cast_move calls made */
    uint32_t hit_count;        /* true number of on_hit calls */
    uint32_t flags;            /* AVN_SPATIAL_SLIDE_* */
} avn_spatial_slide_f32;
typedef struct avn_spatial_slide_f64 {
    double position[3];
    double projected_velocity[3];
    uint32_t iterations_run;
    uint32_t hit_count;
    uint32_t flags;
    uint32_t reserved;         /* always written as 0 */
} avn_spatial_slide_f64;
/* MoveAndSlideHitData of one on_hit call.  48 / 80 bytes. */
typedef struct avn_spatial_slide_hit_f32 {
    uint32_t collider;         /* kind 0: the sweep's collider; kind 1: the contact plane's own collider */
    uint32_t entity;
    uint32_t iteration;        /* round of the loop, from 0 */
    uint32_t kind;             /* 0: the sweep hit, 1: a contact plane */
    float point[3];
    float normal[3];           /* the Dir handed to on_hit (f32, widened) */
    float distance;            /* the sweep's safe distance */
    float collision_distance;
} avn_spatial_slide_hit_f32;
typedef struct avn_spatial_slide_hit_f64 {
    uint32_t collider;
    uint32_t entity;
    uint32_t iteration;
    uint32_t kind;
    double point[3];
    double normal[3];
    double distance;
    double collision_distance;
} avn_spatial_slide_hit_f64;
typedef struct avn_spatial_slides_out {
    void* slides;        /* avn_spatial_slide_fNN [n] */
    void* hits;          /* avn_spatial_slide_hit_fNN [n * hit_cap]; NULL is legal when hit_cap == 0 */
} avn_spatial_slides_out;

typedef struct avn_spatial_shape_hits_out {
    void* hits;          /* avn_spatial_shape_hit_fNN [n] (cast_shapes) or [n * max_hits] (shape_hits; unused slots are misses) */
    uint32_t* count;     /* [n] true number of hits (shape_hits); ignored by cast_shapes */
} avn_spatial_shape_hits_out;

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
    uint32_t host_skipped;     /* AVN_SHAPE_HOST colliders in the snapshot (never candidates); AVN_SHAPE_CAPSULE ones too unless avn_spatial_capsule_colliders_set switched them in, AVN_SHAPE_TRIANGLE ones unless avn_spatial_triangle_colliders_set did */
    uint32_t valid;            /* 1: the snapshot can be queried */
    uint64_t nodes_visited;    /* last query call: node boxes tested, all queries together */
    uint64_t leaves_visited;   /* last query call: exact per-collider tests run, all queries together */
} avn_spatial_stats;

/* update_spatial_query_pipeline / SpatialQueryPipeline::update (pipeline.rs:96-133): builds the LBVH from the poses the device holds when the
 * call runs, enqueued on the world's stream after any step work.  avn_step never calls it. */
AVN_API avn_status avn_spatial_update(avn_world* w);
/* Capsule colliders as candidates of the queries ("queries against capsule colliders"): a sticky per-world switch, 0 (off) in a new world.  It
 * invalidates the snapshot -- a query before the next avn_spatial_update is AVN_ERR_STATE -- and holds for every later avn_spatial_update, the
 * one inside avn_spatial_casters_run included.  A world without a capsule collider launches the same kernels with the switch on as with it off. */
AVN_API avn_status avn_spatial_capsule_colliders_set(avn_world* w, uint32_t enabled);
/* Triangle colliders (avian_mi355x_trimesh.h) as candidates of the queries ("queries against triangle colliders"): a sticky per-world switch, 0 (off) in
 * a new world, independent of the capsule switch.  It invalidates the snapshot as that one does and holds for every later avn_spatial_update, the one
 * inside avn_spatial_casters_run included.  With it on avn_spatial_update needs the triangle table (AVN_ERR_STATE while AVN_SHAPE_TRIANGLE colliders
 * exist without avn_collider_triangles_upload).  A world without a triangle collider launches the same kernels with the switch on as with it off. */
AVN_API avn_status avn_spatial_triangle_colliders_set(avn_world* w, uint32_t enabled);
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
/* SpatialQueryPipeline::cast_shape (pipeline.rs:335-374); ShapeCaster with max_hits = 1: per cast the closest hit within max_distance, or a miss */
AVN_API avn_status avn_spatial_cast_shapes(avn_world* w, const avn_spatial_shape_casts* casts, const avn_spatial_shape_hits_out* out);
/* SpatialQueryPipeline::shape_hits (pipeline.rs:443-487); ShapeCaster / ShapeHits: per cast the max_hits nearest hits, sorted, plus the true count.
 * 1 <= max_hits <= AVN_SPATIAL_MAX_HITS, else AVN_ERR_BAD_ARG. */
AVN_API avn_status avn_spatial_shape_hits(avn_world* w, const avn_spatial_shape_casts* casts, uint32_t max_hits, const avn_spatial_shape_hits_out* out);
/* MoveAndSlide::intersections (move_and_slide.rs:1032-1078): per query shape the deepest contact with every collider nearer than its
 * prediction distance, ascending collider index, the first `cap`, plus the true count.  0 <= cap <= AVN_SPATIAL_MAX_HITS, else AVN_ERR_BAD_ARG. */
AVN_API avn_status avn_spatial_shape_contacts(avn_world* w, const avn_spatial_shape_contact_queries* queries, uint32_t cap, const avn_spatial_shape_contacts_out* out);
/* MoveAndSlide::depenetrate (move_and_slide.rs:868-897, 982-1009): the contacts of every query shape with prediction skin_width, then the Gauss-Seidel
 * depenetration over them.  shapes->flags may carry AVN_SPATIAL_SKIP_SENSORS.  The world keeps a device buffer of
 * count * AVN_SPATIAL_MAX_HITS contact records for this call (3.8 KB per query in f32, 7.7 KB in f64); it grows and is never shrunk. */
AVN_API avn_status avn_spatial_depenetrate(avn_world* w, const avn_spatial_shapes* shapes, const avn_spatial_depenetration_config* config, const avn_spatial_depenetrations_out* out);
/* project_velocity (velocity_project.rs:122) per query; needs no snapshot.  stride > AVN_SPATIAL_MAX_PLANES is AVN_ERR_BAD_ARG. */
AVN_API avn_status avn_spatial_project_velocities(avn_world* w, const avn_spatial_velocity_projections* in, const avn_spatial_velocities_out* out);
/* MoveAndSlide::cast_move (move_and_slide.rs:745-793) per move: the first collider on the way, the distance pulled back by the skin width.  The
 * colliders that overlap a move's shape at its start go through a list of AVN_SPATIAL_MAX_HITS slots per move in a buffer the world keeps (it grows
 * and is never shrunk); a move with more of them makes the call AVN_ERR_CAPACITY (avn_spatial_move_and_slide too). */
AVN_API avn_status avn_spatial_cast_moves(avn_world* w, const avn_spatial_moves* moves, const avn_spatial_move_hits_out* out);
/* MoveAndSlide::move_and_slide (move_and_slide.rs:464-609) per character, as a fixed sequence of launches with the per-character state in buffers
 * the world keeps (they grow and are never shrunk).  0 <= hit_cap <= AVN_SPATIAL_MAX_HITS; limits exceeded are AVN_ERR_BAD_ARG.  The traversal
 * counters of avn_spatial_stats are the totals of all the call's launches. */
AVN_API avn_status avn_spatial_move_and_slide(avn_world* w, const avn_spatial_characters* characters, const avn_spatial_move_and_slide_config* config, uint32_t hit_cap,
                                              const avn_spatial_slides_out* out);

/* anchors of a caster and the two kinds of caster */
enum { AVN_SPATIAL_ANCHOR_WORLD = 0, AVN_SPATIAL_ANCHOR_BODY = 1, AVN_SPATIAL_ANCHOR_COLLIDER = 2 };
enum { AVN_SPATIAL_CASTER_RAY = 0, AVN_SPATIAL_CASTER_SHAPE = 1 };
/* RayCaster definitions (ray_caster.rs).  Host pointers only: configuration, not per-step data. */
typedef struct avn_spatial_ray_casters {
    uint32_t count;                  /* n; 0 clears the ray casters */
    uint32_t hit_cap;                /* record slots per caster, 1 .. AVN_SPATIAL_MAX_HITS */
    const uint8_t* anchor_kind;      /* [n] AVN_SPATIAL_ANCHOR_* */
    const uint32_t* anchor;          /* [n] body-table / collider-table index (ignored for a world anchor) */
    const void* origin;              /* [3n] local origin, the world's scalar */
    const float* direction;          /* [3n] local direction, unit (Dir is f32 in an f64 world too) */
    const void* max_distance;        /* [n] (+inf is legal) */
    const uint32_t* max_hits;        /* [n] 0 is legal (count 0); above hit_cap is read as hit_cap (Avian's default is u32::MAX) */
    const uint8_t* solid;            /* [n] */
    const uint8_t* enabled;          /* [n]; NULL = all enabled */
    const uint32_t* mask;            /* [n]; NULL = LayerMask::ALL */
    const uint32_t* self_entity;     /* [n] entity_index the caster never hits (ignore_self); NULL or AVN_SPATIAL_MISS = none */
    const uint32_t* excluded_offset; /* [n + 1] CSR offsets into `excluded`, ascending from 0; NULL = no excluded entities */
    const uint32_t* excluded;        /* [excluded_offset[n]] entity_index values; the library sorts each caster's slice */
} avn_spatial_ray_casters;
/* ShapeCaster definitions (shape_caster.rs) */
typedef struct avn_spatial_shape_casters {
    uint32_t count;
    uint32_t hit_cap;
    const uint8_t* anchor_kind;
    const uint32_t* anchor;
    const void* origin;              /* [3n] */
    const float* direction;          /* [3n] */
    const void* max_distance;        /* [n] */
    const uint32_t* max_hits;        /* [n] */
    const uint8_t* shape;            /* [n] AVN_SHAPE_CUBOID / AVN_SHAPE_BALL / AVN_SHAPE_CAPSULE */
    const void* half_extents;        /* [3n] (ball: radius in x) */
    const void* shape_rotation;      /* [4n] xyzw, local */
    const uint8_t* enabled;
    const uint32_t* mask;
    const uint32_t* self_entity;
    const uint32_t* excluded_offset;
    const uint32_t* excluded;
} avn_spatial_shape_casters;
/* the re-aimed casters of the last run */
typedef struct avn_spatial_caster_poses_out {
    void* origin;        /* [3n] global origins, the world's scalar */
    float* direction;    /* [3n] global directions */
    void* rotation;      /* [4n] global shape rotations (AVN_SPATIAL_CASTER_SHAPE only; ignored for rays, may be NULL) */
} avn_spatial_caster_poses_out;

/* Define the world's ray / shape casters (each call replaces the kind's whole table; count == 0 clears it).  An anchor outside its table, a
 * hit_cap outside 1 .. AVN_SPATIAL_MAX_HITS, an anchor kind above 2 or offsets that do not ascend are AVN_ERR_BAD_ARG.  The results of an
 * earlier run are dropped. */
AVN_API avn_status avn_spatial_ray_casters_upload(avn_world* w, const avn_spatial_ray_casters* casters);
AVN_API avn_status avn_spatial_shape_casters_upload(avn_world* w, const avn_spatial_shape_casters* casters);
/* update_ray_caster_positions / update_shape_caster_positions, update_spatial_query_pipeline, raycast, shapecast (mod.rs:236-435): snapshot,
 * re-aim, cast, all enqueued; nothing is read back.  flags: 0 or AVN_SPATIAL_SKIP_HOST_SHAPES.  Without casters it is avn_spatial_update.
 * An anchor outside the current tables is AVN_ERR_STATE. */
AVN_API avn_status avn_spatial_casters_run(avn_world* w, uint32_t flags);
/* RayHits / ShapeHits of the last run: hits [n * hit_cap] in caster order, count [n].  flags: 0 or AVN_SPATIAL_DEVICE_POINTERS.  The getters
 * wait for the run, return AVN_ERR_CAPACITY if its traversal overflowed, and make avn_spatial_stats_get report the run's totals.  Before any
 * run, or after a table change that invalidated the snapshot, AVN_ERR_STATE. */
AVN_API avn_status avn_spatial_ray_caster_hits_get(avn_world* w, uint32_t flags, const avn_spatial_hits_out* out);
AVN_API avn_status avn_spatial_shape_caster_hits_get(avn_world* w, uint32_t flags, const avn_spatial_shape_hits_out* out);
/* the re-aimed origins, directions and (shapes) rotations of the last run; kind: AVN_SPATIAL_CASTER_* */
AVN_API avn_status avn_spatial_caster_poses_get(avn_world* w, uint32_t kind, uint32_t flags, const avn_spatial_caster_poses_out* out);
/* snapshot sizes and the traversal counters of the last query call */
AVN_API avn_status avn_spatial_stats_get(avn_world* w, avn_spatial_stats* out);

#ifdef __cplusplus
}
#endif

#endif /* AVIAN_MI355X_SPATIAL_H */
