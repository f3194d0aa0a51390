// avn_capsule_pair.h — the contact manifolds of a Capsule COLLIDER (AVN_SHAPE_CAPSULE, include/avian_mi355x.h "capsule colliders") against a
// Ball, a Cuboid or another Capsule, in either order.  parry is not vendored: the header defines these manifolds with their operation order
// (no FMA contraction), parity with parry is UNPINNED; tests/capsule_collider_reference.py does the same operations in order.  The core
// geometry is the capsule query shape's (avn_spatial_pair.h: sp_capsule_core, sp_seg_point, sp_seg_box, sp_seg_box_axis) -- there is one
// segment-box routine.  Only contact_manifolds_pair_sink<.., CAP = true> reaches this file: the narrow phase's general (HS) heavy kernel and
// the batch query's capsule instantiation.
#pragma once
#include "avn_spatial_pair.h"

namespace avn {

template <class T> __device__ __forceinline__ V3<T> cp_set(V3<T> v, int i, T x) { return V3<T>{i == 0 ? x : v.x, i == 1 ? x : v.y, i == 2 ? x : v.z}; }
// (cp_clamp01, cp_parallel and the closest points of two segments, sp_seg_seg: avn_spatial_pair.h)

// pos12: shape 2 in shape 1's frame (of the two make_isometry poses); em.rotation1 / em.sink are set.  Sets em.normal and pushes the points;
// false = no manifold (the caller also drops a manifold without points).
template <class T, class Em>
__device__ bool capsule_pair_manifold(uint32_t shape1, V3<T> he1, uint32_t shape2, V3<T> he2, const Iso<T>& pos12, T prediction, Em& em) {
    const bool cap1 = shape1 == AVN_SHAPE_CAPSULE, cap2 = shape2 == AVN_SHAPE_CAPSULE;
    if (cap1 && cap2) {
        // ---- capsule / capsule, in shape 1's frame: the closest points of the two core segments A1 + s u1, A2 + t u2, parameters clamped
        const T r1 = he1.x, r2 = he2.x;
        const V3<T> A1{T(0), -he1.y, T(0)}, u1{T(0), he1.y * T(2), T(0)};
        V3<T> A2, u2;
        sp_capsule_core<T>(pos12, he2.y, A2, u2);
        const SegSeg<T> ss = sp_seg_seg<T>(A1, u1, A2, u2);
        const T a = ss.a, e = ss.e, f = ss.f, c = ss.c, b = ss.b, s = ss.s, t = ss.t;
        const bool par = ss.par;
        if (par) {
            // parallel axes: segment 2's ends projected onto segment 1's parameter; an overlap [lo, hi] with lo < hi gives two points
            const T sa = -c / a, sb = (b - c) / a;
            T lo = sa < sb ? sa : sb, hi = sa < sb ? sb : sa;
            lo = lo < T(0) ? T(0) : lo;
            hi = hi > T(1) ? T(1) : hi;
            if (lo < hi) {
                // the normal: from segment 1 to segment 2 at the middle of the overlap, the part perpendicular to u1
                const T sm = (lo + hi) * T(0.5), tm = cp_clamp01<T>((b * sm + f) / e);
                const V3<T> dm = (A2 + u2 * tm) - (A1 + u1 * sm);
                const V3<T> dp = dm - u1 * (na_dot(dm, u1) / a);
                const T len = na_norm(dp);
                if (!(len > T(0))) return false;   // coincident cores
                const V3<T> n = dp / len;
                if (!np_world_normal(em.rotation1, n, em.normal)) return false;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const T sk = k == 0 ? lo : hi, tk = cp_clamp01<T>((b * sk + f) / e);
                    const V3<T> p1 = A1 + u1 * sk;
                    const T dk = na_dot((A2 + u2 * tk) - p1, n);
                    if (!(dk <= (r1 + r2) + prediction)) continue;
                    em.push(p1 + n * r1, (dk - r1) - r2, fid_vertex((uint32_t)k), fid_vertex((uint32_t)k));
                }
                return true;
            }
        }
        const V3<T> p1 = A1 + u1 * s;
        const V3<T> d = (A2 + u2 * t) - p1;
        const T dist = na_norm(d);
        if (!(dist > T(0))) return false;   // the cores touch or cross: no direction
        if (!(dist <= (r1 + r2) + prediction)) return false;
        const V3<T> n = d / dist;
        if (!np_world_normal(em.rotation1, n, em.normal)) return false;
        em.push(p1 + n * r1, (dist - r1) - r2, fid_face(0), fid_face(0));
        return true;
    }
    const bool flipped = !cap1;   // the capsule is shape 2
    const uint32_t other = flipped ? shape1 : shape2;
    const V3<T> heo = flipped ? he1 : he2;
    const T r = flipped ? he2.x : he1.x, h = flipped ? he2.y : he1.y;
    if (other == AVN_SHAPE_BALL) {
        // ---- capsule / ball: P with the ball's centre in the capsule's frame
        const Iso<T> p = flipped ? iso_inverse(pos12) : pos12;
        const T rb = heo.x;
        const V3<T> A{T(0), -h, T(0)}, u{T(0), h * T(2), T(0)};
        T s;
        const T d2 = sp_seg_point<T>(A, u, p.t, s);
        const T dist = sqrt_t(d2);
        if (!(dist > T(0))) return false;   // the centre on the segment: no direction (contact_manifold_convex_ball's precedent)
        if (!(dist <= (r + rb) + prediction)) return false;
        const V3<T> ps = A + u * s;
        const V3<T> n_cap = (p.t - ps) / dist;   // from the capsule towards the ball, the capsule's frame
        const T sd = (dist - r) - rb;
        if (flipped) {   // shape 1 is the ball: its own direction towards the capsule, its own surface point
            const V3<T> n_ball = iso_inv_vec(p, -n_cap);
            if (!np_world_normal(em.rotation1, n_ball, em.normal)) return false;
            em.push(n_ball * rb, sd, fid_face(0), fid_face(0));
        } else {
            if (!np_world_normal(em.rotation1, n_cap, em.normal)) return false;
            em.push(ps + n_cap * r, sd, fid_face(0), fid_face(0));
        }
        return true;
    }
    // ---- capsule / cuboid, in the cuboid's frame: X
    const Iso<T> q = flipped ? pos12 : iso_inverse(pos12);   // the capsule in the cuboid's frame
    V3<T> A, u;
    sp_capsule_core<T>(q, h, A, u);
    const SegBox<T> sb = sp_seg_box<T>(A, u, heo);
    const T dist = sqrt_t(sb.f);
    const bool apart = dist > T(0);
    V3<T> n;   // from the box towards the capsule
    T best = T(0), brb = T(0);
    if (apart) n = (sb.ps - sb.pb) / dist;
    else sp_seg_box_axis<T>(A, u, heo, n, best, brb);
    if (!np_world_normal(em.rotation1, flipped ? n : iso_inv_vec(q, -n), em.normal)) return false;
    // a face normal of the box: exactly one component is not zero
    const int fa = (n.y == T(0) && n.z == T(0)) ? 0 : ((n.x == T(0) && n.z == T(0)) ? 1 : ((n.x == T(0) && n.y == T(0)) ? 2 : -1));
    const T sg = fa >= 0 && sp_vget(n, fa) > T(0) ? T(1) : T(-1);
    const uint32_t fidb = fa >= 0 ? fid_face((uint32_t)fa + (sg > T(0) ? 3u : 0u) + 10u) : 0u;   // (cuboid_support_face's numbering; an edge / a vertex: unknown)
    T lo = T(0), hi = T(1);
    bool two = false;
    if (fa >= 0 && na_dot(u, u) > T(0)) {
        // the segment clipped to the face's four side planes (the slabs of the two other axes)
        bool empty = false;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j == fa) continue;
            const T aj = sp_vget(A, j), uj = sp_vget(u, j), hj = sp_vget(heo, j);
            if (uj != T(0)) {
                T t1 = (-hj - aj) / uj, t2 = (hj - aj) / uj;
                if (uj < T(0)) { const T x = t1; t1 = t2; t2 = x; }
                if (t1 > lo) lo = t1;
                if (t2 < hi) hi = t2;
            } else if (aj < -hj || aj > hj) empty = true;
        }
        two = !empty && lo < hi;
    }
    if (two) {
        const T hf = sp_vget(heo, fa);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const V3<T> x = A + u * (k == 0 ? lo : hi);
            const T dcore = sg * sp_vget(x, fa) - hf;   // the core point's signed distance to the face's plane
            if (!(dcore <= r + prediction)) continue;
            if (flipped) em.push(cp_set<T>(x, fa, sg * hf), dcore - r, fidb, fid_vertex((uint32_t)k));
            else em.push(iso_inv_point(q, x - n * r), dcore - r, fid_vertex((uint32_t)k), fidb);
        }
    } else if (apart) {
        if (!(dist <= r + prediction)) return false;
        if (flipped) em.push(sb.pb, dist - r, fidb, fid_face(0));
        else em.push(iso_inv_point(q, sb.ps - n * r), dist - r, fid_face(0), fidb);
    } else {
        // the segment touches or crosses the box: its end deepest along -n (the lower s on a tie) against the box's supporting plane of n
        const V3<T> pd = na_dot(n, u) < T(0) ? A + u : A;
        const T sd = -(best + r);
        if (flipped) em.push(pd + n * (brb - na_dot(n, pd)), sd, fidb, fid_face(0));
        else em.push(iso_inv_point(q, pd - n * r), sd, fid_face(0), fidb);
    }
    return true;
}

}  // namespace avn
