// avn_spatial_triangle_pair.h — the pair tests of the spatial queries against a Triangle COLLIDER (AVN_SHAPE_TRIANGLE; include/avian_mi355x_spatial.h
// "queries against triangle colliders"): the CTRI instantiations of k_spatial.hip.  The header defines these tests with their operation order (no FMA
// contraction), parity with parry is UNPINNED; tests/spatial_triangle_collider_reference.py does the same operations in order.  Everything works in the
// COLLIDER's frame on the triangle (a, b, c) of its table record, passed by value; the triangle is two-sided and has no interior.  Only the contacts read the
// edge flags (they are the narrow phase's manifolds, avn_triangle_pair.h).  The file compiles as plain host C++ (tests/spatial_triangle_main.cpp runs it under
// the host sanitizers).  Nothing here is an array indexed by a run-time value: vertices and axes are picked by select chains (tri_pick3, sp_sel3).
#pragma once
#include "avn_triangle_pair.h"

namespace avn {

// The ray ol + t dl against the triangle: the plane of tri_unit_normal first (a denominator of exactly 0 -- a parallel or coplanar ray, a zero direction --
// is a miss; t = 0, the origin on the plane, is a hit), then the inside test.  The inside test never looks at the plane: the sign of edge k is that of
// dl . ((v_k - o_k) x (v_k+1 - o_k)), o_k the point of the ray nearest the edge's midpoint (v_k + v_k+1) / 2.  o_k and the cross product are exactly
// symmetric / antisymmetric in the two vertices, so the two faces that share an edge compute opposite signs bit for bit: a ray is inside a face when no
// sign is negative or none is positive, and a ray through a shared edge cannot miss both of its faces.  nl: the face normal turned against dl.
template <class T> __device__ __forceinline__ bool sp_tri_ray(V3<T> a, V3<T> b, V3<T> c, V3<T> ol, V3<T> dl, T& t, V3<T>& nl) {
    const V3<T> N = tri_unit_normal<T>(a, b, c);
    const T den = na_dot(N, dl);
    if (!(den != T(0))) return false;
    const T t0 = na_dot(N, a - ol) / den;
    if (!(t0 >= T(0))) return false;
    const T dd = na_dot(dl, dl);
    bool neg = false, pos = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const V3<T> vk = k == 0 ? a : (k == 1 ? b : c), vn = k == 0 ? b : (k == 1 ? c : a);
        const V3<T> m = (vk + vn) * T(0.5);
        const V3<T> o = ol + dl * (na_dot(dl, m - ol) / dd);
        const T s = na_dot(dl, na_cross(vk - o, vn - o));
        if (!(s >= T(0))) neg = true;   // (a NaN is both: a miss)
        if (!(s <= T(0))) pos = true;
    }
    if (neg && pos) return false;
    t = t0;
    nl = den > T(0) ? -N : N;
    return true;
}
// the point is on the triangle: its closest point is the point itself, component for component
template <class T> __device__ __forceinline__ bool sp_tri_point(V3<T> a, V3<T> b, V3<T> c, V3<T> pl) {
    int rg;
    const V3<T> q = tri_closest_point<T>(a, b, c, pl, rg);
    return q.x == pl.x && q.y == pl.y && q.z == pl.z;
}

// The squared distance of the segment A + s u, s in [0, 1], from the triangle, with the closest points ps (segment) and pt (triangle).  A segment whose
// ends lie strictly on opposite sides of the plane and whose crossing point projects into the face (tri_capsule's test) touches it: 0, both points the
// crossing point's.  Otherwise tri_seg_closest, the routine of the narrow phase.
template <class T> __device__ __forceinline__ T sp_seg_tri_d2(V3<T> a, V3<T> b, V3<T> c, V3<T> A, V3<T> u, V3<T>& ps, V3<T>& pt) {
    const V3<T> B = A + u;
    const V3<T> N = tri_unit_normal<T>(a, b, c);
    const T da = na_dot(N, A - a), db = na_dot(N, B - a);
    if ((da > T(0) && db < T(0)) || (da < T(0) && db > T(0))) {
        int rg;
        const V3<T> X = A + u * (da / (da - db));
        const V3<T> q = tri_closest_point<T>(a, b, c, X, rg);
        if (rg == 0) { ps = X; pt = q; return T(0); }
    }
    const TriBest<T> best = tri_seg_closest<T>(a, b, c, A, u);
    ps = best.ps; pt = best.pt;
    return best.d2;
}

// Intersection of the query shape (shape2, he2, iso2 = make_isometry of its pose) with the triangle collider at (pos1, rot1).  A ball: the squared
// distance of its centre from the triangle against r^2, in the collider's frame.  CAPSULE (a capsule query): sp_seg_tri_d2 of its core against r^2.
// A cuboid: no separating axis among the 13 of tri_box_axis, in the QUERY's frame and in tri_cuboid's order (the box's faces, the triangle's normal,
// edge k x e_i with k outer).
template <class T, bool CAPSULE>
__device__ __forceinline__ bool sp_tricol_intersects(uint32_t shape2, V3<T> he2, const Iso<T>& iso2, NpTri<T> tri, V3<T> pos1, Q4<T> rot1) {
    if (CAPSULE || shape2 == AVN_SHAPE_BALL) {
        const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
        if (CAPSULE) {
            V3<T> A, u, ps, pt;
            sp_capsule_core<T>(q, he2.y, A, u);
            return sp_seg_tri_d2<T>(tri.a, tri.b, tri.c, A, u, ps, pt) <= he2.x * he2.x;
        }
        int rg;
        const V3<T> d = q.t - tri_closest_point<T>(tri.a, tri.b, tri.c, q.t, rg);
        return na_dot(d, d) <= he2.x * he2.x;
    }
    const Iso<T> qc = iso_inv_mul(iso2, Iso<T>{rot1, pos1});   // the collider in the query's frame
    const V3<T> v0 = iso_point(qc, tri.a), v1 = iso_point(qc, tri.b), v2 = iso_point(qc, tri.c);
    V3<T> d;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (tri_box_axis<T>(he2, v0, v1, v2, tri_axis<T>(i, T(1)), d) > T(0)) return false;
    if (tri_box_axis<T>(he2, v0, v1, v2, tri_unit_normal<T>(v0, v1, v2), d) > T(0)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const V3<T> vk = k == 0 ? v0 : (k == 1 ? v1 : v2), vn = k == 0 ? v1 : (k == 1 ? v2 : v0);
        const V3<T> ek = vn - vk;
        const T el = na_norm(ek);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const V3<T> cx = i == 0 ? V3<T>{T(0), -ek.z, ek.y} : (i == 1 ? V3<T>{ek.z, T(0), -ek.x} : V3<T>{-ek.y, ek.x, T(0)});
            const T nl = na_norm(cx);
            if (!(nl > Limits<T>::eps * el)) continue;
            if (tri_box_axis<T>(he2, v0, v1, v2, cx / nl, d) > T(0)) return false;
        }
    }
    return true;
}

// The swept SAT of the triangle (fixed, in its own frame) and the query's cuboid he2 at pose q moving along dl, over 13 axes in the order: the triangle's
// normal; u_0..u_2 (the query's faces); edge_k x u_b with b outer and k inner, an axis of norm <= eps skipped.  Per axis the triangle's interval
// [lo, hi] (min / max of the three vertices) against the box's s0 +- r2 moving at v: sp_sat_cast's entry / exit rule.  kin = the axis of the largest
// entry (0; 1 + b; 4 + 3 b + k), n = that axis oriented from the triangle towards the query.
template <class T> __device__ __forceinline__ bool sp_tri_sat_cast(V3<T> a, V3<T> b, V3<T> c, V3<T> he2, const Iso<T>& q, V3<T> dl, T& t_out, int& kin_out, V3<T>& n_out, bool& pen_out) {
    const V3<T> u0 = iso_vec(q, V3<T>{T(1), T(0), T(0)}), u1 = iso_vec(q, V3<T>{T(0), T(1), T(0)}), u2 = iso_vec(q, V3<T>{T(0), T(0), T(1)});
    const V3<T> N = tri_unit_normal<T>(a, b, c);
    const V3<T> e0 = b - a, e1 = c - b, e2 = a - c;
    T tin = -sp_inf<T>(), tout = sp_inf<T>();
    int kin = -1;
    V3<T> nin = vzero<T>();
    for (int k = 0; k < 13; ++k) {
        V3<T> ax;
        if (k == 0) ax = N;
        else if (k < 4) ax = sp_sel3(k - 1, u0, u1, u2);
        else {
            const int ib = (k - 4) / 3, ie = (k - 4) % 3;
            const V3<T> axis = na_cross(sp_sel3(ie, e0, e1, e2), sp_sel3(ib, u0, u1, u2));
            const T norm1 = na_norm(axis);
            if (!(norm1 > Limits<T>::eps)) continue;
            ax = axis / norm1;
        }
        const T p0 = na_dot(ax, a), p1 = na_dot(ax, b), p2 = na_dot(ax, c);
        T lo = p0 < p1 ? p0 : p1, hi = p0 < p1 ? p1 : p0;
        lo = p2 < lo ? p2 : lo;
        hi = p2 > hi ? p2 : hi;
        const T s0 = na_dot(ax, q.t), v = na_dot(ax, dl);
        const T r2 = fabs_t(na_dot(ax, u0)) * he2.x + fabs_t(na_dot(ax, u1)) * he2.y + fabs_t(na_dot(ax, u2)) * he2.z;
        if (v != T(0)) {
            const T inv = T(1) / v;
            T t1 = ((lo - r2) - s0) * inv, t2 = ((hi + r2) - s0) * inv;
            T sg = T(-1);
            if (inv < T(0)) { const T x = t1; t1 = t2; t2 = x; sg = T(1); }
            if (t1 > tin) { tin = t1; kin = k; nin = ax * sg; }
            if (t2 < tout) tout = t2;
        } else if (s0 + r2 < lo || s0 - r2 > hi) {
            return false;   // a parallel slab, separated
        }
    }
    if (!(tin <= tout) || tout < T(0)) return false;
    pen_out = tin < T(0);
    t_out = pen_out ? T(0) : tin;
    kin_out = kin; n_out = nin;
    return true;
}
// the box's closest point to p, the box he2 at rotation q.r and centre tp
template <class T> __device__ __forceinline__ V3<T> sp_tri_box_point(V3<T> he2, const Iso<T>& q, V3<T> tp, V3<T> p) { return iso_vec(q, sp_clamp3(iso_inv_vec(q, p - tp), he2)) + tp; }
// The witnesses of sp_tri_sat_cast's answer at the impact pose (tp: the query's centre there), in the collider's frame.  The triangle's face: the query's
// support vertex against n and its projection onto the plane.  A face of the query: the triangle's support vertex along n (the first largest) and its
// projection onto the face's plane.  An edge pair: the closest points of the two lines.  A witness outside its feature: onto the triangle
// (tri_closest_point), onto the box (sp_clamp3), once more onto the triangle, and the box's closest point to that.
template <class T> __device__ __forceinline__ CastWitness<T> sp_tri_sat_witness(V3<T> a, V3<T> b, V3<T> c, V3<T> he2, const Iso<T>& q, V3<T> tp, int kin, V3<T> n) {
    const V3<T> s2 = iso_vec(q, cuboid_support_point(he2, iso_inv_vec(q, -n))) + tp;
    V3<T> p1, p2;
    bool in;
    int rg;
    if (kin == 0) {
        const V3<T> N = tri_unit_normal<T>(a, b, c);
        p2 = s2;
        p1 = s2 - N * na_dot(N, s2 - a);
        (void)tri_closest_point<T>(a, b, c, p1, rg);
        in = rg == 0;
    } else if (kin < 4) {
        const T da = na_dot(n, a), db = na_dot(n, b), dc = na_dot(n, c);
        V3<T> s1 = a;
        T dm = da;
        if (db > dm) { dm = db; s1 = b; }
        if (dc > dm) { dm = dc; s1 = c; }
        const T h = kin == 1 ? he2.x : (kin == 2 ? he2.y : he2.z);
        p1 = s1;
        p2 = s1 - n * (na_dot(s1 - tp, n) + h);
        const V3<T> x = iso_inv_vec(q, s1 - tp);
        in = (kin == 1 || fabs_t(x.x) <= he2.x) && (kin == 2 || fabs_t(x.y) <= he2.y) && (kin == 3 || fabs_t(x.z) <= he2.z);
    } else {
        // the lines v_k + lambda e_k and s2 + mu u_b
        const int ib = (kin - 4) / 3, ie = (kin - 4) % 3;
        const V3<T> vk = tri_pick3<T>(a, b, c, ie);
        const V3<T> ek = tri_pick3<T>(b, c, a, ie) - vk;
        const V3<T> ub = iso_vec(q, sp_unit<T>(ib, T(1)));
        const V3<T> w = vk - s2;
        const T aa = na_dot(ek, ek), bc = na_dot(ek, ub), cc = na_dot(ub, ub), dd = na_dot(ek, w), ee = na_dot(ub, w);
        const T den = aa * cc - bc * bc;
        const bool cross = den > Limits<T>::eps * (aa * cc);
        const T lam = (bc * ee - cc * dd) / den, mu = (aa * ee - bc * dd) / den;
        // (edges too nearly parallel for the quotient: the middle of the triangle's edge)
        p1 = cross ? vk + ek * lam : vk + ek * T(0.5);
        p2 = s2 + ub * mu;
        const V3<T> x = iso_inv_vec(q, p2 - tp);
        in = cross && lam >= T(0) && lam <= T(1) && fabs_t(ib == 0 ? x.x : (ib == 1 ? x.y : x.z)) <= (ib == 0 ? he2.x : (ib == 1 ? he2.y : he2.z));
    }
    if (in) return {p1, p2};
    p1 = tri_closest_point<T>(a, b, c, p1, rg);
    p2 = sp_tri_box_point<T>(he2, q, tp, p1);
    p1 = tri_closest_point<T>(a, b, c, p2, rg);
    return {p1, sp_tri_box_point<T>(he2, q, tp, p1)};
}

// The cast of the query shape (shape2, he2, pose iso2) along d against the triangle collider, in the collider's frame.  A ball: sp_newton_cast on the
// distance of its centre from the triangle (tri_closest_point), R = r.  CAPSULE: sp_newton_cast on sp_seg_tri_d2 of its core, R = r.  A cuboid:
// sp_tri_sat_cast and its witnesses.  Same answer as sp_cast_exact: p1 / n1 the collider's, p2 the query's at the impact pose; everything zero when the
// shapes overlap at the start.
template <class T, bool CAPSULE>
__device__ __forceinline__ bool sp_tricol_cast_exact(uint32_t shape2, V3<T> he2, const Iso<T>& iso2, V3<T> d, T max_distance, NpTri<T> tri, V3<T> pos1, Q4<T> rot1,
                                                     T& toi, V3<T>& p1, V3<T>& p2, V3<T>& n1) {
    const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
    const V3<T> dl = na_qrot(qinverse(rot1), d);
    const V3<T> ta = tri.a, tb = tri.b, tc = tri.c;
    T t = T(0);
    bool pen = false;
    V3<T> w1 = vzero<T>(), w2 = vzero<T>(), wn = vzero<T>();
    if (CAPSULE || shape2 == AVN_SHAPE_BALL) {
        V3<T> A = q.t, u = vzero<T>();
        if (CAPSULE) sp_capsule_core<T>(q, he2.y, A, u);
        V3<T> n, pq, pc;
        const bool hit = sp_newton_cast<T>([&](T tt, V3<T>& pa, V3<T>& pb) {
            if (CAPSULE) return sp_seg_tri_d2<T>(ta, tb, tc, A + dl * tt, u, pa, pb);
            int rg;
            pa = A + dl * tt;
            pb = tri_closest_point<T>(ta, tb, tc, pa, rg);
            const V3<T> df = pa - pb;
            return na_dot(df, df);
        }, dl, he2.x, max_distance, t, n, pq, pc, pen);
        if (!hit || !(t <= max_distance) || !finite_t(t)) return false;
        if (!pen) {
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, pc) + pos1;
            w2 = na_qrot(rot1, pq - n * he2.x) + pos1;
        }
    } else {
        int kin = -1;
        V3<T> n;
        if (!sp_tri_sat_cast<T>(ta, tb, tc, he2, q, dl, t, kin, n, pen)) return false;
        if (!(t <= max_distance) || !finite_t(t)) return false;
        if (!pen) {
            const CastWitness<T> wt = sp_tri_sat_witness<T>(ta, tb, tc, he2, q, q.t + dl * t, kin, n);
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, wt.p1) + pos1;
            w2 = na_qrot(rot1, wt.p2) + pos1;
        }
    }
    toi = t; p1 = w1; p2 = w2; n1 = wn;
    return true;
}

}  // namespace avn
