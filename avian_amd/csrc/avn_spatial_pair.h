// avn_spatial_pair.h — the per-pair device functions of the shape casts and of the origin-penetration rule (include/avian_mi355x_spatial.h
// "shape cast", "shape contacts"): shared by the spatial queries (k_spatial.hip) and the swept CCD pass (k_ccd.hip).  The header defines
// the per-pair tests, operation order included; tests/spatial_cast_reference.py does the same operations in order.  The capsule query
// shape's pair tests (the spatial queries only) follow: tests/spatial_capsule_reference.py.  The capsule COLLIDER's pair tests of the spatial
// queries (the CCAP instantiations of k_spatial.hip) are at the end: tests/spatial_capsule_collider_reference.py.
#pragma once
#include "avn_kernels.h"
#include "avn_narrow.h"
#include "../../include/avian_mi355x_spatial.h"

namespace avn {

template <class T> __device__ __forceinline__ T sp_inf() { return (T)__builtin_huge_val(); }
template <class T> __device__ __forceinline__ T sp_vget(const V3<T>& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }

// the header's ball-ray test (solid) of a local ray: false = a miss; an origin inside answers t = 0 with `inside` set
template <class T> __device__ __forceinline__ bool sp_ball_ray(V3<T> o, V3<T> d, T r, T& t, bool& inside) {
    const T a = dot(d, d), b = dot(o, d), c = dot(o, o) - r * r;
    if (c > T(0) && b > T(0)) return false;
    const V3<T> f = o - d * (b / a);
    const T delta = a * (r * r - dot(f, f));
    if (delta < T(0)) return false;
    t = (-b - sqrt_t(delta)) / a;
    inside = t <= T(0);
    if (inside) t = T(0);
    return true;
}
// the header's slab clip (solid) of a local ray against the box of half extents h: axis = -1 when the origin is inside
template <class T> __device__ __forceinline__ bool sp_slab_ray(V3<T> o, V3<T> d, V3<T> h, T& t, int& axis, T& sg) {
    T tmin = -sp_inf<T>(), tmax = sp_inf<T>();
    int na = -1;
    T nsg = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const T oi = sp_vget(o, i), di = sp_vget(d, i), hi = sp_vget(h, i);
        if (di != T(0)) {
            const T inv = T(1) / di;
            T t1 = (-hi - oi) * inv, t2 = (hi - oi) * inv;
            T sn = T(-1);
            if (inv < T(0)) { const T x = t1; t1 = t2; t2 = x; sn = T(1); }
            if (t1 > tmin) { tmin = t1; na = i; nsg = sn; }
            if (t2 < tmax) tmax = t2;
        } else if (oi < -hi || oi > hi) {
            return false;
        }
    }
    if (!(tmin <= tmax) || tmax < T(0)) return false;
    if (tmin < T(0)) { t = T(0); axis = -1; sg = T(0); }
    else { t = tmin; axis = na; sg = nsg; }
    return true;
}
template <class T> __device__ __forceinline__ V3<T> sp_unit(int i, T s) { return V3<T>{i == 0 ? s : T(0), i == 1 ? s : T(0), i == 2 ? s : T(0)}; }

// The ray (o, d) of a ball's centre against the cuboid `he` rounded by the ball's radius r, in the cuboid's frame: the union of the three
// boxes he + r e_i, and for r > 0 the twelve clipped edge cylinders and the eight corner spheres, in that order; the smallest entry wins
// (strict <), its primitive gives the normal.  pen: the origin is inside the winning primitive (distance 0, no normal).
template <class T> __device__ __forceinline__ bool sp_round_box_ray(V3<T> o, V3<T> d, V3<T> he, T r, T& t_out, V3<T>& n_out, bool& pen_out) {
    T best = sp_inf<T>();
    V3<T> bn = vzero<T>();
    bool bpen = false, found = false;
    for (int i = 0; i < 3; ++i) {
        const V3<T> h = he + sp_unit<T>(i, r);
        T t, sg; int axis;
        if (sp_slab_ray<T>(o, d, h, t, axis, sg) && t < best) { best = t; found = true; bpen = axis < 0; bn = axis < 0 ? vzero<T>() : sp_unit<T>(axis, sg); }
    }
    if (r > T(0)) {
        // edge cylinders: edge direction k, the edge through (sa he_a, sb he_b) in the plane of a = k + 1, b = k + 2 (mod 3)
        for (int e = 0; e < 12; ++e) {
            const int k = e >> 2, ia = (k + 1) % 3, ib = (k + 2) % 3;
            const T sa = (e & 1) ? T(1) : T(-1), sb = (e & 2) ? T(1) : T(-1);
            const T oa = sp_vget(o, ia) - sa * sp_vget(he, ia), ob = sp_vget(o, ib) - sb * sp_vget(he, ib);
            const T da = sp_vget(d, ia), db = sp_vget(d, ib), ok = sp_vget(o, k), dk = sp_vget(d, k), hk = sp_vget(he, k);
            const T a = da * da + db * db;
            if (!(a > T(0))) continue;   // parallel to the edge: the boxes and the corner spheres decide
            const T b = oa * da + ob * db, c = (oa * oa + ob * ob) - r * r;
            if (c > T(0) && b > T(0)) continue;
            const T q = b / a;
            const T fa = oa - da * q, fb = ob - db * q;
            const T delta = a * (r * r - (fa * fa + fb * fb));
            if (delta < T(0)) continue;
            T t = (-b - sqrt_t(delta)) / a;
            const bool inside = t <= T(0);
            if (inside) t = T(0);
            const T z = ok + dk * t;
            if (!(fabs_t(z) <= hk)) continue;   // beyond the edge's extent: a corner sphere's
            if (t < best) {
                best = t; found = true; bpen = inside;
                const T pa = oa + da * t, pb = ob + db * t;
                const T l = sqrt_t(pa * pa + pb * pb);
                if (inside || !(l > T(0))) bn = vzero<T>();
                else {
                    const T na = pa / l, nb = pb / l;
                    bn = V3<T>{ia == 0 ? na : (ib == 0 ? nb : T(0)), ia == 1 ? na : (ib == 1 ? nb : T(0)), ia == 2 ? na : (ib == 2 ? nb : T(0))};
                }
            }
        }
        // corner spheres: bit 0 / 1 / 2 of s = the sign of x / y / z
        for (int s = 0; s < 8; ++s) {
            const V3<T> cen{(s & 1) ? he.x : -he.x, (s & 2) ? he.y : -he.y, (s & 4) ? he.z : -he.z};
            const V3<T> oc = o - cen;
            T t; bool inside;
            if (!sp_ball_ray<T>(oc, d, r, t, inside)) continue;
            if (t < best) {
                best = t; found = true; bpen = inside;
                const V3<T> p = oc + d * t;
                const T l = length(p);
                bn = (inside || !(l > T(0))) ? vzero<T>() : p / l;
            }
        }
    }
    if (!found) return false;
    t_out = best; n_out = bn; pen_out = bpen;
    return true;
}

template <class T> __device__ __forceinline__ V3<T> sp_sel3(int i, V3<T> a, V3<T> b, V3<T> c) { return i == 0 ? a : (i == 1 ? b : c); }
// The swept SAT of the collider's cuboid he1 (at the origin of its own frame) and the query's cuboid he2 at pose q moving along dl:
// the 15 axes in the order e_0..e_2 (collider faces), u_0..u_2 (query faces), e_a x u_b with b outer and a inner (sat_edge_twoway's
// order).  kin = the axis of the largest entry, n = that axis oriented from the collider towards the query.
template <class T> __device__ __forceinline__ bool sp_sat_cast(V3<T> he1, V3<T> he2, const Iso<T>& q, V3<T> dl, T& t_out, int& kin_out, V3<T>& n_out, bool& pen_out) {
    const V3<T> u0 = iso_vec(q, V3<T>{T(1), T(0), T(0)}), u1 = iso_vec(q, V3<T>{T(0), T(1), T(0)}), u2 = iso_vec(q, V3<T>{T(0), T(0), T(1)});
    T tin = -sp_inf<T>(), tout = sp_inf<T>();
    int kin = -1;
    V3<T> nin = vzero<T>();
    for (int k = 0; k < 15; ++k) {
        V3<T> ax;
        if (k < 3) ax = sp_unit<T>(k, T(1));
        else if (k < 6) ax = sp_sel3(k - 3, u0, u1, u2);
        else {
            const int b = (k - 6) / 3, a = (k - 6) % 3;
            const V3<T> u = sp_sel3(b, u0, u1, u2);
            const V3<T> axis = a == 0 ? V3<T>{T(0), -u.z, u.y} : (a == 1 ? V3<T>{u.z, T(0), -u.x} : V3<T>{-u.y, u.x, T(0)});
            const T norm1 = na_norm(axis);
            if (!(norm1 > Limits<T>::eps)) continue;
            ax = axis / norm1;
        }
        const T s0 = na_dot(ax, q.t), v = na_dot(ax, dl);
        const T r1 = fabs_t(ax.x) * he1.x + fabs_t(ax.y) * he1.y + fabs_t(ax.z) * he1.z;
        const T r2 = fabs_t(na_dot(ax, u0)) * he2.x + fabs_t(na_dot(ax, u1)) * he2.y + fabs_t(na_dot(ax, u2)) * he2.z;
        const T rr = r1 + r2;
        if (v != T(0)) {
            const T inv = T(1) / v;
            T t1 = (-rr - s0) * inv, t2 = (rr - s0) * inv;
            T sg = T(-1);
            if (inv < T(0)) { const T x = t1; t1 = t2; t2 = x; sg = T(1); }
            if (t1 > tin) { tin = t1; kin = k; nin = ax * sg; }
            if (t2 < tout) tout = t2;
        } else if (s0 < -rr || s0 > rr) {
            return false;   // a parallel slab, separated
        }
    }
    if (!(tin <= tout) || tout < T(0)) return false;
    pen_out = tin < T(0);
    t_out = pen_out ? T(0) : tin;
    kin_out = kin; n_out = nin;
    return true;
}
// the witnesses of sp_sat_cast's answer at the impact pose, in the collider's frame
template <class T> struct CastWitness { V3<T> p1, p2; };
template <class T> __device__ __forceinline__ V3<T> sp_clamp3(V3<T> p, V3<T> h) {
    return V3<T>{p.x < -h.x ? -h.x : (p.x > h.x ? h.x : p.x), p.y < -h.y ? -h.y : (p.y > h.y ? h.y : p.y), p.z < -h.z ? -h.z : (p.z > h.z ? h.z : p.z)};
}
// When the support feature's witness falls outside the other shape's face or edge (parallel faces or edges: the contact is a polygon or a
// segment), the witness is clamped onto the collider's cuboid and the query's witness is the query cuboid's closest point to it.
template <class T> __device__ __forceinline__ CastWitness<T> sp_sat_witness(V3<T> he1, V3<T> he2, const Iso<T>& q, V3<T> tp, int kin, V3<T> n) {
    const V3<T> s1 = cuboid_support_point(he1, n);
    const V3<T> s2 = iso_vec(q, cuboid_support_point(he2, iso_inv_vec(q, -n))) + tp;
    V3<T> p1, p2;
    bool in;
    if (kin < 3) {
        // a face of the collider: the query's support vertex against the normal and its projection onto the face
        p1 = V3<T>{kin == 0 ? n.x * he1.x : s2.x, kin == 1 ? n.y * he1.y : s2.y, kin == 2 ? n.z * he1.z : s2.z};
        p2 = s2;
        in = (kin == 0 || fabs_t(s2.x) <= he1.x) && (kin == 1 || fabs_t(s2.y) <= he1.y) && (kin == 2 || fabs_t(s2.z) <= he1.z);
    } else if (kin < 6) {
        // a face of the query: the collider's support vertex towards the query and its projection onto the face's plane
        const T h = kin == 3 ? he2.x : (kin == 4 ? he2.y : he2.z);
        p1 = s1;
        p2 = s1 - n * (na_dot(s1 - tp, n) + h);
        const V3<T> x = iso_inv_vec(q, s1 - tp);
        in = (kin == 3 || fabs_t(x.x) <= he2.x) && (kin == 4 || fabs_t(x.y) <= he2.y) && (kin == 5 || fabs_t(x.z) <= he2.z);
        if (!in) {
            // start from the point of the query's face nearest the vertex
            const V3<T> xl = iso_inv_vec(q, -n);
            const V3<T> xc = sp_clamp3(x, he2);
            const V3<T> xf{kin == 3 ? copysign_t(he2.x, xl.x) : xc.x, kin == 4 ? copysign_t(he2.y, xl.y) : xc.y, kin == 5 ? copysign_t(he2.z, xl.z) : xc.z};
            p1 = iso_vec(q, xf) + tp;
        }
    } else {
        // an edge pair: the closest points of the two support edges' lines, s1 + lambda e_a and s2 + mu u_b
        const int b = (kin - 6) / 3, a = (kin - 6) % 3;
        const V3<T> ea = sp_unit<T>(a, T(1));
        const V3<T> ub = iso_vec(q, sp_unit<T>(b, T(1)));
        const V3<T> w = s1 - s2;
        const T bc = na_dot(ea, ub), cc = na_dot(ub, ub), dd = na_dot(ea, w), ee = na_dot(ub, w);
        const T den = cc - bc * bc;
        const bool cross = den > Limits<T>::eps;
        const T lam = (bc * ee - cc * dd) / den, mu = (ee - bc * dd) / den;
        // (edges too nearly parallel for the quotient: the middle of the collider's edge)
        p1 = cross ? s1 + ea * lam : s1 - ea * na_dot(ea, s1);
        p2 = s2 + ub * mu;
        const V3<T> x = iso_inv_vec(q, p2 - tp);
        in = cross && fabs_t(na_dot(ea, p1)) <= (a == 0 ? he1.x : (a == 1 ? he1.y : he1.z)) && fabs_t(b == 0 ? x.x : (b == 1 ? x.y : x.z)) <= (b == 0 ? he2.x : (b == 1 ? he2.y : he2.z));
    }
    if (in) return {p1, p2};
    // onto the collider, onto the query, and once more: for faces whose edges are parallel this ends in the overlap of the two faces
    p1 = sp_clamp3(p1, he1);
    p2 = iso_vec(q, sp_clamp3(iso_inv_vec(q, p1 - tp), he2)) + tp;
    p1 = sp_clamp3(p2, he1);
    return {p1, iso_vec(q, sp_clamp3(iso_inv_vec(q, p1 - tp), he2)) + tp};
}

// The header's cast of the query shape (shape2, he2, pose iso2 = make_isometry of its position and rotation) along d against one collider
// (shape 1).  World-space answer: toi, the witnesses p1 (collider) / p2 (query shape at the impact pose) and the collider's normal n1
// (the record's normal2 is -n1); all zero when the shapes overlap at the start.
template <class T>
__device__ __forceinline__ bool sp_cast_exact(uint32_t shape2, V3<T> he2, const Iso<T>& iso2, V3<T> d, T max_distance, uint32_t shape1, V3<T> he1, V3<T> pos1, Q4<T> rot1,
                                              T& toi, V3<T>& p1, V3<T>& p2, V3<T>& n1) {
    const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
    const V3<T> dl = na_qrot(qinverse(rot1), d);
    const bool ball1 = shape1 == AVN_SHAPE_BALL, ball2 = shape2 == AVN_SHAPE_BALL;
    T t; bool pen; V3<T> n;
    int kin = -1;
    if (ball1 && ball2) {
        if (!sp_ball_ray<T>(q.t, dl, he1.x + he2.x, t, pen)) return false;
    } else if (ball1 || ball2) {
        // the ball's centre against the rounded cuboid, in the cuboid's frame (the query cuboid's: the ray reversed)
        const V3<T> o = ball2 ? q.t : iso_inv_point(q, vzero<T>());
        const V3<T> dd = ball2 ? dl : -iso_inv_vec(q, dl);
        if (!sp_round_box_ray<T>(o, dd, ball2 ? he1 : he2, ball2 ? he2.x : he1.x, t, n, pen)) return false;
    } else {
        if (!sp_sat_cast<T>(he1, he2, q, dl, t, kin, n, pen)) return false;
    }
    if (!(t <= max_distance) || !finite_t(t)) return false;
    toi = t;
    V3<T> w1 = vzero<T>(), w2 = vzero<T>(), wn = vzero<T>();
    if (!pen) {
        const V3<T> c2 = iso2.t + d * t;   // the query shape's position at the impact
        if (ball1 && ball2) {
            const V3<T> p = q.t + dl * t;
            const T l = length(p);
            n = l > T(0) ? p / l : vzero<T>();
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, n * he1.x) + pos1;
            w2 = c2 + (-wn) * he2.x;
        } else if (ball2) {
            const V3<T> pk = (q.t + dl * t) - n * he2.x;
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, pk) + pos1;
            w2 = c2 + (-wn) * he2.x;
        } else if (ball1) {
            const V3<T> o = iso_inv_point(q, vzero<T>());
            const V3<T> dd = -iso_inv_vec(q, dl);
            const V3<T> pk = (o + dd * t) - n * he1.x;
            wn = -na_qrot(iso2.r, n);
            w2 = na_qrot(iso2.r, pk) + c2;
            w1 = pos1 + wn * he1.x;
        } else {
            const CastWitness<T> wt = sp_sat_witness<T>(he1, he2, q, q.t + dl * t, kin, n);
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, wt.p1) + pos1;
            w2 = na_qrot(rot1, wt.p2) + pos1;
        }
    }
    p1 = w1; p2 = w2; n1 = wn;
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// The capsule as a QUERY shape (AVN_SHAPE_CAPSULE, include/avian_mi355x_spatial.h "capsule query shapes"): parry's Capsule::new_y, the
// segment (0, -h, 0) .. (0, +h, 0) of the shape's frame swept by a ball of radius r.  Every pair test works on the capsule's core segment
// A + s u, s in [0, 1], in the collider's frame; a ball collider's core is its centre, a cuboid's the box.  The header defines the tests,
// operation order included; tests/spatial_capsule_reference.py does the same operations in order.
template <class T> __device__ __forceinline__ void sp_capsule_core(const Iso<T>& q, T h, V3<T>& A, V3<T>& u) {
    const V3<T> hv = na_qrot(q.r, V3<T>{T(0), h, T(0)});
    A = q.t - hv;
    u = hv * T(2);
}
// segment - point: the squared distance and the parameter of the nearest point
template <class T> __device__ __forceinline__ T sp_seg_point(V3<T> A, V3<T> u, V3<T> c, T& s_out) {
    const T uu = na_dot(u, u);
    T s = na_dot(c - A, u) / uu;
    s = s < T(0) ? T(0) : (s > T(1) ? T(1) : s);
    if (uu == T(0)) s = T(0);
    const V3<T> e = c - (A + u * s);
    s_out = s;
    return na_dot(e, e);
}
template <class T> __device__ __forceinline__ T cp_clamp01(T x) { return x < T(0) ? T(0) : (x > T(1) ? T(1) : x); }
// sin^2 of the angle under which two capsule axes count as parallel (two-point manifold): parallel to rounding, not a tuning knob
template <class T> __device__ __forceinline__ T cp_parallel() { return Limits<T>::eps * T(64); }
// segment - segment: the clamped closest points A1 + s u1, A2 + t u2 with the dot products they came from.  par: both segments have a length
// and their axes count as parallel (s = 0 is tried first; the capsule manifold then looks for an overlap).  ONE routine for the capsule
// collider's manifold (avn_capsule_pair.h) and the spatial queries of a capsule against a capsule collider (below).
template <class T> struct SegSeg { T a, e, f, c, b, s, t; bool par; };
template <class T> __device__ __forceinline__ SegSeg<T> sp_seg_seg(V3<T> A1, V3<T> u1, V3<T> A2, V3<T> u2) {
    const V3<T> w = A1 - A2;
    const T a = na_dot(u1, u1), e = na_dot(u2, u2), f = na_dot(u2, w), c = na_dot(u1, w), b = na_dot(u1, u2);
    T s = T(0), t = T(0);
    bool par = false;
    if (a == T(0) && e == T(0)) {}                       // two points
    else if (a == T(0)) t = cp_clamp01<T>(f / e);        // segment 1 is a point
    else if (e == T(0)) s = cp_clamp01<T>(-c / a);       // segment 2 is a point
    else {
        const T ae = a * e;
        const T den = ae - b * b;
        par = !(den > cp_parallel<T>() * ae);
        s = par ? T(0) : cp_clamp01<T>((b * f - c * e) / den);
        t = (b * s + f) / e;
        if (t < T(0)) { t = T(0); s = cp_clamp01<T>(-c / a); }
        else if (t > T(1)) { t = T(1); s = cp_clamp01<T>((b - c) / a); }
    }
    return SegSeg<T>{a, e, f, c, b, s, t, par};
}
// The squared distance of two segments for the QUERIES, with the two points.  sp_seg_seg's quotient (b f - c e) / den cancels for nearly parallel
// axes (its s is wrong by about eps / sin^2), and under its parallel rule s is simply 0: good enough for the manifold, which then looks for an
// overlap, but an over-estimate of the distance of converging or crossing cores.  So six candidate pairs are evaluated in full, in this order, and
// the first with the smallest |p2 - p1|^2 wins (strict <; a NaN candidate never wins): sp_seg_seg's (s, t); the interior point in its
// well-conditioned form -- with u2p = u2 - u1 (b / a) and wp = w - u1 (c / a), the parts perpendicular to u1: t = clamp(dot(wp, u2p) / dot(u2p, u2p)),
// s = clamp((b t - c) / a), t = clamp((b s + f) / e) --; and the four ends against the other segment: (0, clamp(f / e)), (1, clamp((b + f) / e)),
// (clamp(-c / a), 0), (clamp((b - c) / a), 1).  The minimum of the convex distance over the square is the interior point or lies on an edge, so
// this is exact up to rounding.  capsule_pair_manifold does not come here: its bits are sp_seg_seg's.
template <class T> __device__ __forceinline__ void sp_seg_seg_try(V3<T> A1, V3<T> u1, V3<T> A2, V3<T> u2, T s, T t, T& best, V3<T>& p1, V3<T>& p2) {
    const V3<T> q1 = A1 + u1 * s, q2 = A2 + u2 * t;
    const V3<T> d = q2 - q1;
    const T d2 = na_dot(d, d);
    if (d2 < best) { best = d2; p1 = q1; p2 = q2; }
}
template <class T> __device__ __forceinline__ T sp_seg_seg_d2(V3<T> A1, V3<T> u1, V3<T> A2, V3<T> u2, V3<T>& p1, V3<T>& p2) {
    const SegSeg<T> ss = sp_seg_seg<T>(A1, u1, A2, u2);
    const T a = ss.a, e = ss.e, f = ss.f, c = ss.c, b = ss.b;
    T best = sp_inf<T>();
    p1 = A1 + u1 * ss.s; p2 = A2 + u2 * ss.t;   // (what stands when every candidate is NaN: non-finite inputs)
    sp_seg_seg_try<T>(A1, u1, A2, u2, ss.s, ss.t, best, p1, p2);
    {
        const V3<T> w = A1 - A2;
        const V3<T> u2p = u2 - u1 * (b / a), wp = w - u1 * (c / a);
        T t = cp_clamp01<T>(na_dot(wp, u2p) / na_dot(u2p, u2p));
        const T s = cp_clamp01<T>((b * t - c) / a);
        t = cp_clamp01<T>((b * s + f) / e);
        sp_seg_seg_try<T>(A1, u1, A2, u2, s, t, best, p1, p2);
    }
    sp_seg_seg_try<T>(A1, u1, A2, u2, T(0), cp_clamp01<T>(f / e), best, p1, p2);
    sp_seg_seg_try<T>(A1, u1, A2, u2, T(1), cp_clamp01<T>((b + f) / e), best, p1, p2);
    sp_seg_seg_try<T>(A1, u1, A2, u2, cp_clamp01<T>(-c / a), T(0), best, p1, p2);
    sp_seg_seg_try<T>(A1, u1, A2, u2, cp_clamp01<T>((b - c) / a), T(1), best, p1, p2);
    const V3<T> d = p2 - p1;
    return na_dot(d, d);
}
// segment - box, exact.  f(s) = sum_i max(|x_i(s)| - he_i, 0)^2 is convex and piecewise quadratic; its breakpoints are the s = (+-he_i - A_i) / u_i
// strictly inside (0, 1) (one that is not counts as 1).  Candidates, in this order: 0, 1, the six breakpoints ascending (a 12-comparator
// network), then per interval between neighbours of 0 <= b_1 <= .. <= b_6 <= 1 the minimiser of the quadratic whose active faces are read at
// the interval's midpoint, clamped to the interval (the midpoint itself when no face is active: f = 0 there; the interval's start when
// the active axes have no slope).  The first candidate with the smallest f, evaluated in full, wins (strict <).
template <class T> struct SegBox { T f, s; V3<T> ps, pb; };
template <class T> __device__ __forceinline__ T sp_seg_break(T a, T u, T h) {
    const T s = (h - a) / u;
    return (u != T(0) && s > T(0) && s < T(1)) ? s : T(1);
}
template <class T> __device__ __forceinline__ void sp_seg_order(T& a, T& b) {
    const bool sw = b < a;
    const T lo = sw ? b : a, hi = sw ? a : b;
    a = lo; b = hi;
}
template <class T> __device__ __forceinline__ void sp_seg_try(V3<T> A, V3<T> u, V3<T> he, T s, T& bf, T& bs) {
    const V3<T> p = A + u * s;
    const V3<T> e = p - sp_clamp3(p, he);
    const T f = na_dot(e, e);
    if (f < bf) { bf = f; bs = s; }
}
template <class T> __device__ __forceinline__ void sp_seg_interval(V3<T> A, V3<T> u, V3<T> he, T lo, T hi, T& bf, T& bs) {
    const T mid = (lo + hi) * T(0.5);
    const V3<T> m = A + u * mid;
    const T sx = m.x > he.x ? T(1) : (m.x < -he.x ? T(-1) : T(0));
    const T sy = m.y > he.y ? T(1) : (m.y < -he.y ? T(-1) : T(0));
    const T sz = m.z > he.z ? T(1) : (m.z < -he.z ? T(-1) : T(0));
    const T den = (sx != T(0) ? u.x * u.x : T(0)) + (sy != T(0) ? u.y * u.y : T(0)) + (sz != T(0) ? u.z * u.z : T(0));
    const T num = (sx != T(0) ? u.x * (A.x - sx * he.x) : T(0)) + (sy != T(0) ? u.y * (A.y - sy * he.y) : T(0)) + (sz != T(0) ? u.z * (A.z - sz * he.z) : T(0));
    T s = -num / den;
    s = s < lo ? lo : (s > hi ? hi : s);
    const bool none = sx == T(0) && sy == T(0) && sz == T(0);
    sp_seg_try<T>(A, u, he, none ? mid : (den > T(0) ? s : lo), bf, bs);
}
template <class T> __device__ __forceinline__ SegBox<T> sp_seg_box(V3<T> A, V3<T> u, V3<T> he) {
    T b0 = sp_seg_break<T>(A.x, u.x, -he.x), b1 = sp_seg_break<T>(A.x, u.x, he.x), b2 = sp_seg_break<T>(A.y, u.y, -he.y), b3 = sp_seg_break<T>(A.y, u.y, he.y),
      b4 = sp_seg_break<T>(A.z, u.z, -he.z), b5 = sp_seg_break<T>(A.z, u.z, he.z);
    sp_seg_order(b0, b5); sp_seg_order(b1, b3); sp_seg_order(b2, b4);
    sp_seg_order(b1, b2); sp_seg_order(b3, b4);
    sp_seg_order(b0, b3); sp_seg_order(b2, b5);
    sp_seg_order(b0, b1); sp_seg_order(b2, b3); sp_seg_order(b4, b5);
    sp_seg_order(b1, b2); sp_seg_order(b3, b4);
    T bf = sp_inf<T>(), bs = T(0);
    sp_seg_try<T>(A, u, he, T(0), bf, bs); sp_seg_try<T>(A, u, he, T(1), bf, bs);
    sp_seg_try<T>(A, u, he, b0, bf, bs); sp_seg_try<T>(A, u, he, b1, bf, bs); sp_seg_try<T>(A, u, he, b2, bf, bs);
    sp_seg_try<T>(A, u, he, b3, bf, bs); sp_seg_try<T>(A, u, he, b4, bf, bs); sp_seg_try<T>(A, u, he, b5, bf, bs);
    sp_seg_interval<T>(A, u, he, T(0), b0, bf, bs); sp_seg_interval<T>(A, u, he, b0, b1, bf, bs); sp_seg_interval<T>(A, u, he, b1, b2, bf, bs);
    sp_seg_interval<T>(A, u, he, b2, b3, bf, bs); sp_seg_interval<T>(A, u, he, b3, b4, bf, bs); sp_seg_interval<T>(A, u, he, b4, b5, bf, bs);
    sp_seg_interval<T>(A, u, he, b5, T(1), bf, bs);
    SegBox<T> r;
    r.f = bf; r.s = bs;
    r.ps = A + u * bs;
    r.pb = sp_clamp3(r.ps, he);
    return r;
}

// intersection of the capsule (r, h) at the relative pose q (the capsule in the collider's frame) with the collider: core distance^2 <= (r + r_c)^2
template <class T> __device__ __forceinline__ bool sp_capsule_intersects(T r, T h, const Iso<T>& q, uint32_t shape1, V3<T> he1) {
    V3<T> A, u;
    sp_capsule_core<T>(q, h, A, u);
    if (shape1 == AVN_SHAPE_BALL) {
        T s;
        const T d2 = sp_seg_point<T>(A, u, vzero<T>(), s);
        const T rr = r + he1.x;
        return d2 <= rr * rr;
    }
    return sp_seg_box<T>(A, u, he1).f <= r * r;
}

// The ray (o, d) of a ball's centre against the capsule (R, h) in the capsule's frame: the cylinder about y clipped to |y| <= h, then the end
// spheres at -h and +h; the smallest entry wins (strict <), its primitive gives the normal.  pen: the origin is inside the winning primitive.
template <class T> __device__ __forceinline__ bool sp_capsule_ray(V3<T> o, V3<T> d, T h, T R, T& t_out, V3<T>& n_out, bool& pen_out) {
    T best = sp_inf<T>();
    V3<T> bn = vzero<T>();
    bool bpen = false, found = false;
    {
        const T a = d.x * d.x + d.z * d.z;
        const T b = o.x * d.x + o.z * d.z, c = (o.x * o.x + o.z * o.z) - R * R;
        const T q = b / a;
        const T fa = o.x - d.x * q, fb = o.z - d.z * q;
        const T delta = a * (R * R - (fa * fa + fb * fb));
        T t = (-b - sqrt_t(delta)) / a;
        const bool inside = t <= T(0);
        if (inside) t = T(0);
        const T y = o.y + d.y * t;
        // (a ray parallel to the axis: the end spheres decide)
        if (a > T(0) && !(c > T(0) && b > T(0)) && !(delta < T(0)) && fabs_t(y) <= h) {
            best = t; found = true; bpen = inside;
            const T pa = o.x + d.x * t, pb = o.z + d.z * t;
            const T l = sqrt_t(pa * pa + pb * pb);
            bn = (inside || !(l > T(0))) ? vzero<T>() : V3<T>{pa / l, T(0), pb / l};
        }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const V3<T> oc{o.x, e == 0 ? o.y + h : o.y - h, o.z};
        T t; bool inside;
        if (!sp_ball_ray<T>(oc, d, R, t, inside)) continue;
        if (t < best) {
            best = t; found = true; bpen = inside;
            const V3<T> p = oc + d * t;
            const T l = length(p);
            bn = (inside || !(l > T(0))) ? vzero<T>() : p / l;
        }
    }
    if (!found) return false;
    t_out = best; n_out = bn; pen_out = bpen;
    return true;
}

#define SP_CAPSULE_ROUNDS 32
// Newton's iteration on g(t) = dist(t) - R from t = 0, which rises monotonically to the root from its left (g is convex): closest(t, a, b)
// answers the squared distance of the moving core displaced by dl t (its point a) from the fixed one (its point b).  At most SP_CAPSULE_ROUNDS
// evaluations, the last t standing.  n: from b towards a; pen: the cores are within R at t = 0.  false = a miss.
template <class T, class Closest>
__device__ __forceinline__ bool sp_newton_cast(Closest closest, V3<T> dl, T R, T max_distance, T& t, V3<T>& n, V3<T>& pm, V3<T>& pf, bool& pen) {
    n = vzero<T>(); pm = vzero<T>(); pf = vzero<T>();
    bool hit = false;
    for (int k = 0; k < SP_CAPSULE_ROUNDS; ++k) {
        V3<T> a, b;
        const T dist = sqrt_t(closest(t, a, b));
        if (dist > T(0)) n = (a - b) / dist;   // (dist == 0, touching cores arriving: the round before's direction stands)
        pm = a; pf = b;
        if (dist <= R) { pen = k == 0; hit = true; break; }
        const T v = -na_dot(n, dl);
        if (!(v > T(0))) return false;
        const T tn = t + (dist - R) / v;
        if (tn > max_distance) return false;
        if (!(tn > t) || k == SP_CAPSULE_ROUNDS - 1) { hit = true; break; }
        t = tn;
    }
    return hit;
}
// The cast of the capsule (r, h) at pose iso2 along d against one collider.  A ball collider: its centre as a ray against the capsule grown by
// the ball's radius, in the capsule's frame with the ray reversed.  A cuboid: Newton's iteration on g(t) = dist(segment + t dl, box) - r
// from t = 0, which rises monotonically to the root from its left (g is convex); at most SP_CAPSULE_ROUNDS evaluations, the last t standing.
// Same answer as sp_cast_exact: everything zero when the shapes overlap at the start.
template <class T>
__device__ __forceinline__ bool sp_capsule_cast_exact(T r, T h, const Iso<T>& iso2, V3<T> d, T max_distance, uint32_t shape1, V3<T> he1, V3<T> pos1, Q4<T> rot1,
                                                      T& toi, V3<T>& p1, V3<T>& p2, V3<T>& n1) {
    const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
    const V3<T> dl = na_qrot(qinverse(rot1), d);
    T t = T(0);
    bool pen = false;
    V3<T> w1 = vzero<T>(), w2 = vzero<T>(), wn = vzero<T>();
    if (shape1 == AVN_SHAPE_BALL) {
        const V3<T> o = iso_inv_point(q, vzero<T>());
        const V3<T> dd = -iso_inv_vec(q, dl);
        V3<T> n;
        if (!sp_capsule_ray<T>(o, dd, h, r + he1.x, t, n, pen)) return false;
        if (!(t <= max_distance) || !finite_t(t)) return false;
        if (!pen) {
            const V3<T> c2 = iso2.t + d * t;
            const V3<T> pc = o + dd * t;   // the ball's centre at the impact, in the capsule's frame
            const T ys = pc.y < -h ? -h : (pc.y > h ? h : pc.y);
            const V3<T> pk = V3<T>{T(0), ys, T(0)} + n * r;
            wn = -na_qrot(iso2.r, n);
            w2 = na_qrot(iso2.r, pk) + c2;
            w1 = pos1 + wn * he1.x;
        }
    } else {
        V3<T> A, u;
        sp_capsule_core<T>(q, h, A, u);
        V3<T> n, ps, pb;
        const bool hit = sp_newton_cast<T>([&](T tt, V3<T>& a, V3<T>& b) { const SegBox<T> sb = sp_seg_box<T>(A + dl * tt, u, he1); a = sb.ps; b = sb.pb; return sb.f; },
                                           dl, r, max_distance, t, n, ps, pb, pen);
        if (!hit || !(t <= max_distance) || !finite_t(t)) return false;
        if (!pen) {
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, pb) + pos1;
            w2 = na_qrot(rot1, ps - n * r) + pos1;
        }
    }
    toi = t; p1 = w1; p2 = w2; n1 = wn;
    return true;
}

// The segment touches or crosses the box (X's f == 0): the smallest overlap over the six axes of their Minkowski difference, e_0..e_2 then
// normalize(u x e_i), the first smallest wins.  n: that axis signed towards the segment's midpoint, best: the overlap, brb: the box's
// radius along n.  Shared by the capsule query's contact (below) and the capsule collider's manifold (avn_capsule_pair.h).
template <class T> __device__ __forceinline__ void sp_seg_box_axis(V3<T> A, V3<T> u, V3<T> he1, V3<T>& n, T& best_out, T& brb_out) {
    const V3<T> hv = u * T(0.5), m = A + hv;
    const T eps2 = Limits<T>::eps * Limits<T>::eps * na_dot(u, u);
    T best = sp_inf<T>(), brb = T(0);
    n = vzero<T>();
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        V3<T> ax;
        if (k < 3) ax = sp_unit<T>(k, T(1));
        else {
            const V3<T> cx = k == 3 ? V3<T>{T(0), u.z, -u.y} : (k == 4 ? V3<T>{-u.z, T(0), u.x} : V3<T>{u.y, -u.x, T(0)});
            const T l2c = na_dot(cx, cx);
            if (!(l2c > eps2)) continue;
            ax = cx / sqrt_t(l2c);
        }
        const T rb = fabs_t(ax.x) * he1.x + fabs_t(ax.y) * he1.y + fabs_t(ax.z) * he1.z;
        const T rs = fabs_t(na_dot(ax, hv));
        const T c = na_dot(ax, m);
        const T ov = (rb + rs) - fabs_t(c);
        if (ov < best) { best = ov; brb = rb; n = c < T(0) ? -ax : ax; }
    }
    best_out = best; brb_out = brb;
}

// The contact of the capsule (r, h) at pose iso2 with one collider within `prediction`: gap = dist - r - r_c between the cores.  Cores
// apart: the normal from the collider's core point to the segment's; a segment crossing a cuboid: the smallest overlap over the six axes of
// their Minkowski difference (e_0..e_2, then normalize(u x e_i)), first smallest wins; a ball's centre on the segment: no contact.
// normal: from the collider towards the capsule (world); anchor1 / anchor2: offsets from the capsule's / the collider's position (world orientation).
template <class T>
__device__ __forceinline__ bool sp_capsule_contact(T r, T h, const Iso<T>& iso2, uint32_t shape1, V3<T> he1, V3<T> pos1, Q4<T> rot1, T prediction,
                                                   T& penetration, V3<T>& normal, V3<T>& anchor1, V3<T>& anchor2) {
    const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
    V3<T> A, u;
    sp_capsule_core<T>(q, h, A, u);
    const bool ball1 = shape1 == AVN_SHAPE_BALL;
    const T rc = ball1 ? he1.x : T(0);
    V3<T> ps, pc;
    T d2;
    if (ball1) {
        T s;
        d2 = sp_seg_point<T>(A, u, vzero<T>(), s);
        ps = A + u * s; pc = vzero<T>();
    } else {
        const SegBox<T> sb = sp_seg_box<T>(A, u, he1);
        d2 = sb.f; ps = sb.ps; pc = sb.pb;
    }
    const T dist = sqrt_t(d2);
    V3<T> n, l1, l2;
    T pen;
    if (dist > T(0)) {
        const T gap = (dist - r) - rc;
        if (gap > prediction) return false;
        n = (ps - pc) / dist;
        pen = -gap;
        l1 = ps - n * r;
        l2 = pc + n * rc;
    } else {
        if (ball1) return false;
        T best, brb;
        sp_seg_box_axis<T>(A, u, he1, n, best, brb);
        pen = best + r;
        const V3<T> pd = na_dot(n, u) < T(0) ? A + u : A;   // the segment's deepest point along -n, the lower s on a tie
        l1 = pd - n * r;
        l2 = pd + n * (brb - na_dot(n, pd));
    }
    penetration = pen;
    normal = na_qrot(rot1, n);
    anchor1 = na_qrot(rot1, l1 - q.t);
    anchor2 = na_qrot(rot1, l2);
    return true;
}

// the sink of contact_manifolds_pair_sink that keeps the running deepest raw point (ContactManifold::find_deepest_contact: Rust's max_by, the
// later point wins a tie) instead of the 16-point manifold
template <class T> struct SpDeepestSink {
    V3<T> anchor1;
    T penetration;
    int count;
    __device__ __forceinline__ int n() const { return count; }
    __device__ __forceinline__ void put(V3<T> a1, T pen, uint32_t, uint32_t) {
        if (count == 0 || !(penetration > pen)) { anchor1 = a1; penetration = pen; }
        ++count;
    }
};

// ---------------------------------------------------------------------------------------------------------
// The capsule as a COLLIDER of the spatial queries (include/avian_mi355x_spatial.h "queries against capsule colliders"; the CCAP
// instantiations of k_spatial.hip): (r_c, h_c) = (he.x, he.y), the core segment (0, -h_c, 0) .. (0, +h_c, 0) of its own frame.  The header
// defines the tests, operation order included; tests/spatial_capsule_collider_reference.py does the same operations in order.
template <class T> __device__ __forceinline__ void sp_capcol_core(T h, V3<T>& A, V3<T>& u) {
    A = V3<T>{T(0), -h, T(0)};
    u = V3<T>{T(0), h * T(2), T(0)};
}
// The exit of the ray (o, d), whose origin is inside the capsule (R, h), in the capsule's frame: the cylinder's far root where |y| <= h, then
// the far roots of the end spheres at -h and +h; the largest wins (strict >), its primitive gives the outward normal.
template <class T> __device__ __forceinline__ bool sp_capsule_ray_exit(V3<T> o, V3<T> d, T h, T R, T& t_out, V3<T>& n_out) {
    T best = -sp_inf<T>();
    V3<T> bn = vzero<T>();
    {
        const T a = d.x * d.x + d.z * d.z;
        const T b = o.x * d.x + o.z * d.z;
        const T q = b / a;
        const T fa = o.x - d.x * q, fb = o.z - d.z * q;
        const T delta = a * (R * R - (fa * fa + fb * fb));
        const T t = (-b + sqrt_t(delta)) / a;
        const T y = o.y + d.y * t;
        if (a > T(0) && !(delta < T(0)) && fabs_t(y) <= h) {
            best = t;
            const T pa = o.x + d.x * t, pb = o.z + d.z * t;
            const T l = sqrt_t(pa * pa + pb * pb);
            bn = l > T(0) ? V3<T>{pa / l, T(0), pb / l} : vzero<T>();
        }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const V3<T> oc{o.x, e == 0 ? o.y + h : o.y - h, o.z};
        const T a = dot(d, d), b = dot(oc, d);
        const V3<T> f = oc - d * (b / a);
        const T delta = a * (R * R - dot(f, f));
        if (delta < T(0)) continue;
        const T t = (-b + sqrt_t(delta)) / a;
        if (t > best) {
            best = t;
            const V3<T> p = oc + d * t;
            const T l = length(p);
            bn = l > T(0) ? p / l : vzero<T>();
        }
    }
    if (!(best > -sp_inf<T>())) return false;
    t_out = best; n_out = bn;
    return true;
}
// The local ray (ol, dl) against the capsule collider: the entry by sp_capsule_ray with R = r_c; an origin inside answers distance 0 and no
// normal when solid, the exit otherwise.  nl: the outward surface normal in the capsule's frame, zero when there is none.
template <class T> __device__ __forceinline__ bool sp_capcol_ray(V3<T> he, V3<T> ol, V3<T> dl, bool solid, T& t, V3<T>& nl) {
    bool pen;
    if (!sp_capsule_ray<T>(ol, dl, he.y, he.x, t, nl, pen)) return false;
    if (pen && !solid && !sp_capsule_ray_exit<T>(ol, dl, he.y, he.x, t, nl)) return false;
    return true;
}
template <class T> __device__ __forceinline__ bool sp_capcol_point(V3<T> he, V3<T> pl) {
    V3<T> A, u;
    sp_capcol_core<T>(he.y, A, u);
    T s;
    return sp_seg_point<T>(A, u, pl, s) <= he.x * he.x;
}
// the ball's projection rule about the nearest core point pc: inside = d^2 <= r_c^2; a point on the core goes to pc + (0, r_c, 0)
template <class T> __device__ __forceinline__ void sp_capcol_project(V3<T> he, V3<T> pl, bool solid, V3<T>& proj, bool& inside) {
    V3<T> A, u;
    sp_capcol_core<T>(he.y, A, u);
    const T r = he.x;
    T s;
    const T d2 = sp_seg_point<T>(A, u, pl, s);
    const V3<T> pc = A + u * s;
    inside = d2 <= r * r;
    if (!(solid && inside)) proj = d2 == T(0) ? pc + V3<T>{T(0), r, T(0)} : pc + (pl - pc) * (r / sqrt_t(d2));
}
// Intersection of the query shape (shape2, he2, iso2) with the capsule collider.  A ball or a cuboid: sp_capsule_intersects with the roles
// exchanged (the collider is the capsule, posed in the query's frame).  CAPSULE (a capsule query): the two cores by sp_seg_seg in the collider's
// frame, the collider's as segment 1; d^2 <= (r_q + r_c)^2.
template <class T, bool CAPSULE>
__device__ __forceinline__ bool sp_capcol_intersects(uint32_t shape2, V3<T> he2, const Iso<T>& iso2, V3<T> he1, V3<T> pos1, Q4<T> rot1) {
    if (!CAPSULE) return sp_capsule_intersects<T>(he1.x, he1.y, iso_inv_mul(iso2, Iso<T>{rot1, pos1}), shape2, he2);
    const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
    V3<T> A1, u1, A2, u2, p1, p2;
    sp_capcol_core<T>(he1.y, A1, u1);
    sp_capsule_core<T>(q, he2.y, A2, u2);
    const T d2 = sp_seg_seg_d2<T>(A1, u1, A2, u2, p1, p2);
    const T rr = he2.x + he1.x;
    return d2 <= rr * rr;
}
// The cast of the query shape (shape2, he2, pose iso2) along d against the capsule collider (he1 = (r_c, h_c, .)).  A ball: its centre as a
// ray against the capsule grown by the ball's radius, in the collider's frame.  A cuboid: sp_newton_cast in the QUERY's frame, the collider's
// core moving by -d against the box.  CAPSULE: sp_newton_cast in the collider's frame on the two cores (sp_seg_seg), R = r_q + r_c.
// Same answer as sp_cast_exact: p1 / n1 the collider's, p2 the query's at the impact pose; everything zero when the shapes overlap at the start.
template <class T, bool CAPSULE>
__device__ __forceinline__ bool sp_capcol_cast_exact(uint32_t shape2, V3<T> he2, const Iso<T>& iso2, V3<T> d, T max_distance, V3<T> he1, V3<T> pos1, Q4<T> rot1,
                                                     T& toi, V3<T>& p1, V3<T>& p2, V3<T>& n1) {
    const T rc = he1.x, hc = he1.y;
    T t = T(0);
    bool pen = false;
    V3<T> w1 = vzero<T>(), w2 = vzero<T>(), wn = vzero<T>();
    if (CAPSULE) {
        const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
        const V3<T> dl = na_qrot(qinverse(rot1), d);
        V3<T> A1, u1, A2, u2;
        sp_capcol_core<T>(hc, A1, u1);
        sp_capsule_core<T>(q, he2.y, A2, u2);
        V3<T> n, pq, pc;
        const bool hit = sp_newton_cast<T>([&](T tt, V3<T>& a, V3<T>& b) { return sp_seg_seg_d2<T>(A1, u1, A2 + dl * tt, u2, b, a); }, dl, he2.x + rc, max_distance, t, n, pq, pc, pen);
        if (!hit || !(t <= max_distance) || !finite_t(t)) return false;
        if (!pen) {
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, pc + n * rc) + pos1;
            w2 = na_qrot(rot1, pq - n * he2.x) + pos1;
        }
    } else if (shape2 == AVN_SHAPE_BALL) {
        const Iso<T> q = iso_inv_mul(Iso<T>{rot1, pos1}, iso2);
        const V3<T> dl = na_qrot(qinverse(rot1), d);
        V3<T> n;
        if (!sp_capsule_ray<T>(q.t, dl, hc, rc + he2.x, t, n, pen)) return false;
        if (!(t <= max_distance) || !finite_t(t)) return false;
        if (!pen) {
            const V3<T> c2 = iso2.t + d * t;
            const V3<T> pb = q.t + dl * t;   // the ball's centre at the impact, in the collider's frame
            const T ys = pb.y < -hc ? -hc : (pb.y > hc ? hc : pb.y);
            const V3<T> pk = V3<T>{T(0), ys, T(0)} + n * rc;
            wn = na_qrot(rot1, n);
            w1 = na_qrot(rot1, pk) + pos1;
            w2 = c2 + (-wn) * he2.x;
        }
    } else {
        const Iso<T> qc = iso_inv_mul(iso2, Iso<T>{rot1, pos1});   // the collider in the query's frame
        const V3<T> dm = -iso_inv_vec(iso2, d);
        V3<T> A, u;
        sp_capsule_core<T>(qc, hc, A, u);
        V3<T> n, ps, pb;
        const bool hit = sp_newton_cast<T>([&](T tt, V3<T>& a, V3<T>& b) { const SegBox<T> sb = sp_seg_box<T>(A + dm * tt, u, he2); a = sb.ps; b = sb.pb; return sb.f; },
                                           dm, rc, max_distance, t, n, ps, pb, pen);
        if (!hit || !(t <= max_distance) || !finite_t(t)) return false;
        if (!pen) {
            const V3<T> c2 = iso2.t + d * t;
            wn = -na_qrot(iso2.r, n);
            w1 = na_qrot(iso2.r, ps - n * rc) + c2;
            w2 = na_qrot(iso2.r, pb) + c2;
        }
    }
    toi = t; p1 = w1; p2 = w2; n1 = wn;
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// swept CCD, SweepMode::NonLinear (include/avian_mi355x_ccd.h, N2): the gap of a Ball / Cuboid pair at the given poses and the unit axis n
// (world, from collider 1 towards 2) along which it was measured.  The rotations are used as they are (no make_isometry).  Ball pairs: the
// distance.  Cuboid - cuboid: the largest SAT separation with the narrow phase's choice among the three sweeps, a lower bound of the distance
// that is positive exactly when the boxes are disjoint.
template <class T>
__device__ __forceinline__ T sp_nl_gap(uint32_t shape1, V3<T> he1, V3<T> p1, Q4<T> q1, uint32_t shape2, V3<T> he2, V3<T> p2, Q4<T> q2, V3<T>& n) {
    const bool ball1 = shape1 == AVN_SHAPE_BALL, ball2 = shape2 == AVN_SHAPE_BALL;
    if (ball1 && ball2) {
        const V3<T> dv = p2 - p1;
        const T dist = length(dv);
        n = dist > T(0) ? dv / dist : V3<T>{T(0), T(1), T(0)};
        return dist - (he1.x + he2.x);
    }
    if (ball1 || ball2) {
        const V3<T> pc = ball1 ? p2 : p1, pb = ball1 ? p1 : p2, he = ball1 ? he2 : he1;
        const Q4<T> qc = ball1 ? q2 : q1;
        const T r = ball1 ? he1.x : he2.x;
        const V3<T> l = qrot(qinverse(qc), pb - pc);   // the ball's centre in the cuboid's frame
        const V3<T> df = l - sp_clamp3(l, he);
        const T dist = length(df);
        V3<T> nl;
        T g;
        if (dist > T(0)) { nl = df / dist; g = dist - r; }
        else {   // the centre is inside: the nearest face (the lowest axis among equals)
            T m = he.x - fabs_t(l.x);
            int axis = 0;
            const T my = he.y - fabs_t(l.y), mz = he.z - fabs_t(l.z);
            if (my < m) { m = my; axis = 1; }
            if (mz < m) { m = mz; axis = 2; }
            nl = sp_unit<T>(axis, copysign_t(T(1), sp_vget(l, axis)));
            g = -r;
        }
        const V3<T> nw = qrot(qc, nl);
        n = ball1 ? -nw : nw;
        return g;
    }
    const Iso<T> pos12 = iso_inv_mul(Iso<T>{q1, p1}, Iso<T>{q2, p2});
    const Iso<T> pos21 = iso_inverse(pos12);
    V3<T> d1, d2, d3;
    const T sep1 = sat_normal_oneway(he1, he2, pos12, d1);
    const T sep2 = sat_normal_oneway(he2, he1, pos21, d2);
    const T sep3 = sat_edge_twoway(he1, he2, pos12, d3);
    V3<T> best = d1;
    T g = sep1;
    if (sep2 > sep1 && sep2 > sep3) { best = iso_vec(pos12, -d2); g = sep2; }
    else if (sep3 > sep1) { best = d3; g = sep3; }
    n = na_qrot(q1, best);
    return g;
}

// N2 with Capsule colliders (avn_swept_ccd_capsules_set; the _cap kernels of k_ccd.hip only, so that no instantiation of sp_nl_gap changes): the
// exact distance of the cores minus the radii.  A capsule's he = (r, h, .).  capsule - ball in the capsule's frame by sp_seg_point; capsule -
// capsule in collider 1's frame by sp_seg_seg_d2 with collider 1's core as segment 1; capsule - cuboid in the cuboid's frame by sp_seg_box.
// !(dist > 0): g as computed (minus the radius or radii), n = (0, 1, 0).  A pair without a capsule (the small ball of N4 against a Ball /
// Cuboid collider 1; never two cuboids) goes to sp_nl_gap.
template <class T>
__device__ __forceinline__ T sp_nl_gap_cap(uint32_t shape1, V3<T> he1, V3<T> p1, Q4<T> q1, uint32_t shape2, V3<T> he2, V3<T> p2, Q4<T> q2, V3<T>& n) {
    const bool cap1 = shape1 == AVN_SHAPE_CAPSULE, cap2 = shape2 == AVN_SHAPE_CAPSULE;
    const V3<T> up{T(0), T(1), T(0)};
    if (cap1 && cap2) {
        const Iso<T> pos12 = iso_inv_mul(Iso<T>{q1, p1}, Iso<T>{q2, p2});
        V3<T> A1, u1, A2, u2, pa, pb;
        sp_capcol_core<T>(he1.y, A1, u1);
        sp_capsule_core<T>(pos12, he2.y, A2, u2);
        const T dist = sqrt_t(sp_seg_seg_d2<T>(A1, u1, A2, u2, pa, pb));
        n = dist > T(0) ? na_qrot(q1, (pb - pa) / dist) : up;
        return dist - (he1.x + he2.x);
    }
    if (cap1 || cap2) {
        const V3<T> pc = cap1 ? p1 : p2, po = cap1 ? p2 : p1, hc = cap1 ? he1 : he2, ho = cap1 ? he2 : he1;
        const Q4<T> qc = cap1 ? q1 : q2, qo = cap1 ? q2 : q1;
        if ((cap1 ? shape2 : shape1) == AVN_SHAPE_BALL) {
            const V3<T> l = qrot(qinverse(qc), po - pc);   // the ball's centre in the capsule's frame
            V3<T> A, u;
            sp_capcol_core<T>(hc.y, A, u);
            T s;
            (void)sp_seg_point<T>(A, u, l, s);
            const V3<T> df = l - (A + u * s);
            const T dist = length(df);
            const V3<T> nw = qrot(qc, df / dist);             // from the capsule towards the ball
            n = dist > T(0) ? (cap1 ? nw : -nw) : up;
            return dist - (hc.x + ho.x);
        }
        const Iso<T> pos = iso_inv_mul(Iso<T>{qo, po}, Iso<T>{qc, pc});   // the capsule in the cuboid's frame
        V3<T> A, u;
        sp_capsule_core<T>(pos, hc.y, A, u);
        const SegBox<T> sb = sp_seg_box<T>(A, u, ho);
        const T dist = sqrt_t(sb.f);
        const V3<T> nw = qrot(qo, (sb.ps - sb.pb) / dist);   // from the box towards the capsule
        n = dist > T(0) ? (cap1 ? -nw : nw) : up;
        return dist - hc.x;
    }
    // (no caller brings two cuboids: said here so that the SAT sweeps stay out of the _cap kernels)
    if (shape1 == AVN_SHAPE_BALL || shape2 == AVN_SHAPE_BALL) return sp_nl_gap<T>(shape1, he1, p1, q1, shape2, he2, p2, q2, n);
    n = up;
    return sp_inf<T>();
}

}  // namespace avn
