// avn_triangle_pair.h — the contact manifolds of a Triangle COLLIDER (AVN_SHAPE_TRIANGLE, include/avian_mi355x_trimesh.h) against a Ball, a
// Capsule or a Cuboid, in either order.  parry is not vendored: the header defines these manifolds with their operation order (no FMA
// contraction), parity with parry is UNPINNED; tests/triangle_collider_reference.py does the same operations in order and this file follows it
// function for function (closest_point, _tri_ball, _tri_capsule, _box_axis, _support_region, _face_axis_admissible, _clip, _tri_cuboid).
// Only contact_manifolds_pair_sink<.., TRI = true> reaches this file: the narrow phase's general (HS) heavy kernel of a world that holds a
// triangle and the batch query avn_triangle_manifolds.  It also compiles as plain host C++ (tests/triangle_pair_main.cpp runs it under the
// host sanitizers).
//
// Storage: nothing here is an array indexed by a run-time value.  The clip polygon (TriPoly: at most TRI_POLY_MAX = 8 corners, the
// reference's `len(out) < 8` cap, which is part of the definition) is read by compile-time indices in unrolled loops and WRITTEN through a
// select chain over its eight slots (tri_poly_append): an index outside 0 .. 7 cannot be formed, there is no address to get wrong, and the
// corners stay in registers (no scratch, no LDS beside the kernel's s_pts).  Triangle vertices, box face corners and their ids are picked by
// select chains in the same way (tri_pick3 / tri_pick4).
#pragma once
#include "avn_spatial_pair.h"   // sp_seg_seg (ONE segment - segment routine), sp_vget, cp_set's neighbours

namespace avn {

#define TRI_POLY_MAX 8
static_assert(TRI_POLY_MAX <= AVN_NP_MAX_RAW, "the raw points of a triangle manifold (one per corner of the clipped polygon) fit a manifold's raw-point storage");

template <class T> __device__ __forceinline__ V3<T> tri_pick3(V3<T> a, V3<T> b, V3<T> c, int k) { return k == 0 ? a : (k == 1 ? b : c); }
__device__ __forceinline__ uint32_t tri_pick4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t k) { return k == 0u ? a : (k == 1u ? b : (k == 2u ? c : d)); }
template <class T> __device__ __forceinline__ V3<T> tri_axis(int i, T s) { return V3<T>{i == 0 ? s : T(0), i == 1 ? s : T(0), i == 2 ? s : T(0)}; }
template <class T> __device__ __forceinline__ V3<T> tri_set(V3<T> v, int i, T x) { return V3<T>{i == 0 ? x : v.x, i == 1 ? x : v.y, i == 2 ? x : v.z}; }

// region 0: the face, 1 + k: edge k of (ab, bc, ca), 4 + k: vertex k
__device__ __forceinline__ uint32_t tri_fid(int region) { return region >= 4 ? fid_vertex((uint32_t)(region - 4)) : (region >= 1 ? fid_edge((uint32_t)(region - 1)) : fid_face(0u)); }
// the interior-edge rule: an edge whose flag is clear, a vertex both of whose edges have theirs clear
__device__ __forceinline__ bool tri_interior(uint32_t flags, int region) {
    if (region >= 4) { const int k = region - 4; return !(flags & (1u << k)) && !(flags & (1u << ((k + 2) % 3))); }
    if (region >= 1) return !(flags & (1u << (region - 1)));
    return false;
}
template <class T> __device__ __forceinline__ V3<T> tri_unit_normal(V3<T> a, V3<T> b, V3<T> c) {
    const V3<T> nrm = na_cross(b - a, c - a);
    return nrm / na_norm(nrm);
}
// Ericson 5.1.5 in its order of tests
template <class T> __device__ __forceinline__ V3<T> tri_closest_point(V3<T> a, V3<T> b, V3<T> c, V3<T> p, int& region) {
    const V3<T> ab = b - a, ac = c - a, ap = p - a;
    const T d1 = na_dot(ab, ap), d2 = na_dot(ac, ap);
    if (d1 <= T(0) && d2 <= T(0)) { region = 4; return a; }
    const V3<T> bp = p - b;
    const T d3 = na_dot(ab, bp), d4 = na_dot(ac, bp);
    if (d3 >= T(0) && d4 <= d3) { region = 5; return b; }
    const T vc = d1 * d4 - d3 * d2;
    if (vc <= T(0) && d1 >= T(0) && d3 <= T(0)) { region = 1; return a + ab * (d1 / (d1 - d3)); }
    const V3<T> cp = p - c;
    const T d5 = na_dot(ab, cp), d6 = na_dot(ac, cp);
    if (d6 >= T(0) && d5 <= d6) { region = 6; return c; }
    const T vb = d5 * d2 - d1 * d6;
    if (vb <= T(0) && d2 >= T(0) && d6 <= T(0)) { region = 3; return a + ac * (d2 / (d2 - d6)); }
    const T va = d3 * d6 - d5 * d4;
    if (va <= T(0) && (d4 - d3) >= T(0) && (d5 - d6) >= T(0)) { region = 2; return b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6))); }
    const V3<T> nrm = na_cross(ab, ac);
    const V3<T> N = nrm / na_norm(nrm);
    region = 0;
    return p - N * na_dot(N, ap);
}

// ---- triangle / ball: p = the ball in the triangle's frame -------------------------------------------------------------------------------
template <class T, class Em>
__device__ __forceinline__ bool tri_ball(V3<T> a, V3<T> b, V3<T> c, uint32_t flags, bool flipped, T r, const Iso<T>& p, T pred, Em& em) {
    int region;
    const V3<T> q = tri_closest_point<T>(a, b, c, p.t, region);
    const V3<T> d = p.t - q;
    const T dist = na_norm(d);
    if (!(dist > T(0)) || !(dist <= r + pred)) return false;
    V3<T> n = d / dist;
    T sd = dist - r;
    if (tri_interior(flags, region)) {
        const V3<T> N = tri_unit_normal<T>(a, b, c);
        n = na_dot(N, d) < T(0) ? -N : N;
        sd = na_dot(d, n) - r;
    }
    if (flipped) {
        const V3<T> n_ball = iso_inv_vec(p, -n);
        if (!np_world_normal(em.rotation1, n_ball, em.normal)) return false;
        em.push(n_ball * r, sd, fid_face(0u), tri_fid(region));
    } else {
        if (!np_world_normal(em.rotation1, n, em.normal)) return false;
        em.push(q, sd, tri_fid(region), fid_face(0u));
    }
    return true;
}

// ---- triangle / capsule: p = the capsule in the triangle's frame -------------------------------------------------------------------------
template <class T> struct TriBest { T d2; V3<T> ps, pt; int region; };
template <class T> __device__ __forceinline__ void tri_attempt(TriBest<T>& best, V3<T> ps, V3<T> pt, int region) {
    const V3<T> d = ps - pt;
    const T d2 = na_dot(d, d);
    if (d2 < best.d2) { best.d2 = d2; best.ps = ps; best.pt = pt; best.region = region; }
}
// The closest points of the segment A + s u, s in [0, 1], and the triangle when the segment does not cross the face: the first smallest of five
// candidate pairs -- the two ends against the triangle (tri_closest_point), then the segment against edge k = 0, 1, 2 (sp_seg_seg).  ONE routine for the
// narrow phase (tri_capsule) and the spatial queries (sp_seg_tri_d2, avn_spatial_triangle_pair.h).
template <class T> __device__ __forceinline__ TriBest<T> tri_seg_closest(V3<T> a, V3<T> b, V3<T> c, V3<T> A, V3<T> u) {
    const V3<T> B = A + u;
    TriBest<T> best{sp_inf<T>(), A, a, 4};
    {
        int rg;
        const V3<T> q0 = tri_closest_point<T>(a, b, c, A, rg);
        tri_attempt<T>(best, A, q0, rg);
        const V3<T> q1 = tri_closest_point<T>(a, b, c, B, rg);
        tri_attempt<T>(best, B, q1, rg);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const V3<T> vk = k == 0 ? a : (k == 1 ? b : c), vn = k == 0 ? b : (k == 1 ? c : a);
        const V3<T> ek = vn - vk;
        const SegSeg<T> ss = sp_seg_seg<T>(A, u, vk, ek);
        tri_attempt<T>(best, A + u * ss.s, vk + ek * ss.t, ss.t == T(0) ? 4 + k : (ss.t == T(1) ? 4 + (k + 1) % 3 : 1 + k));
    }
    return best;
}
template <class T, class Em>
__device__ __forceinline__ bool tri_capsule(V3<T> a, V3<T> b, V3<T> c, uint32_t flags, bool flipped, T r, T h, const Iso<T>& p, T pred, Em& em) {
    const V3<T> hv = na_qrot(p.r, V3<T>{T(0), h, T(0)});
    const V3<T> A = p.t - hv, u = hv * T(2);
    const V3<T> B = A + u;
    const V3<T> N = tri_unit_normal<T>(a, b, c);
    const T da = na_dot(N, A - a), db = na_dot(N, B - a);
    if ((da > T(0) && db < T(0)) || (da < T(0) && db > T(0))) {
        int rg;
        (void)tri_closest_point<T>(a, b, c, A + u * (da / (da - db)), rg);
        if (rg == 0) {   // the core crosses the face: the deeper end against the face's plane
            const V3<T> mid = A + u * T(0.5);
            const V3<T> n = na_dot(N, mid - a) < T(0) ? -N : N;
            const V3<T> pd = na_dot(n, u) < T(0) ? B : A;
            const T dd = na_dot(n, pd - a);
            if (flipped) {
                if (!np_world_normal(em.rotation1, iso_inv_vec(p, -n), em.normal)) return false;
                em.push(iso_inv_point(p, pd - n * r), dd - r, fid_face(0u), fid_face(0u));
            } else {
                if (!np_world_normal(em.rotation1, n, em.normal)) return false;
                em.push(pd - n * dd, dd - r, fid_face(0u), fid_face(0u));
            }
            return true;
        }
    }
    const TriBest<T> best = tri_seg_closest<T>(a, b, c, A, u);
    const T dist = sqrt_t(best.d2);
    if (!(dist > T(0)) || !(dist <= r + pred)) return false;
    const V3<T> d = best.ps - best.pt;
    V3<T> n = d / dist;
    T sd = dist - r;
    const bool face = best.region == 0;
    if (face || tri_interior(flags, best.region)) {
        n = na_dot(N, d) < T(0) ? -N : N;
        sd = na_dot(d, n) - r;
    }
    if (!np_world_normal(em.rotation1, flipped ? iso_inv_vec(p, -n) : n, em.normal)) return false;
    if (face && na_dot(u, u) > T(0)) {
        // the core clipped to the prism over the face: an interval [lo, hi] with lo < hi gives two points
        T lo = T(0), hi = T(1);
        bool empty = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const V3<T> vk = k == 0 ? a : (k == 1 ? b : c), vn = k == 0 ? b : (k == 1 ? c : a);
            const V3<T> m = na_cross(N, vn - vk);
            const T g0 = na_dot(m, A - vk), gu = na_dot(m, u);
            if (gu != T(0)) {
                const T tk = -g0 / gu;
                if (gu > T(0)) { if (tk > lo) lo = tk; }
                else if (tk < hi) hi = tk;
            } else if (g0 < T(0)) empty = true;
        }
        if (!empty && lo < hi) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const V3<T> x = A + u * (k == 0 ? lo : hi);
                const T dcore = na_dot(n, x - a);
                if (!(dcore <= r + pred)) continue;
                if (flipped) em.push(iso_inv_point(p, x - n * r), dcore - r, fid_vertex((uint32_t)k), fid_face(0u));
                else em.push(x - n * dcore, dcore - r, fid_face(0u), fid_vertex((uint32_t)k));
            }
            return true;
        }
    }
    if (flipped) em.push(iso_inv_point(p, best.ps - n * r), sd, fid_face(0u), tri_fid(best.region));
    else em.push(best.pt, sd, tri_fid(best.region), fid_face(0u));
    return true;
}

// ---- triangle / cuboid, in the cuboid's frame: q = the triangle's pose there ---------------------------------------------------------------
// the separation along the unit axis L; d = +-L from the box towards the triangle
template <class T> __device__ __forceinline__ T tri_box_axis(V3<T> he, V3<T> v0, V3<T> v1, V3<T> v2, V3<T> L, V3<T>& d) {
    const T p0 = na_dot(L, v0), p1 = na_dot(L, v1), p2 = na_dot(L, v2);
    T tmin = p0 < p1 ? p0 : p1, tmax = p0 < p1 ? p1 : p0;
    tmin = p2 < tmin ? p2 : tmin;
    tmax = p2 > tmax ? p2 : tmax;
    const T rb = (fabs_t(L.x) * he.x + fabs_t(L.y) * he.y) + fabs_t(L.z) * he.z;
    const T sp = tmin - rb, sm = -tmax - rb;
    if (sp >= sm) { d = L; return sp; }
    d = -L;
    return sm;
}
template <class T> __device__ __forceinline__ int tri_support_region(V3<T> v0, V3<T> v1, V3<T> v2, V3<T> d) {
    const T p0 = na_dot(d, v0), p1 = na_dot(d, v1), p2 = na_dot(d, v2);
    T m = p0 < p1 ? p0 : p1;
    m = p2 < m ? p2 : m;
    const bool e0 = p0 == m, e1 = p1 == m, e2 = p2 == m;
    if (e0 && e1 && e2) return 0;
    if (e0 && e1) return 1;
    if (e1 && e2) return 2;
    if (e2 && e0) return 3;
    return e0 ? 4 : (e1 ? 5 : 6);
}
// |x_j| <= he_j on the two axes other than i
template <class T> __device__ __forceinline__ bool tri_over_face(V3<T> x, V3<T> he, int i) {
    return (i == 0 || fabs_t(x.x) <= he.x) && (i == 1 || fabs_t(x.y) <= he.y) && (i == 2 || fabs_t(x.z) <= he.z);
}
template <class T> __device__ __forceinline__ bool tri_face_axis_admissible(uint32_t flags, V3<T> v0, V3<T> v1, V3<T> v2, V3<T> d, int i, V3<T> he) {
    const int region = tri_support_region<T>(v0, v1, v2, d);
    if (region == 0) return true;
    if (tri_interior(flags, region)) return false;
    if (region < 4) return tri_over_face<T>(tri_pick3<T>(v0, v1, v2, region - 1), he, i) || tri_over_face<T>(tri_pick3<T>(v0, v1, v2, region % 3), he, i);
    return tri_over_face<T>(tri_pick3<T>(v0, v1, v2, region - 4), he, i);
}

// The clip polygon: corner k = (point, raw id | tag of the edge that leaves it << 16).  n <= TRI_POLY_MAX always: tri_poly_append is the only writer.
template <class T> struct TriPoly { V3<T> p[TRI_POLY_MAX]; uint32_t it[TRI_POLY_MAX]; int n; };
template <class T> __device__ __forceinline__ void tri_poly_append(TriPoly<T>& o, V3<T> P, uint32_t pid, uint32_t tag) {
    if (o.n >= TRI_POLY_MAX) return;   // the reference's `len(out) < 8`
#pragma unroll
    for (int k = 0; k < TRI_POLY_MAX; ++k) {   // (selects on values, slot by slot: nothing the compiler could turn into an indexed store)
        const bool here = k == o.n;
        o.p[k].x = here ? P.x : o.p[k].x; o.p[k].y = here ? P.y : o.p[k].y; o.p[k].z = here ? P.z : o.p[k].z;
        o.it[k] = here ? (pid | (tag << 16)) : o.it[k];
    }
    ++o.n;
}
// Sutherland - Hodgman, one plane: keeps dot(m, x) + c >= 0
template <class T> __device__ __forceinline__ void tri_clip(const TriPoly<T>& in, V3<T> m, T c, uint32_t plane, TriPoly<T>& out) {
    out.n = 0;
#pragma unroll
    for (int k = 0; k < TRI_POLY_MAX; ++k) { out.p[k] = vzero<T>(); out.it[k] = 0u; }
#pragma unroll
    for (int i = 0; i < TRI_POLY_MAX; ++i) {
        if (i < in.n) {
            const V3<T> P = in.p[i];
            const uint32_t pid = in.it[i] & 0xFFFFu, tag = in.it[i] >> 16;
            const V3<T> Q = (i + 1 < TRI_POLY_MAX && i + 1 < in.n) ? in.p[(i + 1) % TRI_POLY_MAX] : in.p[0];
            const T gp = na_dot(m, P) + c, gq = na_dot(m, Q) + c;
            const bool pin = gp >= T(0), qin = gq >= T(0);
            if (pin) tri_poly_append<T>(out, P, pid, tag);
            if (pin != qin) {
                const V3<T> X = P + (Q - P) * (gp / (gp - gq));
                tri_poly_append<T>(out, X, tag < 4u ? ((1u << 8) | (tag << 4) | plane) : ((2u << 8) | ((tag - 4u) << 4) | plane), pin ? 4u + plane : tag);
            }
        }
    }
}

template <class T, class Em>
__device__ __forceinline__ bool tri_cuboid(V3<T> ta, V3<T> tb, V3<T> tc, uint32_t flags, bool flipped, V3<T> he, const Iso<T>& q, T pred, Em& em) {
    const V3<T> v0 = iso_point(q, ta), v1 = iso_point(q, tb), v2 = iso_point(q, tc);
    const V3<T> N = tri_unit_normal<T>(v0, v1, v2);
    T best = -Limits<T>::max;
    V3<T> bd = vzero<T>();
    int kind = 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        V3<T> d;
        const T sep = tri_box_axis<T>(he, v0, v1, v2, tri_axis<T>(i, T(1)), d);
        if (sep > pred) return false;
        if (tri_face_axis_admissible<T>(flags, v0, v1, v2, d, i, he) && sep > best) { best = sep; bd = d; kind = i; }
    }
    {
        V3<T> d;
        const T sep = tri_box_axis<T>(he, v0, v1, v2, N, d);
        if (sep > pred) return false;
        if (sep > best) { best = sep; bd = d; kind = 3; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const V3<T> vk = k == 0 ? v0 : (k == 1 ? v1 : v2), vn = k == 0 ? v1 : (k == 1 ? v2 : v0), vo = k == 0 ? v2 : (k == 1 ? v0 : v1);
        const V3<T> ek = vn - vk;
        const T el = na_norm(ek);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const V3<T> cx = i == 0 ? V3<T>{T(0), -ek.z, ek.y} : (i == 1 ? V3<T>{ek.z, T(0), -ek.x} : V3<T>{-ek.y, ek.x, T(0)});
            const T nl = na_norm(cx);
            if (!(nl > Limits<T>::eps * el)) continue;
            V3<T> d;
            const T sep = tri_box_axis<T>(he, v0, v1, v2, cx / nl, d);
            if (sep > pred) return false;
            // (a flagged edge gives the direction only where the edge itself is the triangle's lowest feature along it)
            if ((flags & (1u << k)) && !(na_dot(d, vo) < na_dot(d, vk)) && sep > best) { best = sep; bd = d; kind = 4 + 3 * k + i; }
        }
    }
    if (!np_world_normal(em.rotation1, flipped ? bd : iso_inv_vec(q, -bd), em.normal)) return false;
    if (kind >= 4) {   // an edge of the triangle against an edge of the box: the closest points of the two segments
        const int k = (kind - 4) / 3, i = (kind - 4) % 3;
        const V3<T> vk = tri_pick3<T>(v0, v1, v2, k);
        const V3<T> ek = tri_pick3<T>(v1, v2, v0, k) - vk;
        const V3<T> sp = cuboid_support_point(he, bd);
        const T hi_ = sp_vget(he, i);
        const V3<T> A1 = tri_set<T>(sp, i, -hi_);
        const V3<T> u1 = tri_axis<T>(i, hi_ * T(2));
        const SegSeg<T> ss = sp_seg_seg<T>(A1, u1, vk, ek);
        const V3<T> pb = A1 + u1 * ss.s, pt = vk + ek * ss.t;
        const T dist = na_dot(pt - pb, bd);
        const uint32_t fidt = fid_edge((uint32_t)k);
        const uint32_t lo = ((i != 0 && sp.x < T(0)) ? 1u : 0u) | ((i != 1 && sp.y < T(0)) ? 2u : 0u) | ((i != 2 && sp.z < T(0)) ? 4u : 0u);
        const uint32_t fidb = fid_edge(((lo | (1u << i)) << 3) | lo | 0xC0u);
        if (flipped) em.push(pb, dist, fidb, fidt);
        else em.push(iso_inv_point(q, pt), dist, fidt, fidb);
        return true;
    }
    TriPoly<T> pa, pb;
#pragma unroll
    for (int k = 0; k < TRI_POLY_MAX; ++k) { pa.p[k] = vzero<T>(); pa.it[k] = 0u; }
    if (kind < 3) {   // a face of the box is the reference: the triangle clipped to the face's four side planes
        const int i = kind;
        const T sg = sp_vget(bd, i) > T(0) ? T(1) : T(-1);
        pa.p[0] = v0; pa.p[1] = v1; pa.p[2] = v2;
        pa.it[0] = 0u | (0u << 16); pa.it[1] = 1u | (1u << 16); pa.it[2] = 2u | (2u << 16);
        pa.n = 3;
        const int j0 = i == 0 ? 1 : 0, j1 = i == 2 ? 1 : 2;   // the two other axes, ascending
        tri_clip<T>(pa, tri_axis<T>(j0, T(-1)), sp_vget(he, j0), 0u, pb);
        tri_clip<T>(pb, tri_axis<T>(j0, T(1)), sp_vget(he, j0), 1u, pa);
        tri_clip<T>(pa, tri_axis<T>(j1, T(-1)), sp_vget(he, j1), 2u, pb);
        tri_clip<T>(pb, tri_axis<T>(j1, T(1)), sp_vget(he, j1), 3u, pa);
        const T hf = sp_vget(he, i);
        const uint32_t fidb = fid_face((uint32_t)i + (sg > T(0) ? 3u : 0u) + 10u);
#pragma unroll
        for (int k = 0; k < TRI_POLY_MAX; ++k) {
            if (k < pa.n) {
                const V3<T> x = pa.p[k];
                const uint32_t pid = pa.it[k] & 0xFFFFu;
                const T dist = sg * sp_vget(x, i) - hf;
                if (dist <= pred) {
                    const uint32_t ka = (pid >> 4) & 15u, kb = pid & 15u;
                    const uint32_t fidt = (pid >> 8) == 0u ? fid_vertex(kb) : ((pid >> 8) == 1u ? fid_edge(ka | ((kb + 1u) << 2)) : fid_face(16u + ka * 4u + kb));
                    if (flipped) em.push(tri_set<T>(x, i, sg * hf), dist, fidb, fidt);
                    else em.push(iso_inv_point(q, x), dist, fidt, fidb);
                }
            }
        }
        return true;
    }
    // the triangle's face is the reference: the box's support face clipped to the prism over the triangle
    Face<T> f;
    cuboid_support_face(he, bd, f);
    pa.p[0] = f.v[0]; pa.p[1] = f.v[1]; pa.p[2] = f.v[2]; pa.p[3] = f.v[3];
    pa.it[0] = 0u | (0u << 16); pa.it[1] = 1u | (1u << 16); pa.it[2] = 2u | (2u << 16); pa.it[3] = 3u | (3u << 16);
    pa.n = 4;
    {
        const V3<T> m0 = na_cross(N, v1 - v0), m1 = na_cross(N, v2 - v1), m2 = na_cross(N, v0 - v2);
        tri_clip<T>(pa, m0, -na_dot(m0, v0), 0u, pb);
        tri_clip<T>(pb, m1, -na_dot(m1, v1), 1u, pa);
        tri_clip<T>(pa, m2, -na_dot(m2, v2), 2u, pb);
    }
#pragma unroll
    for (int k = 0; k < TRI_POLY_MAX; ++k) {
        if (k < pb.n) {
            const V3<T> x = pb.p[k];
            const uint32_t pid = pb.it[k] & 0xFFFFu;
            const T dist = na_dot(bd, v0 - x);
            if (dist <= pred) {
                const uint32_t ka = (pid >> 4) & 15u, kb = pid & 15u;
                const uint32_t fidb = (pid >> 8) == 0u ? tri_pick4(f.vid[0], f.vid[1], f.vid[2], f.vid[3], kb & 3u)
                                    : ((pid >> 8) == 1u ? (tri_pick4(f.eid[0], f.eid[1], f.eid[2], f.eid[3], ka & 3u) | ((kb + 1u) << 8)) : (f.fid | ((1u + ka * 3u + kb) << 8)));
                if (flipped) em.push(x, dist, fidb, fid_face(0u));
                else em.push(iso_inv_point(q, x + bd * dist), dist, fid_face(0u), fidb);
            }
        }
    }
    return true;
}

// pos12: shape 2 in shape 1's frame (of the two make_isometry poses); em.rotation1 / em.sink are set; tri: the triangle of whichever shape is
// AVN_SHAPE_TRIANGLE.  Sets em.normal and pushes the points; false = no manifold (the caller also drops a manifold without points).
// Two triangles, and a triangle against anything but a Ball, a Capsule or a Cuboid: no manifold.
template <class T, class Em>
__device__ __forceinline__ bool triangle_pair_manifold(uint32_t shape1, V3<T> he1, uint32_t shape2, V3<T> he2, const Iso<T>& pos12, T prediction, const NpTri<T>& tri, Em& em) {
    const bool tri1 = shape1 == AVN_SHAPE_TRIANGLE, tri2 = shape2 == AVN_SHAPE_TRIANGLE;
    if (tri1 && tri2) return false;   // (not built: it cannot arise for meshes on static bodies)
    const bool flipped = !tri1;   // the triangle is shape 2
    const uint32_t other = flipped ? shape1 : shape2;
    const V3<T> heo = flipped ? he1 : he2;
    if (other == AVN_SHAPE_CUBOID) return tri_cuboid<T, Em>(tri.a, tri.b, tri.c, tri.flags, flipped, heo, flipped ? pos12 : iso_inverse(pos12), prediction, em);
    const Iso<T> p = flipped ? iso_inverse(pos12) : pos12;   // the other shape in the triangle's frame
    if (other == AVN_SHAPE_BALL) return tri_ball<T, Em>(tri.a, tri.b, tri.c, tri.flags, flipped, heo.x, p, prediction, em);
    if (other == AVN_SHAPE_CAPSULE) return tri_capsule<T, Em>(tri.a, tri.b, tri.c, tri.flags, flipped, heo.x, heo.y, p, prediction, em);
    return false;
}

}  // namespace avn
