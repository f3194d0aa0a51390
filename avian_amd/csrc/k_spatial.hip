// k_spatial.hip — spatial queries on the device (include/avian_mi355x_spatial.h): an LBVH over the collider table and one-lane-per-query
// traversals for ray casts, ray hits, point and AABB intersections (k_sp_query), point projection (k_sp_project), shape intersections
// (k_sp_shapes), shape casts (k_sp_cast), shape contacts (k_sp_contacts), the depenetration over them (k_sp_depenetrate), velocity
// projection (k_sp_project_velocity), cast_move (k_sp_cast_move), the phases of the move-and-slide loop (k_sp_slide), and the casters: their
// re-aiming (k_sp_reaim) and the per-caster filter of k_sp_query / k_sp_cast (PQ).  The kernels that take a query shape have a second,
// CAPSULE instantiation for AVN_SHAPE_CAPSULE queries, launched behind the first (sp_lane_kind, sp_next_chunk).  The kernels
// that reach a collider's geometry have a CCAP instantiation each, whose leaf tests know the capsule COLLIDER: the host launches it when the
// world's switch is on and the snapshot holds a capsule collider, and the ones it always has otherwise.  Likewise a CTRI
// instantiation each for the triangle COLLIDER (avn_spatial_triangle_colliders_set): its first argument carries the world's triangle
// table, which the leaf reads by value where a candidate's shape is AVN_SHAPE_TRIANGLE; a CTRI launch always takes CCAP as well.
//
// avn_spatial_update (launch_spatial_build), all on the world's stream:
//   1. k_sp_snapshot   one thread per collider: its pose (collider_pose), the exact shape AABB (shape_aabb), padded, as the leaf box;
//                      integer atomics of order-preserving keys give the bounds of the box centres (deterministic, no float atomics)
//   2. k_sp_morton     30-bit Morton code of the box centre in those bounds
//   3. the hand-written stable radix sort of the codes with the collider index as value: the order of the unique 64-bit keys
//      (Morton << 32 | collider index), so the tree is the same run to run
//   4. k_sp_karras     the Karras (2012) hierarchy over the sorted keys: children and parents of every internal node
//   5. k_sp_refit      one thread per leaf walks to the root; per internal node the SECOND arriving thread unions the two child boxes
//                      (exact min / max) -- the hand-over between workgroups is an agent-scope release before the arrival counter's
//                      atomic and an agent-scope acquire after it (L1 is per CU, L2 per XCD): never co-location
//
// Queries: one lane per query, a per-lane DFS stack in LDS (64 entries: the depth of a Karras tree over unique 64-bit keys is at most 64);
// the six traversal kernels share one walk (sp_walk) and hand it their node test and their leaf test.  The BVH only culls; every answer is the exact per-collider test below, so the result equals a brute-force pass with the same tests.  A
// leaf box is the exact shape AABB grown by 64 eps * its largest coordinate, and every node test of a query grows the node box by 64 eps
// * the query's largest coordinate: the rounding of shape_aabb, of the local-frame transform, of the slab test and of the ball's
// discriminant (taken as a (r^2 - |f|^2) with f = o_l - d_l (b / a), whose error grows with |o_l|, not with |o_l|^2 as parry's b^2 - a c
// does) are all a few eps of those magnitudes, so no point that an exact test accepts lies outside the boxes the traversal tests.
// Non-finite data never reaches an exact test: a collider with a non-finite position, rotation or shape AABB is not a candidate and has
// an empty leaf box; a query with a non-finite origin, direction, point or box corner answers a miss / count 0 without traversing.
// Projection culls with a lower bound of the distance to the node box and shape intersections with the query shape's padded AABB: their
// padding arguments are in DESIGN.md 4.4.5.  A shape cast culls with the ray of the query AABB's centre against the node box grown by that
// AABB's half widths.
#include <cstddef>

#include "avn_kernels.h"
#include "avn_narrow.h"
#include "avn_spatial_pair.h"
#include "avn_capsule_pair.h"   // capsule colliders: the CAP instantiation of contact_manifolds_pair_sink (the CCAP contact kernels)
#include "avn_spatial_triangle_pair.h"   // triangle colliders: the pair tests of the CTRI instantiations (and avn_triangle_pair.h: their contacts)
#include "../../include/avian_mi355x_spatial.h"

namespace avn {

#define SP_STACK 64
#define SP_WAVE 64

// order-preserving uint32 key of a float (min / max by integer atomics)
__device__ __forceinline__ uint32_t sp_fkey(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float sp_funkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ uint32_t sp_expand10(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
template <class T> __device__ __forceinline__ T sp_maxabs(V3<T> v) { return smax(smax(fabs_t(v.x), fabs_t(v.y)), fabs_t(v.z)); }
// a box grown by 64 eps * its largest coordinate: a leaf box, and the box of a query shape
template <class T> __device__ __forceinline__ void sp_pad_box(V3<T> a, V3<T> b, V3<T>& mn, V3<T>& mx) {
    const T pad = T(64) * Limits<T>::eps * smax(sp_maxabs(a), sp_maxabs(b));
    const V3<T> pp{pad, pad, pad};
    mn = a - pp; mx = b + pp;
}

// ---------------------------------------------------------------------------------------------------------
// build
// CCAP: a capsule collider is a candidate, its leaf box shape_aabb<T, true> padded like every other
// TRI: the world holds AVN_SHAPE_TRIANGLE colliders (include/avian_mi355x_trimesh.h): left out exactly as a host shape is (no device geometry for the queries);
// a world without one launches the instantiations it always has
// CTRI (avn_spatial_triangle_colliders_set is on and the world holds a triangle; BP::col_tri is set): a triangle collider is a candidate, its leaf box
// shape_aabb's TRI case (the min / max of its three posed vertices) padded like every other
template <class T, bool CCAP = false, bool TRI = false, bool CTRI = false>
__global__ __launch_bounds__(256) void k_sp_snapshot(DW<T> w, BP<T> bp, SP<T> sp) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= sp.n) return;
    const uint4 ci = bp.col_info[c];
    const uint32_t shape = ci.z & 0xFFu;
    const int body = (int)ci.y;
    V3<T> pos; Q4<T> rot;
    collider_pose<T>(bp, c, xyz<T>(w.pos[body]), quat<T>(w.rot[body]), pos, rot);
    const V3<T> h = xyz<T>(bp.col_he[c]);
    sp.pos[c] = make4<T>(pos, T(0));
    sp.rot[c] = make4<T>(rot);
    sp.he[c] = make4<T>(h, T(0));
    // a candidate has device geometry for the queries (without CCAP a capsule COLLIDER is left out as a host shape is) and a finite
    // position, rotation and shape AABB; the others get an empty leaf box and never reach an exact test
    bool candidate = false;
    V3<T> mn{sp_inf<T>(), sp_inf<T>(), sp_inf<T>()}, mx{-sp_inf<T>(), -sp_inf<T>(), -sp_inf<T>()};
    if (shape != AVN_SHAPE_HOST && (CCAP || shape != AVN_SHAPE_CAPSULE) && (!TRI || CTRI || shape != AVN_SHAPE_TRIANGLE) && is_finite(pos) && is_finite(V3<T>{rot.x, rot.y, rot.z}) && finite_t(rot.w)) {
        V3<T> a, b;
        if (CTRI) shape_aabb<T, CCAP, true>(shape, h, pos, rot, a, b, bp.col_tri + 3 * (size_t)c);
        else shape_aabb<T, CCAP>(shape, h, pos, rot, a, b);
        if (is_finite(a) && is_finite(b)) {
            candidate = true;
            sp_pad_box(a, b, mn, mx);
            const V3<T> m = (a + b) * T(0.5);
            atomicMin(&sp.bounds[0], sp_fkey((float)m.x)); atomicMin(&sp.bounds[1], sp_fkey((float)m.y)); atomicMin(&sp.bounds[2], sp_fkey((float)m.z));
            atomicMax(&sp.bounds[3], sp_fkey((float)m.x)); atomicMax(&sp.bounds[4], sp_fkey((float)m.y)); atomicMax(&sp.bounds[5], sp_fkey((float)m.z));
        }
    }
    // (the sensor bit rides on candidates only: every reader's `!info.w` keeps its meaning)
    sp.info[c] = make_uint4(ci.x, bp.col_layers[c].x, shape, candidate ? (1u | ((((ci.z >> 8) & AVN_COLLIDER_SENSOR) != 0u) ? SP_INFO_SENSOR : 0u)) : 0u);
    sp.smin[c] = make4<T>(mn, T(0));
    sp.smax[c] = make4<T>(mx, T(0));
}

template <class T>
__global__ __launch_bounds__(256) void k_sp_morton(SP<T> sp) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= sp.n) return;
    const Vec4<T> a = sp.smin[c], b = sp.smax[c];
    uint32_t code = 0;
    if (a.x <= b.x) {   // (empty: host shapes and non-finite poses sort first, code 0)
        float lo[3], hi[3], m[3] = {(float)((a.x + b.x) * T(0.5)), (float)((a.y + b.y) * T(0.5)), (float)((a.z + b.z) * T(0.5))};
        for (int k = 0; k < 3; ++k) { lo[k] = sp_funkey(sp.bounds[k]); hi[k] = sp_funkey(sp.bounds[3 + k]); }
        uint32_t q[3];
        for (int k = 0; k < 3; ++k) {
            const float ext = hi[k] - lo[k];
            float f = ext > 0.0f ? (m[k] - lo[k]) / ext * 1024.0f : 0.0f;
            f = f > 0.0f ? (f < 1023.0f ? f : 1023.0f) : 0.0f;   // (NaN -> 0: f64 centres beyond FLT_MAX are inf as floats)
            q[k] = (uint32_t)f;
        }
        code = (sp_expand10(q[0]) << 2) | (sp_expand10(q[1]) << 1) | sp_expand10(q[2]);
    }
    sp.keys_a[c] = code;
    sp.vals_a[c] = c;
}

// common prefix length of the 64-bit keys of sorted positions i and j (-1 outside the range)
__device__ __forceinline__ int sp_delta(const uint32_t* __restrict__ code, const uint32_t* __restrict__ idx, uint32_t n, int i, int j) {
    if (j < 0 || j >= (int)n) return -1;
    const uint64_t ki = ((uint64_t)code[i] << 32) | idx[i], kj = ((uint64_t)code[j] << 32) | idx[j];
    return __clzll((long long)(ki ^ kj));
}
// Karras, "Maximizing parallelism in the construction of BVHs, octrees, and k-d trees" (HPG 2012), Figure 4
template <class T>
__global__ __launch_bounds__(256) void k_sp_karras(SP<T> sp, const uint32_t* __restrict__ code, const uint32_t* __restrict__ idx) {
    const uint32_t n = sp.n;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) sp.leaf_col[t] = idx[t];
    if (t == 0) sp.parent[0] = AVN_SPATIAL_MISS;
    if (t + 1 >= n) return;   // internal nodes 0 .. n-2
    const int i = (int)t;
    const int d = sp_delta(code, idx, n, i, i + 1) > sp_delta(code, idx, n, i, i - 1) ? 1 : -1;
    const int dmin = sp_delta(code, idx, n, i, i - d);
    int lmax = 2;
    while (sp_delta(code, idx, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int s = lmax / 2; s >= 1; s /= 2)
        if (sp_delta(code, idx, n, i, i + (l + s) * d) > dmin) l += s;
    const int j = i + l * d;
    const int dnode = sp_delta(code, idx, n, i, j);
    int s = 0;
    for (int div = 2;; div *= 2) {
        const int st = (l + div - 1) / div;
        if (sp_delta(code, idx, n, i, i + (s + st) * d) > dnode) s += st;
        if (st <= 1) break;
    }
    const int gamma = i + s * d + (d < 0 ? -1 : 0);
    const uint32_t left = (min(i, j) == gamma) ? (n - 1 + (uint32_t)gamma) : (uint32_t)gamma;
    const uint32_t right = (max(i, j) == gamma + 1) ? (n - 1 + (uint32_t)gamma + 1) : (uint32_t)gamma + 1;
    sp.child[i] = make_uint2(left, right);
    sp.parent[left] = (uint32_t)i;
    sp.parent[right] = (uint32_t)i;
}

// bottom-up refit.  The boxes of another workgroup's subtree are handed over through the arrival counter: plain stores of the box, an
// agent-scope release fence and its wait, the counter's atomic; the second arriver's agent-scope acquire, then plain vector loads.
template <class T>
__global__ __launch_bounds__(256) void k_sp_refit(SP<T> sp) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= sp.n) return;
    Vec4<T>* bmin = sp.bmin;   // (no __restrict__ / const: loads of handed-over boxes stay ordinary vector loads behind the acquire)
    Vec4<T>* bmax = sp.bmax;
    const uint32_t leaf = sp.n - 1 + j;
    const uint32_t c = sp.leaf_col[j];
    Vec4<T> lo = sp.smin[c], hi = sp.smax[c];
    bmin[leaf] = lo; bmax[leaf] = hi;
    uint32_t node = sp.parent[leaf];
    while (node != AVN_SPATIAL_MISS) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t before = __hip_atomic_fetch_add(&sp.arrivals[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before == 0u) return;   // the sibling subtree is not done: its last thread carries on
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const uint2 ch = sp.child[node];
        const Vec4<T> a0 = bmin[ch.x], a1 = bmax[ch.x], b0 = bmin[ch.y], b1 = bmax[ch.y];
        lo = make4<T>(vmin(xyz<T>(a0), xyz<T>(b0)), T(0));
        hi = make4<T>(vmax(xyz<T>(a1), xyz<T>(b1)), T(0));
        bmin[node] = lo; bmax[node] = hi;
        node = sp.parent[node];
    }
}

template <class T> void launch_spatial_build(const DW<T>& w, const BP<T>& bp, const SP<T>& sp, hipStream_t s, bool ccap, bool triangles, bool ctri) {
    const uint32_t n = sp.n;
    if (n == 0) return;
    const uint32_t nb = (n + 255) / 256;
    // bounds: min keys start at ~0, max keys at 0 (one memset each half)
    (void)hipMemsetAsync(sp.bounds, 0xFF, 3 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(sp.bounds + 3, 0x00, 5 * sizeof(uint32_t), s);
    // (the snapshot keeps both CCAP forms under CTRI: it is the one kernel in which CCAP decides whether a capsule is a candidate at all)
    if (ctri) { if (ccap) hipLaunchKernelGGL((k_sp_snapshot<T, true, true, true>), dim3(nb), dim3(256), 0, s, w, bp, sp); else hipLaunchKernelGGL((k_sp_snapshot<T, false, true, true>), dim3(nb), dim3(256), 0, s, w, bp, sp); }
    else
    if (triangles) { if (ccap) hipLaunchKernelGGL((k_sp_snapshot<T, true, true>), dim3(nb), dim3(256), 0, s, w, bp, sp); else hipLaunchKernelGGL((k_sp_snapshot<T, false, true>), dim3(nb), dim3(256), 0, s, w, bp, sp); }
    else
    if (ccap) hipLaunchKernelGGL((k_sp_snapshot<T, true>), dim3(nb), dim3(256), 0, s, w, bp, sp);
    else hipLaunchKernelGGL((k_sp_snapshot<T>), dim3(nb), dim3(256), 0, s, w, bp, sp);
    hipLaunchKernelGGL((k_sp_morton<T>), dim3(nb), dim3(256), 0, s, sp);
    uint32_t *ko = nullptr, *vo = nullptr;
    launch_radix_sort<uint32_t>(sp.keys_a, sp.vals_a, sp.keys_b, sp.vals_b, n, sp.hist, sp.block_sums, nullptr, &ko, &vo, s);
    hipLaunchKernelGGL((k_sp_karras<T>), dim3(nb), dim3(256), 0, s, sp, (const uint32_t*)ko, (const uint32_t*)vo);
    if (n > 1) (void)hipMemsetAsync(sp.arrivals, 0, (size_t)(n - 1) * sizeof(uint32_t), s);
    hipLaunchKernelGGL((k_sp_refit<T>), dim3(nb), dim3(256), 0, s, sp);
}

// ---------------------------------------------------------------------------------------------------------
// exact per-collider tests (the header's restatement of parry3d; tests/spatial_query_reference.py does the same operations in order)
// The triangle of collider c (CTRI): the three records of its slot in the world's table BP::col_tri, which SPT::tri names.  The snapshot does not copy the
// table: avn_colliders_upload and avn_collider_triangles_upload both clear sp_valid, so no query reads a table newer than its snapshot.
template <class T> __device__ __forceinline__ const Vec4<T>* sp_tri(const SP<T>&) { return nullptr; }
template <class T> __device__ __forceinline__ const Vec4<T>* sp_tri(const SPT<T>& sp) { return sp.tri; }
template <class T> __device__ __forceinline__ NpTri<T> sp_load_tri(const Vec4<T>* tri, uint32_t c) {
    const Vec4<T> a = tri[3 * (size_t)c], b = tri[3 * (size_t)c + 1], cc = tri[3 * (size_t)c + 2];
    return NpTri<T>{xyz<T>(a), xyz<T>(b), xyz<T>(cc), scalar_to_bits(a.w) & 7u};
}
// CTRI: `tri` is the triangle of a collider whose shape is AVN_SHAPE_TRIANGLE (by value; not read otherwise)
template <class T, bool CCAP = false, bool CTRI = false>
__device__ __forceinline__ bool sp_ray_exact(uint32_t shape, V3<T> he, V3<T> pos, Q4<T> rot, V3<T> o, V3<T> d, T max_distance, bool solid, T& toi, V3<T>& normal, NpTri<T> tri = NpTri<T>()) {
    const Q4<T> ci = qinverse(rot);
    const V3<T> ol = qrot(ci, o - pos);
    const V3<T> dl = qrot(ci, d);
    T t;
    bool zero_normal = false;
    V3<T> nl = vzero<T>();
    if (CTRI && shape == AVN_SHAPE_TRIANGLE) {
        if (!sp_tri_ray<T>(tri.a, tri.b, tri.c, ol, dl, t, nl)) return false;
        if (!(t <= max_distance)) return false;
    } else if (CCAP && shape == AVN_SHAPE_CAPSULE) {
        if (!sp_capcol_ray<T>(he, ol, dl, solid, t, nl)) return false;
        if (!(t <= max_distance)) return false;
        zero_normal = nl.x == T(0) && nl.y == T(0) && nl.z == T(0);
    } else if (shape == AVN_SHAPE_BALL) {
        const T r = he.x;
        const T a = dot(dl, dl), b = dot(ol, dl), c = dot(ol, ol) - r * r;
        if (c > T(0) && b > T(0)) return false;
        // b^2 - a c in its well-conditioned form: f is the origin's offset from the ray's closest point to the centre, so the rounding
        // grows with |ol|, not |ol|^2 (parry's b^2 - a c cancels two terms of size |ol|^2 and misjudges far grazing rays)
        const V3<T> f = ol - dl * (b / a);
        const T delta = a * (r * r - dot(f, f));
        if (delta < T(0)) return false;
        const T sq = sqrt_t(delta);
        t = (-b - sq) / a;
        if (t <= T(0)) {
            if (solid) { t = T(0); zero_normal = true; }
            else t = (-b + sq) / a;
        }
        if (!(t <= max_distance)) return false;
        if (!zero_normal) {
            const V3<T> p = ol + dl * t;
            const T l = length(p);
            if (l > T(0)) nl = p / l; else zero_normal = true;
        }
    } else {
        T tmin = -sp_inf<T>(), tmax = sp_inf<T>();
        int na = -1, fa = -1;
        T nsg = T(0), fsg = T(0);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const T oi = sp_vget(ol, i), di = sp_vget(dl, i), hi = sp_vget(he, i);
            if (di != T(0)) {
                const T inv = T(1) / di;
                T t1 = (-hi - oi) * inv, t2 = (hi - oi) * inv;
                T sn = T(-1), sf = T(1);
                if (inv < T(0)) { const T x = t1; t1 = t2; t2 = x; sn = T(1); sf = T(-1); }
                if (t1 > tmin) { tmin = t1; na = i; nsg = sn; }
                if (t2 < tmax) { tmax = t2; fa = i; fsg = sf; }
            } else if (oi < -hi || oi > hi) {
                return false;   // parallel to this slab and outside it
            }
        }
        if (!(tmin <= tmax) || tmax < T(0)) return false;
        int axis; T sg;
        if (tmin < T(0)) {   // the origin is inside
            if (solid) { t = T(0); zero_normal = true; axis = -1; sg = T(0); }
            else { t = tmax; axis = fa; sg = fsg; }
        } else { t = tmin; axis = na; sg = nsg; }
        if (!(t <= max_distance)) return false;
        if (axis < 0) zero_normal = true;
        else nl = V3<T>{axis == 0 ? sg : T(0), axis == 1 ? sg : T(0), axis == 2 ? sg : T(0)};
    }
    if (!finite_t(t)) return false;   // a hit needs a finite distance (max_distance = +inf stays legal)
    toi = t;
    normal = zero_normal ? vzero<T>() : qrot(rot, nl);
    return true;
}
template <class T, bool CCAP = false, bool CTRI = false> __device__ __forceinline__ bool sp_point_exact(uint32_t shape, V3<T> he, V3<T> pos, Q4<T> rot, V3<T> p, NpTri<T> tri = NpTri<T>()) {
    const V3<T> pl = qrot(qinverse(rot), p - pos);
    if (CTRI && shape == AVN_SHAPE_TRIANGLE) return sp_tri_point<T>(tri.a, tri.b, tri.c, pl);
    if (CCAP && shape == AVN_SHAPE_CAPSULE) return sp_capcol_point<T>(he, pl);
    if (shape == AVN_SHAPE_BALL) return dot(pl, pl) <= he.x * he.x;
    return fabs_t(pl.x) <= he.x && fabs_t(pl.y) <= he.y && fabs_t(pl.z) <= he.z;
}
// tri3 (CTRI): the three table records of the collider (read only where its shape is AVN_SHAPE_TRIANGLE)
template <class T, bool CCAP = false, bool CTRI = false> __device__ __forceinline__ bool sp_aabb_exact(uint32_t shape, V3<T> he, V3<T> pos, Q4<T> rot, V3<T> qmin, V3<T> qmax, const Vec4<T>* tri3 = nullptr) {
    V3<T> mn, mx;
    shape_aabb<T, CCAP, CTRI>(shape, he, pos, rot, mn, mx, tri3);
    return mn.x <= qmax.x && mn.y <= qmax.y && mn.z <= qmax.z && mx.x >= qmin.x && mx.y >= qmin.y && mx.z >= qmin.z;
}

// ---------------------------------------------------------------------------------------------------------
// traversal
template <class T> struct RayCtx { V3<T> o, d, inv; uint32_t zero; T tol; };
// entry distance of the ray into the node box grown by tol (+inf = miss); the node test of every ray query
template <class T> __device__ __forceinline__ T sp_ray_box(const RayCtx<T>& r, Vec4<T> lo4, Vec4<T> hi4, T limit) {
    T tmin = -sp_inf<T>(), tmax = sp_inf<T>();
    const V3<T> lo = xyz<T>(lo4), hi = xyz<T>(hi4);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const T l = sp_vget(lo, i) - r.tol, h = sp_vget(hi, i) + r.tol, oi = sp_vget(r.o, i);
        if (r.zero & (1u << i)) {
            if (!(oi >= l && oi <= h)) return sp_inf<T>();
        } else {
            const T iv = sp_vget(r.inv, i);
            T t1 = (l - oi) * iv, t2 = (h - oi) * iv;
            if (iv < T(0)) { const T x = t1; t1 = t2; t2 = x; }
            tmin = smax(tmin, t1);
            tmax = smin(tmax, t2);
        }
    }
    if (!(tmin <= tmax) || tmax < T(0) || !(tmin <= limit)) return sp_inf<T>();
    return smax(tmin, T(0));
}
template <class T> __device__ __forceinline__ bool sp_point_box(V3<T> p, T tol, Vec4<T> lo, Vec4<T> hi) {
    return p.x >= lo.x - tol && p.x <= hi.x + tol && p.y >= lo.y - tol && p.y <= hi.y + tol && p.z >= lo.z - tol && p.z <= hi.z + tol;
}
template <class T> __device__ __forceinline__ bool sp_box_box(V3<T> qmin, V3<T> qmax, Vec4<T> lo, Vec4<T> hi) {
    return lo.x <= qmax.x && lo.y <= qmax.y && lo.z <= qmax.z && hi.x >= qmin.x && hi.y >= qmin.y && hi.z >= qmin.z;
}
__device__ __forceinline__ bool sp_excluded(const uint32_t* __restrict__ ex, uint32_t n, uint32_t e) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (ex[m] < e) lo = m + 1; else hi = m; }
    return lo < n && ex[lo] == e;
}

// ---------------------------------------------------------------------------------------------------------
// what the traversal kernels share: the loads of a query, the leaf filter, the output lists, the counters and the walk itself
template <class T> __device__ __forceinline__ V3<T> sp_load3(const T* p, uint32_t i) { return V3<T>{p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]}; }

// the ray from o along d; the node test of a ray grows every node box by tol = 64 eps * the origin's largest coordinate
template <class T> __device__ __forceinline__ RayCtx<T> sp_ray_ctx(V3<T> o, V3<T> d) {
    RayCtx<T> r;
    r.o = o; r.d = d;
    r.inv = V3<T>{d.x != T(0) ? T(1) / d.x : T(0), d.y != T(0) ? T(1) / d.y : T(0), d.z != T(0) ? T(1) / d.z : T(0)};
    r.zero = (d.x == T(0) ? 1u : 0u) | (d.y == T(0) ? 2u : 0u) | (d.z == T(0) ? 4u : 0u);
    r.tol = T(64) * Limits<T>::eps * sp_maxabs(o);
    return r;
}

// The query shape of lane i.  valid: a Ball or a Cuboid with a finite pose, finite half extents that are not negative and a finite AABB
// [a, b] at its pose (shape_aabb: exact).  Every caller answers an invalid shape a miss / count 0 without traversing.
template <class T> struct QShape { uint32_t shape; V3<T> he, pos; Q4<T> rot; V3<T> a, b; bool valid; };
// CAPSULE (the second instantiation of a query kernel, launched behind the first): valid = an AVN_SHAPE_CAPSULE with finite r (x) and h (y) that are
// not negative; he = (r, h, 0), z is not read; [a, b] = pos +- (|qrot(rot, (0, h, 0))| + (r, r, r)).  Without it a capsule is an invalid kind.
template <class T, bool CAPSULE = false> __device__ __forceinline__ QShape<T> sp_load_shape(const uint8_t* shape, const T* pos, const T* he, const T* rot, uint32_t i) {
    QShape<T> s;
    s.shape = shape[i];
    s.pos = sp_load3(pos, i);
    s.he = sp_load3(he, i);
    s.rot = Q4<T>{rot[4 * (size_t)i], rot[4 * (size_t)i + 1], rot[4 * (size_t)i + 2], rot[4 * (size_t)i + 3]};
    if (s.shape == AVN_SHAPE_BALL) s.he = V3<T>{s.he.x, s.he.x, s.he.x};   // (a ball has its radius in x: y and z are not read)
    if (CAPSULE) s.he.z = T(0);
    s.a = s.b = vzero<T>();
    s.valid = (CAPSULE ? s.shape == AVN_SHAPE_CAPSULE : s.shape <= AVN_SHAPE_BALL) && is_finite(s.pos) && is_finite(V3<T>{s.rot.x, s.rot.y, s.rot.z}) && finite_t(s.rot.w) && is_finite(s.he) &&
              s.he.x >= T(0) && s.he.y >= T(0) && s.he.z >= T(0);
    if (s.valid) {
        if (CAPSULE) capsule_aabb<T>(s.he, s.pos, s.rot, s.a, s.b);
        else shape_aabb<T>(s.shape, s.he, s.pos, s.rot, s.a, s.b);
        s.valid = is_finite(s.a) && is_finite(s.b);
    }
    return s;
}
// the kind of a valid query shape as the instantiation knows it (a CAPSULE one: a capsule; the first: a ball or a cuboid): the triangle manifold of the
// contacts then compiles the one or two pair tests the instantiation can reach, not all three
template <bool CAPSULE> __device__ __forceinline__ uint32_t sp_query_kind(uint32_t shape) { return CAPSULE ? (uint32_t)AVN_SHAPE_CAPSULE : (shape == AVN_SHAPE_BALL ? (uint32_t)AVN_SHAPE_BALL : (uint32_t)AVN_SHAPE_CUBOID); }
// a lane of a CAPSULE instantiation whose query is no capsule is passed over: the first launch has answered it
template <bool CAPSULE> __device__ __forceinline__ bool sp_lane_kind(const uint8_t* shape, uint32_t i) { return !CAPSULE || shape[i] == AVN_SHAPE_CAPSULE; }
// The chunks of SP_WAVE queries a block answers.  The first launch has one block per chunk.  A CAPSULE launch has at most SP_CAPSULE_GRID blocks
// that stride over the chunks: with no capsule in the call (device arrays are not read back, so the launch still goes) it costs a few
// thousand one-wave blocks that read one byte per query, not a block -- with its 16 KB of LDS and ~200 VGPRs -- per 64 queries.
#define SP_CAPSULE_GRID 2048u
template <bool CAPSULE> __device__ __forceinline__ uint32_t sp_next_chunk(uint32_t base, uint32_t n) {
    if (!CAPSULE) return n;
    const uint32_t next = base + gridDim.x * SP_WAVE;
    return next < base ? n : next;
}
static inline dim3 sp_capsule_grid(uint32_t n) { const uint32_t g = (n + SP_WAVE - 1) / SP_WAVE; return dim3(g < SP_CAPSULE_GRID ? g : SP_CAPSULE_GRID); }
// the ray of a shape cast: from the centre of the query shape's padded AABB along d, against the node boxes grown by that AABB's half widths hw
template <class T> __device__ __forceinline__ RayCtx<T> sp_cast_ray(const QShape<T>& s, V3<T> d, V3<T>& hw) {
    V3<T> qmin, qmax;
    sp_pad_box(s.a, s.b, qmin, qmax);
    hw = (qmax - qmin) * T(0.5);
    return sp_ray_ctx<T>((qmin + qmax) * T(0.5), d);
}
template <class T> __device__ __forceinline__ T sp_cast_box(const RayCtx<T>& r, V3<T> hw, Vec4<T> lo, Vec4<T> hi, T limit) {
    return sp_ray_box(r, make4<T>(lo.x - hw.x, lo.y - hw.y, lo.z - hw.z, T(0)), make4<T>(hi.x + hw.x, hi.y + hw.y, hi.z + hw.z, T(0)), limit);
}

// the leaf filter: a candidate (live, with device geometry) in the query's mask that is neither the query's own entity nor in the sorted list ex
__device__ __forceinline__ bool sp_leaf_ok(uint4 info, uint32_t mask, uint32_t self, const uint32_t* ex, uint32_t ex_n) {
    return info.w && (info.y & mask) != 0u && !(self != AVN_SPATIAL_MISS && info.x == self) && !(ex_n && sp_excluded(ex, ex_n, info.x));
}

// The output lists: the best k of the `found` accepted so far, kept sorted by insertion into the query's own output slots.  Both return the
// slot of the new entry, the worse ones moved up, or AVN_SPATIAL_MISS when it does not make the list.
__device__ __forceinline__ uint32_t sp_collider_of(uint32_t id) { return id; }
template <class T> __device__ __forceinline__ uint32_t sp_collider_of(const SpatialShapeContact<T>& r) { return r.collider; }
// ascending collider index (ids, contact records)
template <class E> __device__ __forceinline__ uint32_t sp_slot_by_collider(E* l, uint32_t k, uint32_t& found, uint32_t c) {
    uint32_t m = found < k ? found : k;
    ++found;
    if (m == k) {
        if (k == 0 || c >= sp_collider_of(l[k - 1])) return AVN_SPATIAL_MISS;
        m = k - 1;
    }
    while (m > 0 && sp_collider_of(l[m - 1]) > c) { l[m] = l[m - 1]; --m; }
    return m;
}
// nearest-k by (distance, collider) (ray hits, shape hits)
template <class E, class T> __device__ __forceinline__ uint32_t sp_slot_by_distance(E* l, uint32_t k, uint32_t& found, T toi, uint32_t c) {
    uint32_t m = found < k ? found : k;
    ++found;
    if (m == k) {
        const T ld = l[k - 1].distance;
        if (!(toi < ld || (toi == ld && c < l[k - 1].collider))) return AVN_SPATIAL_MISS;
        m = k - 1;
    }
    while (m > 0 && (l[m - 1].distance > toi || (l[m - 1].distance == toi && l[m - 1].collider > c))) { l[m] = l[m - 1]; --m; }
    return m;
}

// the records.  normal2 = -normal1, a zero component staying +0 (a miss and an overlap at the start: every byte 0)
template <class T> __device__ __forceinline__ void sp_put(SpatialHit<T>& h, uint32_t c, uint32_t e, T t, V3<T> n) {
    h.collider = c; h.entity = e; h.distance = t;
    h.normal[0] = n.x; h.normal[1] = n.y; h.normal[2] = n.z;
}
template <class T> __device__ __forceinline__ void sp_put(SpatialShapeHit<T>& h, uint32_t c, uint32_t e, T t, V3<T> p1, V3<T> p2, V3<T> n1) {
    h.collider = c; h.entity = e; h.distance = t;
    h.point1[0] = p1.x; h.point1[1] = p1.y; h.point1[2] = p1.z;
    h.point2[0] = p2.x; h.point2[1] = p2.y; h.point2[2] = p2.z;
    h.normal1[0] = n1.x; h.normal1[1] = n1.y; h.normal1[2] = n1.z;
    h.normal2[0] = n1.x == T(0) ? T(0) : -n1.x; h.normal2[1] = n1.y == T(0) ? T(0) : -n1.y; h.normal2[2] = n1.z == T(0) ? T(0) : -n1.z;
}
// the miss of every list
__device__ __forceinline__ void sp_put_miss(uint32_t& id) { id = AVN_SPATIAL_MISS; }
template <class T> __device__ __forceinline__ void sp_put_miss(SpatialHit<T>& h) { sp_put<T>(h, AVN_SPATIAL_MISS, AVN_SPATIAL_MISS, T(0), vzero<T>()); }
template <class T> __device__ __forceinline__ void sp_put_miss(SpatialShapeHit<T>& h) { sp_put<T>(h, AVN_SPATIAL_MISS, AVN_SPATIAL_MISS, T(0), vzero<T>(), vzero<T>(), vzero<T>()); }
template <class T> __device__ __forceinline__ void sp_put_miss(SpatialShapeContact<T>& r) {
    r.collider = AVN_SPATIAL_MISS; r.entity = AVN_SPATIAL_MISS; r.penetration = T(0);
    for (int i = 0; i < 3; ++i) r.normal[i] = r.point[i] = r.anchor1[i] = r.anchor2[i] = T(0);
    sp_clear_reserved(r);
}
template <class E> __device__ __forceinline__ void sp_fill_miss(E* l, uint32_t from, uint32_t to) {
    E miss;
    sp_put_miss(miss);
    for (uint32_t m = from; m < to; ++m) l[m] = miss;
}

// totals of the call, by every lane of the wave: one atomic per wave.  flags: bit 0 a stack overflow; bit 1 (k_sp_cast_move) more than
// AVN_SPATIAL_MAX_HITS pending colliders
__device__ __forceinline__ void sp_add_stats(unsigned long long* stats, uint32_t nodes_tested, uint32_t leaves_tested, uint32_t flags) {
    uint32_t a = nodes_tested, b = leaves_tested, o = flags;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); o |= __shfl_xor(o, off); }
    if (threadIdx.x == 0) {
        atomicAdd(&stats[0], (unsigned long long)a);
        atomicAdd(&stats[1], (unsigned long long)b);
        if (o) atomicOr(&stats[2], (unsigned long long)o);
    }
}

// The walk of every query kernel: one lane per query in blocks of one wave, a depth-first descent of the LBVH with the lane's own SP_STACK-
// entry column of the LDS stack.  test(node) is the kernel's key of the node box, +inf = culled (the kinds without a distance answer 0 or
// +inf); leaf(c) is its exact test of collider c.  The nearer child goes first, the left one on a tie, so the kinds without a distance go
// left to right.  PRUNE (the closest-hit kinds, `best` their best distance so far): a leaf or a child whose key the leaf before it has left
// STRICTLY above `best` is dropped, and a popped node is re-tested -- only strictly, so a collider at the best distance with a lower index is
// still reached.  Without PRUNE a node is tested once: a re-test would count it twice.
template <class T, bool PRUNE, class Test, class Leaf>
__device__ __forceinline__ void sp_walk(const SP<T>& sp, uint32_t& overflow, const T& best, Test test, Leaf leaf) {
    __shared__ uint32_t stack[SP_STACK * SP_WAVE];
    const uint32_t n = sp.n, lane = threadIdx.x;
    if (n == 0 || test(0u) == sp_inf<T>()) return;
    uint32_t sp_top = 0, node = 0;
    for (;;) {
        // (a tree of one collider: its root is the leaf, handled by the same leaf call site)
        uint2 ch = make_uint2(0u, 0u);
        T e0 = T(0), e1 = sp_inf<T>();
        if (n > 1) { ch = sp.child[node]; e0 = test(ch.x); e1 = test(ch.y); }
        const bool l0 = ch.x >= n - 1, l1 = ch.y >= n - 1;
        // one leaf call site: the pair tests are emitted once
        uint32_t pending = (l0 && e0 != sp_inf<T>() ? 1u : 0u) | (l1 && e1 != sp_inf<T>() ? 2u : 0u);
        while (pending) {
            const bool first = (pending & 1u) != 0;
            // (the first leaf may have shrunk the best distance below the second one's key)
            if (first || !PRUNE || !(e1 > best)) leaf(sp.leaf_col[(first ? ch.x : ch.y) - (n - 1)]);
            pending &= first ? ~1u : ~2u;
        }
        const bool g0 = !l0 && e0 != sp_inf<T>() && (!PRUNE || !(e0 > best)), g1 = !l1 && e1 != sp_inf<T>() && (!PRUNE || !(e1 > best));
        if (g0 && g1) {
            const bool first0 = !(e1 < e0);
            if (sp_top < SP_STACK) { stack[sp_top * SP_WAVE + lane] = first0 ? ch.y : ch.x; ++sp_top; }
            else overflow |= 1u;   // (cannot happen: the depth of a Karras tree over unique 64-bit keys is at most 64)
            node = first0 ? ch.x : ch.y;
            continue;
        }
        if (g0) { node = ch.x; continue; }
        if (g1) { node = ch.y; continue; }
        // pop; a node pushed before the best distance shrank is re-tested against it
        node = AVN_SPATIAL_MISS;
        while (sp_top > 0) {
            --sp_top;
            const uint32_t cand = stack[sp_top * SP_WAVE + lane];
            if (!PRUNE || test(cand) != sp_inf<T>()) { node = cand; break; }
        }
        if (node == AVN_SPATIAL_MISS) break;
    }
}

// one lane per query.  PQ (a caster run, SPQ_CLOSEST / SPQ_HITS only): the lane answers caster q.index[lane's query] with that caster's own
// self_entity, excluded slice, live flag and k, into its row of q.cap record slots.
// CTRI (here and in every traversal kernel below): a triangle collider is a candidate; the kernel's first argument then carries the world's triangle
// table (SPT), and the leaf reads the collider's triangle from it BY VALUE where the collider's shape says triangle
template <class T, int KIND, bool PQ = false, bool CCAP = false, bool CTRI = false>
__global__ __launch_bounds__(SP_WAVE) void k_sp_query(typename SpArg<T, CTRI>::type sp, SQ<T> q) {
    constexpr bool RAY = KIND == SPQ_CLOSEST || KIND == SPQ_HITS;
    const uint32_t li = blockIdx.x * SP_WAVE + threadIdx.x;
    uint32_t nodes_tested = 0, leaves_tested = 0, overflow = 0;
    if (li < q.n) {
        const uint32_t qi = PQ ? q.index[li] : li;
        const uint32_t mask = q.mask ? q.mask[qi] : 0xFFFFFFFFu;
        const uint32_t self = PQ ? q.self_entity[qi] : AVN_SPATIAL_MISS;
        const uint32_t ex0 = PQ ? q.ex_offset[qi] : 0u, ex_n = PQ ? q.ex_offset[qi + 1] - ex0 : q.n_excluded;
        const uint32_t kq = PQ ? q.kq[qi] : q.cap;   // the list length of SPQ_HITS
        // per-query state: a ray from pa along pb, the point pa, or the box [pa, pb]
        const V3<T> pa = sp_load3(q.a, qi);
        const V3<T> pb = KIND != SPQ_POINTS ? sp_load3(q.b, qi) : vzero<T>();
        const T max_distance = RAY ? q.max_distance[qi] : T(0);
        const bool solid = RAY && q.solid[qi] != 0;
        const RayCtx<T> r = sp_ray_ctx<T>(pa, pb);
        const T tol = T(64) * Limits<T>::eps * sp_maxabs(pa);
        // a non-finite origin, direction, point or box corner answers a miss / count 0 without traversing the tree
        const bool finite_query = is_finite(pa) && (KIND == SPQ_POINTS || is_finite(pb)) && (!PQ || q.live[qi] != 0);
        // results
        T best = sp_inf<T>();
        uint32_t best_c = AVN_SPATIAL_MISS;
        V3<T> best_n = vzero<T>();
        uint32_t found = 0;
        SpatialHit<T>* hl = RAY ? q.hits + (size_t)qi * q.cap : nullptr;
        uint32_t* il = RAY ? nullptr : q.ids + (size_t)qi * q.cap;

        // node test: entry distance for rays (+inf = miss), 0 / +inf for the others
        auto test = [&](uint32_t node) -> T {
            ++nodes_tested;
            const Vec4<T> lo = sp.bmin[node], hi = sp.bmax[node];
            if (KIND == SPQ_CLOSEST) return sp_ray_box(r, lo, hi, smin(best, max_distance));
            if (KIND == SPQ_HITS) return sp_ray_box(r, lo, hi, max_distance);
            if (KIND == SPQ_POINTS) return sp_point_box(pa, tol, lo, hi) ? T(0) : sp_inf<T>();
            return sp_box_box(pa, pb, lo, hi) ? T(0) : sp_inf<T>();
        };
        auto leaf = [&](uint32_t c) {
            const uint4 info = sp.info[c];
            if (!sp_leaf_ok(info, mask, self, q.excluded + ex0, ex_n)) return;
            ++leaves_tested;
            const V3<T> pos = xyz<T>(sp.pos[c]), he = xyz<T>(sp.he[c]);
            const Q4<T> rot = quat<T>(sp.rot[c]);
            NpTri<T> tri = NpTri<T>();
            if (CTRI && KIND != SPQ_AABBS && info.z == AVN_SHAPE_TRIANGLE) tri = sp_load_tri<T>(sp_tri(sp), c);
            if (RAY) {
                T toi; V3<T> nrm;
                if (!sp_ray_exact<T, CCAP, CTRI>(info.z, he, pos, rot, r.o, r.d, max_distance, solid, toi, nrm, tri)) return;
                if (KIND == SPQ_CLOSEST) {
                    if (toi < best || (toi == best && c < best_c)) { best = toi; best_c = c; best_n = nrm; }
                } else {
                    const uint32_t m = sp_slot_by_distance(hl, kq, found, toi, c);
                    if (m == AVN_SPATIAL_MISS) return;
                    SpatialHit<T> h;
                    sp_put<T>(h, c, info.x, toi, nrm);
                    hl[m] = h;
                }
            } else {
                const bool hit = KIND == SPQ_POINTS ? sp_point_exact<T, CCAP, CTRI>(info.z, he, pos, rot, pa, tri)
                                                    : sp_aabb_exact<T, CCAP, CTRI>(info.z, he, pos, rot, pa, pb, CTRI ? sp_tri(sp) + 3 * (size_t)c : nullptr);
                if (!hit) return;
                const uint32_t m = sp_slot_by_collider(il, q.cap, found, c);
                if (m != AVN_SPATIAL_MISS) il[m] = c;
            }
        };
        if (finite_query) sp_walk<T, KIND == SPQ_CLOSEST>(sp, overflow, best, test, leaf);

        // write the results
        if (KIND == SPQ_CLOSEST) {
            SpatialHit<T> h;
            sp_put<T>(h, best_c, best_c == AVN_SPATIAL_MISS ? AVN_SPATIAL_MISS : sp.info[best_c].x, best_c == AVN_SPATIAL_MISS ? T(0) : best, best_n);
            if (!PQ) q.hits[qi] = h;
            else {
                // the caster's row: the hit or a miss, then misses; count 0 or 1
                hl[0] = h;
                sp_fill_miss(hl, 1u, q.cap);
                q.count[qi] = best_c == AVN_SPATIAL_MISS ? 0u : 1u;
            }
        } else {
            if (KIND == SPQ_HITS) sp_fill_miss(hl, found < kq ? found : kq, q.cap);
            else sp_fill_miss(il, found, q.cap);
            q.count[qi] = found;
        }
    }
    sp_add_stats(q.stats, nodes_tested, leaves_tested, overflow);
}

// ---------------------------------------------------------------------------------------------------------
// point projection and shape intersections

// the header's projection of a point onto one collider: false when the distance is not finite
// CTRI, a triangle collider: tri_closest_point; is_inside iff that is the point itself (sp_tri_point's test); `solid` has no effect (a triangle has no
// interior: the point answered is always the projection carried back to the world)
template <class T, bool CCAP = false, bool CTRI = false>
__device__ __forceinline__ bool sp_project_exact(uint32_t shape, V3<T> he, V3<T> pos, Q4<T> rot, V3<T> p, bool solid, T& distance, V3<T>& point, bool& is_inside, NpTri<T> tri = NpTri<T>()) {
    const V3<T> pl = qrot(qinverse(rot), p - pos);
    V3<T> proj;
    bool inside;
    if (CTRI && shape == AVN_SHAPE_TRIANGLE) {
        int rg;
        proj = tri_closest_point<T>(tri.a, tri.b, tri.c, pl, rg);
        inside = proj.x == pl.x && proj.y == pl.y && proj.z == pl.z;
        solid = false;
    } else if (CCAP && shape == AVN_SHAPE_CAPSULE) sp_capcol_project<T>(he, pl, solid, proj, inside);
    else if (shape == AVN_SHAPE_BALL) {
        const T r = he.x;
        const T d2 = dot(pl, pl);
        inside = d2 <= r * r;
        if (!(solid && inside)) proj = d2 == T(0) ? V3<T>{T(0), r, T(0)} : pl * (r / sqrt_t(d2));
    } else {
        inside = fabs_t(pl.x) <= he.x && fabs_t(pl.y) <= he.y && fabs_t(pl.z) <= he.z;
        if (!inside) {
            proj = V3<T>{pl.x < -he.x ? -he.x : (pl.x > he.x ? he.x : pl.x), pl.y < -he.y ? -he.y : (pl.y > he.y ? he.y : pl.y),
                         pl.z < -he.z ? -he.z : (pl.z > he.z ? he.z : pl.z)};
        } else if (!solid) {
            // the nearest face: the smallest he.i - |pl.i|, strict <, so the first axis in x, y, z order wins a tie
            T m = he.x - fabs_t(pl.x);
            int axis = 0;
            const T my = he.y - fabs_t(pl.y), mz = he.z - fabs_t(pl.z);
            if (my < m) { m = my; axis = 1; }
            if (mz < m) { m = mz; axis = 2; }
            proj = V3<T>{axis == 0 ? copysign_t(he.x, pl.x) : pl.x, axis == 1 ? copysign_t(he.y, pl.y) : pl.y, axis == 2 ? copysign_t(he.z, pl.z) : pl.z};
        }
    }
    is_inside = inside;
    if (solid && inside) { distance = T(0); point = p; return true; }
    const V3<T> diff = pl - proj;
    distance = sqrt_t(dot(diff, diff));
    point = qrot(rot, proj) + pos;
    return finite_t(distance);
}
// A lower bound of the projection distance of every collider under a node, or -1 for an empty box: the distance from the point to the
// node box grown by the query's tolerance plus 64 eps * the box's largest coordinate, times (1 - 8 eps) for the rounding of this
// function's own squares, sum and square root (DESIGN.md 4.4.5 has the argument).
template <class T> __device__ __forceinline__ T sp_point_box_distance(V3<T> p, T tol, Vec4<T> lo, Vec4<T> hi) {
    if (!(lo.x <= hi.x)) return T(-1);
    const T m = smax(smax(smax(fabs_t(lo.x), fabs_t(lo.y)), smax(fabs_t(lo.z), fabs_t(hi.x))), smax(fabs_t(hi.y), fabs_t(hi.z)));
    const T g = tol + T(64) * Limits<T>::eps * m;
    const V3<T> d{smax(smax((lo.x - g) - p.x, p.x - (hi.x + g)), T(0)), smax(smax((lo.y - g) - p.y, p.y - (hi.y + g)), T(0)),
                  smax(smax((lo.z - g) - p.z, p.z - (hi.z + g)), T(0))};
    return sqrt_t(dot(d, d)) * (T(1) - T(8) * Limits<T>::eps);
}

template <class T, bool CCAP = false, bool CTRI = false>
__global__ __launch_bounds__(SP_WAVE) void k_sp_project(typename SpArg<T, CTRI>::type sp, SQ<T> q) {
    const uint32_t qi = blockIdx.x * SP_WAVE + threadIdx.x;
    uint32_t nodes_tested = 0, leaves_tested = 0, overflow = 0;
    if (qi < q.n) {
        const uint32_t mask = q.mask ? q.mask[qi] : 0xFFFFFFFFu;
        const V3<T> p = sp_load3(q.a, qi);
        const bool solid = q.solid[qi] != 0;
        const T tol = T(64) * Limits<T>::eps * sp_maxabs(p);
        T best = sp_inf<T>();
        uint32_t best_c = AVN_SPATIAL_MISS, best_in = 0;
        V3<T> best_p = vzero<T>();
        // the node's lower bound, or +inf when the node is empty or culled: only a bound STRICTLY above the best distance culls, so a collider
        // at the best distance with a lower index is still reached
        auto test = [&](uint32_t node) -> T {
            ++nodes_tested;
            const T b = sp_point_box_distance<T>(p, tol, sp.bmin[node], sp.bmax[node]);
            return (b >= T(0) && !(b > best)) ? b : sp_inf<T>();
        };
        auto leaf = [&](uint32_t c) {
            const uint4 info = sp.info[c];
            if (!sp_leaf_ok(info, mask, AVN_SPATIAL_MISS, q.excluded, q.n_excluded)) return;
            ++leaves_tested;
            T d; V3<T> pt; bool in;
            NpTri<T> tri = NpTri<T>();
            if (CTRI && info.z == AVN_SHAPE_TRIANGLE) tri = sp_load_tri<T>(sp_tri(sp), c);
            if (!sp_project_exact<T, CCAP, CTRI>(info.z, xyz<T>(sp.he[c]), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]), p, solid, d, pt, in, tri)) return;
            if (d < best || (d == best && c < best_c)) { best = d; best_c = c; best_p = pt; best_in = in ? 1u : 0u; }
        };
        if (is_finite(p)) sp_walk<T, true>(sp, overflow, best, test, leaf);
        SpatialProjection<T> r;
        r.collider = best_c;
        r.entity = best_c == AVN_SPATIAL_MISS ? AVN_SPATIAL_MISS : sp.info[best_c].x;
        r.is_inside = best_in;
        sp_clear_reserved(r);
        r.point[0] = best_p.x; r.point[1] = best_p.y; r.point[2] = best_p.z;
        r.distance = best_c == AVN_SPATIAL_MISS ? T(0) : best;
        q.proj[qi] = r;
    }
    sp_add_stats(q.stats, nodes_tested, leaves_tested, overflow);
}

// the header's intersection test of a query shape (shape 1, isometry iso1 = make_isometry of its pose) with one collider (shape 2)
template <class T>
__device__ __forceinline__ bool sp_shape_exact(uint32_t shape1, V3<T> he1, const Iso<T>& iso1, uint32_t shape2, V3<T> he2, V3<T> pos2, Q4<T> rot2) {
    const Iso<T> pos12 = iso_inv_mul(iso1, Iso<T>{rot2, pos2});
    if (shape1 == AVN_SHAPE_BALL && shape2 == AVN_SHAPE_BALL) {
        const T rr = he1.x + he2.x;
        return na_dot(pos12.t, pos12.t) <= rr * rr;
    }
    if (shape1 == AVN_SHAPE_BALL || shape2 == AVN_SHAPE_BALL) {
        // the ball's centre in the cuboid's frame
        const bool ball1 = shape1 == AVN_SHAPE_BALL;
        const V3<T> c = ball1 ? iso_inv_point(pos12, vzero<T>()) : pos12.t;
        const V3<T> he = ball1 ? he2 : he1;
        const T r = ball1 ? he1.x : he2.x;
        if (fabs_t(c.x) <= he.x && fabs_t(c.y) <= he.y && fabs_t(c.z) <= he.z) return true;
        const V3<T> cl{c.x < -he.x ? -he.x : (c.x > he.x ? he.x : c.x), c.y < -he.y ? -he.y : (c.y > he.y ? he.y : c.y), c.z < -he.z ? -he.z : (c.z > he.z ? he.z : c.z)};
        const V3<T> d = c - cl;
        return na_dot(d, d) <= r * r;
    }
    V3<T> dir;
    if (sat_normal_oneway(he1, he2, pos12, dir) > T(0)) return false;
    if (sat_normal_oneway(he2, he1, iso_inverse(pos12), dir) > T(0)) return false;
    if (sat_edge_twoway(he1, he2, pos12, dir) > T(0)) return false;
    return true;
}

template <class T, bool CAPSULE = false, bool CCAP = false, bool CTRI = false>
__global__ __launch_bounds__(SP_WAVE) void k_sp_shapes(typename SpArg<T, CTRI>::type sp, SQ<T> q) {
    uint32_t nodes_tested = 0, leaves_tested = 0, overflow = 0;
    uint32_t base = blockIdx.x * SP_WAVE;
    do {   // (once; a CAPSULE launch: every chunk of this block's stride)
    const uint32_t qi = base + threadIdx.x;
    if (qi < q.n && sp_lane_kind<CAPSULE>(q.shape, qi)) {
        const uint32_t mask = q.mask ? q.mask[qi] : 0xFFFFFFFFu;
        const QShape<T> s = sp_load_shape<T, CAPSULE>(q.shape, q.a, q.he, q.rot, qi);
        // the query shape's exact AABB at its pose, grown as the leaf boxes are
        V3<T> qmin, qmax;
        sp_pad_box(s.a, s.b, qmin, qmax);
        const Iso<T> iso1 = make_isometry(s.pos, s.rot);
        uint32_t found = 0;
        uint32_t* il = q.ids + (size_t)qi * q.cap;
        auto test = [&](uint32_t node) -> T {
            ++nodes_tested;
            return sp_box_box(qmin, qmax, sp.bmin[node], sp.bmax[node]) ? T(0) : sp_inf<T>();
        };
        auto leaf = [&](uint32_t c) {
            const uint4 info = sp.info[c];
            if (!sp_leaf_ok(info, mask, AVN_SPATIAL_MISS, q.excluded, q.n_excluded)) return;
            ++leaves_tested;
            if (CTRI && info.z == AVN_SHAPE_TRIANGLE) {
                if (!sp_tricol_intersects<T, CAPSULE>(s.shape, s.he, iso1, sp_load_tri<T>(sp_tri(sp), c), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]))) return;
            } else if (CCAP && info.z == AVN_SHAPE_CAPSULE) {
                if (!sp_capcol_intersects<T, CAPSULE>(s.shape, s.he, iso1, xyz<T>(sp.he[c]), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]))) return;
            } else if (CAPSULE) {
                if (!sp_capsule_intersects<T>(s.he.x, s.he.y, iso_inv_mul(Iso<T>{quat<T>(sp.rot[c]), xyz<T>(sp.pos[c])}, iso1), info.z, xyz<T>(sp.he[c]))) return;
            } else if (!sp_shape_exact<T>(s.shape, s.he, iso1, info.z, xyz<T>(sp.he[c]), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]))) return;
            const uint32_t m = sp_slot_by_collider(il, q.cap, found, c);
            if (m != AVN_SPATIAL_MISS) il[m] = c;
        };
        if (s.valid) sp_walk<T, false>(sp, overflow, T(0), test, leaf);
        sp_fill_miss(il, found, q.cap);
        q.count[qi] = found;
    }
    } while (CAPSULE && (base = sp_next_chunk<CAPSULE>(base, q.n)) < q.n);
    sp_add_stats(q.stats, nodes_tested, leaves_tested, overflow);
}

// ---------------------------------------------------------------------------------------------------------
// shape casts.  The header defines the per-pair tests, operation order included; tests/spatial_cast_reference.py does the same operations in
// order.  DESIGN.md 4.4.6 has the padding argument.

// one lane per cast; MANY: the nearest-k list (shape_hits), else the closest hit (cast_shapes).  PQ: a caster run, as in k_sp_query
template <class T, bool MANY, bool PQ = false, bool CAPSULE = false, bool CCAP = false, bool CTRI = false>
__global__ __launch_bounds__(SP_WAVE) void k_sp_cast(typename SpArg<T, CTRI>::type sp, SQ<T> q) {
    uint32_t nodes_tested = 0, leaves_tested = 0, overflow = 0;
    uint32_t base = blockIdx.x * SP_WAVE;
    do {   // (once; a CAPSULE launch: every chunk of this block's stride)
    const uint32_t li = base + threadIdx.x;
    if (li < q.n && sp_lane_kind<CAPSULE>(q.shape, PQ ? q.index[li] : li)) {
        const uint32_t qi = PQ ? q.index[li] : li;
        const uint32_t mask = q.mask ? q.mask[qi] : 0xFFFFFFFFu;
        const uint32_t self = PQ ? q.self_entity[qi] : AVN_SPATIAL_MISS;
        const uint32_t ex0 = PQ ? q.ex_offset[qi] : 0u, ex_n = PQ ? q.ex_offset[qi + 1] - ex0 : q.n_excluded;
        const uint32_t kq = PQ ? q.kq[qi] : q.cap;   // the list length of MANY
        const QShape<T> s = sp_load_shape<T, CAPSULE>(q.shape, q.a, q.he, q.rot, qi);
        const V3<T> d = sp_load3(q.b, qi);
        const T max_distance = q.max_distance[qi];
        // a valid shape, a finite direction and a max_distance that is not NaN: otherwise a miss / count 0
        const bool valid = s.valid && is_finite(d) && max_distance == max_distance && (!PQ || q.live[qi] != 0);
        V3<T> hw;
        const RayCtx<T> r = sp_cast_ray(s, d, hw);
        const Iso<T> iso2 = make_isometry(s.pos, s.rot);
        T best = sp_inf<T>();
        uint32_t best_c = AVN_SPATIAL_MISS;
        V3<T> best_p1 = vzero<T>(), best_p2 = vzero<T>(), best_n1 = vzero<T>();
        uint32_t found = 0;
        SpatialShapeHit<T>* hl = q.cast + (size_t)qi * q.cap;
        // entry distance of the cast ray (+inf = culled: only an entry STRICTLY above the best distance culls, so a collider at the best
        // distance with a lower index is still reached)
        auto test = [&](uint32_t node) -> T {
            ++nodes_tested;
            return sp_cast_box(r, hw, sp.bmin[node], sp.bmax[node], MANY ? max_distance : smin(best, max_distance));
        };
        auto leaf = [&](uint32_t c) {
            const uint4 info = sp.info[c];
            if (!sp_leaf_ok(info, mask, self, q.excluded + ex0, ex_n)) return;
            ++leaves_tested;
            T toi; V3<T> p1, p2, n1;
            if (CTRI && info.z == AVN_SHAPE_TRIANGLE) {
                if (!sp_tricol_cast_exact<T, CAPSULE>(s.shape, s.he, iso2, d, max_distance, sp_load_tri<T>(sp_tri(sp), c), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]), toi, p1, p2, n1)) return;
            } else if (CCAP && info.z == AVN_SHAPE_CAPSULE) {
                if (!sp_capcol_cast_exact<T, CAPSULE>(s.shape, s.he, iso2, d, max_distance, xyz<T>(sp.he[c]), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]), toi, p1, p2, n1)) return;
            } else if (CAPSULE) {
                if (!sp_capsule_cast_exact<T>(s.he.x, s.he.y, iso2, d, max_distance, info.z, xyz<T>(sp.he[c]), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]), toi, p1, p2, n1)) return;
            } else if (!sp_cast_exact<T>(s.shape, s.he, iso2, d, max_distance, info.z, xyz<T>(sp.he[c]), xyz<T>(sp.pos[c]), quat<T>(sp.rot[c]), toi, p1, p2, n1)) return;
            if (!MANY) {
                if (toi < best || (toi == best && c < best_c)) { best = toi; best_c = c; best_p1 = p1; best_p2 = p2; best_n1 = n1; }
            } else {
                const uint32_t m = sp_slot_by_distance(hl, kq, found, toi, c);
                if (m == AVN_SPATIAL_MISS) return;
                SpatialShapeHit<T> h;
                sp_put<T>(h, c, info.x, toi, p1, p2, n1);
                hl[m] = h;
            }
        };
        if (valid) sp_walk<T, !MANY>(sp, overflow, best, test, leaf);
        if (!MANY) {
            SpatialShapeHit<T> h;
            sp_put<T>(h, best_c, best_c == AVN_SPATIAL_MISS ? AVN_SPATIAL_MISS : sp.info[best_c].x, best_c == AVN_SPATIAL_MISS ? T(0) : best, best_p1, best_p2, best_n1);
            if (!PQ) q.cast[qi] = h;
            else {
                // the caster's row: the hit or a miss, then misses; count 0 or 1
                hl[0] = h;
                sp_fill_miss(hl, 1u, q.cap);
                q.count[qi] = best_c == AVN_SPATIAL_MISS ? 0u : 1u;
            }
        } else {
            sp_fill_miss(hl, found < kq ? found : kq, q.cap);
            q.count[qi] = found;
        }
    }
    } while (CAPSULE && (base = sp_next_chunk<CAPSULE>(base, q.n)) < q.n);
    sp_add_stats(q.stats, nodes_tested, leaves_tested, overflow);
}

// ---------------------------------------------------------------------------------------------------------
// shape contacts and depenetration.  The header defines a contact; the pair arithmetic is the narrow phase's contact_manifolds_pair_sink,
// untouched.  DESIGN.md 4.4.7.

// one lane per query shape; records inserted in ascending collider index as k_sp_shapes inserts ids
// CTRI, a triangle collider: the narrow phase's triangle manifold (contact_manifolds_pair_sink<.., CAP, TRI>, avn_triangle_pair.h) with the query as shape 1
// -- a Ball, a Cuboid or a Capsule alike -- and the collider's triangle, edge flags included, as tri2; the deepest point is kept
template <class T, bool CAPSULE = false, bool CCAP = false, bool CTRI = false>
__global__ __launch_bounds__(SP_WAVE) void k_sp_contacts(typename SpArg<T, CTRI>::type sp, SC<T> sc) {
    const SQ<T>& q = sc.q;
    uint32_t nodes_tested = 0, leaves_tested = 0, overflow = 0;
    uint32_t base = blockIdx.x * SP_WAVE;
    do {   // (once; a CAPSULE launch: every chunk of this block's stride)
    const uint32_t qi = base + threadIdx.x;
    if (qi < q.n && sp_lane_kind<CAPSULE>(q.shape, qi)) {
        const uint32_t mask = q.mask ? q.mask[qi] : 0xFFFFFFFFu;
        const QShape<T> s = sp_load_shape<T, CAPSULE>(q.shape, q.a, q.he, q.rot, qi);
        const Iso<T> iso2 = make_isometry(s.pos, s.rot);   // (the capsule's pair test; unused otherwise)
        const T pred = sc.prediction ? sc.prediction[qi] : sc.prediction_all;
        const uint32_t self = sc.self_entity ? sc.self_entity[qi] : AVN_SPATIAL_MISS;
        // a valid shape and a prediction distance that is finite and not negative: otherwise count 0
        const bool valid = s.valid && finite_t(pred) && pred >= T(0);
        // (b)'s box: the query shape's exact AABB grown by the prediction; the node test pads it as a leaf box is padded
        const V3<T> pv{pred, pred, pred};
        const V3<T> gmin = s.a - pv, gmax = s.b + pv;
        V3<T> qmin, qmax;
        sp_pad_box(gmin, gmax, qmin, qmax);
        uint32_t found = 0;
        SpatialShapeContact<T>* rl = sc.rec + (size_t)qi * q.cap;
        auto test = [&](uint32_t node) -> T {
            ++nodes_tested;
            return sp_box_box(qmin, qmax, sp.bmin[node], sp.bmax[node]) ? T(0) : sp_inf<T>();
        };
        auto leaf = [&](uint32_t c) {
            const uint4 info = sp.info[c];
            if (!sp_leaf_ok(info, mask, self, q.excluded, q.n_excluded) || (sc.skip_sensors && (info.w & SP_INFO_SENSOR))) return;
            ++leaves_tested;
            const V3<T> pos2 = xyz<T>(sp.pos[c]), he2 = xyz<T>(sp.he[c]);
            const Q4<T> rot2 = quat<T>(sp.rot[c]);
            // (b) the collider's exact box, by the snapshot's own arithmetic
            V3<T> mn, mx;
            shape_aabb<T, CCAP, CTRI>(info.z, he2, pos2, rot2, mn, mx, CTRI ? sp_tri(sp) + 3 * (size_t)c : nullptr);
            if (!sp_box_box(gmin, gmax, make4<T>(mn, T(0)), make4<T>(mx, T(0)))) return;
            // (c), (d)
            SpDeepestSink<T> sink{vzero<T>(), T(0), 0};
            V3<T> nrm, a1, a2;
            if (CTRI && info.z == AVN_SHAPE_TRIANGLE) {
                const NpTri<T> tri = sp_load_tri<T>(sp_tri(sp), c);
                bool ok;
                AVN_INLINE_CALL ok = contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, true, true>(sp_query_kind<CAPSULE>(s.shape), s.he, s.pos, s.rot, AVN_SHAPE_TRIANGLE, he2, pos2, rot2, pred, sink, nrm, nullptr, nullptr, NpTri<T>(), tri);
                if (!ok) return;
                a1 = sink.anchor1; a2 = a1 + (s.pos - pos2);
            } else if (CAPSULE && CCAP && info.z == AVN_SHAPE_CAPSULE) {
                // (two capsules: the narrow phase's capsule-capsule manifold, the query as shape 1)
                if (!contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, true>(AVN_SHAPE_CAPSULE, s.he, s.pos, s.rot, AVN_SHAPE_CAPSULE, he2, pos2, rot2, pred, sink, nrm)) return;
                a1 = sink.anchor1; a2 = a1 + (s.pos - pos2);
            } else if (CAPSULE) {
                // (the capsule's own contact: the normal already points from the collider towards the query)
                V3<T> cn;
                if (!sp_capsule_contact<T>(s.he.x, s.he.y, iso2, info.z, he2, pos2, rot2, pred, sink.penetration, cn, a1, a2)) return;
                nrm = -cn;
            } else {
                // (CTRI: inlined by statement attribute like the triangle manifold above -- left to the inliner this call stayed a real call in the CTRI
                // instantiations, with the sink and the normal in 64 / 192 bytes of scratch memory.  Nothing but the compiler's figures pins this: after a ROCm
                // update re-run the recipe at the head of profiles/spatial_triangle_colliders_resource_usage.txt and look for scratch 0 in every CTRI kernel)
                if constexpr (CTRI) { bool ok; AVN_INLINE_CALL ok = contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, CCAP>(s.shape, s.he, s.pos, s.rot, info.z, he2, pos2, rot2, pred, sink, nrm); if (!ok) return; }
                else if (!contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, CCAP>(s.shape, s.he, s.pos, s.rot, info.z, he2, pos2, rot2, pred, sink, nrm)) return;
                a1 = sink.anchor1; a2 = a1 + (s.pos - pos2);
            }
            const uint32_t m = sp_slot_by_collider(rl, q.cap, found, c);
            if (m == AVN_SPATIAL_MISS) return;
            const V3<T> pt = s.pos + a1;
            SpatialShapeContact<T> r;
            r.collider = c; r.entity = info.x; r.penetration = sink.penetration;
            r.normal[0] = -nrm.x; r.normal[1] = -nrm.y; r.normal[2] = -nrm.z;
            r.point[0] = pt.x; r.point[1] = pt.y; r.point[2] = pt.z;
            r.anchor1[0] = a1.x; r.anchor1[1] = a1.y; r.anchor1[2] = a1.z;
            r.anchor2[0] = a2.x; r.anchor2[1] = a2.y; r.anchor2[2] = a2.z;
            sp_clear_reserved(r);
            rl[m] = r;
        };
        if (valid) sp_walk<T, false>(sp, overflow, T(0), test, leaf);
        if (sc.pad_unused) sp_fill_miss(rl, found, q.cap);
        q.count[qi] = found;
    }
    } while (CAPSULE && (base = sp_next_chunk<CAPSULE>(base, q.n)) < q.n);
    sp_add_stats(q.stats, nodes_tested, leaves_tested, overflow);
}

// Dir is f32: an f64 world rounds every normal component through float (Dir::new_unchecked(-manifold.normal.f32()), adjust_precision())
__device__ __forceinline__ float sp_dir_round(float x) { return x; }
__device__ __forceinline__ double sp_dir_round(double x) { return (double)(float)x; }

// MoveAndSlide::depenetrate_intersections (move_and_slide.rs:982-1009), one lane per query over its contact records
template <class T>
__global__ __launch_bounds__(SP_WAVE) void k_sp_depenetrate(SD<T> d) {
    const uint32_t qi = blockIdx.x * SP_WAVE + threadIdx.x;
    if (qi >= d.n) return;
    const uint32_t count = d.count[qi];
    const uint32_t m = count < AVN_SPATIAL_MAX_HITS ? count : AVN_SPATIAL_MAX_HITS;
    const SpatialShapeContact<T>* rl = d.rec + (size_t)qi * AVN_SPATIAL_MAX_HITS;
    V3<T> fixup = vzero<T>();
    uint32_t it = 0;
    while (it < d.iterations) {
        ++it;
        T total_error = T(0);
        for (uint32_t k = 0; k < m; ++k) {
            const T dist = rl[k].penetration + d.skin_width;
            if (dist > d.rejection) continue;
            const V3<T> nv{sp_dir_round(rl[k].normal[0]), sp_dir_round(rl[k].normal[1]), sp_dir_round(rl[k].normal[2])};
            const T diff = dist - (fixup.x * nv.x + fixup.y * nv.y + fixup.z * nv.z);
            const T error = diff > T(0) ? diff : T(0);
            total_error += error;
            fixup = V3<T>{fixup.x + error * nv.x, fixup.y + error * nv.y, fixup.z + error * nv.z};
        }
        if (total_error < d.max_error) break;
    }
    SpatialDepenetration<T> r;
    r.fixup[0] = fixup.x; r.fixup[1] = fixup.y; r.fixup[2] = fixup.z;
    r.count = count; r.iterations_run = it; r.truncated = count > AVN_SPATIAL_MAX_HITS ? 1u : 0u;
    sp_clear_reserved(r);
    d.out[qi] = r;
}

// CTRI (the `_as` helpers of every launcher): sp is the snapshot with the world's triangle table (SPT), made by the launcher from its `tri` argument
template <class T, bool CCAP, bool CTRI = false> static void launch_spatial_contacts_as(const typename SpArg<T, CTRI>::type& sp, const SC<T>& sc, hipStream_t s, bool capsule) {
    hipLaunchKernelGGL((k_sp_contacts<T, false, CCAP, CTRI>), dim3((sc.q.n + SP_WAVE - 1) / SP_WAVE), dim3(SP_WAVE), 0, s, sp, sc);
    if (capsule) hipLaunchKernelGGL((k_sp_contacts<T, true, CCAP, CTRI>), sp_capsule_grid(sc.q.n), dim3(SP_WAVE), 0, s, sp, sc);
}
// ccap (here and in every launch_spatial_* below): the snapshot holds capsule colliders as candidates -- the CCAP instantiations go
// tri (here and in every launch_spatial_* below): the world's triangle table when the snapshot holds triangle colliders as candidates -- the CTRI
// instantiations go, always with CCAP (a snapshot built with the capsule switch off holds no capsule candidate, so the branch is never taken); nullptr: the
// launches of a world without the triangle switch, exactly as before
template <class T> void launch_spatial_contacts(const SP<T>& sp, const SC<T>& sc, hipStream_t s, bool zero_stats, bool capsule, bool ccap, const Vec4<T>* tri) {
    if (zero_stats) (void)hipMemsetAsync(sc.q.stats, 0, 4 * sizeof(unsigned long long), s);
    if (sc.q.n == 0) return;
    if (tri) launch_spatial_contacts_as<T, true, true>(SPT<T>{sp, tri}, sc, s, capsule);
    else if (ccap) launch_spatial_contacts_as<T, true>(sp, sc, s, capsule);
    else launch_spatial_contacts_as<T, false>(sp, sc, s, capsule);
}
template <class T> void launch_spatial_depenetrate(const SD<T>& d, hipStream_t s) {
    if (d.n == 0) return;
    hipLaunchKernelGGL((k_sp_depenetrate<T>), dim3((d.n + SP_WAVE - 1) / SP_WAVE), dim3(SP_WAVE), 0, s, d);
}

// ---------------------------------------------------------------------------------------------------------
// move and slide.  The header defines project_velocity, cast_move and the loop, operation order included; tests/spatial_move_reference.py
// does the same operations in order.  DESIGN.md 4.4.8.

// Scalar::total_cmp as an integer key
__device__ __forceinline__ long long sp_total_key(float x) { const int b = __float_as_int(x); return b < 0 ? (b ^ 0x7FFFFFFF) : b; }
__device__ __forceinline__ long long sp_total_key(double x) { const long long b = __double_as_longlong(x); return b < 0 ? (b ^ 0x7FFFFFFFFFFFFFFFll) : b; }
template <class T> __device__ __forceinline__ T sp_dot3(V3<T> a, V3<T> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// glam's cross
template <class T> __device__ __forceinline__ V3<T> sp_cross3(V3<T> a, V3<T> b) { return V3<T>{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
template <class T> __device__ __forceinline__ V3<T> sp_plane(const float* __restrict__ p, uint32_t k) { return V3<T>{(T)p[3 * k], (T)p[3 * k + 1], (T)p[3 * k + 2]}; }

// Dir::new_and_length(v as f32): false when the length is not finite or not > 0
template <class T> __device__ __forceinline__ bool sp_dir_and_length(V3<T> v, V3<T>& dir, T& dist) {
    const float x = (float)v.x, y = (float)v.y, z = (float)v.z;
    const float len = sqrt_t(x * x + y * y + z * z);
    if (!(finite_t(len) && len > 0.0f)) return false;
    dir = V3<T>{(T)(x / len), (T)(y / len), (T)(z / len)};
    dist = (T)len;
    return true;
}

// project_velocity (velocity_project.rs:122-324) over the `cnt` normals at nrm (xyz interleaved, f32)
template <class T> __device__ __forceinline__ V3<T> sp_project_velocity(V3<T> v, const float* __restrict__ nrm, uint32_t cnt) {
    bool ok = is_finite(v);
    for (uint32_t k = 0; k < cnt; ++k) ok = ok && finite_t(nrm[3 * k]) && finite_t(nrm[3 * k + 1]) && finite_t(nrm[3 * k + 2]);
    if (!ok) return v;
    const T eps = T(0.005);
    const V3<T> x0{-v.x, -v.y, -v.z};
    V3<T> s = x0, n1 = vzero<T>(), n2 = vzero<T>();
    int cone = 0;   // 0: Origin, 1: Ray(n1), 2: Wedge(n1, n2)
    for (int it = 0; it < 10; ++it) {
        if (sp_dot3(s, s) < eps * eps || cnt == 0) break;
        uint32_t best = 0;
        T best_dot = sp_dot3(sp_plane<T>(nrm, 0), s);
        for (uint32_t k = 1; k < cnt; ++k) {
            const T d = sp_dot3(sp_plane<T>(nrm, k), s);
            if (!(sp_total_key(best_dot) > sp_total_key(d))) { best_dot = d; best = k; }   // the last maximum
        }
        if (best_dot <= eps) break;
        const V3<T> n = sp_plane<T>(nrm, best);
        if (cone == 0) {
            const T d = sp_dot3(n, x0);
            s = V3<T>{x0.x - d * n.x, x0.y - d * n.y, x0.z - d * n.z};
            n1 = n; cone = 1;
        } else if (cone == 1) {
            const V3<T> c = sp_cross3(n, n1);
            const T d = sp_dot3(x0, c), cc = sp_dot3(c, c);
            s = V3<T>{d * c.x / cc, d * c.y / cc, d * c.z / cc};
            if (d > T(0)) { n2 = n1; n1 = n; } else n2 = n;
            cone = 2;
        } else {
            const V3<T> c1 = sp_cross3(n1, n);
            const T q1 = sp_dot3(c1, c1), d1 = sp_dot3(x0, c1);
            const V3<T> c2 = sp_cross3(n, n2);
            const T q2 = sp_dot3(c2, c2), d2 = sp_dot3(x0, c2);
            if (d1 <= T(0) && d2 <= T(0)) { s = vzero<T>(); break; }   // inside the solid wedge
            if (d1 * fabs_t(d1) * q2 > d2 * fabs_t(d2) * q1) { n2 = n; s = V3<T>{d1 * c1.x / q1, d1 * c1.y / q1, d1 * c1.z / q1}; }
            else { n1 = n; s = V3<T>{d2 * c2.x / q2, d2 * c2.y / q2, d2 * c2.z / q2}; }
        }
    }
    return V3<T>{-s.x, -s.y, -s.z};
}

template <class T>
__global__ __launch_bounds__(SP_WAVE) void k_sp_project_velocity(SV<T> p) {
    const uint32_t qi = blockIdx.x * SP_WAVE + threadIdx.x;
    if (qi >= p.n) return;
    const V3<T> v{p.velocity[3 * (size_t)qi], p.velocity[3 * (size_t)qi + 1], p.velocity[3 * (size_t)qi + 2]};
    const uint32_t c = p.count[qi];
    const V3<T> r = sp_project_velocity<T>(v, p.normals + (size_t)qi * p.stride * 3, c < p.stride ? c : p.stride);
    p.out[3 * (size_t)qi] = r.x; p.out[3 * (size_t)qi + 1] = r.y; p.out[3 * (size_t)qi + 2] = r.z;
}

template <class T> __device__ __forceinline__ void sp_put_move(SpatialMoveHit<T>& h, uint32_t c, uint32_t e, T safe, T dist, V3<T> p1, V3<T> p2, V3<T> n1) {
    h.collider = c; h.entity = e; h.distance = safe; h.collision_distance = dist;
    h.point1[0] = p1.x; h.point1[1] = p1.y; h.point1[2] = p1.z;
    h.point2[0] = p2.x; h.point2[1] = p2.y; h.point2[2] = p2.z;
    h.normal1[0] = n1.x; h.normal1[1] = n1.y; h.normal1[2] = n1.z;
    h.normal2[0] = n1.x == T(0) ? T(0) : -n1.x; h.normal2[1] = n1.y == T(0) ? T(0) : -n1.y; h.normal2[2] = n1.z == T(0) ? T(0) : -n1.z;
}

// MoveAndSlide::cast_move in two launches.  k_sp_cast_move is k_sp_cast's closest-hit traversal over the ordinary hits; a collider that
// overlaps the query at the start is only noted in the query's pending list.  k_sp_cast_move_resolve, one lane per query and no traversal,
// applies the origin-penetration rule to the pending colliders with the narrow phase's contact_manifolds_pair_sink, merges them with the
// traversal's hit by (distance, collider index) and pulls the distance back.  The contact manifold so stays out of the traversal's live
// range (fused into the leaf the kernel needed 256 VGPRs + 13 / 72 AGPRs, one wave per SIMD: profiles/spatial_moves_resource_usage.txt).
template <class T, bool CAPSULE = false, bool CCAP = false, bool CTRI = false>
__global__ __launch_bounds__(SP_WAVE) void k_sp_cast_move(typename SpArg<T, CTRI>::type sp, SM<T> m) {
    const SQ<T>& q = m.q;
    uint32_t nodes_tested = 0, leaves_tested = 0, overflow = 0;
    uint32_t base = blockIdx.x * SP_WAVE;
    do {   // (once; a CAPSULE launch: every chunk of this block's stride)
    const uint32_t qi = base + threadIdx.x;
    if (qi < q.n && sp_lane_kind<CAPSULE>(q.shape, qi)) {
        const uint32_t mask = q.mask ? q.mask[qi] : 0xFFFFFFFFu;
        const uint32_t self = m.self_entity ? m.self_entity[qi] : AVN_SPATIAL_MISS;
        const QShape<T> s = sp_load_shape<T, CAPSULE>(q.shape, q.a, q.he, q.rot, qi);
        const V3<T> mv = sp_load3(m.movement, qi);
        const T skin = m.skin ? m.skin[qi] : m.skin_all;
        // a valid shape, a finite movement and a skin width that is finite and not negative; a slide's finished character: a miss
        const bool valid = s.valid && is_finite(mv) && finite_t(skin) && skin >= T(0) && (!m.state || (m.state[qi] & SP_SLIDE_LIVE));
        V3<T> d{T(1), T(0), T(0)};
        T dist = T(0);
        if (valid && !sp_dir_and_length<T>(mv, d, dist)) { d = V3<T>{T(1), T(0), T(0)}; dist = T(0); }
        V3<T> hw;
        const RayCtx<T> r = sp_cast_ray(s, d, hw);
        const Iso<T> iso2 = make_isometry(s.pos, s.rot);
        T best = sp_inf<T>();
        uint32_t best_c = AVN_SPATIAL_MISS;
        V3<T> best_p1 = vzero<T>(), best_p2 = vzero<T>(), best_n1 = vzero<T>();
        uint32_t n_pending = 0;
        uint32_t* pend = m.pending + (size_t)qi * AVN_SPATIAL_MAX_HITS;
        auto test = [&](uint32_t node) -> T {
            ++nodes_tested;
            return sp_cast_box(r, hw, sp.bmin[node], sp.bmax[node], smin(best, dist));
        };
        auto leaf = [&](uint32_t c) {
            const uint4 info = sp.info[c];
            if (!sp_leaf_ok(info, mask, self, q.excluded, q.n_excluded) || (info.w & SP_INFO_SENSOR)) return;
            ++leaves_tested;
            const V3<T> pos1 = xyz<T>(sp.pos[c]), he1 = xyz<T>(sp.he[c]);
            const Q4<T> rot1 = quat<T>(sp.rot[c]);
            T toi; V3<T> p1, p2, n1;
            if (CTRI && info.z == AVN_SHAPE_TRIANGLE) {
                if (!sp_tricol_cast_exact<T, CAPSULE>(s.shape, s.he, iso2, d, dist, sp_load_tri<T>(sp_tri(sp), c), pos1, rot1, toi, p1, p2, n1)) return;
            } else if (CCAP && info.z == AVN_SHAPE_CAPSULE) {
                if (!sp_capcol_cast_exact<T, CAPSULE>(s.shape, s.he, iso2, d, dist, he1, pos1, rot1, toi, p1, p2, n1)) return;
            } else if (CAPSULE) {
                if (!sp_capsule_cast_exact<T>(s.he.x, s.he.y, iso2, d, dist, info.z, he1, pos1, rot1, toi, p1, p2, n1)) return;
            } else if (!sp_cast_exact<T>(s.shape, s.he, iso2, d, dist, info.z, he1, pos1, rot1, toi, p1, p2, n1)) return;
            if (toi == T(0) && n1.x == T(0) && n1.y == T(0) && n1.z == T(0)) {
                // overlapping at the start: the pair's contact decides, in k_sp_cast_move_resolve
                if (n_pending < AVN_SPATIAL_MAX_HITS) pend[n_pending] = c;
                else overflow |= 2u;
                ++n_pending;
                return;
            }
            if (toi < best || (toi == best && c < best_c)) { best = toi; best_c = c; best_p1 = p1; best_p2 = p2; best_n1 = n1; }
        };
        if (valid) sp_walk<T, true>(sp, overflow, best, test, leaf);
        // the traversal's own answer (the hit's distance, not yet pulled back) and the pending count: k_sp_cast_move_resolve finishes the record
        SpatialMoveHit<T> h;
        if (best_c == AVN_SPATIAL_MISS) sp_put_move<T>(h, AVN_SPATIAL_MISS, AVN_SPATIAL_MISS, T(0), T(0), vzero<T>(), vzero<T>(), vzero<T>());
        else sp_put_move<T>(h, best_c, sp.info[best_c].x, best, dist, best_p1, best_p2, best_n1);
        m.out[qi] = h;
        m.pending_count[qi] = n_pending;
    }
    } while (CAPSULE && (base = sp_next_chunk<CAPSULE>(base, q.n)) < q.n);
    sp_add_stats(q.stats, nodes_tested, leaves_tested, overflow);
}

template <class T, bool CAPSULE, bool CCAP, bool CTRI> __device__ __forceinline__ void sp_cast_move_resolve_lane(const typename SpArg<T, CTRI>::type& sp, const SM<T>& m, uint32_t qi);
template <class T, bool CAPSULE = false, bool CCAP = false, bool CTRI = false>
__global__ __launch_bounds__(SP_WAVE) void k_sp_cast_move_resolve(typename SpArg<T, CTRI>::type sp, SM<T> m) {
    uint32_t base = blockIdx.x * SP_WAVE;
    do sp_cast_move_resolve_lane<T, CAPSULE, CCAP, CTRI>(sp, m, base + threadIdx.x);
    while (CAPSULE && (base = sp_next_chunk<CAPSULE>(base, m.q.n)) < m.q.n);
}
template <class T, bool CAPSULE, bool CCAP, bool CTRI> __device__ __forceinline__ void sp_cast_move_resolve_lane(const typename SpArg<T, CTRI>::type& sp, const SM<T>& m, uint32_t qi) {
    const SQ<T>& q = m.q;
    if (qi >= q.n || !sp_lane_kind<CAPSULE>(q.shape, qi)) return;
    SpatialMoveHit<T> h = m.out[qi];
    const uint32_t count = m.pending_count[qi];
    const uint32_t np = count < AVN_SPATIAL_MAX_HITS ? count : AVN_SPATIAL_MAX_HITS;
    if (h.collider == AVN_SPATIAL_MISS && np == 0) return;   // a miss, an invalid query, a slide's finished character: the record stands
    const QShape<T> s = sp_load_shape<T, CAPSULE>(q.shape, q.a, q.he, q.rot, qi);   // (valid: k_sp_cast_move hit or noted something)
    const Iso<T> iso2 = make_isometry(s.pos, s.rot);   // (the capsule's pair test; unused otherwise)
    const V3<T> mv = sp_load3(m.movement, qi);
    const T skin = m.skin ? m.skin[qi] : m.skin_all;
    V3<T> d{T(1), T(0), T(0)};
    T dist = T(0);
    if (!sp_dir_and_length<T>(mv, d, dist)) { d = V3<T>{T(1), T(0), T(0)}; dist = T(0); }
    T best = h.collider == AVN_SPATIAL_MISS ? sp_inf<T>() : h.distance;
    uint32_t best_c = h.collider, best_e = h.entity;
    V3<T> best_p1{h.point1[0], h.point1[1], h.point1[2]}, best_p2{h.point2[0], h.point2[1], h.point2[2]}, best_n1{h.normal1[0], h.normal1[1], h.normal1[2]};
    const uint32_t* pend = m.pending + (size_t)qi * AVN_SPATIAL_MAX_HITS;
    for (uint32_t k = 0; k < np; ++k) {
        const uint32_t c = pend[k];
        // a hit at distance 0 only matters when it beats the best by (distance, collider index)
        if (!(T(0) < best || (best == T(0) && c < best_c))) continue;
        const uint4 info = sp.info[c];
        const V3<T> pos1 = xyz<T>(sp.pos[c]), he1 = xyz<T>(sp.he[c]);
        const Q4<T> rot1 = quat<T>(sp.rot[c]);
        // the pair's contact at prediction 0, the query as shape 1
        V3<T> p1 = vzero<T>(), p2 = vzero<T>(), n1 = vzero<T>();
        SpDeepestSink<T> sink{vzero<T>(), T(0), 0};
        V3<T> nrm, a1, a2;
        bool contact;
        if (CTRI && info.z == AVN_SHAPE_TRIANGLE) {
            const NpTri<T> tri = sp_load_tri<T>(sp_tri(sp), c);
            AVN_INLINE_CALL contact = contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, true, true>(sp_query_kind<CAPSULE>(s.shape), s.he, s.pos, s.rot, AVN_SHAPE_TRIANGLE, he1, pos1, rot1, T(0), sink, nrm, nullptr, nullptr, NpTri<T>(), tri);
            a1 = sink.anchor1; a2 = a1 + (s.pos - pos1);
        } else if (CAPSULE && CCAP && info.z == AVN_SHAPE_CAPSULE) {
            contact = contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, true>(AVN_SHAPE_CAPSULE, s.he, s.pos, s.rot, AVN_SHAPE_CAPSULE, he1, pos1, rot1, T(0), sink, nrm);
            a1 = sink.anchor1; a2 = a1 + (s.pos - pos1);
        } else if (CAPSULE) {
            V3<T> cn;
            contact = sp_capsule_contact<T>(s.he.x, s.he.y, iso2, info.z, he1, pos1, rot1, T(0), sink.penetration, cn, a1, a2);
            nrm = -cn;
        } else {
            // (inlined by statement attribute in the CTRI instantiations, as in k_sp_contacts: see the note there and the recipe it names)
            if constexpr (CTRI) { AVN_INLINE_CALL contact = contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, CCAP>(s.shape, s.he, s.pos, s.rot, info.z, he1, pos1, rot1, T(0), sink, nrm); }
            else contact = contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, CCAP>(s.shape, s.he, s.pos, s.rot, info.z, he1, pos1, rot1, T(0), sink, nrm);
            a1 = sink.anchor1; a2 = a1 + (s.pos - pos1);
        }
        if (contact) {
            const V3<T> cn{-nrm.x, -nrm.y, -nrm.z};
            if (d.x * cn.x + d.y * cn.y + d.z * cn.z >= T(0)) continue;   // on its way out: ignored by this cast
            n1 = cn; p1 = pos1 + a2; p2 = s.pos + a1;
        }
        best = T(0); best_c = c; best_e = info.x; best_p1 = p1; best_p2 = p2; best_n1 = n1;
    }
    if (best_c == AVN_SPATIAL_MISS) return;   // every pending collider was ignored and nothing else was hit: the miss stands
    // pull_back: at least skin_width away from the hit along the movement
    T safe = T(0);
    if (dist != T(0)) {
        const T dp = d.x * (-best_n1.x) + d.y * (-best_n1.y) + d.z * (-best_n1.z);
        const T dm = dp > T(0.005) ? dp : T(0.005);
        const T x = best - skin / dm;
        safe = x > T(0) ? x : T(0);
    }
    sp_put_move<T>(h, best_c, best_e, safe, dist, best_p1, best_p2, best_n1);
    m.out[qi] = h;
}

template <class T> __device__ __forceinline__ void sp_log_hit(const SL<T>& l, uint32_t qi, uint32_t collider, uint32_t entity, uint32_t kind, V3<T> point, V3<T> normal, T distance, T collision_distance) {
    const uint32_t k = l.hit_count[qi];
    l.hit_count[qi] = k + 1;
    if (k >= l.hit_cap) return;
    SpatialSlideHit<T> h;
    h.collider = collider; h.entity = entity; h.iteration = l.iteration; h.kind = kind;
    h.point[0] = point.x; h.point[1] = point.y; h.point[2] = point.z;
    h.normal[0] = normal.x; h.normal[1] = normal.y; h.normal[2] = normal.z;
    h.distance = distance; h.collision_distance = collision_distance;
    l.hits[(size_t)qi * l.hit_cap + k] = h;
}

// The phases of MoveAndSlide::move_and_slide (move_and_slide.rs:475-608) between the traversal launches, one lane per character over the state
// the world keeps.  A finished character is inert: its flags lose SP_SLIDE_LIVE, k_sp_cast_move answers it a miss and its prediction distance
// is NaN, so k_sp_contacts answers it count 0, both without traversing.
template <class T, int PHASE>
__global__ __launch_bounds__(SP_WAVE) void k_sp_slide(SL<T> l) {
    const uint32_t qi = blockIdx.x * SP_WAVE + threadIdx.x;
    if (qi >= l.n) return;
    const size_t q3 = 3 * (size_t)qi;
    if (PHASE == SPL_BEGIN) {
        const bool valid = sp_load_shape<T>(l.shape, l.pos_in, l.he, l.rot, qi).valid || sp_load_shape<T, true>(l.shape, l.pos_in, l.he, l.rot, qi).valid;
        for (int i = 0; i < 3; ++i) { l.pos[q3 + i] = l.pos_in[q3 + i]; l.vel[q3 + i] = l.vel_in[q3 + i]; l.movement[q3 + i] = T(0); }
        l.time_left[qi] = l.delta_time;
        l.flags[qi] = valid ? (SP_SLIDE_VALID | SP_SLIDE_LIVE) : 0u;
        l.iters[qi] = 0u; l.hit_count[qi] = 0u; l.plane_count[qi] = 0u;
        l.pred[qi] = T(0);
        return;
    }
    const uint32_t flags = l.flags[qi];
    if (PHASE == SPL_DEPENETRATE) {
        // position += depenetrate_intersections over the contacts of the launch before (k_sp_depenetrate's loop)
        if (!(flags & SP_SLIDE_VALID)) return;
        V3<T> fixup = vzero<T>();
        if (l.depen_iterations) {
            const uint32_t count = l.count[qi];
            const uint32_t m = count < AVN_SPATIAL_MAX_HITS ? count : AVN_SPATIAL_MAX_HITS;
            if (count > AVN_SPATIAL_MAX_HITS) l.flags[qi] = flags | SP_SLIDE_TRUNCATED;
            const SpatialShapeContact<T>* rl = l.rec + (size_t)qi * AVN_SPATIAL_MAX_HITS;
            uint32_t it = 0;
            while (it < l.depen_iterations) {
                ++it;
                T total_error = T(0);
                for (uint32_t k = 0; k < m; ++k) {
                    const T dist = rl[k].penetration + l.skin;
                    if (dist > l.rejection) continue;
                    const V3<T> nv{sp_dir_round(rl[k].normal[0]), sp_dir_round(rl[k].normal[1]), sp_dir_round(rl[k].normal[2])};
                    const T diff = dist - (fixup.x * nv.x + fixup.y * nv.y + fixup.z * nv.z);
                    const T error = diff > T(0) ? diff : T(0);
                    total_error += error;
                    fixup = V3<T>{fixup.x + error * nv.x, fixup.y + error * nv.y, fixup.z + error * nv.z};
                }
                if (total_error < l.max_error) break;
            }
        }
        l.pos[q3] += fixup.x; l.pos[q3 + 1] += fixup.y; l.pos[q3 + 2] += fixup.z;
        return;
    }
    if (PHASE == SPL_END) {
        SpatialSlide<T> r;
        for (int i = 0; i < 3; ++i) { r.position[i] = l.pos[q3 + i]; r.velocity[i] = l.vel[q3 + i]; }
        r.iterations_run = l.iters[qi]; r.hit_count = l.hit_count[qi]; r.flags = (flags & SP_SLIDE_TRUNCATED) ? 1u : 0u;
        sp_clear_reserved(r);
        l.out[qi] = r;
        SpatialSlideHit<T> miss;
        miss.collider = AVN_SPATIAL_MISS; miss.entity = AVN_SPATIAL_MISS; miss.iteration = 0u; miss.kind = 0u;
        for (int i = 0; i < 3; ++i) miss.point[i] = miss.normal[i] = T(0);
        miss.distance = miss.collision_distance = T(0);
        for (uint32_t k = r.hit_count; k < l.hit_cap; ++k) l.hits[(size_t)qi * l.hit_cap + k] = miss;
        return;
    }
    if (!(flags & SP_SLIDE_LIVE)) {
        if (PHASE == SPL_ADVANCE) l.pred[qi] = __builtin_nan("");   // inert: the contacts launch answers count 0 without traversing
        return;
    }
    const V3<T> vel{l.vel[q3], l.vel[q3 + 1], l.vel[q3 + 2]};
    if (PHASE == SPL_SWEEP) {
        const T tl = l.time_left[qi];
        const V3<T> sweep{tl * vel.x, tl * vel.y, tl * vel.z};
        V3<T> dir; T dist;
        l.movement[q3] = sweep.x; l.movement[q3 + 1] = sweep.y; l.movement[q3 + 2] = sweep.z;
        if (!sp_dir_and_length<T>(sweep, dir, dist) || dist < T(1e-4)) { l.flags[qi] = flags & ~SP_SLIDE_LIVE; return; }
        l.iters[qi] += 1u;
        return;
    }
    if (PHASE == SPL_ADVANCE) {
        const SpatialMoveHit<T> h = l.mh[qi];
        const V3<T> sweep{l.movement[q3], l.movement[q3 + 1], l.movement[q3 + 2]};
        const V3<T> pos{l.pos[q3], l.pos[q3 + 1], l.pos[q3 + 2]};
        if (h.collider == AVN_SPATIAL_MISS) {
            // no collision: the full distance, and the loop ends
            l.pos[q3] = pos.x + sweep.x; l.pos[q3 + 1] = pos.y + sweep.y; l.pos[q3 + 2] = pos.z + sweep.z;
            l.flags[qi] = flags & ~SP_SLIDE_LIVE;
            l.pred[qi] = __builtin_nan("");
            return;
        }
        V3<T> dir; T dist;
        (void)sp_dir_and_length<T>(sweep, dir, dist);   // (valid: SPL_SWEEP checked it)
        const V3<T> point{h.point2[0] + pos.x, h.point2[1] + pos.y, h.point2[2] + pos.z};
        const T tl = l.time_left[qi];
        l.time_left[qi] = tl - tl * (h.distance / dist);
        l.pos[q3] = pos.x + dir.x * h.distance; l.pos[q3 + 1] = pos.y + dir.y * h.distance; l.pos[q3 + 2] = pos.z + dir.z * h.distance;
        float* pl = l.planes + (size_t)qi * SP_SLIDE_PLANES * 3;
        for (uint32_t k = 0; k < 3 * l.n_planes; ++k) pl[k] = l.cfg_planes[k];
        const float nx = (float)h.normal1[0], ny = (float)h.normal1[1], nz = (float)h.normal1[2];
        sp_log_hit<T>(l, qi, h.collider, h.entity, 0u, point, V3<T>{(T)nx, (T)ny, (T)nz}, h.distance, h.collision_distance);
        pl[3 * l.n_planes] = nx; pl[3 * l.n_planes + 1] = ny; pl[3 * l.n_planes + 2] = nz;
        l.plane_count[qi] = l.n_planes + 1;
        l.pred[qi] = l.skin * T(2);
        return;
    }
    if (PHASE == SPL_PLANES) {
        const uint32_t count = l.count[qi];
        const uint32_t m = count < AVN_SPATIAL_MAX_HITS ? count : AVN_SPATIAL_MAX_HITS;
        if (count > AVN_SPATIAL_MAX_HITS) l.flags[qi] = flags | SP_SLIDE_TRUNCATED;
        const SpatialShapeContact<T>* rl = l.rec + (size_t)qi * AVN_SPATIAL_MAX_HITS;
        float* pl = l.planes + (size_t)qi * SP_SLIDE_PLANES * 3;
        uint32_t np = l.plane_count[qi];
        const T safe = l.mh[qi].distance, cd = l.mh[qi].collision_distance;
        for (uint32_t k = 0; k < m; ++k) {
            const float nx = (float)rl[k].normal[0], ny = (float)rl[k].normal[1], nz = (float)rl[k].normal[2];
            const V3<T> nv{(T)nx, (T)ny, (T)nz};
            bool similar = false;
            for (uint32_t e = 0; e < np && !similar; ++e) {
                const float ex = pl[3 * e], ey = pl[3 * e + 1], ez = pl[3 * e + 2];
                if ((T)(nx * ex + ny * ey + nz * ez) >= l.threshold) {
                    // keep the more blocking version of the plane
                    if (sp_dot3(nv, vel) < sp_dot3(V3<T>{(T)ex, (T)ey, (T)ez}, vel)) { pl[3 * e] = nx; pl[3 * e + 1] = ny; pl[3 * e + 2] = nz; }
                    similar = true;
                }
            }
            if (similar || np >= l.max_planes) continue;
            sp_log_hit<T>(l, qi, rl[k].collider, rl[k].entity, 1u, V3<T>{rl[k].point[0], rl[k].point[1], rl[k].point[2]}, nv, safe, cd);
            pl[3 * np] = nx; pl[3 * np + 1] = ny; pl[3 * np + 2] = nz;
            ++np;
        }
        l.plane_count[qi] = np;
        const V3<T> pv = sp_project_velocity<T>(vel, pl, np);
        l.vel[q3] = pv.x; l.vel[q3 + 1] = pv.y; l.vel[q3 + 2] = pv.z;
    }
}

template <class T> void launch_spatial_project_velocity(const SV<T>& p, hipStream_t s) {
    if (p.n == 0) return;
    hipLaunchKernelGGL((k_sp_project_velocity<T>), dim3((p.n + SP_WAVE - 1) / SP_WAVE), dim3(SP_WAVE), 0, s, p);
}
template <class T, bool CCAP, bool CTRI = false> static void launch_spatial_cast_move_as(const typename SpArg<T, CTRI>::type& sp, const SM<T>& m, hipStream_t s, bool capsule) {
    hipLaunchKernelGGL((k_sp_cast_move<T, false, CCAP, CTRI>), dim3((m.q.n + SP_WAVE - 1) / SP_WAVE), dim3(SP_WAVE), 0, s, sp, m);
    hipLaunchKernelGGL((k_sp_cast_move_resolve<T, false, CCAP, CTRI>), dim3((m.q.n + SP_WAVE - 1) / SP_WAVE), dim3(SP_WAVE), 0, s, sp, m);
    if (!capsule) return;
    hipLaunchKernelGGL((k_sp_cast_move<T, true, CCAP, CTRI>), sp_capsule_grid(m.q.n), dim3(SP_WAVE), 0, s, sp, m);
    hipLaunchKernelGGL((k_sp_cast_move_resolve<T, true, CCAP, CTRI>), sp_capsule_grid(m.q.n), dim3(SP_WAVE), 0, s, sp, m);
}
template <class T> void launch_spatial_cast_move(const SP<T>& sp, const SM<T>& m, bool zero_stats, hipStream_t s, bool capsule, bool ccap, const Vec4<T>* tri) {
    if (zero_stats) (void)hipMemsetAsync(m.q.stats, 0, 4 * sizeof(unsigned long long), s);
    if (m.q.n == 0) return;
    if (tri) launch_spatial_cast_move_as<T, true, true>(SPT<T>{sp, tri}, m, s, capsule);
    else if (ccap) launch_spatial_cast_move_as<T, true>(sp, m, s, capsule);
    else launch_spatial_cast_move_as<T, false>(sp, m, s, capsule);
}
template <class T> void launch_spatial_slide_phase(const SL<T>& l, int phase, hipStream_t s) {
    if (l.n == 0) return;
    const dim3 g((l.n + SP_WAVE - 1) / SP_WAVE), b(SP_WAVE);
    switch (phase) {
        case SPL_BEGIN: hipLaunchKernelGGL((k_sp_slide<T, SPL_BEGIN>), g, b, 0, s, l); break;
        case SPL_DEPENETRATE: hipLaunchKernelGGL((k_sp_slide<T, SPL_DEPENETRATE>), g, b, 0, s, l); break;
        case SPL_SWEEP: hipLaunchKernelGGL((k_sp_slide<T, SPL_SWEEP>), g, b, 0, s, l); break;
        case SPL_ADVANCE: hipLaunchKernelGGL((k_sp_slide<T, SPL_ADVANCE>), g, b, 0, s, l); break;
        case SPL_PLANES: hipLaunchKernelGGL((k_sp_slide<T, SPL_PLANES>), g, b, 0, s, l); break;
        default: hipLaunchKernelGGL((k_sp_slide<T, SPL_END>), g, b, 0, s, l); break;
    }
}

// ---------------------------------------------------------------------------------------------------------
// casters: one thread per caster re-aims it from its anchor's pose, in the header's operation order.  The anchors were checked
// against the tables by the host (world/spatial.hpp: casters_run) before the launch.
template <class T>
__global__ __launch_bounds__(256) void k_sp_reaim(DW<T> w, SP<T> sp, SCA<T> c) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const uint32_t kind = c.anchor_kind[i], a = c.anchor[i];
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    V3<T> go{c.origin[i3], c.origin[i3 + 1], c.origin[i3 + 2]};
    float gd[3] = {c.direction[i3], c.direction[i3 + 1], c.direction[i3 + 2]};
    Q4<T> gr{T(0), T(0), T(0), T(1)};
    if (c.shape_rotation) gr = Q4<T>{c.shape_rotation[i4], c.shape_rotation[i4 + 1], c.shape_rotation[i4 + 2], c.shape_rotation[i4 + 3]};
    if (kind != AVN_SPATIAL_ANCHOR_WORLD) {   // (a world anchor: the local values, bit for bit)
        const bool body = kind == AVN_SPATIAL_ANCHOR_BODY;
        const V3<T> pos = body ? xyz<T>(w.pos[a]) : xyz<T>(sp.pos[a]);
        const Q4<T> rot = body ? quat<T>(w.rot[a]) : quat<T>(sp.rot[a]);
        go = pos + qrot(rot, go);
        const V3<T> d = qrot(rot, V3<T>{(T)gd[0], (T)gd[1], (T)gd[2]});
        gd[0] = (float)d.x; gd[1] = (float)d.y; gd[2] = (float)d.z;
        gr = qmul(gr, rot);
    }
    c.g_origin[i3] = go.x; c.g_origin[i3 + 1] = go.y; c.g_origin[i3 + 2] = go.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) { c.g_direction[i3 + k] = gd[k]; c.g_direction_t[i3 + k] = (T)gd[k]; }
    if (c.g_rotation) { c.g_rotation[i4] = gr.x; c.g_rotation[i4 + 1] = gr.y; c.g_rotation[i4 + 2] = gr.z; c.g_rotation[i4 + 3] = gr.w; }
}
template <class T> void launch_spatial_reaim(const DW<T>& w, const SP<T>& sp, const SCA<T>& c, hipStream_t s) {
    if (c.n == 0) return;
    hipLaunchKernelGGL((k_sp_reaim<T>), dim3((c.n + 255) / 256), dim3(256), 0, s, w, sp, c);
}
template <class T, bool CCAP, bool CTRI = false> static void launch_spatial_casters_as(const typename SpArg<T, CTRI>::type& sp, const SQ<T>& q, int kind, hipStream_t s, bool capsule) {
    const dim3 g((q.n + SP_WAVE - 1) / SP_WAVE), b(SP_WAVE);
    switch (kind) {
        case SPQ_CLOSEST: hipLaunchKernelGGL((k_sp_query<T, SPQ_CLOSEST, true, CCAP, CTRI>), g, b, 0, s, sp, q); break;
        case SPQ_HITS: hipLaunchKernelGGL((k_sp_query<T, SPQ_HITS, true, CCAP, CTRI>), g, b, 0, s, sp, q); break;
        case SPQ_CAST:
            hipLaunchKernelGGL((k_sp_cast<T, false, true, false, CCAP, CTRI>), g, b, 0, s, sp, q);
            if (capsule) hipLaunchKernelGGL((k_sp_cast<T, false, true, true, CCAP, CTRI>), sp_capsule_grid(q.n), b, 0, s, sp, q);
            break;
        default:
            hipLaunchKernelGGL((k_sp_cast<T, true, true, false, CCAP, CTRI>), g, b, 0, s, sp, q);
            if (capsule) hipLaunchKernelGGL((k_sp_cast<T, true, true, true, CCAP, CTRI>), sp_capsule_grid(q.n), b, 0, s, sp, q);
            break;
    }
}
template <class T> void launch_spatial_casters(const SP<T>& sp, const SQ<T>& q, int kind, hipStream_t s, bool capsule, bool ccap, const Vec4<T>* tri) {
    if (q.n == 0) return;
    if (tri) launch_spatial_casters_as<T, true, true>(SPT<T>{sp, tri}, q, kind, s, capsule);
    else if (ccap) launch_spatial_casters_as<T, true>(sp, q, kind, s, capsule);
    else launch_spatial_casters_as<T, false>(sp, q, kind, s, capsule);
}

// capsule (SPQ_SHAPES / SPQ_CAST / SPQ_CAST_HITS): the call may hold AVN_SHAPE_CAPSULE query shapes -- the CAPSULE instantiation runs behind the
// first launch on the same stream and answers exactly those lanes
template <class T, bool CCAP, bool CTRI = false> static void launch_spatial_query_as(const typename SpArg<T, CTRI>::type& sp, const SQ<T>& q, int kind, hipStream_t s, bool capsule) {
    const dim3 g((q.n + SP_WAVE - 1) / SP_WAVE), b(SP_WAVE);
    switch (kind) {
        case SPQ_CLOSEST: hipLaunchKernelGGL((k_sp_query<T, SPQ_CLOSEST, false, CCAP, CTRI>), g, b, 0, s, sp, q); break;
        case SPQ_HITS: hipLaunchKernelGGL((k_sp_query<T, SPQ_HITS, false, CCAP, CTRI>), g, b, 0, s, sp, q); break;
        case SPQ_POINTS: hipLaunchKernelGGL((k_sp_query<T, SPQ_POINTS, false, CCAP, CTRI>), g, b, 0, s, sp, q); break;
        case SPQ_PROJECT: hipLaunchKernelGGL((k_sp_project<T, CCAP, CTRI>), g, b, 0, s, sp, q); break;
        case SPQ_SHAPES:
            hipLaunchKernelGGL((k_sp_shapes<T, false, CCAP, CTRI>), g, b, 0, s, sp, q);
            if (capsule) hipLaunchKernelGGL((k_sp_shapes<T, true, CCAP, CTRI>), sp_capsule_grid(q.n), b, 0, s, sp, q);
            break;
        case SPQ_CAST:
            hipLaunchKernelGGL((k_sp_cast<T, false, false, false, CCAP, CTRI>), g, b, 0, s, sp, q);
            if (capsule) hipLaunchKernelGGL((k_sp_cast<T, false, false, true, CCAP, CTRI>), sp_capsule_grid(q.n), b, 0, s, sp, q);
            break;
        case SPQ_CAST_HITS:
            hipLaunchKernelGGL((k_sp_cast<T, true, false, false, CCAP, CTRI>), g, b, 0, s, sp, q);
            if (capsule) hipLaunchKernelGGL((k_sp_cast<T, true, false, true, CCAP, CTRI>), sp_capsule_grid(q.n), b, 0, s, sp, q);
            break;
        default: hipLaunchKernelGGL((k_sp_query<T, SPQ_AABBS, false, CCAP, CTRI>), g, b, 0, s, sp, q); break;
    }
}
template <class T> void launch_spatial_query(const SP<T>& sp, const SQ<T>& q, int kind, hipStream_t s, bool capsule, bool ccap, const Vec4<T>* tri) {
    (void)hipMemsetAsync(q.stats, 0, 4 * sizeof(unsigned long long), s);
    if (q.n == 0) return;
    if (tri) launch_spatial_query_as<T, true, true>(SPT<T>{sp, tri}, q, kind, s, capsule);
    else if (ccap) launch_spatial_query_as<T, true>(sp, q, kind, s, capsule);
    else launch_spatial_query_as<T, false>(sp, q, kind, s, capsule);
}

static_assert(sizeof(SpatialHit<float>) == sizeof(avn_spatial_hit_f32) && sizeof(SpatialHit<double>) == sizeof(avn_spatial_hit_f64), "hit record layout");
static_assert(sizeof(SpatialProjection<float>) == sizeof(avn_spatial_projection_f32) && sizeof(SpatialProjection<double>) == sizeof(avn_spatial_projection_f64) &&
              offsetof(SpatialProjection<double>, point) == offsetof(avn_spatial_projection_f64, point) && offsetof(SpatialProjection<double>, reserved) == offsetof(avn_spatial_projection_f64, reserved) && offsetof(SpatialProjection<float>, distance) == offsetof(avn_spatial_projection_f32, distance),
              "projection record layout");
static_assert(sizeof(SpatialShapeHit<float>) == sizeof(avn_spatial_shape_hit_f32) && sizeof(SpatialShapeHit<double>) == sizeof(avn_spatial_shape_hit_f64) &&
              sizeof(avn_spatial_shape_hit_f32) == 60 && sizeof(avn_spatial_shape_hit_f64) == 112 &&
              offsetof(SpatialShapeHit<float>, distance) == offsetof(avn_spatial_shape_hit_f32, distance) && offsetof(SpatialShapeHit<double>, distance) == offsetof(avn_spatial_shape_hit_f64, distance) &&
              offsetof(SpatialShapeHit<float>, point2) == offsetof(avn_spatial_shape_hit_f32, point2) && offsetof(SpatialShapeHit<double>, point2) == offsetof(avn_spatial_shape_hit_f64, point2) &&
              offsetof(SpatialShapeHit<float>, normal2) == offsetof(avn_spatial_shape_hit_f32, normal2) && offsetof(SpatialShapeHit<double>, normal2) == offsetof(avn_spatial_shape_hit_f64, normal2),
              "shape hit record layout");
static_assert(sizeof(SpatialShapeContact<float>) == sizeof(avn_spatial_shape_contact_f32) && sizeof(SpatialShapeContact<double>) == sizeof(avn_spatial_shape_contact_f64) &&
              sizeof(avn_spatial_shape_contact_f32) == 60 && sizeof(avn_spatial_shape_contact_f64) == 120 &&
              offsetof(SpatialShapeContact<float>, penetration) == offsetof(avn_spatial_shape_contact_f32, penetration) && offsetof(SpatialShapeContact<double>, penetration) == offsetof(avn_spatial_shape_contact_f64, penetration) &&
              offsetof(SpatialShapeContact<float>, point) == offsetof(avn_spatial_shape_contact_f32, point) && offsetof(SpatialShapeContact<double>, point) == offsetof(avn_spatial_shape_contact_f64, point) &&
              offsetof(SpatialShapeContact<float>, anchor2) == offsetof(avn_spatial_shape_contact_f32, anchor2) && offsetof(SpatialShapeContact<double>, anchor2) == offsetof(avn_spatial_shape_contact_f64, anchor2) &&
              offsetof(SpatialShapeContact<double>, reserved) == offsetof(avn_spatial_shape_contact_f64, reserved),
              "shape contact record layout");
static_assert(sizeof(SpatialDepenetration<float>) == sizeof(avn_spatial_depenetration_f32) && sizeof(SpatialDepenetration<double>) == sizeof(avn_spatial_depenetration_f64) &&
              sizeof(avn_spatial_depenetration_f32) == 24 && sizeof(avn_spatial_depenetration_f64) == 40 &&
              offsetof(SpatialDepenetration<float>, truncated) == offsetof(avn_spatial_depenetration_f32, truncated) && offsetof(SpatialDepenetration<double>, truncated) == offsetof(avn_spatial_depenetration_f64, truncated),
              "depenetration record layout");
static_assert(sizeof(SpatialMoveHit<float>) == sizeof(avn_spatial_move_hit_f32) && sizeof(SpatialMoveHit<double>) == sizeof(avn_spatial_move_hit_f64) &&
              sizeof(avn_spatial_move_hit_f32) == 64 && sizeof(avn_spatial_move_hit_f64) == 120 &&
              offsetof(SpatialMoveHit<float>, collision_distance) == offsetof(avn_spatial_move_hit_f32, collision_distance) && offsetof(SpatialMoveHit<double>, collision_distance) == offsetof(avn_spatial_move_hit_f64, collision_distance) &&
              offsetof(SpatialMoveHit<float>, point2) == offsetof(avn_spatial_move_hit_f32, point2) && offsetof(SpatialMoveHit<double>, point2) == offsetof(avn_spatial_move_hit_f64, point2) &&
              offsetof(SpatialMoveHit<float>, normal2) == offsetof(avn_spatial_move_hit_f32, normal2) && offsetof(SpatialMoveHit<double>, normal2) == offsetof(avn_spatial_move_hit_f64, normal2),
              "move hit record layout");
static_assert(sizeof(SpatialSlideHit<float>) == sizeof(avn_spatial_slide_hit_f32) && sizeof(SpatialSlideHit<double>) == sizeof(avn_spatial_slide_hit_f64) &&
              sizeof(avn_spatial_slide_hit_f32) == 48 && sizeof(avn_spatial_slide_hit_f64) == 80 &&
              offsetof(SpatialSlideHit<float>, point) == offsetof(avn_spatial_slide_hit_f32, point) && offsetof(SpatialSlideHit<double>, point) == offsetof(avn_spatial_slide_hit_f64, point) &&
              offsetof(SpatialSlideHit<float>, collision_distance) == offsetof(avn_spatial_slide_hit_f32, collision_distance) && offsetof(SpatialSlideHit<double>, collision_distance) == offsetof(avn_spatial_slide_hit_f64, collision_distance),
              "slide hit record layout");
static_assert(sizeof(SpatialSlide<float>) == sizeof(avn_spatial_slide_f32) && sizeof(SpatialSlide<double>) == sizeof(avn_spatial_slide_f64) &&
              sizeof(avn_spatial_slide_f32) == 36 && sizeof(avn_spatial_slide_f64) == 64 &&
              offsetof(SpatialSlide<float>, flags) == offsetof(avn_spatial_slide_f32, flags) && offsetof(SpatialSlide<double>, flags) == offsetof(avn_spatial_slide_f64, flags) &&
              offsetof(SpatialSlide<double>, reserved) == offsetof(avn_spatial_slide_f64, reserved),
              "slide record layout");
static_assert(SP_SLIDE_PLANES >= AVN_SPATIAL_MAX_PLANES + 1, "plane slots");
template void launch_spatial_build<float>(const DW<float>&, const BP<float>&, const SP<float>&, hipStream_t, bool, bool, bool);
template void launch_spatial_build<double>(const DW<double>&, const BP<double>&, const SP<double>&, hipStream_t, bool, bool, bool);
template void launch_spatial_query<float>(const SP<float>&, const SQ<float>&, int, hipStream_t, bool, bool, const Vec4<float>*);
template void launch_spatial_query<double>(const SP<double>&, const SQ<double>&, int, hipStream_t, bool, bool, const Vec4<double>*);
template void launch_spatial_reaim<float>(const DW<float>&, const SP<float>&, const SCA<float>&, hipStream_t);
template void launch_spatial_reaim<double>(const DW<double>&, const SP<double>&, const SCA<double>&, hipStream_t);
template void launch_spatial_casters<float>(const SP<float>&, const SQ<float>&, int, hipStream_t, bool, bool, const Vec4<float>*);
template void launch_spatial_casters<double>(const SP<double>&, const SQ<double>&, int, hipStream_t, bool, bool, const Vec4<double>*);
template void launch_spatial_contacts<float>(const SP<float>&, const SC<float>&, hipStream_t, bool, bool, bool, const Vec4<float>*);
template void launch_spatial_contacts<double>(const SP<double>&, const SC<double>&, hipStream_t, bool, bool, bool, const Vec4<double>*);
template void launch_spatial_project_velocity<float>(const SV<float>&, hipStream_t);
template void launch_spatial_project_velocity<double>(const SV<double>&, hipStream_t);
template void launch_spatial_cast_move<float>(const SP<float>&, const SM<float>&, bool, hipStream_t, bool, bool, const Vec4<float>*);
template void launch_spatial_cast_move<double>(const SP<double>&, const SM<double>&, bool, hipStream_t, bool, bool, const Vec4<double>*);
template void launch_spatial_slide_phase<float>(const SL<float>&, int, hipStream_t);
template void launch_spatial_slide_phase<double>(const SL<double>&, int, hipStream_t);
template void launch_spatial_depenetrate<float>(const SD<float>&, hipStream_t);
template void launch_spatial_depenetrate<double>(const SD<double>&, hipStream_t);

}  // namespace avn
