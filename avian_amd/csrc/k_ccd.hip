// k_ccd.hip — swept CCD (solve_swept_ccd, dynamics/ccd/mod.rs:523-687; SweepMode::Linear and NonLinear) as a parallel pass over the contact rows of the
// device closed loop (include/avian_mi355x_ccd.h has the definition).  The reference's loop is serial (`// TODO: Parallelize.`): per SweptCcd
// entity it walks the ContactGraph's edges of the body's collider, keeps the smallest time of impact and then rewinds both bodies.  Here:
//
//   k_ccd_begin        records, per-entry minima and the write list back to their empty state; the candidate counter and the statistics to 0
//   k_ccd_candidates   one lane per contact row: a live row with a CCD collider in slot 1 / slot 2 appends (row, entry, side), one atomic per wave
//   k_ccd_toi          one lane per candidate, blocks of one wave (the swept SAT is register-heavy, as in k_sp_cast): the reference's filters,
//                      the header's shape cast of the other collider against the CCD body's own along v2 - v1 with max_distance = dt; an
//                      accepted time (0 < t < dt) goes into the entry's minimum by an integer atomicMin on its bits (positive floats order
//                      as unsigned integers); t == 0 is left to k_ccd_origin
//   k_ccd_origin       only with a bounded default_speculative_margin: the ORIGIN-PENETRATION RULE for the candidates that start overlapping
//                      (the pair's contact at prediction 0, then the "small ball" fallback); a kernel of its own so that the manifold stays
//                      out of the cast's live range, as k_sp_cast_move_resolve does it
//   k_ccd_toi_nl       only when the list in force has a SweepMode::NonLinear entry (k_ccd_toi then skips the NonLinear pairs, rule N0): the
//                      header's conservative advancement N1 - N3 over both bodies' linear and angular motion, at most CCD_NL_ROUNDS rounds; the
//                      same atomicMin; the statistics of avn_swept_ccd_stats_get go into the spare words of CCD::ctr
//   k_ccd_origin_nl    its t == 0 pairs with a bounded margin: the contact at prediction 0, then the small ball by the same advancement (N4)
//   k_ccd_toi_cap, k_ccd_toi_nl_cap, k_ccd_origin_nl_cap, k_ccd_origin_cap
//                      only with avn_swept_ccd_capsules_set on and a capsule in the collider table, behind the four above: the same for the pairs
//                      with an AVN_SHAPE_CAPSULE collider (the casts of the capsule query / the capsule collider, sp_nl_gap_cap, the capsule manifold)
//   k_ccd_pick         among the candidates whose time equals the entry's minimum: atomicMin of (incoming << 63 | ~seq), which is the
//                      position of the edge in the reference's `neighbors` order (outgoing edges newest first, then incoming newest first)
//   k_ccd_resolve      the one candidate that holds both minima writes the entry's record and its two writes (target body, 2 entry + side)
//   (stable radix sort of the writes by target body: a body's writes end up in list order)
//   k_ccd_apply        one lane per segment head applies its body's writes in order: delta_position = t' v (the last one stays),
//                      delta_rotation = from_scaled_axis(omega t') * delta_rotation, t' = t * 1.0001
//
// Nothing is read back and no float atomic is used: every result is independent of the order in which lanes arrive.
#include <algorithm>

#include "avn_spatial_pair.h"
#include "avn_capsule_pair.h"   // capsule colliders: the CAP instantiation of contact_manifolds_pair_sink (k_ccd_origin_cap, k_ccd_origin_nl_cap)

namespace avn {

#define CCD_WAVE 64
#define CCD_KEY_MASK 0x7FFFFFFFFFFFFFFFull

__device__ __forceinline__ unsigned long long ccd_bits(float t) { return (unsigned long long)__float_as_uint(t); }
__device__ __forceinline__ unsigned long long ccd_bits(double t) { return (unsigned long long)__double_as_longlong(t); }
__device__ __forceinline__ float ccd_unbits(unsigned long long b, float) { return __uint_as_float((uint32_t)b); }
__device__ __forceinline__ double ccd_unbits(unsigned long long b, double) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ void ccd_clear_reserved(SweptCcdResult<float>&) {}
__device__ __forceinline__ void ccd_clear_reserved(SweptCcdResult<double>& r) { r.reserved = 0u; }

template <class T>
__global__ __launch_bounds__(256) void k_ccd_own(BP<T> bp, CCD<T> c, uint32_t n_bodies) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= bp.n_colliders) return;
    const uint32_t body = bp.col_info[slot].y;
    const bool child = bp.col_lpos && bp.col_lpos[slot].w != T(0);
    if (!child && body < n_bodies) atomicMin(&c.own[body], slot);
}
template <class T>
__global__ __launch_bounds__(256) void k_ccd_entry(CCD<T> c) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    const uint32_t slot = c.own[c.body[i]];
    if (slot != CCD_NONE) c.entry[slot] = i;   // (a body is listed once: no two entries write one slot)
}

template <class T>
__global__ __launch_bounds__(256) void k_ccd_begin(CCD<T> c, uint32_t n_bodies) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) { c.ctr[CCD_CTR_CAND] = 0u; c.ctr[CCD_CTR_NL_TESTED] = 0u; c.ctr[CCD_CTR_ROUNDS_MAX] = 0u; c.ctr[CCD_CTR_EXHAUSTED] = 0u; }
    if (i < c.n) {
        SweptCcdResult<T> r;
        r.toi = T(0); r.hit_collider = CCD_NONE; r.hit_body = -1; r.tested = 0u;
        ccd_clear_reserved(r);
        c.rec[i] = r;
        c.min_t[i] = CCD_T_NONE; c.min_key[i] = CCD_T_NONE;
    }
    if (i < 2u * c.n) { c.wkey_a[i] = n_bodies; c.wval_a[i] = i; }
}

template <class T>
__global__ __launch_bounds__(256) void k_ccd_candidates(CT<T> ct, CCD<T> c, uint32_t n_rows, uint32_t n_colliders) {
    const uint32_t row = blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t e1 = CCD_NONE, e2 = CCD_NONE;
    if (row < n_rows) {
        const uint4 m = ct.meta[row];
        if ((m.z & AVN_CP_ROW_USED) && m.x < n_colliders && m.y < n_colliders) { e1 = c.entry[m.x]; e2 = c.entry[m.y]; }
    }
    const uint32_t cnt = (e1 != CCD_NONE ? 1u : 0u) + (e2 != CCD_NONE ? 1u : 0u);
    // the wave's candidates take one range of the list: an inclusive scan of the lanes' counts, one atomic by the last lane
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(incl, off); if ((int)lane >= off) incl += v; }
    const uint32_t total = __shfl(incl, 63);
    if (total == 0u) return;
    uint32_t base = 0u;
    if (lane == 63u) base = atomicAdd(&c.ctr[0], total);
    base = __shfl(base, 63);
    uint32_t pos = base + incl - cnt;
    if (e1 != CCD_NONE) { if (pos < c.cand_cap) c.cand[pos] = make_uint2(row, e1 << 1); ++pos; }
    if (e2 != CCD_NONE) { if (pos < c.cand_cap) c.cand[pos] = make_uint2(row, (e2 << 1) | 1u); }
}

// what a candidate's pair test reads: the CCD body's own collider (1) and the other collider (2) at their bodies' step-start poses
template <class T> struct CcdPair {
    uint32_t e, b1, b2, shape1, shape2;
    V3<T> he1, he2, pos1, pos2, d;
    Q4<T> rot1, rot2;
};
// the reference's filters, in its order; false: the pair is not tested.  CAP (the _cap kernels): AVN_SHAPE_CAPSULE passes, AVN_SHAPE_HOST does not
template <class T, bool CAP = false>
__device__ __forceinline__ bool ccd_pair(const DW<T>& w, const BP<T>& bp, const CT<T>& ct, const CCD<T>& c, uint2 cd, CcdPair<T>& p) {
    const uint4 m = ct.meta[cd.x];
    const uint32_t side = cd.y & 1u;
    p.e = cd.y >> 1;
    const uint32_t c1 = side ? m.y : m.x, c2 = side ? m.x : m.y;
    const uint4 i1 = bp.col_info[c1], i2 = bp.col_info[c2];
    p.b1 = i1.y; p.b2 = i2.y;
    if (p.b1 >= w.n_bodies || p.b2 >= w.n_bodies) return false;
    if (!meta_has_solver_body(w.bmeta[p.b1])) return false;                    // `solver_body: Some(..)`
    if (bp.col_lpos && bp.col_lpos[c2].w != T(0)) return false;                 // a child collider (declared deviation)
    p.shape1 = i1.z & 0xFFu; p.shape2 = i2.z & 0xFFu;
    if constexpr (CAP) { if (p.shape1 == AVN_SHAPE_HOST || p.shape2 == AVN_SHAPE_HOST || p.shape1 > AVN_SHAPE_CAPSULE || p.shape2 > AVN_SHAPE_CAPSULE) return false; }
    else if (p.shape1 > AVN_SHAPE_BALL || p.shape2 > AVN_SHAPE_BALL) return false;   // AVN_SHAPE_HOST, AVN_SHAPE_CAPSULE, AVN_SHAPE_TRIANGLE (declared deviations; kind 4 is above AVN_SHAPE_CAPSULE: the CAP form skips it too)
    const uint32_t bm2 = w.bmeta[p.b2];
    if (!c.include_dynamic[p.e] && meta_rb_type(bm2) == AVN_RB_DYNAMIC) return false;
    const bool has2 = meta_has_solver_body(bm2);
    const V3<T> v1 = xyz<T>(w.sb_lin[p.b1]), o1 = xyz<T>(w.sb_ang[p.b1]);
    const V3<T> v2 = has2 ? xyz<T>(w.sb_lin[p.b2]) : vzero<T>(), o2 = has2 ? xyz<T>(w.sb_ang[p.b2]) : vzero<T>();
    if (length_squared(o1 - o2) < c.ang2[p.e] && length_squared(v1 - v2) < c.lin2[p.e]) return false;
    p.he1 = xyz<T>(bp.col_he[c1]); p.he2 = xyz<T>(bp.col_he[c2]);
    p.pos1 = xyz<T>(w.pos[p.b1]); p.rot1 = quat<T>(w.rot[p.b1]);
    p.pos2 = xyz<T>(w.pos[p.b2]); p.rot2 = quat<T>(w.rot[p.b2]);
    p.d = v2 - v1;
    return true;
}
template <class T> __device__ __forceinline__ void ccd_accept(const CCD<T>& c, uint32_t e, T t, T dt, unsigned long long& bits) {
    if (t > T(0) && t < dt) { bits = ccd_bits(t); atomicMin(&c.min_t[e], bits); }
}

// N0: the pair's mode goes by body (`body2.ccd.is_none_or(..)`): the entry's own mode, or the mode b2 is listed with
template <class T> __device__ __forceinline__ bool ccd_pair_nl(const CCD<T>& c, const CcdPair<T>& p) { return c.mode[p.e] != 0u || c.body_mode[p.b2] != 0u; }   // (0: AVN_SWEEP_LINEAR)

// MIXED: the list in force has NonLinear entries; their pairs are left to k_ccd_toi_nl (which then writes their cand_t)
template <class T, bool MIXED>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_toi(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, bool origin_rule) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        unsigned long long bits = CCD_T_NONE;
        CcdPair<T> p;
        if (ccd_pair<T>(w, bp, ct, c, c.cand[i], p)) {
            if constexpr (MIXED) { if (ccd_pair_nl<T>(c, p)) continue; }
            atomicAdd(&c.rec[p.e].tested, 1u);
            T toi; V3<T> p1, p2, n1;
            if (sp_cast_exact<T>(p.shape2, p.he2, make_isometry(p.pos2, p.rot2), p.d, dt, p.shape1, p.he1, p.pos1, p.rot1, toi, p1, p2, n1)) {
                // t == 0 (overlapping or touching at the start): with an unbounded margin the fallback's ball contains the collider for the whole
                // motion and answers nothing, whatever the contact says
                if (toi == T(0)) { if (origin_rule) bits = CCD_T_ORIGIN; }
                else ccd_accept<T>(c, p.e, toi, dt, bits);
            }
        }
        c.cand_t[i] = bits;
    }
}

template <class T>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_origin(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, T margin) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        if (c.cand_t[i] != CCD_T_ORIGIN) continue;
        unsigned long long bits = CCD_T_NONE;
        CcdPair<T> p;
        if (ccd_pair<T>(w, bp, ct, c, c.cand[i], p)) {
            // the pair's contact at prediction 0 with the cast shape (2) as shape 1: n = -manifold.normal points from the CCD collider towards it
            SpDeepestSink<T> sink{vzero<T>(), T(0), 0};
            V3<T> nrm;
            const V3<T> hq = p.shape2 == AVN_SHAPE_BALL ? V3<T>{p.he2.x, p.he2.x, p.he2.x} : p.he2;
            bool leaving = false;
            if (contact_manifolds_pair_sink<T, SpDeepestSink<T>>(p.shape2, hq, p.pos2, p.rot2, p.shape1, p.he1, p.pos1, p.rot1, T(0), sink, nrm)) {
                const V3<T> cn{-nrm.x, -nrm.y, -nrm.z};
                leaving = p.d.x * cn.x + p.d.y * cn.y + p.d.z * cn.z >= T(0);
            }
            if (!leaving) {
                // the reference's "small ball": radius default_speculative_margin at body 2's position
                T toi; V3<T> p1, p2, n1;
                if (sp_cast_exact<T>(AVN_SHAPE_BALL, V3<T>{margin, margin, margin}, make_isometry(p.pos2, p.rot2), p.d, dt, p.shape1, p.he1, p.pos1, p.rot1, toi, p1, p2, n1))
                    ccd_accept<T>(c, p.e, toi, dt, bits);
            }
        }
        c.cand_t[i] = bits;
    }
}

// ---- SweepMode::NonLinear (the header's N1 - N4) ----
// N1: a body's motion over the step, always evaluated from its step-start pose
template <class T> struct CcdMotion { V3<T> c0, v, om, com; Q4<T> rot; T R; };
template <class T> __device__ __forceinline__ T ccd_rho(uint32_t shape, V3<T> he) { return shape == AVN_SHAPE_BALL ? he.x : length(he); }
template <class T> __device__ __forceinline__ CcdMotion<T> ccd_motion(const DW<T>& w, uint32_t b, V3<T> pos, Q4<T> rot, T rho) {
    CcdMotion<T> m;
    const bool has = meta_has_solver_body(w.bmeta[b]);
    m.v = has ? xyz<T>(w.sb_lin[b]) : vzero<T>();
    m.om = has ? xyz<T>(w.sb_ang[b]) : vzero<T>();
    m.com = xyz<T>(w.com[b]);
    m.rot = rot;
    m.c0 = pos + qrot(rot, m.com);
    m.R = length(m.com) + rho;
    return m;
}
template <class T> __device__ __forceinline__ void ccd_pose(const CcdMotion<T>& m, T t, V3<T>& p, Q4<T>& q) {
    q = qmul(from_scaled_axis(m.om * t), m.rot);
    p = (m.c0 + t * m.v) - qrot(q, m.com);
}
// N3: conservative advancement from t = 0.  1: a hit at t_out, 0: a miss, 2: out of rounds (answers nothing)
template <class T, bool CAP = false>
__device__ __forceinline__ int ccd_nl_advance(uint32_t shape1, V3<T> he1, const CcdMotion<T>& m1, uint32_t shape2, V3<T> he2, const CcdMotion<T>& m2, V3<T> d, T dt, T tol,
                                              T& t_out, uint32_t& rounds) {
    T t = T(0);
    for (uint32_t r = 0; r < CCD_NL_ROUNDS; ++r) {
        rounds = r + 1u;
        V3<T> p1, p2, n;
        Q4<T> q1, q2;
        ccd_pose<T>(m1, t, p1, q1);
        ccd_pose<T>(m2, t, p2, q2);
        T g;
        if constexpr (CAP) g = sp_nl_gap_cap<T>(shape1, he1, p1, q1, shape2, he2, p2, q2, n);
        else g = sp_nl_gap<T>(shape1, he1, p1, q1, shape2, he2, p2, q2, n);
        if (g <= tol) { t_out = t; return 1; }
        const T B = (-dot(d, n) + length(cross(m1.om, n)) * m1.R) + length(cross(m2.om, n)) * m2.R;
        if (!(B > T(0))) return 0;
        const T tn = t + g / B;
        if (tn > dt) return 0;
        if (!(tn > t)) { t_out = t; return 1; }
        t = tn;
    }
    return 2;
}
template <class T> __device__ __forceinline__ void ccd_nl_stats(const CCD<T>& c, int res, uint32_t rounds) {
    atomicMax(&c.ctr[CCD_CTR_ROUNDS_MAX], rounds);
    if (res == 2) atomicAdd(&c.ctr[CCD_CTR_EXHAUSTED], 1u);
}

template <class T>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_toi_nl(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, T tol, bool origin_rule) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        CcdPair<T> p;
        if (!ccd_pair<T>(w, bp, ct, c, c.cand[i], p) || !ccd_pair_nl<T>(c, p)) continue;   // (k_ccd_toi wrote the candidate's cand_t)
        atomicAdd(&c.rec[p.e].tested, 1u);
        atomicAdd(&c.ctr[CCD_CTR_NL_TESTED], 1u);
        const CcdMotion<T> m1 = ccd_motion<T>(w, p.b1, p.pos1, p.rot1, ccd_rho<T>(p.shape1, p.he1));
        const CcdMotion<T> m2 = ccd_motion<T>(w, p.b2, p.pos2, p.rot2, ccd_rho<T>(p.shape2, p.he2));
        T toi = T(0);
        uint32_t rounds = 0u;
        const int res = ccd_nl_advance<T>(p.shape1, p.he1, m1, p.shape2, p.he2, m2, p.d, dt, tol, toi, rounds);
        ccd_nl_stats<T>(c, res, rounds);
        unsigned long long bits = CCD_T_NONE;
        if (res == 1) {
            if (toi == T(0)) { if (origin_rule) bits = CCD_T_ORIGIN_NL; }
            else ccd_accept<T>(c, p.e, toi, dt, bits);
        }
        c.cand_t[i] = bits;
    }
}

// N4: step 4 for the NonLinear pairs that start within the tolerance.  The contact runs first and only `leaving` survives it, so the manifold
// stays out of the advancement loop's live range.
template <class T>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_origin_nl(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, T tol, T margin) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        if (c.cand_t[i] != CCD_T_ORIGIN_NL) continue;
        unsigned long long bits = CCD_T_NONE;
        CcdPair<T> p;
        if (ccd_pair<T>(w, bp, ct, c, c.cand[i], p)) {
            SpDeepestSink<T> sink{vzero<T>(), T(0), 0};
            V3<T> nrm;
            const V3<T> hq = p.shape2 == AVN_SHAPE_BALL ? V3<T>{p.he2.x, p.he2.x, p.he2.x} : p.he2;
            bool leaving = false;
            if (contact_manifolds_pair_sink<T, SpDeepestSink<T>>(p.shape2, hq, p.pos2, p.rot2, p.shape1, p.he1, p.pos1, p.rot1, T(0), sink, nrm)) {
                const V3<T> cn{-nrm.x, -nrm.y, -nrm.z};
                leaving = p.d.x * cn.x + p.d.y * cn.y + p.d.z * cn.z >= T(0);
            }
            if (!leaving) {
                // the "small ball" rides body 2's motion: shape 2 = Ball(margin) at body 2's origin, rho = margin
                const CcdMotion<T> m1 = ccd_motion<T>(w, p.b1, p.pos1, p.rot1, ccd_rho<T>(p.shape1, p.he1));
                const CcdMotion<T> m2 = ccd_motion<T>(w, p.b2, p.pos2, p.rot2, margin);
                T toi = T(0);
                uint32_t rounds = 0u;
                const int res = ccd_nl_advance<T>(p.shape1, p.he1, m1, AVN_SHAPE_BALL, V3<T>{margin, margin, margin}, m2, p.d, dt, tol, toi, rounds);
                ccd_nl_stats<T>(c, res, rounds);
                if (res == 1) ccd_accept<T>(c, p.e, toi, dt, bits);
            }
        }
        c.cand_t[i] = bits;
    }
}

// ---- Capsule colliders (avn_swept_ccd_capsules_set; the header's "capsule colliders") ----
// Kernels of their own behind the ones above, launched only when the switch is on and the collider table holds a capsule: the segment - box
// routine and the Newton casts stay out of the Ball / Cuboid kernels, which have written CCD_T_NONE for every pair with a capsule.  Each passes
// over the candidates without one and overwrites cand_t of the others.
template <class T> __device__ __forceinline__ bool ccd_has_capsule(const CcdPair<T>& p) { return p.shape1 == AVN_SHAPE_CAPSULE || p.shape2 == AVN_SHAPE_CAPSULE; }
template <class T> __device__ __forceinline__ T ccd_rho_cap(uint32_t shape, V3<T> he) { return shape == AVN_SHAPE_CAPSULE ? he.y + he.x : ccd_rho<T>(shape, he); }
// step 3 by role: collider = c1, cast shape = c2
template <class T>
__device__ __forceinline__ bool ccd_cast_cap(const CcdPair<T>& p, T dt, T& toi) {
    V3<T> p1, p2, n1;
    const Iso<T> iso2 = make_isometry(p.pos2, p.rot2);
    if (p.shape1 != AVN_SHAPE_CAPSULE) return sp_capsule_cast_exact<T>(p.he2.x, p.he2.y, iso2, p.d, dt, p.shape1, p.he1, p.pos1, p.rot1, toi, p1, p2, n1);
    if (p.shape2 != AVN_SHAPE_CAPSULE) return sp_capcol_cast_exact<T, false>(p.shape2, p.he2, iso2, p.d, dt, p.he1, p.pos1, p.rot1, toi, p1, p2, n1);
    return sp_capcol_cast_exact<T, true>(p.shape2, p.he2, iso2, p.d, dt, p.he1, p.pos1, p.rot1, toi, p1, p2, n1);
}
// step 4's contact at prediction 0 with the cast shape (2) as shape 1: true when the pair is leaving
template <class T>
__device__ __forceinline__ bool ccd_leaving_cap(const CcdPair<T>& p) {
    SpDeepestSink<T> sink{vzero<T>(), T(0), 0};
    V3<T> nrm;
    const V3<T> hq = p.shape2 == AVN_SHAPE_BALL ? V3<T>{p.he2.x, p.he2.x, p.he2.x} : p.he2;
    if (!contact_manifolds_pair_sink<T, SpDeepestSink<T>, 0, true>(p.shape2, hq, p.pos2, p.rot2, p.shape1, p.he1, p.pos1, p.rot1, T(0), sink, nrm)) return false;
    const V3<T> cn{-nrm.x, -nrm.y, -nrm.z};
    return p.d.x * cn.x + p.d.y * cn.y + p.d.z * cn.z >= T(0);
}

template <class T, bool MIXED>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_toi_cap(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, bool origin_rule) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        CcdPair<T> p;
        if (!ccd_pair<T, true>(w, bp, ct, c, c.cand[i], p) || !ccd_has_capsule<T>(p)) continue;   // (k_ccd_toi wrote the candidate's cand_t)
        if constexpr (MIXED) { if (ccd_pair_nl<T>(c, p)) continue; }
        atomicAdd(&c.rec[p.e].tested, 1u);
        unsigned long long bits = CCD_T_NONE;
        T toi;
        if (ccd_cast_cap<T>(p, dt, toi)) {
            if (toi == T(0)) { if (origin_rule) bits = CCD_T_ORIGIN; }
            else ccd_accept<T>(c, p.e, toi, dt, bits);
        }
        c.cand_t[i] = bits;
    }
}

template <class T>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_origin_cap(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, T margin) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        if (c.cand_t[i] != CCD_T_ORIGIN) continue;   // (k_ccd_origin has resolved its own: only k_ccd_toi_cap's marks are left)
        unsigned long long bits = CCD_T_NONE;
        CcdPair<T> p;
        if (ccd_pair<T, true>(w, bp, ct, c, c.cand[i], p) && ccd_has_capsule<T>(p) && !ccd_leaving_cap<T>(p)) {
            // the "small ball" against c1: a capsule collider by sp_capcol_cast_exact, a Ball / Cuboid one (the capsule is the cast shape) as ever
            T toi; V3<T> p1, p2, n1;
            const V3<T> hb{margin, margin, margin};
            const Iso<T> iso2 = make_isometry(p.pos2, p.rot2);
            const bool hit = p.shape1 == AVN_SHAPE_CAPSULE ? sp_capcol_cast_exact<T, false>(AVN_SHAPE_BALL, hb, iso2, p.d, dt, p.he1, p.pos1, p.rot1, toi, p1, p2, n1)
                                                           : sp_cast_exact<T>(AVN_SHAPE_BALL, hb, iso2, p.d, dt, p.shape1, p.he1, p.pos1, p.rot1, toi, p1, p2, n1);
            if (hit) ccd_accept<T>(c, p.e, toi, dt, bits);
        }
        c.cand_t[i] = bits;
    }
}

template <class T>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_toi_nl_cap(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, T tol, bool origin_rule) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        CcdPair<T> p;
        if (!ccd_pair<T, true>(w, bp, ct, c, c.cand[i], p) || !ccd_has_capsule<T>(p) || !ccd_pair_nl<T>(c, p)) continue;
        atomicAdd(&c.rec[p.e].tested, 1u);
        atomicAdd(&c.ctr[CCD_CTR_NL_TESTED], 1u);
        const CcdMotion<T> m1 = ccd_motion<T>(w, p.b1, p.pos1, p.rot1, ccd_rho_cap<T>(p.shape1, p.he1));
        const CcdMotion<T> m2 = ccd_motion<T>(w, p.b2, p.pos2, p.rot2, ccd_rho_cap<T>(p.shape2, p.he2));
        T toi = T(0);
        uint32_t rounds = 0u;
        const int res = ccd_nl_advance<T, true>(p.shape1, p.he1, m1, p.shape2, p.he2, m2, p.d, dt, tol, toi, rounds);
        ccd_nl_stats<T>(c, res, rounds);
        unsigned long long bits = CCD_T_NONE;
        if (res == 1) {
            if (toi == T(0)) { if (origin_rule) bits = CCD_T_ORIGIN_NL; }
            else ccd_accept<T>(c, p.e, toi, dt, bits);
        }
        c.cand_t[i] = bits;
    }
}

template <class T>
__global__ __launch_bounds__(CCD_WAVE) void k_ccd_origin_nl_cap(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, T dt, T tol, T margin) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * CCD_WAVE + threadIdx.x; i < count; i += gridDim.x * CCD_WAVE) {
        if (c.cand_t[i] != CCD_T_ORIGIN_NL) continue;   // (k_ccd_origin_nl has resolved its own)
        unsigned long long bits = CCD_T_NONE;
        CcdPair<T> p;
        if (ccd_pair<T, true>(w, bp, ct, c, c.cand[i], p) && ccd_has_capsule<T>(p) && !ccd_leaving_cap<T>(p)) {
            const CcdMotion<T> m1 = ccd_motion<T>(w, p.b1, p.pos1, p.rot1, ccd_rho_cap<T>(p.shape1, p.he1));
            const CcdMotion<T> m2 = ccd_motion<T>(w, p.b2, p.pos2, p.rot2, margin);
            T toi = T(0);
            uint32_t rounds = 0u;
            const int res = ccd_nl_advance<T, true>(p.shape1, p.he1, m1, AVN_SHAPE_BALL, V3<T>{margin, margin, margin}, m2, p.d, dt, tol, toi, rounds);
            ccd_nl_stats<T>(c, res, rounds);
            if (res == 1) ccd_accept<T>(c, p.e, toi, dt, bits);
        }
        c.cand_t[i] = bits;
    }
}

__device__ __forceinline__ unsigned long long ccd_edge_key(uint32_t side, unsigned long long seq) { return ((unsigned long long)side << 63) | (~seq & CCD_KEY_MASK); }

template <class T>
__global__ __launch_bounds__(256) void k_ccd_pick(CCD<T> c, const unsigned long long* __restrict__ seq) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const unsigned long long t = c.cand_t[i];
        if (t == CCD_T_NONE) continue;
        const uint2 cd = c.cand[i];
        if (t == c.min_t[cd.y >> 1]) atomicMin(&c.min_key[cd.y >> 1], ccd_edge_key(cd.y & 1u, seq[cd.x]));
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_ccd_resolve(DW<T> w, BP<T> bp, CT<T> ct, CCD<T> c, const unsigned long long* __restrict__ seq) {
    const uint32_t count = c.ctr[0] < c.cand_cap ? c.ctr[0] : c.cand_cap;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) {
        const unsigned long long t = c.cand_t[i];
        if (t == CCD_T_NONE) continue;
        const uint2 cd = c.cand[i];
        const uint32_t e = cd.y >> 1, side = cd.y & 1u;
        if (t != c.min_t[e] || ccd_edge_key(side, seq[cd.x]) != c.min_key[e]) continue;
        const uint4 m = ct.meta[cd.x];
        const uint32_t c1 = side ? m.y : m.x, c2 = side ? m.x : m.y;
        const uint4 i2 = bp.col_info[c2];
        SweptCcdResult<T>& r = c.rec[e];
        r.toi = ccd_unbits(t, T(0));
        r.hit_collider = i2.x; r.hit_body = (int32_t)i2.y;
        c.wkey_a[2u * e] = bp.col_info[c1].y;
        if (meta_has_solver_body(w.bmeta[i2.y])) c.wkey_a[2u * e + 1u] = i2.y;   // (the reference's dummy SolverBody otherwise: nothing is written)
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_ccd_apply(DW<T> w, CCD<T> c, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals) {
    const uint32_t n2 = 2u * c.n;
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n2) return;
    const uint32_t b = keys[p];
    if (b >= w.n_bodies || (p > 0 && keys[p - 1] == b)) return;   // no write, or not the head of its body's segment
    const V3<T> v = xyz<T>(w.sb_lin[b]), om = xyz<T>(w.sb_ang[b]);
    Vec4<T> dp4 = w.sb_dp[b];
    Q4<T> dq = quat<T>(w.sb_dq[b]);
    V3<T> dp = xyz<T>(dp4);
    for (uint32_t k = p; k < n2 && keys[k] == b; ++k) {
        // "Overshoot slightly to make sure the bodies advance and don't get stuck."
        const T t = c.rec[vals[k] >> 1].toi * T(1.0001);
        dp = t * v;
        dq = qmul(from_scaled_axis(om * t), dq);   // (onto the full step's delta_rotation, as the reference does)
    }
    w.sb_dp[b] = make4<T>(dp, dp4.w);
    w.sb_dq[b] = make4<T>(dq);
}

template <class T> void launch_ccd_tables(const DW<T>& w, const BP<T>& bp, const CCD<T>& c, hipStream_t s) {
    if (w.n_bodies) (void)hipMemsetAsync(c.own, 0xFF, (size_t)w.n_bodies * 4, s);
    if (bp.n_colliders) (void)hipMemsetAsync(c.entry, 0xFF, (size_t)bp.n_colliders * 4, s);
    if (!bp.n_colliders || !c.n) return;
    hipLaunchKernelGGL(k_ccd_own<T>, dim3((bp.n_colliders + 255) / 256), dim3(256), 0, s, bp, c, w.n_bodies);
    hipLaunchKernelGGL(k_ccd_entry<T>, dim3((c.n + 255) / 256), dim3(256), 0, s, c);
}

static uint32_t ccd_bits_for(uint32_t max_value) { uint32_t b = 1; while (b < 32 && (max_value >> b)) ++b; return b; }

template <class T> uint32_t launch_ccd_pass(const DW<T>& w, const BP<T>& bp, const CT<T>& ct, const PG& pg, const CCD<T>& c, const StepParams<T>& p, uint32_t n_rows, hipStream_t s, bool capsules) {
    if (!c.n) return 0;
    uint32_t launches = 0;
    const uint32_t n2 = 2u * c.n;
    hipLaunchKernelGGL(k_ccd_begin<T>, dim3((n2 + 255) / 256), dim3(256), 0, s, c, w.n_bodies); ++launches;
    if (!n_rows) return launches;
    hipLaunchKernelGGL(k_ccd_candidates<T>, dim3((n_rows + 255) / 256), dim3(256), 0, s, ct, c, n_rows, bp.n_colliders); ++launches;
    // the candidate count stays on the device: grids sized for the most a table of n_rows rows can yield, capped; the kernels stride
    const uint32_t most = 2u * n_rows < c.cand_cap ? 2u * n_rows : c.cand_cap;
    const uint32_t wave_blocks = std::min<uint32_t>((most + CCD_WAVE - 1) / CCD_WAVE, 8192u), flat_blocks = std::min<uint32_t>((most + 255) / 256, 2048u);
    const bool origin_rule = p.default_speculative_margin < Limits<T>::max;
    const bool nl = c.mode != nullptr;   // the list in force has a NonLinear entry: known since the upload
    if (!nl) { hipLaunchKernelGGL((k_ccd_toi<T, false>), dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, origin_rule); ++launches; }
    else {
        hipLaunchKernelGGL((k_ccd_toi<T, true>), dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, origin_rule); ++launches;
        hipLaunchKernelGGL(k_ccd_toi_nl<T>, dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, p.contact_tolerance, origin_rule); ++launches;
        if (origin_rule) { hipLaunchKernelGGL(k_ccd_origin_nl<T>, dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, p.contact_tolerance, p.default_speculative_margin); ++launches; }
    }
    if (origin_rule) { hipLaunchKernelGGL(k_ccd_origin<T>, dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, p.default_speculative_margin); ++launches; }
    if (capsules) {   // the switch is on and the collider table holds a capsule: each origin kernel behind the _cap kernel that marks for it
        if (!nl) { hipLaunchKernelGGL((k_ccd_toi_cap<T, false>), dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, origin_rule); ++launches; }
        else {
            hipLaunchKernelGGL((k_ccd_toi_cap<T, true>), dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, origin_rule); ++launches;
            hipLaunchKernelGGL(k_ccd_toi_nl_cap<T>, dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, p.contact_tolerance, origin_rule); ++launches;
            if (origin_rule) { hipLaunchKernelGGL(k_ccd_origin_nl_cap<T>, dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, p.contact_tolerance, p.default_speculative_margin); ++launches; }
        }
        if (origin_rule) { hipLaunchKernelGGL(k_ccd_origin_cap<T>, dim3(wave_blocks), dim3(CCD_WAVE), 0, s, w, bp, ct, c, p.dt_adj, p.default_speculative_margin); ++launches; }
    }
    hipLaunchKernelGGL(k_ccd_pick<T>, dim3(flat_blocks), dim3(256), 0, s, c, pg.seq); ++launches;
    hipLaunchKernelGGL(k_ccd_resolve<T>, dim3(flat_blocks), dim3(256), 0, s, w, bp, ct, c, pg.seq); ++launches;
    uint32_t *keys = c.wkey_a, *vals = c.wval_a;
    const uint32_t bits = ccd_bits_for(w.n_bodies);
    launch_radix_sort_bits(c.wkey_a, c.wval_a, c.wkey_b, c.wval_b, n2, bits, c.hist, c.block_sums, &keys, &vals, s);
    launches += ((bits + 7) / 8) * radix_pass_launches(n2);   // (an upper bound: small lists sort in one launch)
    hipLaunchKernelGGL(k_ccd_apply<T>, dim3((n2 + 255) / 256), dim3(256), 0, s, w, c, keys, vals); ++launches;
    return launches;
}

static_assert(sizeof(SweptCcdResult<float>) == 16 && sizeof(SweptCcdResult<double>) == 24, "swept CCD record layout");
template void launch_ccd_tables<float>(const DW<float>&, const BP<float>&, const CCD<float>&, hipStream_t);
template void launch_ccd_tables<double>(const DW<double>&, const BP<double>&, const CCD<double>&, hipStream_t);
template uint32_t launch_ccd_pass<float>(const DW<float>&, const BP<float>&, const CT<float>&, const PG&, const CCD<float>&, const StepParams<float>&, uint32_t, hipStream_t, bool);
template uint32_t launch_ccd_pass<double>(const DW<double>&, const BP<double>&, const CT<double>&, const PG&, const CCD<double>&, const StepParams<double>&, uint32_t, hipStream_t, bool);

}  // namespace avn
