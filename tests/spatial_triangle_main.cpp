// spatial_triangle_main.cpp — avian_amd/csrc/avn_spatial_triangle_pair.h (the pair tests of the spatial queries against a Triangle collider, with
// avn_triangle_pair.h's tri_closest_point / tri_seg_closest under them) as a plain host program: reads a file of rows, runs the pair function each row
// names exactly as the CTRI leaves of k_spatial.hip call it, and writes the answers.  tests/test_spatial_triangle_host.py builds it with
// -fsanitize=address,undefined -ffp-contract=off and compares the answers with tests/spatial_triangle_collider_reference.py bit for bit.
//
//   spatial_triangle_main <in> <out>
//   in:  int32 bits (32 | 64), int32 n, u8 op[n], u8 kind[n] (the query's shape: 0 cuboid, 1 ball, 3 capsule), then in the scalar: tri[9n] (a, b, c in the
//        collider's frame) pos1[3n] rot1[4n] (the collider's pose) he2[3n] pos2[3n] rot2[4n] (the query shape and its pose) d[3n] max_distance[n]
//        op 0 ray:        o_l = pos2, d_l = d (already in the collider's frame)        -> hit, t, n_l
//        op 1 projection: point_l = pos2                                               -> hit = the point is on the triangle, C(point_l), region
//        op 2 intersects: the query shape against the collider                         -> hit
//        op 3 cast:       the query shape along d within max_distance                  -> hit, toi, point1, point2, normal1
//        op 4 segment:    A = pos2, u = d against the triangle (sp_seg_tri_d2)         -> hit = 1, d2, p_seg, p_tri
//   out: u8 hit[n], scalar out[10n] (the values above in that order, the rest 0)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// the two device intrinsics the headers use (ulps_apart_le4)
static inline uint32_t __float_as_uint(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static inline long long __double_as_longlong(double x) { long long u; std::memcpy(&u, &x, 8); return u; }

#include "avn_narrow.h"
#include "avn_capsule_pair.h"
#include "avn_spatial_triangle_pair.h"

using namespace avn;

template <class T> static bool read_vec(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static bool write_vec(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <class T> static int run(FILE* in, FILE* out, size_t n) {
    std::vector<uint8_t> op, kind;
    std::vector<T> tri, pos1, rot1, he2, pos2, rot2, dir, maxd;
    if (!read_vec(in, op, n) || !read_vec(in, kind, n) || !read_vec(in, tri, 9 * n) || !read_vec(in, pos1, 3 * n) || !read_vec(in, rot1, 4 * n) || !read_vec(in, he2, 3 * n) ||
        !read_vec(in, pos2, 3 * n) || !read_vec(in, rot2, 4 * n) || !read_vec(in, dir, 3 * n) || !read_vec(in, maxd, n)) { std::fprintf(stderr, "short input\n"); return 2; }
    const size_t W = 10;
    std::vector<uint8_t> hit(n, 0);
    std::vector<T> res(W * n, T(0));
    auto ld3 = [](const std::vector<T>& a, size_t i) { return V3<T>{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; };
    auto ldq = [](const std::vector<T>& a, size_t i) { return Q4<T>{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}; };
    for (size_t i = 0; i < n; ++i) {
        const NpTri<T> t{V3<T>{tri[9 * i], tri[9 * i + 1], tri[9 * i + 2]}, V3<T>{tri[9 * i + 3], tri[9 * i + 4], tri[9 * i + 5]}, V3<T>{tri[9 * i + 6], tri[9 * i + 7], tri[9 * i + 8]}, 7u};
        const V3<T> p1 = ld3(pos1, i), p2 = ld3(pos2, i), h2 = ld3(he2, i), d = ld3(dir, i);
        const Q4<T> r1 = ldq(rot1, i), r2 = ldq(rot2, i);
        T* o = res.data() + W * i;
        auto put3 = [&](size_t at, V3<T> v) { o[at] = v.x; o[at + 1] = v.y; o[at + 2] = v.z; };
        if (op[i] == 0) {
            T tt = T(0); V3<T> nl = vzero<T>();
            if (sp_tri_ray<T>(t.a, t.b, t.c, p2, d, tt, nl)) { hit[i] = 1; o[0] = tt; put3(1, nl); }
        } else if (op[i] == 1) {
            int rg = -1;
            const V3<T> q = tri_closest_point<T>(t.a, t.b, t.c, p2, rg);
            if (rg < 0 || rg > 6) { std::fprintf(stderr, "row %zu: region %d\n", i, rg); return 3; }
            hit[i] = sp_tri_point<T>(t.a, t.b, t.c, p2) ? 1 : 0;
            put3(0, q); o[3] = (T)rg;
        } else if (op[i] == 2) {
            const Iso<T> iso2 = make_isometry(p2, r2);
            const bool h = kind[i] == AVN_SHAPE_CAPSULE ? sp_tricol_intersects<T, true>(kind[i], h2, iso2, t, p1, r1) : sp_tricol_intersects<T, false>(kind[i], h2, iso2, t, p1, r1);
            hit[i] = h ? 1 : 0;
        } else if (op[i] == 3) {
            const Iso<T> iso2 = make_isometry(p2, r2);
            T toi = T(0); V3<T> w1 = vzero<T>(), w2 = vzero<T>(), n1 = vzero<T>();
            const bool h = kind[i] == AVN_SHAPE_CAPSULE ? sp_tricol_cast_exact<T, true>(kind[i], h2, iso2, d, maxd[i], t, p1, r1, toi, w1, w2, n1)
                                                        : sp_tricol_cast_exact<T, false>(kind[i], h2, iso2, d, maxd[i], t, p1, r1, toi, w1, w2, n1);
            if (h) { hit[i] = 1; o[0] = toi; put3(1, w1); put3(4, w2); put3(7, n1); }
        } else if (op[i] == 4) {
            V3<T> ps = vzero<T>(), pt = vzero<T>();
            o[0] = sp_seg_tri_d2<T>(t.a, t.b, t.c, p2, d, ps, pt);
            put3(1, ps); put3(4, pt);
            hit[i] = 1;
        } else { std::fprintf(stderr, "row %zu: unknown op\n", i); return 2; }
    }
    if (!write_vec(out, hit) || !write_vec(out, res)) { std::fprintf(stderr, "short output\n"); return 2; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t head[2];
    if (std::fread(head, 4, 2, in) != 2 || head[1] < 0 || (head[0] != 32 && head[0] != 64)) { std::fprintf(stderr, "bad header\n"); return 2; }
    const int rc = head[0] == 32 ? run<float>(in, out, (size_t)head[1]) : run<double>(in, out, (size_t)head[1]);
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    if (rc == 0) std::printf("SPATIAL_TRIANGLE_OK %d\n", head[1]);
    return rc;
}
