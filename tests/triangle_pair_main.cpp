// triangle_pair_main.cpp — avian_amd/csrc/avn_triangle_pair.h (with avn_narrow.h and avn_capsule_pair.h) as a plain host program: reads a file of
// shape pairs, computes their manifolds through contact_manifolds_pair_sink<.., CAP = true, TRI = true> and NpArraySink exactly as the batch
// kernel k_triangle_manifolds_query does, and writes the output arrays.  tests/test_triangle_pair_host.py builds it with
// -fsanitize=address,undefined -ffp-contract=off and compares the arrays with tests/triangle_collider_reference.py bit for bit.
//
//   triangle_pair_main <in> <out>
//   in:  int32 bits (32 | 64), int32 n, u8 shape1[n], shape2[n], flags1[n], flags2[n], then in the scalar: he1[3n] pos1[3n] rot1[4n]
//        he2[3n] pos2[3n] rot2[4n] prediction[n] vertices1[9n] vertices2[9n]
//   out: u8 point_count[n], scalar normal[3n] anchor1[48n] anchor2[48n] point[48n] penetration[16n], u32 fid1[16n] fid2[16n]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// the two device intrinsics the headers use (ulps_apart_le4)
static inline uint32_t __float_as_uint(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static inline long long __double_as_longlong(double x) { long long u; std::memcpy(&u, &x, 8); return u; }

#include "avn_narrow.h"
#include "avn_capsule_pair.h"
#include "avn_triangle_pair.h"

using namespace avn;

template <class T> static bool read_vec(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static bool write_vec(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <class T> static int run(FILE* in, FILE* out, size_t n) {
    std::vector<uint8_t> shape1, shape2, flags1, flags2;
    std::vector<T> he1, pos1, rot1, he2, pos2, rot2, pred, v1, v2;
    if (!read_vec(in, shape1, n) || !read_vec(in, shape2, n) || !read_vec(in, flags1, n) || !read_vec(in, flags2, n) || !read_vec(in, he1, 3 * n) || !read_vec(in, pos1, 3 * n) ||
        !read_vec(in, rot1, 4 * n) || !read_vec(in, he2, 3 * n) || !read_vec(in, pos2, 3 * n) || !read_vec(in, rot2, 4 * n) || !read_vec(in, pred, n) || !read_vec(in, v1, 9 * n) ||
        !read_vec(in, v2, 9 * n)) { std::fprintf(stderr, "short input\n"); return 2; }
    const size_t Q = AVN_MAX_QUERY_POINTS;
    std::vector<uint8_t> point_count(n, 0);
    std::vector<T> normal(3 * n, T(0)), anchor1(3 * Q * n, T(0)), anchor2(3 * Q * n, T(0)), point(3 * Q * n, T(0)), penetration(Q * n, T(0));
    std::vector<uint32_t> fid1(Q * n, 0u), fid2(Q * n, 0u);
    auto ld3 = [](const std::vector<T>& a, size_t i) { return V3<T>{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; };
    auto ldq = [](const std::vector<T>& a, size_t i) { return Q4<T>{a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]}; };
    auto ldt = [](const std::vector<T>& a, size_t i, uint8_t f) { return NpTri<T>{V3<T>{a[9 * i], a[9 * i + 1], a[9 * i + 2]}, V3<T>{a[9 * i + 3], a[9 * i + 4], a[9 * i + 5]}, V3<T>{a[9 * i + 6], a[9 * i + 7], a[9 * i + 8]}, (uint32_t)f}; };
    for (size_t i = 0; i < n; ++i) {
        const V3<T> p1 = ld3(pos1, i), p2 = ld3(pos2, i);
        NpManifold<T> m;
        m.n = 0;
        m.normal = vzero<T>();
        NpArraySink<T> sink{&m, p1 - p2};
        const NpTri<T> t1 = ldt(v1, i, flags1[i]), t2 = ldt(v2, i, flags2[i]);
        const bool has = contact_manifolds_pair_sink<T, NpArraySink<T>, 0, true, true>(shape1[i], ld3(he1, i), p1, ldq(rot1, i), shape2[i], ld3(he2, i), p2, ldq(rot2, i), pred[i], sink, m.normal,
                                                                                      nullptr, nullptr, t1, t2);
        if (m.n < 0 || m.n > AVN_NP_MAX_RAW) { std::fprintf(stderr, "row %zu: %d raw points\n", i, m.n); return 3; }
        const int cnt = has ? m.n : 0;
        point_count[i] = (uint8_t)cnt;
        if (has) { normal[3 * i] = m.normal.x; normal[3 * i + 1] = m.normal.y; normal[3 * i + 2] = m.normal.z; }
        for (int k = 0; k < cnt; ++k) {
            const size_t s = Q * i + (size_t)k;
            const V3<T> a1 = m.pts[k].anchor1, a2 = m.pts[k].anchor2, wp = p1 + a1;
            anchor1[3 * s] = a1.x; anchor1[3 * s + 1] = a1.y; anchor1[3 * s + 2] = a1.z;
            anchor2[3 * s] = a2.x; anchor2[3 * s + 1] = a2.y; anchor2[3 * s + 2] = a2.z;
            point[3 * s] = wp.x; point[3 * s + 1] = wp.y; point[3 * s + 2] = wp.z;
            penetration[s] = m.pts[k].penetration; fid1[s] = m.pts[k].fid1; fid2[s] = m.pts[k].fid2;
        }
    }
    if (!write_vec(out, point_count) || !write_vec(out, normal) || !write_vec(out, anchor1) || !write_vec(out, anchor2) || !write_vec(out, point) || !write_vec(out, penetration) ||
        !write_vec(out, fid1) || !write_vec(out, fid2)) { std::fprintf(stderr, "short output\n"); return 2; }
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
    if (rc == 0) std::printf("TRIANGLE_PAIRS_OK %d\n", head[1]);
    return rc;
}
