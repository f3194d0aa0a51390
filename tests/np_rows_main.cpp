// np_rows_main.cpp — the narrow phase's row descriptor (NpRows, np_row_args, np_row_id in avian_amd/csrc/avn_kernels.h) as a plain host program: for every
// case of the input file it builds the NpRows through its named constructor, derives the kernel arguments and maps every lane to its row id, as k_narrow_phase does.
// Each id is also compared with what the three former entry points (launch_narrow_phase, _dense, _rows) passed to the kernel and the expression the kernel held.
// tests/test_np_rows_host.py builds it with -fsanitize=address,undefined and compares the ids with the definition of the three forms.
//
//   np_rows_main <in> <out>
//   in:  u32 cases, then per case u32 form (0 active | 1 dense | 2 added), n_list, range_base, n_range, list[n_list]
//   out: per case u32 n, ids[n]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "avn_kernels.h"

using namespace avn;

// the launch layer before NpRows: the kernel arguments of the three entry points, and the kernel's id expression
static uint32_t former_id(uint32_t form, const uint32_t* list, uint32_t n_list, uint32_t range_base, uint32_t a) {
    const uint32_t* active = list;
    bool dense = true;
    if (form == 0) dense = false;                                       // launch_narrow_phase: (active, n_active, 0, 0)
    else if (form == 1) { active = nullptr; n_list = 0; range_base = 0; }   // launch_narrow_phase_dense: (nullptr, n_rows, 0, 0)
    else if (!n_list && !range_base) active = nullptr;                  // launch_narrow_phase_rows: its special branch
    return !dense ? active[a] : (active || n_list || range_base) ? (a < n_list ? active[a] : range_base + (a - n_list)) : a;
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    uint32_t cases = 0;
    if (!in || !out || std::fread(&cases, 4, 1, in) != 1) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    for (uint32_t k = 0; k < cases; ++k) {
        uint32_t h[4];
        if (std::fread(h, 4, 4, in) != 4 || h[0] > 2) { std::fprintf(stderr, "bad case %u\n", k); return 2; }
        // (exactly n_list words on the heap, also when that is none: a read past the list is a sanitizer report)
        uint32_t* list = (uint32_t*)std::malloc(h[1] ? (size_t)h[1] * 4 : 1);
        if (h[1] && std::fread(list, 4, h[1], in) != h[1]) { std::fprintf(stderr, "short case %u\n", k); return 2; }
        const NpRows rows = h[0] == 0 ? NpRows::active(list, h[1]) : h[0] == 1 ? NpRows::dense(h[3]) : NpRows::added(list, h[1], h[2], h[3]);
        const NpRowArgs r = np_row_args(rows);
        if (r.n != rows.count()) { std::fprintf(stderr, "case %u: %u lanes for %u rows\n", k, r.n, rows.count()); return 3; }
        std::vector<uint32_t> ids(r.n);
        for (uint32_t a = 0; a < r.n; ++a) {
            ids[a] = h[0] == 0 ? np_row_id<false>(r.list, r.n_list, r.range_base, a) : np_row_id<true>(r.list, r.n_list, r.range_base, a);
            const uint32_t was = former_id(h[0], list, h[1], h[2], a);
            if (ids[a] != was) { std::fprintf(stderr, "case %u lane %u: id %u, formerly %u\n", k, a, ids[a], was); return 3; }
        }
        if (std::fwrite(&r.n, 4, 1, out) != 1 || (r.n && std::fwrite(ids.data(), 4, r.n, out) != r.n)) { std::fprintf(stderr, "short output\n"); return 2; }
        std::free(list);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("NP_ROWS_OK %u\n", cases);
    return 0;
}
