// The staging arena's layout arithmetic (avian_amd/csrc/avn_stage.h) on its own: no device, no library.  tests/test_stage_layout.py compiles this
// file with -fsanitize=address,undefined and runs it; every CHECK that fails is printed and the exit status is 1.
#include "avn_stage.h"

#include <cstdio>
#include <vector>

using avn_stage::IN;
using avn_stage::OUT;
using avn_stage::SCRATCH;
using avn_stage::Layout;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static size_t up64(size_t x) { return (x + 63) / 64 * 64; }

int main() {
    static char host[1];   // a non-null host address; the layout never reads through it
    {   // an empty plan
        Layout l;
        CHECK(l.n == 0 && l.total == 0 && l.ok);
        CHECK(l.assign(nullptr, 0));
    }
    {   // absent arrays: no space, a null result, whatever the direction
        Layout l;
        void* d[5];
        for (void*& p : d) p = host;
        l.add(IN, nullptr, 10, 4, &d[0]);
        l.add(IN, host, 0, 4, &d[1]);
        l.add(OUT, nullptr, 10, 8, &d[2]);
        l.add(OUT, host, 0, 8, &d[3]);
        l.add(SCRATCH, nullptr, 0, 8, &d[4]);
        CHECK(l.ok && l.n == 0 && l.total == 0);
        for (void* p : d) CHECK(p == nullptr);
        void* s = nullptr;
        l.add(SCRATCH, nullptr, 3, 8, &s);   // (scratch has no host side: only its count decides)
        CHECK(l.ok && l.n == 1 && l.total == 24);
    }
    {   // counts 1, 63, 64, 65 of 1-, 4-, 8- and 3 * sizeof(double)-byte elements, mixed, with absent arrays in between
        const size_t counts[4] = {1, 63, 64, 65}, elems[4] = {1, 4, 8, 3 * sizeof(double)};
        struct Decl { size_t count, elem; };
        std::vector<Decl> decl;
        for (int k = 0; k < 16; ++k) decl.push_back({counts[(k * 7 + 3) % 4], elems[(k * 5 + k / 4) % 4]});   // every (count, elem) pair once
        for (int c = 0; c < 4; ++c)
            for (int e = 0; e < 4; ++e) {
                int seen = 0;
                for (const Decl& d : decl) seen += d.count == counts[c] && d.elem == elems[e];
                CHECK(seen == 1);
            }
        Layout l;
        void* dev[16];
        void* absent = host;
        size_t expect_off[16], run = 0;
        for (int k = 0; k < 16; ++k) {
            l.add(k % 3 == 0 ? IN : k % 3 == 1 ? OUT : SCRATCH, host, decl[k].count, decl[k].elem, &dev[k]);
            if (k % 5 == 0) l.add(IN, nullptr, 100, 4, &absent);
            expect_off[k] = up64(run);                       // the independent recomputation: round the running end up, place, advance
            run = expect_off[k] + decl[k].count * decl[k].elem;
        }
        CHECK(l.ok && l.n == 16 && absent == nullptr);
        CHECK(l.total == run);
        for (int k = 0; k < 16; ++k) {
            CHECK(l.item[k].off == expect_off[k]);
            CHECK(l.item[k].off % 64 == 0);
            CHECK(l.item[k].bytes == decl[k].count * decl[k].elem);
            if (k) CHECK(l.item[k].off >= l.item[k - 1].off + l.item[k - 1].bytes);   // declaration order, no overlap
        }
        CHECK(l.total >= l.item[15].off + l.item[15].bytes);
        // an arena one byte short is refused and hands nothing out; one that fits hands out base + offset
        static char arena[16384];
        CHECK(run <= sizeof arena);
        for (void*& p : dev) p = nullptr;
        CHECK(!l.assign(arena, run - 1));
        for (void* p : dev) CHECK(p == nullptr);
        CHECK(l.assign(arena, run));
        for (int k = 0; k < 16; ++k) CHECK(dev[k] == arena + expect_off[k]);
    }
    {   // sizes beyond size_t: the product, the alignment step and the running total
        void* d = host;
        Layout a;
        a.add(IN, host, SIZE_MAX / 8 + 1, 8, &d);
        CHECK(!a.ok && a.n == 0 && d == nullptr && !a.assign(nullptr, SIZE_MAX));
        Layout b;
        b.add(IN, host, SIZE_MAX - 10, 1, &d);
        CHECK(b.ok && b.total == SIZE_MAX - 10);
        b.add(IN, host, 1, 1, &d);   // (rounding SIZE_MAX - 10 up to 64 wraps)
        CHECK(!b.ok && b.n == 1);
        Layout c;
        c.add(IN, host, 64, 1, &d);
        c.add(IN, host, SIZE_MAX - 64, 1, &d);   // (64 + (SIZE_MAX - 64) fits; one more does not)
        CHECK(c.ok && c.total == SIZE_MAX);
        Layout e;
        e.add(IN, host, 65, 1, &d);
        e.add(IN, host, SIZE_MAX - 127, 1, &d);   // (offset 128 + SIZE_MAX - 127 wraps)
        CHECK(!e.ok && e.n == 1);
    }
    {   // one item more than the capacity: refused, nothing written (the sanitizer watches item[])
        Layout l;
        void* d[avn_stage::CAPACITY + 1];
        for (int k = 0; k <= avn_stage::CAPACITY; ++k) l.add(SCRATCH, nullptr, 1, 1, &d[k]);
        CHECK(!l.ok && l.n == avn_stage::CAPACITY);
        CHECK(l.total == (size_t)(avn_stage::CAPACITY - 1) * 64 + 1);
        CHECK(d[avn_stage::CAPACITY] == nullptr);
        static char arena[64 * avn_stage::CAPACITY];
        CHECK(!l.assign(arena, sizeof arena));
    }
    if (failures) return 1;
    std::printf("STAGE_LAYOUT_OK\n");
    return 0;
}
