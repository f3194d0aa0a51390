// avn_stage.h -- the layout of one call's transfers through the staging arena.  A call declares each array once (host pointer, element size,
// count, where its device pointer goes, direction); the offsets, the arena size and the device pointers all follow from that one list, in
// declaration order.  Nothing of HIP here: the copies and the arena itself are World<T>::StagePlan's (avn_world.hip), and a host compiler
// can test this file alone (tests/stage_layout_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace avn_stage {

constexpr size_t ALIGN = 64;   // every item starts on a 64-byte boundary of the arena
constexpr int CAPACITY = 24;   // items of one call; the largest callers (bodies_upload, joints_upload) declare 18

enum Dir : uint8_t { IN, OUT, SCRATCH };   // IN: copied from the host at commit; OUT: copied back at finish; SCRATCH: arena space only

struct Item {
    void* host;    // IN: the source, OUT: the destination, SCRATCH: unused
    void** dev;    // receives the base + off at assign()
    size_t bytes, off;
    Dir dir;
};

struct Layout {
    Item item[CAPACITY];
    int n = 0;
    size_t total = 0;   // the last offset plus size: what the arena must hold
    bool ok = true;     // false once a declaration was refused (too many items, or a size beyond size_t)

    // An absent array (null host pointer of an IN / OUT, or count 0) gets a null device pointer and no space.
    void add(Dir dir, const void* host, size_t count, size_t elem, void** dev) {
        *dev = nullptr;
        if (count == 0 || (dir != SCRATCH && !host)) return;
        if (n == CAPACITY || count > SIZE_MAX / elem) { ok = false; return; }
        const size_t bytes = count * elem;
        if (total > SIZE_MAX - (ALIGN - 1)) { ok = false; return; }
        const size_t off = (total + (ALIGN - 1)) & ~(ALIGN - 1);
        if (bytes > SIZE_MAX - off) { ok = false; return; }
        item[n++] = Item{const_cast<void*>(host), dev, bytes, off, dir};
        total = off + bytes;
    }
    // Hands every item its place in an arena of `capacity` bytes at `base`; false (and nothing written) when the layout does not fit.
    bool assign(void* base, size_t capacity) {
        if (!ok || total > capacity) return false;
        for (int i = 0; i < n; ++i) *item[i].dev = (char*)base + item[i].off;
        return true;
    }
};

}  // namespace avn_stage
