// avn_devbuf.h — the two grow-only allocations of the host side: DevBuf (device memory) and Pinned (page-locked host memory).
// Both report failure through a [[nodiscard]] hipError_t, and the build runs with -Werror=unused-result: an allocation whose
// result is dropped does not compile.  Inside World every call is wrapped in ALLOC (avn_world.hip).
// Only the HIP runtime API and the standard library: tests/devbuf_main.cpp builds this header against stubs of the six calls below.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>

namespace avn {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // Grows (never shrinks) to max(bytes, cap + cap/2), rounded up to 256.  *moved is set when the pointer changed and never cleared, so calls
    // chain on one flag.  Contents are NOT preserved unless keep: then the old cap bytes are copied on s and s is synchronised.  A failed
    // hipMalloc leaves p and cap as they were; a failed keep copy returns its error with the new block installed and the old one freed.
    [[nodiscard]] hipError_t ensure(size_t bytes, bool* moved = nullptr, bool keep = false, hipStream_t s = nullptr) {
        return bytes <= cap ? hipSuccess : grow(bytes, moved, keep, s);   // (the usual call is this one comparison)
    }
    // ensure() sized by element count; *field always ends up naming the buffer as it is now
    template <class U> [[nodiscard]] hipError_t ensure_as(size_t count, U** field, bool* moved = nullptr, bool keep = false, hipStream_t s = nullptr) {
        hipError_t err = ensure(count * sizeof(U), moved, keep, s);
        *field = (U*)p;
        return err;
    }
    template <class U> U* as() const { return (U*)p; }

private:
    // out of line: about 150 buffers are ensured from several hundred call sites, which should each cost a comparison and a cold call
    __attribute__((noinline)) hipError_t grow(size_t bytes, bool* moved, bool keep, hipStream_t s) {
        size_t ncap = std::max(bytes, cap + cap / 2);
        ncap = (ncap + 255) & ~(size_t)255;
        void* np = nullptr;
        hipError_t err = hipMalloc(&np, ncap);
        if (err != hipSuccess) return err;
        if (p) {
            if (keep) { err = hipMemcpyAsync(np, p, cap, hipMemcpyDeviceToDevice, s); if (err == hipSuccess) err = hipStreamSynchronize(s); }
            (void)hipFree(p);
        }
        p = np;
        cap = ncap;
        if (moved) *moved = true;
        return err;
    }
};

// pinned host staging (grow-only, contents never kept): the old block is freed first; after a failure p == nullptr and cap == 0
struct Pinned {
    void* p = nullptr;
    size_t cap = 0;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    [[nodiscard]] hipError_t ensure(size_t bytes) { return bytes <= cap ? hipSuccess : grow(bytes); }

private:
    __attribute__((noinline)) hipError_t grow(size_t bytes) {
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        size_t c = (bytes + bytes / 2 + 4095) & ~(size_t)4095;
        hipError_t e = hipHostMalloc(&p, c, hipHostMallocDefault);
        if (e == hipSuccess) cap = c;
        return e;
    }
};

}  // namespace avn
