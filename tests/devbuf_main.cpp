// DevBuf and Pinned (avian_amd/csrc/avn_devbuf.h) on their own: no device, no HIP runtime, no library.  The six runtime calls the header makes are
// defined here over malloc / free / memcpy, with a countdown that makes the n-th allocation (or the next copy) fail.  tests/test_devbuf_cpu.py
// compiles this file with -fsanitize=address,undefined and runs it; every CHECK that fails is printed and the exit status is 1.
#include "avn_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// ---- the stub runtime ----
static int fail_alloc_in = 0;      // n > 0: the n-th allocation from now returns hipErrorOutOfMemory
static bool fail_next_copy = false;
static int live_dev = 0, live_host = 0, n_copies = 0, n_syncs = 0;
static size_t last_copy_bytes = 0;
static hipStream_t last_stream = nullptr;

static bool alloc_fails() { return fail_alloc_in > 0 && --fail_alloc_in == 0; }
hipError_t hipMalloc(void** ptr, size_t size) {
    if (alloc_fails()) return hipErrorOutOfMemory;
    *ptr = std::malloc(size);
    ++live_dev;
    return hipSuccess;
}
hipError_t hipFree(void* ptr) { std::free(ptr); --live_dev; return hipSuccess; }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
    if (alloc_fails()) return hipErrorOutOfMemory;
    *ptr = std::malloc(size);
    ++live_host;
    return hipSuccess;
}
hipError_t hipHostFree(void* ptr) { std::free(ptr); --live_host; return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    CHECK(kind == hipMemcpyDeviceToDevice);
    ++n_copies; last_copy_bytes = bytes; last_stream = s;
    if (fail_next_copy) { fail_next_copy = false; return hipErrorInvalidValue; }
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { ++n_syncs; CHECK(s == last_stream); return hipSuccess; }

using avn::DevBuf;
using avn::Pinned;

static void fill(void* p, size_t n, unsigned seed) { for (size_t i = 0; i < n; ++i) ((unsigned char*)p)[i] = (unsigned char)(seed + 7 * i); }
static bool holds(const void* p, size_t n, unsigned seed) {
    for (size_t i = 0; i < n; ++i) if (((const unsigned char*)p)[i] != (unsigned char)(seed + 7 * i)) return false;
    return true;
}

int main() {
    static int stream_tag;
    hipStream_t stream = (hipStream_t)&stream_tag;   // (never dereferenced: the stub only compares it)
    {   // growth policy and `moved`
        DevBuf b;
        bool moved = false;
        CHECK(b.ensure(0, &moved) == hipSuccess && !moved && b.p == nullptr && b.cap == 0);   // nothing asked, nothing allocated
        CHECK(b.ensure(1, &moved) == hipSuccess && moved && b.p && b.cap == 256);             // the first size is rounded to 256
        CHECK(live_dev == 1);
        void* p0 = b.p;
        moved = false;
        CHECK(b.ensure(256, &moved) == hipSuccess && !moved && b.p == p0 && b.cap == 256);    // at cap: no-op
        CHECK(b.ensure(100, &moved) == hipSuccess && !moved && b.p == p0 && b.cap == 256);    // below cap: no-op
        moved = true;
        CHECK(b.ensure(10, &moved) == hipSuccess && moved);                                   // ... which never clears the flag
        moved = false;
        CHECK(b.ensure(257, &moved) == hipSuccess && moved && b.p && b.cap == 512);           // just above cap: cap + cap/2 = 384, rounded up to 256s
        CHECK(b.ensure(513, nullptr) == hipSuccess && b.cap == 768);                          // 512 + 256 is a multiple already; no flag is fine
        CHECK(b.ensure(10000) == hipSuccess && b.cap == 10240);                               // a large request wins over cap + cap/2
        CHECK(b.ensure(10241, &moved) == hipSuccess && b.cap == 15360);
        CHECK(live_dev == 1 && n_copies == 0 && n_syncs == 0);                                // without keep no copy is issued
        // the flag chains: one of three calls moves, the flag stays set through the two that do not
        DevBuf c;
        CHECK(c.ensure(64) == hipSuccess);
        moved = false;
        CHECK(b.ensure(1, &moved) == hipSuccess && c.ensure(257, &moved) == hipSuccess && b.ensure(2, &moved) == hipSuccess && moved);
        // the typed form: sized by element count, the pointer assigned
        double* d = nullptr;
        moved = false;
        CHECK(c.ensure_as(100, &d, &moved) == hipSuccess && moved && c.cap == 1024 && (void*)d == c.p && c.as<double>() == d);
        const float* f = nullptr;
        CHECK(c.ensure_as(3, &f) == hipSuccess && (const void*)f == c.p && c.cap == 1024);
    }
    CHECK(live_dev == 0);   // the destructors freed exactly what was allocated
    {   // keep: the old cap bytes arrive in the new block, copied on the stream given, which is then synchronised
        DevBuf b;
        CHECK(b.ensure(300, nullptr, true, stream) == hipSuccess && b.cap == 512 && n_copies == 0);   // (nothing to keep yet)
        fill(b.p, 512, 3);
        n_copies = n_syncs = 0;
        bool moved = false;
        CHECK(b.ensure(513, &moved, true, stream) == hipSuccess && moved && b.cap == 768);
        CHECK(n_copies == 1 && n_syncs == 1 && last_copy_bytes == 512 && last_stream == stream);
        CHECK(holds(b.p, 512, 3));
        CHECK(b.ensure(700, &moved, true, stream) == hipSuccess && n_copies == 1);                     // no growth, no copy
        CHECK(b.ensure(769, nullptr, false, stream) == hipSuccess && n_copies == 1 && n_syncs == 1);   // growth without keep: no copy
        CHECK(live_dev == 1);
        // a failed keep copy, as it is: the error is returned with the new block installed and the old one freed
        const size_t cap0 = b.cap;
        void* p0 = b.p;
        fail_next_copy = true;
        moved = false;
        CHECK(b.ensure(cap0 + 1, &moved, true, stream) == hipErrorInvalidValue);
        CHECK(moved && b.p && b.p != p0 && b.cap > cap0 && live_dev == 1);
    }
    CHECK(live_dev == 0);
    {   // a failed device allocation: the error comes back, p and cap are untouched, the contents still there, the next call works
        DevBuf b;
        fail_alloc_in = 1;
        bool moved = false;
        CHECK(b.ensure(100, &moved) == hipErrorOutOfMemory && !moved && b.p == nullptr && b.cap == 0 && live_dev == 0);
        CHECK(b.ensure(100, &moved) == hipSuccess && moved && b.cap == 256);
        fill(b.p, 256, 11);
        void* p0 = b.p;
        moved = false;
        n_copies = 0;
        fail_alloc_in = 1;
        CHECK(b.ensure(1000, &moved, true, stream) == hipErrorOutOfMemory);
        CHECK(!moved && b.p == p0 && b.cap == 256 && n_copies == 0 && live_dev == 1);
        CHECK(holds(b.p, 256, 11));
        int* typed = (int*)&stream_tag;
        fail_alloc_in = 1;
        CHECK(b.ensure_as(1000, &typed) == hipErrorOutOfMemory && (void*)typed == p0);   // the typed pointer names the buffer as it is
        CHECK(b.ensure(1000, &moved, true, stream) == hipSuccess && moved && b.cap == 1024 && holds(b.p, 256, 11));
    }
    CHECK(live_dev == 0);
    {   // three in a row, the first failing (rebuild_incidence_device's shape): the failure is what the sequence reports
        DevBuf a, b, c;
        auto three = [&]() -> hipError_t {
            hipError_t e;
            if ((e = a.ensure(1024)) != hipSuccess) return e;
            if ((e = b.ensure(1024)) != hipSuccess) return e;
            return c.ensure(4096);
        };
        fail_alloc_in = 1;
        CHECK(three() == hipErrorOutOfMemory);
        CHECK(a.p == nullptr && b.p == nullptr && c.p == nullptr && live_dev == 0);   // ... and nothing behind it ran
        fail_alloc_in = 2;
        CHECK(three() == hipErrorOutOfMemory && a.p && b.p == nullptr && c.p == nullptr);
        CHECK(three() == hipSuccess && a.p && b.p && c.p && live_dev == 3);
    }
    CHECK(live_dev == 0);
    {   // Pinned: bytes + bytes/2 rounded up to 4096, the old block freed first, contents never kept
        Pinned h;
        CHECK(h.ensure(0) == hipSuccess && h.p == nullptr && h.cap == 0);
        CHECK(h.ensure(1) == hipSuccess && h.p && h.cap == 4096 && live_host == 1);
        void* p0 = h.p;
        CHECK(h.ensure(4096) == hipSuccess && h.p == p0 && h.cap == 4096);
        CHECK(h.ensure(4097) == hipSuccess && h.cap == 8192 && live_host == 1);   // 4097 + 2048 = 6145 -> 8192
        CHECK(h.ensure(100000) == hipSuccess && h.cap == 151552 && live_host == 1);   // 150000 -> 37 pages
        // a failure leaves nothing: the old block is gone (it was freed first)
        fail_alloc_in = 1;
        CHECK(h.ensure(200000) == hipErrorOutOfMemory && h.p == nullptr && h.cap == 0 && live_host == 0);
        CHECK(h.ensure(10) == hipSuccess && h.p && h.cap == 4096 && live_host == 1);
        CHECK(live_dev == 0);   // (Pinned never touches device memory)
    }
    CHECK(live_host == 0);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("DEVBUF_OK\n");
    return 0;
}
