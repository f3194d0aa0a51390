// k_levels.hip -- level compaction of a host-uploaded manifold set (manifolds_upload, once per upload).
// The reference fixes, per body, the ORDER in which its manifolds touch it (overflow list, then colours 0..22); which manifolds share a
// launch is free.  level(m) = max over m's ordering bodies of next[body]; next[body] = level(m) + 1, colours visited in order: the same
// per-body sequences in as few launches as the deepest body allows.  The kernels here build the levels from the STAGED body1 / body2 (upload
// order, colour-major) and the permutation upload position -> level-major position; the solve kernels never see any of it.
#include "avn_kernels.h"

namespace avn {

#define LVL_NONORD 0x80000000u   // mask bit: two manifolds of one colour name the body -- the host coloured it as static: it orders nothing

// pass 1: per body the set of colours 0..22 that name it; a colour seen twice raises LVL_NONORD.  The rule reads the lists alone, never body state: a later
// bodies_upload cannot invalidate it.  Same-address atomics serialise and cfg2's ground slab is named by the 2 500 manifolds of ONE colour, which
// sit side by side in the list: a run of neighbouring lanes with the same (body, colour) sends ONE atomic, from its first lane, with the verdict already in it;
// and a body already known to be shared costs a plain load.  (An index out of range is skipped here and rejected by the host pass of the upload.)
__global__ __launch_bounds__(256) void k_level_masks(const int32_t* __restrict__ body1, const int32_t* __restrict__ body2, uint32_t n_bodies, LevelOffsets offs, uint32_t* __restrict__ mask) {
    const uint32_t m = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = m < offs.o[AVN_COLOR_OVERFLOW_INDEX];
    uint32_t c = 0;
    while (c + 1 < (uint32_t)AVN_COLOR_OVERFLOW_INDEX && m >= offs.o[c + 1]) ++c;
    const uint32_t bit = 1u << c;
    const int32_t bb[2] = {live ? body1[m] : -1, live ? body2[m] : -1};
    bool send[2], same_next[2];
    for (int s = 0; s < 2; ++s) {   // (all lanes of the wave take part in the shuffles: nothing has diverged yet)
        // key of the run: (body, colour); negative and unlike its neighbours' for a lane that sends nothing
        const long long key = (uint32_t)bb[s] < n_bodies && !(s == 1 && bb[1] == bb[0]) ? ((long long)bb[s] << 5 | c) : -1ll - (long long)lane;
        const int klo = (int)(uint32_t)key, khi = (int)(uint32_t)((unsigned long long)key >> 32);
        const bool same_prev = lane > 0u && __shfl_up(klo, 1) == klo && __shfl_up(khi, 1) == khi;
        same_next[s] = lane < 63u && __shfl_down(klo, 1) == klo && __shfl_down(khi, 1) == khi;
        send[s] = key >= 0 && !same_prev;
    }
    for (int s = 0; s < 2; ++s) {
        if (!send[s]) continue;
        uint32_t* p = mask + bb[s];
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & LVL_NONORD) continue;
        if (same_next[s]) atomicOr(p, bit | LVL_NONORD);
        else if (atomicOr(p, bit) & bit) atomicOr(p, LVL_NONORD);
    }
}

// pass 2: the largest number of colours on one ordering body = the floor of launches under the reference's per-body order
__global__ __launch_bounds__(256) void k_level_max_degree(const uint32_t* __restrict__ mask, uint32_t n_bodies, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = b < n_bodies ? mask[b] : 0u;
    const uint32_t deg = (v & LVL_NONORD) ? 0u : (uint32_t)__popc(v);
    if (deg) atomicMax(&s_max, deg);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(out, s_max);
}

// pass 3, one launch per populated colour, in order: inside a colour no two manifolds share an ordering body, so next[] has one writer per entry
__global__ __launch_bounds__(256) void k_level_colour(const int32_t* __restrict__ body1, const int32_t* __restrict__ body2,
                                                      uint32_t n_bodies, const uint32_t* __restrict__ mask, uint32_t first, uint32_t count,
                                                      uint32_t* __restrict__ next, uint8_t* __restrict__ level) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint32_t m = first + i;
    const int32_t a = body1[m], b = body2[m];
    const bool oa = (uint32_t)a < n_bodies && !(mask[a] & LVL_NONORD);
    const bool ob = (uint32_t)b < n_bodies && !(mask[b] & LVL_NONORD);
    const uint32_t la = oa ? next[a] : 0u, lb = ob ? next[b] : 0u;
    const uint32_t lv = la > lb ? la : lb;
    level[m] = (uint8_t)lv;
    if (oa) next[a] = lv + 1u;
    if (ob) next[b] = lv + 1u;
}

// pass 4: stable counting sort by level over tiles of LVL_TILE manifolds (one per thread): tile histograms, one scan over [level][tile], ranks.
// Manifolds of the overflow colour (positions >= n_coloured) keep their place.
__device__ __forceinline__ uint32_t lvl_tile_counts(uint32_t lv, uint32_t (*cnt)[AVN_COLOR_OVERFLOW_INDEX], uint32_t* prefix_in_wave) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t mine = 0u;
    for (uint32_t k = 0; k < (uint32_t)AVN_COLOR_OVERFLOW_INDEX; ++k) {
        const unsigned long long bal = __ballot(lv == k);
        if (lane == 0u) cnt[wv][k] = (uint32_t)__popcll(bal);
        if (lv == k) mine = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    }
    *prefix_in_wave = mine;
    __syncthreads();
    return wv;
}
__global__ __launch_bounds__(LVL_TILE) void k_level_hist(const uint8_t* __restrict__ level, uint32_t n_coloured, uint32_t n_tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[LVL_TILE / 64][AVN_COLOR_OVERFLOW_INDEX];
    const uint32_t m = blockIdx.x * LVL_TILE + threadIdx.x;
    const uint32_t lv = m < n_coloured ? level[m] : 0xFFu;
    uint32_t unused;
    lvl_tile_counts(lv, cnt, &unused);
    if (threadIdx.x < (uint32_t)AVN_COLOR_OVERFLOW_INDEX) {
        uint32_t s = 0u;
        for (uint32_t w = 0; w < LVL_TILE / 64; ++w) s += cnt[w][threadIdx.x];
        hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = s;
    }
}
// perm[m] = level-major position of upload position m.  res[0..23) = the offsets the solver runs, res[23] = 1 when some manifold changes place.
// The early out is decided HERE, from the degree the second kernel left in *max_degree: when it equals the populated colours no schedule has fewer launches,
// the permutation is the identity and the offsets are the uploaded ones -- the host learns of it with the read-back its upload ends with anyway.
__global__ __launch_bounds__(LVL_TILE) void k_level_scatter(const uint8_t* __restrict__ level, LevelOffsets offs, uint32_t n_tiles, const uint32_t* __restrict__ scanned,
                                                            const uint32_t* __restrict__ max_degree, uint32_t populated, uint32_t* __restrict__ perm, uint32_t* __restrict__ res) {
    __shared__ uint32_t cnt[LVL_TILE / 64][AVN_COLOR_OVERFLOW_INDEX];
    const uint32_t n_coloured = offs.o[AVN_COLOR_OVERFLOW_INDEX], n_manifolds = offs.o[AVN_GRAPH_COLOR_COUNT];
    const uint32_t m = blockIdx.x * LVL_TILE + threadIdx.x;
    const uint32_t lv = m < n_coloured ? level[m] : 0xFFu;
    uint32_t in_wave;
    const uint32_t wv = lvl_tile_counts(lv, cnt, &in_wave);
    const bool early = *max_degree == populated;
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)AVN_COLOR_OVERFLOW_INDEX) res[threadIdx.x] = early ? offs.o[threadIdx.x] : scanned[(size_t)threadIdx.x * n_tiles];
    if (m >= n_manifolds) return;
    uint32_t dst = m;
    if (!early && lv < (uint32_t)AVN_COLOR_OVERFLOW_INDEX) {
        dst = scanned[(size_t)lv * n_tiles + blockIdx.x] + in_wave;
        for (uint32_t w = 0; w < wv; ++w) dst += cnt[w][lv];
        if (dst != m) res[AVN_COLOR_OVERFLOW_INDEX] = 1u;   // (every writer stores the same word)
    }
    perm[m] = dst;
}

// back to upload order (a world that turns out to be a level-2 rank): dst[m] = src[perm[m]]
template <class E> __global__ __launch_bounds__(256) void k_level_unpermute(E* __restrict__ dst, const E* __restrict__ src, const uint32_t* __restrict__ perm, uint32_t n) {
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m < n) dst[m] = src[perm[m]];
}

static inline dim3 g256(uint32_t n) { return dim3((n + 255) / 256); }
uint32_t level_tiles(uint32_t n_manifolds) { return (n_manifolds + LVL_TILE - 1) / LVL_TILE; }
uint32_t level_zeroed_words(uint32_t n_bodies, uint32_t n_manifolds) { return 2u * n_bodies + LVL_RES_WORDS + scan_block_sums_needed((uint32_t)AVN_COLOR_OVERFLOW_INDEX * level_tiles(n_manifolds)); }
uint32_t launch_level_build(const int32_t* body1, const int32_t* body2, uint32_t n_bodies, const LevelOffsets& offs, uint32_t populated,
                            uint32_t* zeroed, uint8_t* level, uint32_t* hist, uint32_t* perm, hipStream_t st) {
    uint32_t* mask = zeroed; uint32_t* next = zeroed + n_bodies; uint32_t* res = zeroed + 2 * (size_t)n_bodies; uint32_t* scan_state = res + LVL_RES_WORDS;
    const uint32_t n = offs.o[AVN_COLOR_OVERFLOW_INDEX], M = offs.o[AVN_GRAPH_COLOR_COUNT], nt = level_tiles(M);
    if (!n || !nt || !n_bodies) return 0;
    uint32_t launches = 5;
    hipLaunchKernelGGL(k_level_masks, g256(n), dim3(256), 0, st, body1, body2, n_bodies, offs, mask);
    hipLaunchKernelGGL(k_level_max_degree, g256(n_bodies), dim3(256), 0, st, (const uint32_t*)mask, n_bodies, res + LVL_RES_MAX_DEGREE);
    for (uint32_t c = 0; c < (uint32_t)AVN_COLOR_OVERFLOW_INDEX; ++c) {
        const uint32_t cnt = offs.o[c + 1] - offs.o[c];
        if (!cnt) continue;
        hipLaunchKernelGGL(k_level_colour, g256(cnt), dim3(256), 0, st, body1, body2, n_bodies, (const uint32_t*)mask, offs.o[c], cnt, next, level);
        ++launches;
    }
    hipLaunchKernelGGL(k_level_hist, dim3(nt), dim3(LVL_TILE), 0, st, (const uint8_t*)level, n, nt, hist);
    launch_exclusive_scan(hist, hist, (uint32_t)AVN_COLOR_OVERFLOW_INDEX * nt, scan_state, nullptr, st);   // (the tree's one-launch chained scan, k_broadphase.hip)
    hipLaunchKernelGGL(k_level_scatter, dim3(nt), dim3(LVL_TILE), 0, st, (const uint8_t*)level, offs, nt, (const uint32_t*)hist, (const uint32_t*)(res + LVL_RES_MAX_DEGREE), populated, perm, res);
    return launches;
}
struct alignas(16) Lvl32 { uint4 a, b; };
bool launch_level_unpermute(void* dst, const void* src, size_t elem_bytes, const uint32_t* perm, uint32_t n, hipStream_t st) {
    if (!n) return true;
    switch (elem_bytes) {
        case 2: hipLaunchKernelGGL(k_level_unpermute<uint16_t>, g256(n), dim3(256), 0, st, (uint16_t*)dst, (const uint16_t*)src, perm, n); return true;
        case 4: hipLaunchKernelGGL(k_level_unpermute<uint32_t>, g256(n), dim3(256), 0, st, (uint32_t*)dst, (const uint32_t*)src, perm, n); return true;
        case 8: hipLaunchKernelGGL(k_level_unpermute<uint2>, g256(n), dim3(256), 0, st, (uint2*)dst, (const uint2*)src, perm, n); return true;
        case 16: hipLaunchKernelGGL(k_level_unpermute<uint4>, g256(n), dim3(256), 0, st, (uint4*)dst, (const uint4*)src, perm, n); return true;
        case 32: hipLaunchKernelGGL(k_level_unpermute<Lvl32>, g256(n), dim3(256), 0, st, (Lvl32*)dst, (const Lvl32*)src, perm, n); return true;
        default: return false;   // no record of the manifold arrays has another size
    }
}

}  // namespace avn
