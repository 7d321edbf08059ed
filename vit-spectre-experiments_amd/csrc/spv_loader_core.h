// The resident loader's sample order (include/spv.h): the keyed bijection on [0, n) that stands in for
// DataLoader(shuffle=True)'s randperm, and the position rule that shards it over the ranks.  ONE definition for the fetch kernel of
// spv_loader.hip and for the host: no HIP type in it outside the __HIPCC__ block at the end (the cursor's protocol, device only);
// tests/test_resident_loader.py compiles it with a plain C++ compiler and holds it, bit for bit, to tests/loader_ref.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SPV_LDR_HD __host__ __device__ __forceinline__
#else
#define SPV_LDR_HD inline
#endif

constexpr int LDR_ROUNDS = 6;   // SPV_LOADER_ROUNDS

// murmur3's 64-bit finaliser, and the 32-bit finaliser of the library's dropout masks (spv_common.h mix32)
SPV_LDR_HD uint64_t ldr_mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
SPV_LDR_HD uint32_t ldr_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// the epoch's 64-bit key: for a given seed, distinct epochs give distinct keys (both steps are bijections of 64-bit words)
SPV_LDR_HD uint64_t ldr_key(uint64_t seed, uint64_t epoch) { return ldr_mix64(ldr_mix64(seed + 0x9e3779b97f4a7c15ULL) + epoch); }

// bits of one Feistel half: the smallest h >= 1 with 2^(2h) >= n
SPV_LDR_HD int ldr_half_bits(uint32_t n) {
    int h = 1;
    while (h < 16 && (1ull << (2 * h)) < (uint64_t)n) ++h;
    return h;
}

// The bijection of [0, n), 1 <= n < 2^31, x < n: a balanced Feistel network of LDR_ROUNDS rounds on 2h bits, re-applied while the
// value lies outside [0, n) (cycle-walking: the network permutes [0, 2^(2h)), so the walk from x < n comes back into [0, n), and
// 2^(2h) < 4 n keeps it short: fewer than four passes on average).
SPV_LDR_HD uint32_t ldr_permute(uint64_t key, uint32_t n, uint32_t x) {
    const int h = ldr_half_bits(n);
    const uint32_t mask = (1u << h) - 1u;
    uint32_t rk[LDR_ROUNDS];
    for (int r = 0; r < LDR_ROUNDS; ++r) rk[r] = (uint32_t)ldr_mix64(key + (uint64_t)(r + 1) * 0x9e3779b97f4a7c15ULL);
    do {
        uint32_t l = x >> h, rt = x & mask;
        for (int r = 0; r < LDR_ROUNDS; ++r) {
            const uint32_t f = ldr_mix32(rt + rk[r]) & mask;
            const uint32_t nl = rt;
            rt = l ^ f;
            l = nl;
        }
        x = (l << h) | rt;
    } while (x >= n);
    return x;
}

// who draws what: the set's size, the batch, the ranks, the steps of one epoch (steps * batch * world <= n, checked by the host)
struct LdrGeom {
    uint32_t n, batch, world, rank, steps;
    int shuffle;
};

// The position of sample r of step t in the epoch's order -- idx[rank::world] cut into batches, the tail dropped -- and the epoch.
// t is the cursor's raw 64 bits taken as unsigned: t mod steps < steps, so the position is < steps * batch * world <= n whatever t is.
SPV_LDR_HD uint64_t ldr_epoch(uint64_t t, const LdrGeom& g) { return t / g.steps; }
SPV_LDR_HD uint32_t ldr_position(uint64_t t, uint32_t r, const LdrGeom& g) {
    return (uint32_t)(((t % g.steps) * g.batch + r) * g.world + g.rank);
}
// the row of the set that sample r of step t is: always < n
SPV_LDR_HD uint32_t ldr_index(uint64_t seed, uint64_t t, uint32_t r, const LdrGeom& g) {
    const uint32_t pos = ldr_position(t, r, g);
    return g.shuffle ? ldr_permute(ldr_key(seed, ldr_epoch(t, g)), g.n, pos) : pos;
}

#if defined(__HIPCC__)
// The cursor block's protocol, ONE definition for every kernel that reads the step from it (spv_loader.hip, spv_augment.hip).
// Every workgroup reads the step, THEN announces itself; the last one to arrive -- every workgroup has its copy of t by then -- moves
// the cursor on and re-arms the counter for the next launch (the scheme of the cross-entropy kernel's join, spv_head.hip).  The read
// is an agent-scope atomic load (never served from a stale line), and the fence keeps it in front of the counter's add.
__device__ __forceinline__ uint64_t ldr_read_step(const unsigned long long* cursor) {
    return __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// FENCED = false is for a caller whose read of t is known to be complete when it arrives: the value went through LDS and a workgroup
// barrier on its way to the arriving thread, so the load has returned and nothing is left for a fence to order (the fence is an L2
// write-back and an L1 invalidate on the one wave the rest of the workgroup then waits for: microseconds).
template <bool FENCED = true>
__device__ __forceinline__ void ldr_arrive(unsigned long long* cursor, uint64_t t, unsigned groups) {
    if constexpr (FENCED) __threadfence();
    unsigned* counter = reinterpret_cast<unsigned*>(cursor + 1);
    if (atomicAdd(counter, 1u) == groups - 1) {
        __hip_atomic_store(cursor, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#endif
