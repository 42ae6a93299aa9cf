// dpt_bpe_table.h -- the pair table of a greedy BPE merge (include/dpt.h dpt_bpe_create): its format and the one
// probe function the builder (dpt_bpe.cpp), the merge kernel (dpt_bpe.hip) and the debug call (dpt_debug_bpe_lookup)
// all run.
//
// The table is a hash keyed by the 64-bit pair (left, right) with the value {merged, rank}: entries of 16 bytes
// {left, right, merged, rank} (left = -1: free), buckets of two entries (32 bytes, one pair of 16-byte loads), and two
// choices per key -- buckets bpe_bucket(.., 0) and bpe_bucket(.., 1), found by cuckoo placement as TokHashHeader's
// table is.  A lookup loads its two buckets at once and compares the whole key: a pair that is absent matches
// nothing, and no lookup ever walks a chain.  n_buckets = n_pairs (not a power of two: the bucket is the high half
// of hash * n_buckets), so the load is 0.5 whatever the size: 32 bytes per pair.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpt {

constexpr uint32_t BPE_NO_RANK = 0xFFFFFFFFu;   // a miss's rank (its merged id is -1)

struct BpeHeader {
    uint32_t n_buckets;   // buckets of two entries
    uint32_t seed;
};

// the key's bucket of choice `which` (0, 1) among n_buckets
__host__ __device__ inline uint32_t bpe_bucket(uint32_t left, uint32_t right, uint32_t seed, uint32_t n_buckets, unsigned which) {
    const uint64_t k = ((uint64_t)left << 32 | right) ^ ((uint64_t)seed << 17 | seed);
    // two multiply-xorshift rounds (the 64-bit finaliser of splitmix64), one odd constant set per choice
    uint64_t x = k * (which ? 0xD6E8FEB86659FD93ull : 0x9E3779B97F4A7C15ull);
    x ^= x >> 32;
    x *= which ? 0xFF51AFD7ED558CCDull : 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    return (uint32_t)(((x >> 32) * (uint64_t)n_buckets) >> 32);
}

// The entry of (left, right) in `entries` (2 * n_buckets x {left, right, merged, rank}): true and its value, or false,
// *merged = -1 and *rank = BPE_NO_RANK.  left, right >= 0.
__host__ __device__ inline bool bpe_probe(const uint4 *__restrict__ entries, BpeHeader h, int32_t left, int32_t right,
                                          int32_t *merged, uint32_t *rank) {
    const uint32_t b0 = bpe_bucket((uint32_t)left, (uint32_t)right, h.seed, h.n_buckets, 0);
    const uint32_t b1 = bpe_bucket((uint32_t)left, (uint32_t)right, h.seed, h.n_buckets, 1);
    // (all four loads are issued before the first compare: one round trip, not two)
    const uint4 e[4] = {entries[2 * (size_t)b0], entries[2 * (size_t)b0 + 1], entries[2 * (size_t)b1], entries[2 * (size_t)b1 + 1]};
    *merged = -1;
    *rank = BPE_NO_RANK;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (e[k].x == (uint32_t)left && e[k].y == (uint32_t)right) {
            *merged = (int32_t)e[k].z;
            *rank = e[k].w;
            hit = true;
        }
    }
    return hit;
}

}  // namespace dpt
