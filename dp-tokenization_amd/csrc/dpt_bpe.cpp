// dpt_bpe.cpp -- the pair table of the default (greedy BPE) encoding (include/dpt.h dpt_bpe_create): its host builder,
// the object that holds its device copy, and the debug lookup.  The format and the probe are in dpt_bpe_table.h; the
// merge kernel is in dpt_bpe.hip and its entry point in dpt_api.cpp.
//
// build_bpe_tables calls no HIP function: testable without a device (dpt_debug_bpe_lookup, tests/test_bpe_abi.py).
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "dpt_bpe_table.h"
#include "dpt_objects.h"

namespace dpt {

const char *build_bpe_tables(const int32_t *left, const int32_t *right, const int32_t *merged, const uint32_t *rank,
                             uint64_t n_pairs, BpeTables *out) try {
    if (!left || !right || !merged || !rank) return "null pair table";
    if (n_pairs == 0 || n_pairs >= (1ull << 31)) return "0 pairs, or 2^31 or more";
    for (uint64_t k = 0; k < n_pairs; k++) {
        if (left[k] < 0 || right[k] < 0 || merged[k] < 0) return "a negative id in the pair table";
        if (rank[k] == BPE_NO_RANK) return "rank 0xFFFFFFFF is the miss value";
    }
    const uint32_t nb = (uint32_t)n_pairs;
    const uint4 free_entry = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, BPE_NO_RANK);
    for (uint32_t seed = 0x2545F491u, tries = 0; tries < 8; tries++, seed = seed * 0x9E3779B9u + 0x7F4A7C15u) {
        std::vector<uint4> tab((size_t)nb * 2, free_entry);
        const BpeHeader h{nb, seed};
        auto bucket = [&](const uint4 &e, unsigned which) { return bpe_bucket(e.x, e.y, seed, nb, which); };
        bool bad = false;
        uint32_t rng = seed | 1u;
        for (uint64_t k = 0; k < n_pairs && !bad; k++) {
            int32_t m;
            uint32_t r;
            if (bpe_probe(tab.data(), h, left[k], right[k], &m, &r)) return "a (left, right) pair given twice";
            // cuckoo placement: a free entry of the key's two buckets, else evict one (a pseudo-random walk) and the
            // evicted key moves on to its other bucket
            uint4 cur = make_uint4((uint32_t)left[k], (uint32_t)right[k], (uint32_t)merged[k], rank[k]);
            uint32_t b = bucket(cur, 0);
            bool placed = false;
            for (int kick = 0; kick < 2000 && !placed; kick++) {
                const uint32_t b0 = bucket(cur, 0), b1 = bucket(cur, 1);
                const uint32_t other = b == b0 ? b1 : b0;
                for (const size_t e : {2 * (size_t)b, 2 * (size_t)b + 1, 2 * (size_t)other, 2 * (size_t)other + 1})
                    if (!placed && tab[e].x == 0xFFFFFFFFu) { tab[e] = cur; placed = true; }
                if (placed) break;
                rng = rng * 1664525u + 1013904223u;
                const size_t ve = 2 * (size_t)((rng >> 16) & 1u ? other : b) + ((rng >> 17) & 1u);
                const uint4 victim = tab[ve];
                tab[ve] = cur;
                cur = victim;
                // the victim moves to the bucket it was not in
                const uint32_t vb = (uint32_t)(ve >> 1);
                b = bucket(cur, 0) == vb ? bucket(cur, 1) : bucket(cur, 0);
            }
            bad = !placed;
        }
        if (bad) continue;
        out->header = h;
        out->entries = std::move(tab);
        return nullptr;
    }
    return "no seed places every pair";
} catch (const std::bad_alloc &) {
    return "out of host memory";
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_debug_bpe_lookup(const int32_t *left, const int32_t *right, const int32_t *merged, const uint32_t *rank,
                         uint64_t n_pairs, const int32_t *q_left, const int32_t *q_right, uint64_t n_q, int32_t *out_merged,
                         uint32_t *out_rank) {
    if (n_q && (!q_left || !q_right || !out_merged || !out_rank)) return fail(DPT_E_ARG, "null query / result");
    BpeTables t;
    if (const char *err = build_bpe_tables(left, right, merged, rank, n_pairs, &t)) return fail(DPT_E_ARG, err);
    for (uint64_t q = 0; q < n_q; q++) {
        out_merged[q] = -1;
        out_rank[q] = BPE_NO_RANK;
        if (q_left[q] >= 0 && q_right[q] >= 0) bpe_probe(t.entries.data(), t.header, q_left[q], q_right[q], &out_merged[q], &out_rank[q]);
    }
    return DPT_OK;
}

int dpt_bpe_create(const int32_t *left, const int32_t *right, const int32_t *merged, const uint32_t *rank, uint64_t n_pairs,
                   int device, dpt_bpe **out) {
    if (!out) return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    BpeTables t;
    if (const char *err = build_bpe_tables(left, right, merged, rank, n_pairs, &t)) return fail(DPT_E_ARG, err);
    if (const int rc = check_device_and_table(device, nullptr, 0)) return rc;
    DeviceGuard g(device);
    dpt_bpe *p = new (std::nothrow) dpt_bpe();
    if (!p) return fail(DPT_E_ARG, "out of host memory");
    p->device = device; p->n_buckets = t.header.n_buckets; p->seed = t.header.seed;
    const hipError_t e = upload(&p->d_entries, t.entries);
    if (e != hipSuccess) {
        dpt_bpe_destroy(p);
        return hip_fail(e, "pair table upload");
    }
    *out = p;
    return DPT_OK;
}

int dpt_bpe_destroy(dpt_bpe *p) {
    if (!p) return DPT_OK;
    DeviceGuard g(p->device);
    (void)hipFree(p->d_entries);
    delete p;
    return DPT_OK;
}

}  // extern "C"
