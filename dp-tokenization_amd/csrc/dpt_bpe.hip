// dpt_bpe.hip -- the tokenizer's own (greedy BPE) encoding on the device (include/dpt.h dpt_bpe_encode).
//
// One wave per string in a grid-stride loop, four waves to a block, as dpt_decode.hip.  A string's bytes come 64 to a
// round with one lane per byte; the lanes on an atom's first byte walk the vocabulary's trie over the atom and get its
// id, and the round's ids are compacted (a ballot and a popcount) into the wave's window in LDS: up to WIN symbols
// of whole words, each slot with its symbol, the cached {rank, merged id} of the pair it opens, the links to its live
// neighbours inside the word and the slot of its word's first symbol.  When the window holds more than WIN - 64
// symbols, or the string ends, all its complete words merge at once:
//   every iteration, every live pair adds (rank << 32 | slot) to its word's 64-bit LDS minimum; the pair that finds
//   its own key there is the word's pair of lowest (rank, position) and merges -- its left slot takes the merged id,
//   its right slot dies, the links close over it -- and only the two pairs beside it are looked up again.
// So the iterations are the most merges any one word takes, the hash lookups one per atom plus two per merge, all in
// parallel, and one merge per word and iteration is exactly the sequential rule (merging every local minimum is not:
// see the header).  The live slots then go out compacted, 64 to a store, with their word index, and the open word
// at the window's end moves to its front.
//
// A word of more than W_LDS atoms that does not fit the window is merged in place in the string's own output slots
// (it holds at most one symbol per atom there): every step scans all its pairs for the lowest (rank, position), 64
// to a load, merges it and closes the gap.  Quadratic and slow, exact for any length, no workspace.
//
// No atomics on global memory, no workspace.  The only stores are counts[s], status[s] and ids / tok_word at indices
// below the string's own byte count from its own base.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_bpe_table.h"
#include "dpt_internal.h"
#include "dpt_wave.h"

namespace dpt {
namespace bpe {

constexpr unsigned WAVES = 4;           // strings per block of 256 threads
constexpr unsigned W_LDS = 256;         // words of up to this many atoms always merge in LDS
constexpr unsigned WIN = W_LDS + 128;   // slots of a wave's window
constexpr unsigned FLUSH = WIN - 64;    // a window holding more than this merges before the next round
constexpr unsigned NIL = 0xFFFFu;       // no neighbour
constexpr int32_t DEAD = -1;            // a slot merged away
constexpr int32_t TERM = (int32_t)0x80000000, LEAF = 0x40000000, BASE_MASK = 0x3FFFFFFF;   // (dpt_vocab.cpp)
static_assert(FLUSH > W_LDS, "a word that fills the window past FLUSH must be longer than W_LDS");

struct Win {
    unsigned long long wmin[WIN];   // per word (at its first slot): the lowest rank << 32 | slot of this iteration
    int32_t sym[WIN];
    uint32_t rank[WIN];             // of the pair (this slot, its next live slot); BPE_NO_RANK: none
    int32_t mrg[WIN];
    uint16_t nxt[WIN], prv[WIN];    // live neighbours inside the word, or NIL
    uint16_t head[WIN];             // the slot of the word's first symbol
};

// The lanes of one wave exchange data through its window: LDS operations of a wave complete in order, so all that
// is needed is that the compiler keeps them in order.
__device__ __forceinline__ void win_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ uint64_t uni64(uint64_t x) { return ((uint64_t)uni((unsigned)(x >> 32)) << 32) | uni((unsigned)x); }
__device__ __forceinline__ unsigned popc64(uint64_t x) { return (unsigned)__builtin_popcountll(x); }
__device__ __forceinline__ uint64_t below(unsigned lane) { return (1ull << lane) - 1ull; }   // lane < 64

// The id of the token with exactly the bytes of the atom that starts at byte p of the string (text / mask + base,
// n bytes), or -1.  The atom ends before the next byte whose mask has bit 0 or 1, or at the string's end.
__device__ __forceinline__ int32_t atom_id(const BpeLaunch &a, uint64_t base, uint64_t n, uint64_t p) {
    int32_t node = 0;
    uint32_t nb = (uint32_t)a.root_base;
    for (uint64_t q = p;; q++) {
        const uint32_t t = nb + a.text[base + q];
        if (t >= a.n_slots) return -1;
        const int4 e = a.slots4[t];
        if (e.y != node) return -1;
        node = (int32_t)t;
        if (q + 1 >= n || (a.cut_mask[base + q + 1] & 3u)) return (e.x & TERM) ? e.z : -1;
        if (e.x & LEAF) return -1;
        nb = (uint32_t)(e.x & BASE_MASK);
    }
}

// The long word g[0 .. m) in global memory (the string's own slots) merged in place; returns its tokens.
__device__ __forceinline__ uint64_t merge_in_place(const BpeLaunch &a, int32_t *g, uint64_t m, unsigned lane) {
    auto ld = [&](uint64_t i) { return __hip_atomic_load(&g[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto st = [&](uint64_t i, int32_t v) { __hip_atomic_store(&g[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    for (;;) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");   // the stores of the step before (or of the caller) are seen
        __builtin_amdgcn_wave_barrier();
        unsigned long long best = ~0ull;
        int32_t best_m = -1;
        for (uint64_t i0 = 0; i0 + 1 < m; i0 += 64) {
            const uint64_t i = i0 + lane;
            if (i + 1 < m) {
                const int32_t l = ld(i), r = ld(i + 1);
                int32_t mg;
                uint32_t rk;
                if (l >= 0 && r >= 0 && bpe_probe(a.entries, a.header, l, r, &mg, &rk)) {
                    const unsigned long long key = (unsigned long long)rk << 32 | (uint32_t)i;
                    if (key < best) best = key, best_m = mg;
                }
            }
        }
        unsigned long long all = best;
#pragma unroll
        for (unsigned k = 1; k < 64; k <<= 1) {
            const unsigned lo = lane_read((unsigned)all, lane ^ k), hi = lane_read((unsigned)(all >> 32), lane ^ k);
            const unsigned long long o = (unsigned long long)hi << 32 | lo;
            all = o < all ? o : all;
        }
        all = uni64(all);
        if (all == ~0ull) break;
        const unsigned owner = (unsigned)__builtin_ctzll(ballot(best == all));
        const int32_t merged = __builtin_amdgcn_readlane(best_m, (int)owner);
        const uint64_t pos = (uint32_t)all;
        if (lane == 0) st(pos, merged);
        // close the gap: g[i] = g[i + 1] from pos + 1 on, 64 to a step -- a step's loads all return before its stores
        // go out (one wait for the whole wave), and the next step's loads lie beyond them
        for (uint64_t i0 = pos + 1; i0 + 1 < m; i0 += 64) {
            const uint64_t i = i0 + lane;
            const bool have = i + 1 < m;
            const int32_t v = have ? ld(i + 1) : 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            __builtin_amdgcn_wave_barrier();
            if (have) st(i, v);
        }
        m -= 1;
    }
    return m;
}

__global__ void __launch_bounds__(WAVES * 64) bpe_kernel(BpeLaunch a) {
    __shared__ Win wins[WAVES];
    Win &w = wins[uni(threadIdx.x >> 6)];
    const unsigned lane = lane_id();
    const uint64_t lt = below(lane), le = lt | 1ull << lane;
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES + uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
    const uint64_t so0 = a.str_off[0];
    for (uint64_t s = wave; s < a.n_str; s += n_waves) {
        const uint64_t base = uni64(a.str_off[s] - so0);
        const uint64_t n = uni64(a.str_off[s + 1] - a.str_off[s]);
        int32_t *const out = a.ids + base;
        uint32_t *const out_word = a.tok_word ? a.tok_word + base : nullptr;
        uint64_t n_out = 0;        // tokens written so far
        uint32_t n_words = 0;      // words they make up
        unsigned fill = 0;         // symbols in the window; slot 0 always opens a word
        unsigned open_head = 0;    // the slot of the window's last word start: the word still open
        bool long_mode = false;    // the open word lives at out[n_out .. n_out + long_len), not in the window
        uint64_t long_len = 0;
        bool bad = false;

        // [0, L) of the window -- whole words -- merged and written out; [L, fill) moves to the front
        auto merge_window = [&](unsigned L) {
            const unsigned n_ch = (L + 63u) / 64u;
            for (unsigned c = 0; c < n_ch; c++) {
                const unsigned i = c * 64u + lane;
                if (i < L) {
                    const unsigned h = w.head[i];
                    const bool has_next = i + 1 < L && w.head[i + 1] == h;
                    int32_t mg = -1;
                    uint32_t rk = BPE_NO_RANK;
                    if (has_next) bpe_probe(a.entries, a.header, w.sym[i], w.sym[i + 1], &mg, &rk);
                    w.rank[i] = rk;
                    w.mrg[i] = mg;
                    w.nxt[i] = (uint16_t)(has_next ? i + 1 : NIL);
                    w.prv[i] = (uint16_t)(i > 0 && w.head[i - 1] == h ? i - 1 : NIL);
                    w.wmin[i] = ~0ull;
                }
            }
            win_sync();
            for (;;) {
                bool some = false;
                for (unsigned c = 0; c < n_ch; c++) {
                    const unsigned i = c * 64u + lane;
                    const uint32_t rk = i < L ? w.rank[i] : BPE_NO_RANK;
                    if (rk != BPE_NO_RANK) {
                        __hip_atomic_fetch_min(&w.wmin[w.head[i]], (unsigned long long)rk << 32 | i, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                        some = true;
                    }
                }
                if (!ballot(some)) break;
                win_sync();
                for (unsigned c = 0; c < n_ch; c++) {
                    const unsigned i = c * 64u + lane;
                    const uint32_t rk = i < L ? w.rank[i] : BPE_NO_RANK;
                    // (a pair beside a merge of an earlier chunk has a new rank by now and finds the word's minimum
                    // reset, or another slot's key in it: one merge per word and iteration)
                    const bool win = rk != BPE_NO_RANK && w.wmin[w.head[i]] == ((unsigned long long)rk << 32 | i);
                    if (win) {
                        const unsigned j = w.nxt[i], nx = w.nxt[j], pv = w.prv[i];
                        const int32_t me = w.mrg[i];
                        w.wmin[w.head[i]] = ~0ull;
                        w.sym[i] = me;
                        w.sym[j] = DEAD;
                        w.rank[j] = BPE_NO_RANK;
                        w.nxt[i] = (uint16_t)nx;
                        if (nx != NIL) w.prv[nx] = (uint16_t)i;
                        int32_t mg = -1;
                        uint32_t r2 = BPE_NO_RANK;
                        if (nx != NIL) bpe_probe(a.entries, a.header, me, w.sym[nx], &mg, &r2);
                        w.rank[i] = r2;
                        w.mrg[i] = mg;
                        if (pv != NIL) {
                            bpe_probe(a.entries, a.header, w.sym[pv], me, &mg, &r2);
                            w.rank[pv] = r2;
                            w.mrg[pv] = mg;
                        }
                    }
                    win_sync();
                }
            }
            win_sync();
            // the live slots, compacted, with the index of their word
            for (unsigned c = 0; c < n_ch; c++) {
                const unsigned i = c * 64u + lane;
                const int32_t v = i < L ? w.sym[i] : DEAD;
                const bool live = v != DEAD;
                const uint64_t lb = ballot(live), hb = ballot(live && w.head[i] == i);
                const uint64_t pos = n_out + popc64(lb & lt);
                if (live && pos < n) {
                    out[pos] = v;
                    if (out_word) out_word[pos] = n_words + popc64(hb & le) - 1u;
                }
                n_out += popc64(lb);
                n_words += popc64(hb);
            }
            // the open word to the front (chunk by chunk: a chunk is read whole before it is written lower down)
            const unsigned rest = fill - L;
            for (unsigned c = 0; c * 64u < rest; c++) {
                const unsigned i = c * 64u + lane;
                const int32_t v = i < rest ? w.sym[L + i] : 0;
                win_sync();
                if (i < rest) {
                    w.sym[i] = v;
                    w.head[i] = 0;
                }
                win_sync();
            }
            fill = rest;
            open_head = 0;
        };
        // the long word's end: merged where it lies
        auto close_long = [&]() {
            const uint64_t m = merge_in_place(a, out + n_out, long_len, lane);
            if (out_word)
                for (uint64_t i = lane; i < m && n_out + i < n; i += 64) out_word[n_out + i] = n_words;
            n_out += m;
            n_words += 1;
            long_mode = false;
            long_len = 0;
        };

        for (uint64_t k0 = 0; k0 < n; k0 += 64) {
            const uint64_t p = k0 + lane;
            const bool have = p < n;
            unsigned m = have ? a.cut_mask[base + p] : 0u;
            if (p == 0) m |= 3u;   // a string opens a word whatever its mask says
            const bool atom = have && (m & 3u), wstart = have && (m & 1u);
            const int32_t id = atom ? atom_id(a, base, n, p) : 0;
            if (ballot(atom && id < 0)) {
                bad = true;
                break;
            }
            const uint64_t ab = ballot(atom), wb = ballot(wstart);
            const unsigned r = popc64(ab & lt), n_atoms = popc64(ab);
            const uint64_t mine = wb & le;   // the word starts of this round at or before this lane
            // the index, among the round's atoms, of the word start this lane's atom belongs to
            const unsigned h_idx = mine ? popc64(ab & below(63u - (unsigned)__builtin_clzll(mine))) : 0u;
            unsigned skip = 0;   // the round's atoms that do not go to the window
            if (long_mode) {
                // the atoms before the round's first word start still belong to the long word
                skip = wb ? popc64(ab & below((unsigned)__builtin_ctzll(wb))) : n_atoms;
                if (atom && r < skip && n_out + long_len + r < n) out[n_out + long_len + r] = id;
                long_len += skip;
                if (!wb) continue;
                close_long();
            }
            if (atom && r >= skip) {
                const unsigned slot = fill + r - skip;
                w.sym[slot] = id;
                w.head[slot] = (uint16_t)(mine ? fill + h_idx - skip : open_head);
            }
            if (wb) open_head = fill + popc64(ab & below(63u - (unsigned)__builtin_clzll(wb))) - skip;
            fill += n_atoms - skip;
            win_sync();
            if (fill > FLUSH) {
                if (open_head != 0) merge_window(open_head);   // the whole words; the open one moves to the front
                if (fill > FLUSH) {
                    // one open word of more than FLUSH atoms is all the window holds: it goes on in the string's own
                    // output slots, and the window is free for the next round whatever that brings
                    for (unsigned i = lane; i < fill; i += 64)
                        if (n_out + i < n) out[n_out + i] = w.sym[i];
                    long_mode = true;
                    long_len = fill;
                    fill = 0;
                    win_sync();
                }
            }
        }
        if (!bad) {
            if (long_mode) close_long();
            else if (fill) merge_window(fill);
        }
        if (lane == 0) {
            a.counts[s] = bad ? 0 : n_out;
            a.status[s] = bad ? DPT_STATUS_NO_TOKENIZATION : DPT_STATUS_OK;
        }
        win_sync();
    }
}

}  // namespace bpe

hipError_t launch_bpe(const BpeLaunch &p, hipStream_t stream) {
    if (p.n_str == 0) return hipSuccess;
    hipLaunchKernelGGL(bpe::bpe_kernel, dim3(wave_per_string_blocks(p.n_str, bpe::WAVES)), dim3(bpe::WAVES * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpt
