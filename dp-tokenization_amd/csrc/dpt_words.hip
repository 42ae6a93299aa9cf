// dpt_words.hip -- two tokenizations of a batch compared word by word (dpt_word_compare_sizes, dpt_word_compare_write).
//
// Each side of a string is a stream of word indices, one per token: 0 0 1 2 2 2 3 ...  A well-formed stream starts
// at 0 and steps by 0 or 1, so word w is a run of equal values and the stream is described by the run ends
//   E_X(w) = the index of the first token of side X whose value is above w (n_X when there is none),
// with first(w) = E_X(w - 1) (0 for w = 0) and cnt_X(w) = E_X(w) - first(w).
//
// One wave per string, 64 words per window: lane j stands for word w0 + j.  Each side streams its values in chunks
// of 64, the next chunk loaded ahead of its use; a chunk is checked as it arrives (first value 0, steps of 0 or 1
// against the lane before -- wave_shift_in with the last value of the chunk before) and only a checked chunk, which
// is monotone, is searched: a lane finds the number of chunk values <= w by the 6-step lane_read search and has its
// run end when that number is below 64 (lanes past the stream's end hold PAD, above every word); otherwise the side
// advances.  Every round resolves a word or advances a side, so a string costs (n_a + n_b + W) / 64 rounds whatever
// the runs are, and a run of any length spans chunks for free: the open run's start is lane 0's first(), the run end
// of the window before (wave_shift_in again).  W comes from each side's last value, read before the walk; when the
// two differ or exceed the token counts the string is malformed at once.  After the last window the last run must
// end at n_X on both sides, which also proves that every chunk was loaded and checked.
//
// The selected words of a window are compacted by a ballot prefix (mbcnt) in registers: no LDS, no atomics, no
// workspace.  write guards every store with the string's own word_off / sel_off range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_internal.h"
#include "dpt_wave.h"

namespace dpt {
namespace wrd {

constexpr unsigned WAVES = 4;            // strings per block of 256 threads
constexpr uint32_t PAD = 0xFFFFFFFFu;    // a chunk lane at or past the stream's end: above every word of a stream

__device__ __forceinline__ bool any(bool p) { return ballot(p) != 0; }
__device__ __forceinline__ uint32_t lane_value(uint32_t v, unsigned l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }

// One side of one string: the stream and the chunk [k0, k0 + 64) of it that the words are searched in.
struct Stream {
    const uint32_t *w;     // the string's first value
    uint64_t n;            // tokens
    uint64_t k0;           // the chunk's first token
    uint32_t v, next;      // lane i: w[k0 + i] and w[k0 + 64 + i], PAD at or past n
};

__device__ __forceinline__ uint32_t chunk_load(const Stream &x, uint64_t k0, unsigned lane) {
    const uint64_t k = k0 + lane;
    return k < x.n ? x.w[k] : PAD;
}

// The chunk at x.k0 is well-formed behind `before`, the value ahead of it (unused at k0 = 0).
__device__ __forceinline__ bool chunk_ok(const Stream &x, uint32_t before, unsigned lane) {
    const uint64_t k = x.k0 + lane;
    const uint32_t prev = wave_shift_in(x.v, before);
    const bool fine = k >= x.n || (k == 0 ? x.v == 0u : x.v - prev <= 1u);
    return !any(!fine);
}

__device__ __forceinline__ bool stream_open(Stream &x, const dpt_word_side &side, uint64_t s, unsigned lane) {
    x.w = side.tok_word + (side.off[s] - side.off[0]);
    x.n = side.counts ? side.counts[s] : side.off[s + 1] - side.off[s];
    x.k0 = 0;
    x.v = chunk_load(x, 0, lane);
    x.next = chunk_load(x, 64, lane);
    return chunk_ok(x, 0u, lane);
}

__device__ __forceinline__ bool stream_advance(Stream &x, unsigned lane) {
    const uint32_t before = lane_value(x.v, 63);   // (a chunk with a successor is full)
    x.k0 += 64;
    x.v = x.next;
    x.next = chunk_load(x, x.k0 + 64, lane);
    return chunk_ok(x, before, lane);
}

// E(w) for the lanes with act: false when a chunk met on the way is malformed.
__device__ __forceinline__ bool run_ends(Stream &x, uint32_t w, bool act, unsigned lane, uint32_t &end) {
    bool pend = act;
    end = 0;
    while (any(pend)) {
        // m = the values <= w among the chunk's first 63 (the chunk is monotone); lane m holds the first one above w,
        // or the chunk has none
        uint32_t m = 0;
#pragma unroll
        for (unsigned step = 32; step; step >>= 1)
            if (lane_read(x.v, m + step - 1) <= w) m += step;
        // (every lane reads, pending or not: a lane switched off by a short-circuit && would hand the lanes that
        // read it nothing, and the lanes already resolved are the ones the pending lanes read)
        const uint32_t above = lane_read(x.v, m);
        const bool can = pend && above > w;
        if (!any(can)) {
            if (!stream_advance(x, lane)) return false;
            continue;
        }
        if (can) end = (uint32_t)(x.k0 + m);
        pend = pend && !can;
    }
    return true;
}

__device__ __forceinline__ void put(uint32_t *dst, uint64_t at, uint32_t value) {
    if (dst) dst[at] = value;
}

template <bool WRITE>
__global__ void __launch_bounds__(WAVES * 64) words_kernel(WordsLaunch p) {
    const unsigned lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES + uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
    const bool less = (p.flags & DPT_WORDS_LESS) != 0, greater = (p.flags & DPT_WORDS_GREATER) != 0;
    for (uint64_t s = wave; s < p.n_str; s += n_waves) {
        const int32_t st_a = p.a.status ? p.a.status[s] : 0, st_b = p.b.status ? p.b.status[s] : 0;
        if (st_a != 0 || st_b != 0) {   // nothing of a failed side is read but its count
            if (lane == 0) {
                p.wc_status[s] = st_a != 0 ? st_a : st_b;
                if (!WRITE) {
                    p.n_words[s] = 0;
                    p.n_sel[s] = 0;
                    const uint64_t na = p.a.counts ? p.a.counts[s] : p.a.off[s + 1] - p.a.off[s];
                    const uint64_t nb = p.b.counts ? p.b.counts[s] : p.b.off[s + 1] - p.b.off[s];
                    put(p.len_a, s, st_a == 0 ? (uint32_t)na : 0u);
                    put(p.len_b, s, st_b == 0 ? (uint32_t)nb : 0u);
                }
            }
            continue;
        }
        Stream xa, xb;
        bool good = stream_open(xa, p.a, s, lane);
        good = stream_open(xb, p.b, s, lane) && good;
        // the word count each side's last value claims: a well-formed stream has a token in every word
        const uint64_t words_a = xa.n ? (uint64_t)xa.w[xa.n - 1] + 1 : 0, words_b = xb.n ? (uint64_t)xb.w[xb.n - 1] + 1 : 0;
        good = good && words_a == words_b && words_a <= xa.n && words_b <= xb.n && xa.n <= 0xFFFFFFFFull && xb.n <= 0xFFFFFFFFull;
        const uint32_t n_words = good ? (uint32_t)words_a : 0u;
        // write: the string's ranges of the per-word and the per-selected-word arrays
        uint64_t word_at = 0, word_room = 0, sel_at = 0, sel_room = 0;
        if (WRITE) {
            if (p.word_off) {
                word_at = p.word_off[s] - p.word_off[0];
                word_room = p.word_off[s + 1] - p.word_off[s];
                good = good && word_room == n_words;
            }
            if (p.sel_off) {
                sel_at = p.sel_off[s] - p.sel_off[0];
                sel_room = p.sel_off[s + 1] - p.sel_off[s];
            }
        }
        uint32_t n_sel = 0;                          // selected words so far
        uint32_t before_a = 0, before_b = 0;         // E(w0 - 1): the first token of word w0
        uint32_t last_a = 0, last_b = 0;             // E(W - 1)
        for (uint32_t w0 = 0; good && w0 < n_words; w0 += 64) {
            const uint32_t w = w0 + lane;
            const bool act = w < n_words;            // (w0 + 63 does not wrap: n_words <= n < 2^32 and w0 < n_words)
            uint32_t end_a, end_b;
            if (!run_ends(xa, w, act, lane, end_a) || !run_ends(xb, w, act, lane, end_b)) {
                good = false;
                break;
            }
            const uint32_t first_a = wave_shift_in(end_a, before_a), first_b = wave_shift_in(end_b, before_b);
            const uint32_t cnt_a = end_a - first_a, cnt_b = end_b - first_b;
            const unsigned last_lane = n_words - w0 < 64u ? n_words - w0 - 1u : 63u;
            before_a = last_a = lane_value(end_a, last_lane);
            before_b = last_b = lane_value(end_b, last_lane);
            const bool sel = act && ((less && cnt_a < cnt_b) || (greater && cnt_a > cnt_b));
            const uint64_t mask = ballot(sel);
            if (WRITE) {
                if (p.word_off && act && w < word_room) {
                    p.cnt_a[word_at + w] = cnt_a;
                    p.cnt_b[word_at + w] = cnt_b;
                }
                const uint64_t d = (uint64_t)n_sel + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                if (p.sel_off && sel && d < sel_room) {
                    put(p.sel_str, sel_at + d, (uint32_t)s);
                    put(p.sel_word, sel_at + d, w);
                    put(p.sel_a_first, sel_at + d, first_a);
                    put(p.sel_a_count, sel_at + d, cnt_a);
                    put(p.sel_b_first, sel_at + d, first_b);
                    put(p.sel_b_count, sel_at + d, cnt_b);
                    // side a's tok_end behind the word before and behind this word (first_a, end_a <= n_a)
                    if (p.sel_begin) p.sel_begin[sel_at + d] = first_a ? p.a.tok_end[(xa.w - p.a.tok_word) + first_a - 1] : 0u;
                    if (p.sel_end) p.sel_end[sel_at + d] = end_a ? p.a.tok_end[(xa.w - p.a.tok_word) + end_a - 1] : 0u;
                }
            }
            n_sel += (uint32_t)__builtin_popcountll(mask);
        }
        // the last run ends with the stream (so every chunk of both sides was loaded and checked)
        good = good && last_a == (uint32_t)xa.n && last_b == (uint32_t)xb.n;
        if (WRITE && p.sel_off) good = good && sel_room == n_sel;
        if (lane == 0) {
            p.wc_status[s] = good ? DPT_STATUS_OK : DPT_STATUS_INTERNAL;
            if (!WRITE) {
                p.n_words[s] = good ? n_words : 0u;
                p.n_sel[s] = good ? n_sel : 0u;
                put(p.len_a, s, (uint32_t)xa.n);
                put(p.len_b, s, (uint32_t)xb.n);
            }
        }
    }
}

}  // namespace wrd

hipError_t launch_words(const WordsLaunch &p, hipStream_t stream) {
    if (p.n_str == 0) return hipSuccess;
    const unsigned blocks = wave_per_string_blocks(p.n_str, wrd::WAVES);
    if (p.write) hipLaunchKernelGGL(wrd::words_kernel<true>, dim3(blocks), dim3(wrd::WAVES * 64), 0, stream, p);
    else hipLaunchKernelGGL(wrd::words_kernel<false>, dim3(blocks), dim3(wrd::WAVES * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpt
