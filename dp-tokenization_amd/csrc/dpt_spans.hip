// dpt_spans.hip -- token byte spans and word indices of an encoded batch (dpt_token_spans).
//
// A DP tokenization tiles the atom-expanded string, so the span of token k follows from the byte
// lengths of the ids before it and a scan of the text (include/dpt.h, dpt_token_spans):
//   E_k   = the sum of the byte lengths of tokens 0..k            (the ids' stream)
//   x(p)  = the expanded offset of input position p                (the text's stream)
//   tok_end[k] = the p with x(p) = E_k,  tok_word[k] = the word starts in [1, tok_end[k-1]]
//
// One wave per string, 64 ids and 64 text bytes per round, everything in registers: lane j of the
// text chunk at tb holds x(tb+j+1) - x(tb) and the word starts in [1, tb+j] (two wave scans plus
// the carries of the chunks before), lane k of the id chunk holds E_k (one wave scan plus carry).
// Both streams are monotone, so the wave merges them: the tokens that end inside the current text
// chunk find their position by a 6-step binary search over the chunk's scan values (ds_bpermute
// reads of the other lanes' registers), the rest wait for the next text chunk.  Every round either
// resolves a token or advances the text, so a string costs (length + tokens) / 64 rounds whatever
// the ids are.  Rows are loaded ahead of their use (the text one chunk, the ids two, their lengths
// one).  No LDS, no workspace, no atomics; the only stores are tok_end / tok_word at
// id_off[s] - id_off[0] + k for k < id_off[s+1] - id_off[s], and span_status[s].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_internal.h"
#include "dpt_wave.h"

namespace dpt {
namespace spn {

constexpr unsigned WAVES = 4;   // strings per block of 256 threads

__device__ __forceinline__ bool any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// The byte a text chunk needs of input position tb + lane: the text's (RAW) or the cut mask's; 0 at or
// past the string's end (nothing is loaded there).  Loaded one chunk ahead of its use.
template <int MODE>
__device__ __forceinline__ unsigned text_load(const uint8_t *__restrict__ text, const uint8_t *__restrict__ cut, uint64_t sb,
                                              uint32_t len, uint64_t tb, unsigned lane) {
    const uint64_t q = tb + lane;
    if (q >= len) return 0u;
    return MODE == DPT_MODE_RAW ? text[sb + q] : cut[sb + q];
}

// One text chunk from its loaded bytes: lane j stands for input position tb + j.  xi = x(tb+j+1) - x(tb)
// (positions at or past the string's end add nothing, so the values stay flat at x(len) there), ci = the
// word starts in [1, tb+j].
template <int MODE>
__device__ __forceinline__ void text_chunk(unsigned b, uint32_t len, uint64_t tb, unsigned lane, uint32_t cbase,
                                           uint32_t &xi, uint32_t &ci) {
    const uint64_t q = tb + lane;
    unsigned w = 0, ws = 0;
    if (q < len) {
        if (MODE == DPT_MODE_RAW) {
            // byte 0 is literal behind the 3-byte word mark; ' ' becomes the mark, '\n' the 6 bytes "<0x0A>"
            w = q == 0 ? 4u : b == 0x20u ? 3u : b == 0x0Au ? 6u : 1u;
            ws = q != 0 && b == 0x20u;
        } else {
            w = 1u;
            ws = q != 0 && (MODE == DPT_MODE_PRESPLIT ? b != 0u : (b & 1u) != 0u);
        }
    }
    xi = wave_incl_scan_add(w);
    ci = cbase + wave_incl_scan_add(ws);
}

// The id of token k0 + lane (0 past the string's last token: nothing is loaded), and its byte length: 0
// for an id outside the table -- checked before the load -- or one that no token has.
__device__ __forceinline__ int32_t id_load(const int32_t *__restrict__ ids, uint64_t ib, uint64_t ntok, uint64_t k0, unsigned lane) {
    const uint64_t k = k0 + lane;
    return k < ntok ? ids[ib + k] : 0;
}
__device__ __forceinline__ uint32_t len_load(const SpansLaunch &a, int32_t id, uint64_t ntok, uint64_t k0, unsigned lane) {
    const int64_t d = (int64_t)id - (int64_t)a.id_min;
    if (k0 + lane >= ntok || d < 0 || d >= (int64_t)a.n_tab) return 0u;
    return a.tok_len[d];
}

template <int MODE>
__global__ void __launch_bounds__(WAVES * 64) spans_kernel(SpansLaunch a) {
    const unsigned lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES + uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
    const uint64_t so0 = a.str_off[0], io0 = a.id_off[0];
    for (uint64_t s = wave; s < a.n_str; s += n_waves) {
        const int32_t st = a.status[s];
        if (st != 0) {   // a failed string has no ids: nothing but its status
            if (lane == 0) a.span_status[s] = st;
            continue;
        }
        const uint64_t sb = a.str_off[s] - so0;
        const uint32_t len = (uint32_t)(a.str_off[s + 1] - a.str_off[s]);
        const uint64_t ib = a.id_off[s] - io0;
        const uint64_t ntok = a.id_off[s + 1] - a.id_off[s];
        // the text stream: chunk [tb, tb+64), x(tb) and the word starts in [1, tb-1]
        // (the rows of both streams are loaded ahead of their use: the text one chunk, the ids two chunks and
        // the lengths gathered from them one chunk, so a round waits for no load it has just issued)
        uint64_t tb = 0, xbase = 0;
        uint32_t cbase = 0, xi, ci;
        int32_t id_next = id_load(a.ids, ib, ntok, 0, lane);
        unsigned b_next = text_load<MODE>(a.text, a.cut_mask, sb, len, 0, lane);
        text_chunk<MODE>(b_next, len, tb, lane, cbase, xi, ci);
        b_next = text_load<MODE>(a.text, a.cut_mask, sb, len, 64, lane);
        uint32_t tl_next = len_load(a, id_next, ntok, 0, lane);
        id_next = id_load(a.ids, ib, ntok, 64, lane);
        // the ids' stream: E of the tokens before this chunk, the last token's end and the word starts up to it
        uint64_t ebase = 0;
        uint32_t last_end = 0, wcarry = 0;
        bool bad = false;
        for (uint64_t k0 = 0; k0 < ntok && !bad; k0 += 64) {
            const uint64_t k = k0 + lane;
            const bool act = k < ntok;
            const uint32_t tl = tl_next;
            tl_next = len_load(a, id_next, ntok, k0 + 64, lane);
            id_next = id_load(a.ids, ib, ntok, k0 + 128, lane);
            if (any(act && tl == 0u)) {
                bad = true;
                break;
            }
            const uint32_t ei = wave_incl_scan_add(tl);   // (64 tokens of at most 65535 bytes)
            const uint64_t e = ebase + ei;
            ebase += (uint32_t)__builtin_amdgcn_readlane((int)ei, 63);
            bool pend = act;
            uint32_t endp = 0, wend = 0;
            while (any(pend)) {
                const bool last_chunk = tb + 64 >= len;
                const uint32_t xtot = (uint32_t)__builtin_amdgcn_readlane((int)xi, 63);
                const uint64_t r64 = e - xbase;   // (pending tokens end at or after x(tb))
                // a token that ends before the chunk's end is found in it; one that ends at x(tb+64) or
                // later waits for the next chunk, which knows the word starts up to tb+64
                const bool can = pend && (last_chunk || r64 < xtot);
                if (!any(can)) {
                    tb += 64;
                    xbase += xtot;
                    cbase = (uint32_t)__builtin_amdgcn_readlane((int)ci, 63);
                    text_chunk<MODE>(b_next, len, tb, lane, cbase, xi, ci);
                    b_next = text_load<MODE>(a.text, a.cut_mask, sb, len, tb + 64, lane);
                    continue;
                }
                const bool over = r64 > xtot;   // (only in the last chunk: past x(len))
                const uint32_t r = over ? xtot : (uint32_t)r64;
                // m = the lanes j with xi[j] < r: the token ends at position tb + m + 1, or at tb when r = 0
                uint32_t m = 0;
#pragma unroll
                for (unsigned step = 32; step; step >>= 1)
                    if (lane_read(xi, m + step - 1) < r) m += step;
                const uint32_t i = r == 0u ? 0u : m + 1u;                   // 0..64
                const uint32_t xat = lane_read(xi, i ? i - 1u : 0u);        // x(tb+i) - x(tb) for i >= 1
                const uint32_t cat = lane_read(ci, i < 64u ? i : 63u);      // word starts in [1, tb+i] (i = 64: the string's end)
                if (any(can && (over || (i != 0u && xat != r)))) {   // an E that no position attains
                    bad = true;
                    break;
                }
                if (can) {
                    endp = (uint32_t)tb + i;
                    wend = cat;
                }
                pend = pend && !can;
            }
            if (bad) break;
            const uint32_t word = wave_shift_in(wend, wcarry);   // the word starts up to the token's start
            if (act) {
                a.tok_end[ib + k] = endp;
                if (a.tok_word) a.tok_word[ib + k] = word;
            }
            const unsigned lastl = (unsigned)((ntok - k0 < 64 ? ntok - k0 : 64) - 1);
            last_end = (uint32_t)__builtin_amdgcn_readlane((int)endp, (int)lastl);
            wcarry = (uint32_t)__builtin_amdgcn_readlane((int)wend, (int)lastl);
        }
        // the ids tile the string: the last token ends at its end (x is strictly increasing, so
        // this is E = x(len)); no ids tile the empty string only
        if (!bad) bad = last_end != len;
        if (lane == 0) a.span_status[s] = bad ? DPT_STATUS_INTERNAL : DPT_STATUS_OK;
    }
}

}  // namespace spn

hipError_t launch_spans(const SpansLaunch &p, hipStream_t stream) {
    if (p.n_str == 0) return hipSuccess;
    const unsigned blocks = wave_per_string_blocks(p.n_str, spn::WAVES);
    const int mode = p.mode & DPT_MODE_MASK;
    if (mode == DPT_MODE_RAW) hipLaunchKernelGGL(spn::spans_kernel<DPT_MODE_RAW>, dim3(blocks), dim3(spn::WAVES * 64), 0, stream, p);
    else if (mode == DPT_MODE_PRESPLIT) hipLaunchKernelGGL(spn::spans_kernel<DPT_MODE_PRESPLIT>, dim3(blocks), dim3(spn::WAVES * 64), 0, stream, p);
    else hipLaunchKernelGGL(spn::spans_kernel<DPT_MODE_ATOMS>, dim3(blocks), dim3(spn::WAVES * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpt
