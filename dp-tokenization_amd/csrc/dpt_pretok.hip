// dpt_pretok.hip -- llama mode's pre-split text made on the device (dpt_pretok_sizes, dpt_pretok_write,
// dpt_pretok_write_atoms).
//
// The rule is in include/dpt.h (dpt_pretok_create): a certified string's pre-split form is a per-character function
// of its text -- ' ' becomes U+2581 opening a word, a character that is a piece of its own stays, any other
// character becomes <0xNN> for each of its bytes -- behind a fixed prefix (the BOS piece, then U+2581).  One wave per
// string in a grid-stride loop, 64 input bytes per round, everything in registers (dpt_decode.hip's shape; the parts
// of the walk that are the same for every splitter are in dpt_utf8_wave.h, this file holds the rule):
//   - lane k holds byte k0 + k of the string (0x100 past its end: no load goes beyond the string's last byte).  The
//     round after this one is already in registers, so a lead-byte lane reads its continuation bytes from its
//     neighbours' registers and from the next round's: a character may straddle a round, and the bytes that follow a
//     string's end never complete a truncated one
//   - a lead-byte lane carries its character's output length: 3 for ' ', the character's own length when it is known
//     (a bitmap below U+10000, a sorted list above; the code points below U+0080 come with the kernel arguments),
//     6 x its length otherwise.  Continuation lanes carry 0
//   - sizes: the lengths are summed (by popcounts of three ballots in a round of ASCII bytes), and a ballot per rule
//     decides the refusals; the literals are compared only at bytes equal to some literal's first byte
//   - write: an inclusive wave scan gives every character's end within the round (the prefix's bytes are added to
//     the first round's ends), and the round's bytes are produced 64 at a time: output byte o belongs to lane o mod
//     64, which finds its character by a 6-step binary search over the scan values (ds_bpermute reads) and takes its
//     source byte from that lane's register.  One store instruction covers 64 consecutive bytes of text and one 64
//     of cut mask, whatever the characters' lengths are
// No LDS, no workspace, no atomics.  The only stores are out_len[s] / pre_status[s] and, in write, bytes at positions
// below out_off[s + 1] - out_off[s] of the string's own output range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_internal.h"
#include "dpt_utf8_wave.h"
#include "dpt_wave.h"

namespace dpt {
namespace pre {

using namespace txt;   // WAVES, NOBYTE, byte_load, ahead, and the walk's shared parts

enum Kind : unsigned { K_SPACE = 0, K_COPY = 1, K_HEX = 2 };

__device__ __forceinline__ bool ascii_known(const PretokLaunch &a, unsigned b) {
    const uint64_t w = b < 64u ? a.ascii_known[0] : a.ascii_known[1];
    return (w >> (b & 63u)) & 1u;
}

__device__ __forceinline__ bool cp_known(const PretokLaunch &a, unsigned cp) {
    if (cp < 0x10000u) return (a.bmp[cp >> 5] >> (cp & 31u)) & 1u;
    unsigned lo = 0, hi = a.n_astral;   // the first entry >= cp
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (a.astral[mid] < cp) lo = mid + 1;
        else hi = mid;
    }
    return lo < a.n_astral && a.astral[lo] == cp;
}

// What one round's lanes carry.  lk = the character's output length | its Kind << 8 on a lead-byte lane, 0 on every
// other lane; bad: a lead byte that opens no well-formed character, or U+2581 itself.
struct Round {
    unsigned lk;
    unsigned extra;   // the continuation bytes a well-formed lead claims
    bool bad;
    bool cont;        // a continuation byte
};

__device__ __forceinline__ Round classify(const PretokLaunch &a, unsigned b, unsigned cur, unsigned nxt, unsigned lane, bool ascii_round) {
    Round r{0u, 0u, false, false};
    if (ascii_round) {   // (wave-uniform)
        if (b < 0x80u) r.lk = b == 0x20u ? 3u | K_SPACE << 8 : ascii_known(a, b) ? 1u | K_COPY << 8 : 6u | K_HEX << 8;
        return r;
    }
    const unsigned b1 = ahead(cur, nxt, lane, 1), b2 = ahead(cur, nxt, lane, 2), b3 = ahead(cur, nxt, lane, 3);
    if (b >= NOBYTE) return r;
    if (b < 0x80u) {
        r.lk = b == 0x20u ? 3u | K_SPACE << 8 : ascii_known(a, b) ? 1u | K_COPY << 8 : 6u | K_HEX << 8;
        return r;
    }
    if ((b & 0xC0u) == 0x80u) {
        r.cont = true;
        return r;
    }
    // (txt::utf8_lead's text: calling it here measured +2 VGPRs in both kernels)
    auto is_cont = [](unsigned x) { return (x & 0x1C0u) == 0x80u; };   // (0x100 is not one)
    unsigned len = 0, cp = 0;
    if (b >= 0xC2u && b < 0xE0u) {
        if (is_cont(b1)) len = 2, cp = (b & 0x1Fu) << 6 | (b1 & 0x3Fu);
    } else if (b >= 0xE0u && b < 0xF0u) {
        const bool second = b == 0xE0u ? b1 >= 0xA0u : b == 0xEDu ? b1 <= 0x9Fu : true;   // no overlong, no surrogate
        if (is_cont(b1) && second && is_cont(b2)) len = 3, cp = (b & 0x0Fu) << 12 | (b1 & 0x3Fu) << 6 | (b2 & 0x3Fu);
    } else if (b >= 0xF0u && b < 0xF5u) {
        const bool second = b == 0xF0u ? b1 >= 0x90u : b == 0xF4u ? b1 <= 0x8Fu : true;   // no overlong, at most U+10FFFF
        if (is_cont(b1) && second && is_cont(b2) && is_cont(b3))
            len = 4, cp = (b & 0x07u) << 18 | (b1 & 0x3Fu) << 12 | (b2 & 0x3Fu) << 6 | (b3 & 0x3Fu);
    }
    if (len == 0 || cp == 0x2581u) {   // (0xC0, 0xC1, 0xF5.. open nothing)
        r.bad = true;
        return r;
    }
    r.extra = len - 1;
    r.lk = cp_known(a, cp) ? len | K_COPY << 8 : 6u * len | K_HEX << 8;
    return r;
}

// A literal starts at one of the lanes of `cand` (their byte is some literal's first byte).
__device__ __forceinline__ bool literal_at(const PretokLaunch &a, bool cand, unsigned b, uint64_t base, uint64_t n, uint64_t p) {
    bool hit = false;
    for (unsigned j = 0; j < a.n_lit; j++) {
        const unsigned lo = a.lit_off[j], ll = a.lit_off[j + 1] - lo;
        bool m = cand && b == a.lit_bytes[lo] && p + ll <= n;
        for (unsigned i = 1; i < ll && ballot(m) != 0; i++)
            if (m) m = a.text[base + p + i] == a.lit_bytes[lo + i];   // (p + i < n)
        hit |= m;
    }
    return ballot(hit) != 0;
}

// ATOMS (write alone): the mask is an ATOMS mask -- 3 where the plain mask has 1, 2 at the first byte of every other atom
// (a character that stays, each <0xNN> of an expansion); the text is the same.
template <bool WRITE, bool ATOMS = false>
__global__ void __launch_bounds__(WAVES * 64) pretok_kernel(PretokLaunch a) {
    const unsigned lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES + uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
    const uint64_t so0 = a.str_off[0];
    for (uint64_t s = wave; s < a.n_str; s += n_waves) {
        if (WRITE && a.pre_status[s] != 0) continue;   // refused: nothing is written
        const Str str = open_string<WRITE>(a, s, so0);
        const uint64_t base = str.base, n = str.n;
        const unsigned P = a.bos_len + (n ? 3u : 0u);   // the prefix: the BOS piece, and U+2581 before a first character
        unsigned cur = byte_load(a.text, base, n, 0, lane);
        unsigned nxt = byte_load(a.text, base, n, 64, lane);
        uint64_t total = 0;                 // output bytes of the rounds before this one
        uint64_t claimed = 0, conts = 0;    // continuation bytes the leads claim / the string holds
        bool refuse = false, prev_space = false;
        uint64_t k0 = 0;
        do {
            const unsigned after = byte_load(a.text, base, n, k0 + 128, lane);
            const unsigned b = cur;
            const bool ascii_round = ballot(b < NOBYTE && b >= 0x80u) == 0;
            const Round r = classify(a, b, cur, nxt, lane, ascii_round);
            const unsigned len = r.lk & 0xFFu;
            if (!WRITE) {
                const uint64_t sp = ballot(b == 0x20u);
                if (ascii_round) {
                    const unsigned n_all = (unsigned)__builtin_popcountll(ballot(b < NOBYTE));
                    const unsigned n_sp = (unsigned)__builtin_popcountll(sp);
                    const unsigned n_kn = (unsigned)__builtin_popcountll(ballot(len == 1u));
                    total += 3u * n_sp + n_kn + 6u * (n_all - n_sp - n_kn);
                } else {
                    total += (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan_add(len), 63);
                    refuse |= ballot(r.bad) != 0;
                    conts += (unsigned)__builtin_popcountll(ballot(r.cont));
                    claimed += (unsigned)__builtin_popcountll(ballot(r.extra >= 1u)) + (unsigned)__builtin_popcountll(ballot(r.extra >= 2u)) +
                               (unsigned)__builtin_popcountll(ballot(r.extra >= 3u));
                }
                refuse |= k0 == 0 && (sp & 1u);                                                   // a leading space
                if (!a.runs_ok) refuse |= (sp & (sp >> 1)) != 0 || (prev_space && (sp & 1u));     // two spaces
                prev_space = sp >> 63;
                if (a.n_lit) {
                    const uint64_t w = b < 64u ? a.lit_first[0] : b < 128u ? a.lit_first[1] : b < 192u ? a.lit_first[2] : a.lit_first[3];
                    const bool cand = b < NOBYTE && ((w >> (b & 63u)) & 1u);
                    if (ballot(cand) != 0) refuse |= literal_at(a, cand, b, base, n, k0 + lane);
                }
                if (refuse) break;
            } else {
                unsigned ei = wave_incl_scan_add(len);
                const unsigned pfx = k0 == 0 ? P : 0u;   // the prefix goes out with the first round
                ei += pfx;
                // output byte o lies in the character of lane m, which ends at `end`
                total += write_round(a, str.obase, str.lim, lane, ei, total, [&](unsigned o, uint64_t g, unsigned m, unsigned end, unsigned *outp, unsigned *mask) {
                    const unsigned lk = lane_read(r.lk, m);
                    const unsigned kind = lk >> 8, k = o - (end - (lk & 0xFFu));   // (garbage where o < pfx or o >= T: not used)
                    const unsigned j = kind == K_COPY ? k : (k * 43u) >> 8;          // the source byte: k / 6 for k < 24
                    const unsigned src = m + j;
                    const unsigned sa = lane_read(cur, src & 63u), sb = lane_read(nxt, src & 63u);
                    const unsigned c = src < 64u ? sa : sb;
                    unsigned out;
                    bool opens = false, atom = false;
                    if (o < pfx) {
                        out = a.prefix[o];
                        opens = o == a.bos_len;
                    } else if (kind == K_SPACE) {
                        out = k == 0 ? 0xE2u : k == 1 ? 0x96u : 0x81u;
                        opens = k == 0;
                    } else if (kind == K_COPY) {
                        out = c;
                        atom = k == 0;
                    } else {
                        const unsigned q = k - 6u * j;
                        const unsigned h = q == 3 ? (c >> 4) & 15u : c & 15u;
                        const unsigned hx = h < 10u ? '0' + h : 'A' + h - 10u;
                        out = q == 0 ? '<' : q == 1 ? '0' : q == 2 ? 'x' : q == 5 ? '>' : hx;
                        atom = q == 0;
                    }
                    *outp = out;
                    const bool word = opens || g == 0;   // (the string's first byte opens a word too)
                    *mask = ATOMS ? (word ? 3 : atom ? 2 : 0) : (word ? 1 : 0);
                });
            }
            cur = nxt;
            nxt = after;
            k0 += 64;
        } while (k0 < n);
        if (!WRITE) close_sizes(a, s, lane, total + P, refuse, claimed, conts);
    }
}

}  // namespace pre

hipError_t launch_pretok(const PretokLaunch &p, hipStream_t stream) {
    return txt::launch_split(pre::pretok_kernel<false>, p.atoms ? pre::pretok_kernel<true, true> : pre::pretok_kernel<true, false>, p, stream);
}

}  // namespace dpt
