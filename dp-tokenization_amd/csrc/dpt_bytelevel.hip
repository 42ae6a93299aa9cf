// dpt_bytelevel.hip -- the BLOOM adapter's ATOMS input made on the device (dpt_bytelevel_sizes, dpt_bytelevel_write).
//
// The rule is in include/dpt.h (dpt_bytelevel_create): words start where a three-character window of separator
// classes says so, and every input byte becomes one atom, its character in the GPT-2 byte alphabet (one byte for 0x21 ..
// 0x7E, two for every other byte).  dpt_pretok.hip's shape, the parts of it that are the same for every splitter
// taken from dpt_utf8_wave.h: one wave per string in a grid-stride loop, 64 input bytes per round, lane k holding
// byte k0 + k (0x100 past the string's end: no load goes beyond its last byte), the round after this one already in
// registers.
//   - sizes: the length is the string's bytes plus the bytes outside 0x21 .. 0x7E (two popcounts a round); a round
//     with a byte >= 0x80 also checks that every lead byte opens a well-formed character and counts the continuation
//     bytes the leads claim against those the string holds.  The separators play no part
//   - write: a lead-byte lane decides whether its character is a separator (a bitmap in the kernel arguments below
//     U+0080, a binary search in a sorted list above; a round without a byte >= 0x80 takes neither the neighbour reads
//     nor the search).  Everything after that is 64-bit mask arithmetic on ballots, the same in every lane: S the bytes
//     of separator characters (continuation bytes take their lead's class, a character begun in the previous round the
//     class carried over), P the bytes equal to 0x20, A = P & ~(S >> 1) the absorbed spaces (the class of the next
//     round's first character comes in at bit 63: decoded from the next round's registers, only when lane 63 holds a
//     space), and the word starts W = A | ~S & S' & ~A' | S & ~A & ~S' with S', A' = S, A shifted up by one byte
//     with last round's bit 63 coming in
//   - an inclusive wave scan of the atoms' lengths gives every input byte's end within the round, and the round's
//     output is produced 64 bytes at a time: output byte o belongs to lane o mod 64, which finds its input byte by a
//     6-step binary search over the scan values (ds_bpermute reads) and takes that lane's two output bytes and word
//     flag from one packed register.  One store instruction covers 64 consecutive bytes of text and one 64 of cut mask
// No LDS, no workspace, no atomics.  The only stores are out_len[s] / pre_status[s] and, in write, bytes at positions
// below out_off[s + 1] - out_off[s] of the string's own output range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_internal.h"
#include "dpt_utf8_wave.h"
#include "dpt_wave.h"

namespace dpt {
namespace bl {

using namespace txt;   // WAVES, NOBYTE, byte_load, ahead, utf8_lead, and the walk's shared parts

__device__ __forceinline__ bool ascii_sep(const ByteLevelLaunch &a, unsigned b) {
    const uint64_t w = b < 64u ? a.ascii_sep[0] : a.ascii_sep[1];
    return (w >> (b & 63u)) & 1u;
}

__device__ __forceinline__ bool high_sep(const ByteLevelLaunch &a, unsigned cp) {
    unsigned lo = 0, hi = a.n_high;   // the first entry >= cp
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (a.high[mid] < cp) lo = mid + 1;
        else hi = mid;
    }
    return lo < a.n_high && a.high[lo] == cp;
}

// The character that starts at b (a byte below NOBYTE that is no continuation byte) is a separator.
__device__ __forceinline__ bool char_sep(const ByteLevelLaunch &a, unsigned b, unsigned b1, unsigned b2, unsigned b3) {
    if (b < 0x80u) return ascii_sep(a, b);
    unsigned cp = 0;
    return utf8_lead(b, b1, b2, b3, &cp) != 0 && high_sep(a, cp);
}

__device__ __forceinline__ unsigned popc(uint64_t m) { return (unsigned)__builtin_popcountll(m); }

template <bool WRITE>
__global__ void __launch_bounds__(WAVES * 64) bytelevel_kernel(ByteLevelLaunch a) {
    const unsigned lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES + uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
    const uint64_t so0 = a.str_off[0];
    for (uint64_t s = wave; s < a.n_str; s += n_waves) {
        if (WRITE && a.pre_status[s] != 0) continue;   // refused: nothing is written
        const Str str = open_string<WRITE>(a, s, so0);
        const uint64_t base = str.base, n = str.n;
        unsigned cur = byte_load(a.text, base, n, 0, lane);
        unsigned nxt = byte_load(a.text, base, n, 64, lane);
        uint64_t total = 0;                 // output bytes of the rounds before this one
        uint64_t claimed = 0, conts = 0;    // continuation bytes the leads claim / the string holds
        bool refuse = false;
        uint64_t carry_s = 0, carry_a = 0;  // bit 63 of the previous round's S and A
        uint64_t k0 = 0;
        do {
            const unsigned after = byte_load(a.text, base, n, k0 + 128, lane);
            const unsigned b = cur;
            const bool valid = b < NOBYTE;
            const bool two = valid && (b < 0x21u || b > 0x7Eu);   // the atom is a two-byte character
            const bool ascii_round = ballot(valid && b >= 0x80u) == 0;
            if (!WRITE) {
                total += popc(ballot(valid)) + popc(ballot(two));
                if (!ascii_round) {
                    const unsigned b1 = ahead(cur, nxt, lane, 1), b2 = ahead(cur, nxt, lane, 2), b3 = ahead(cur, nxt, lane, 3);
                    const bool lead = valid && b >= 0xC0u;
                    unsigned cp = 0;
                    const unsigned len = lead ? utf8_lead(b, b1, b2, b3, &cp) : 0u;
                    refuse |= ballot(lead && len == 0u) != 0;
                    conts += popc(ballot(valid && (b & 0xC0u) == 0x80u));
                    claimed += popc(ballot(len >= 2u)) + popc(ballot(len >= 3u)) + popc(ballot(len >= 4u));
                    if (refuse) break;
                }
            } else {
                const uint64_t V = ballot(valid), C = ballot(valid && (b & 0xC0u) == 0x80u), P = ballot(b == 0x20u);
                uint64_t S;
                if (ascii_round) {   // (wave-uniform)
                    S = ballot(valid && ascii_sep(a, b));
                } else {
                    const unsigned b1 = ahead(cur, nxt, lane, 1), b2 = ahead(cur, nxt, lane, 2), b3 = ahead(cur, nxt, lane, 3);
                    const bool lead = valid && (b & 0xC0u) != 0x80u;
                    S = ballot(lead && char_sep(a, b, b1, b2, b3));
                    for (int k = 0; k < 3; k++) S |= (S << 1 | carry_s) & C;   // continuation bytes: their lead's class
                }
                // the byte after lane 63: the next round's first character, when there is one
                uint64_t next_valid = 0, next_sep = 0;
                if (P >> 63) {       // (wave-uniform: a space in lane 63)
                    const unsigned n0 = (unsigned)__builtin_amdgcn_readlane((int)nxt, 0), n1 = (unsigned)__builtin_amdgcn_readlane((int)nxt, 1);
                    const unsigned n2 = (unsigned)__builtin_amdgcn_readlane((int)nxt, 2), n3 = (unsigned)__builtin_amdgcn_readlane((int)nxt, 3);
                    if (n0 < NOBYTE) {
                        next_valid = 1;
                        next_sep = (n0 & 0xC0u) != 0x80u && char_sep(a, n0, n1, n2, n3) ? 1 : 0;
                    }
                }
                const uint64_t A = P & ~(S >> 1 | next_sep << 63) & (V >> 1 | next_valid << 63);   // absorbed spaces
                const uint64_t Sp = S << 1 | carry_s, Ap = A << 1 | carry_a;                        // the byte before
                const uint64_t W = (V & ~C) & ((k0 == 0 ? 1ull : 0ull) | A | (~S & Sp & ~Ap) | (S & ~A & ~Sp));
                carry_s = S >> 63;
                carry_a = A >> 63;
                // the atom of this lane's byte: its code point in the byte alphabet, as one or two UTF-8 bytes
                const unsigned ch = !two ? b : b <= 0x20u ? 0x100u + b : b <= 0xA0u ? b + 0xA2u : b == 0xADu ? 0x143u : b;
                const unsigned pack = (two ? (0xC0u | ch >> 6) | (0x80u | (ch & 0x3Fu)) << 8 | 1u << 17 : b & 0xFFu) |
                                      (unsigned)((W >> lane) & 1u) << 16;
                const unsigned ei = wave_incl_scan_add(valid ? (two ? 2u : 1u) : 0u);
                // output byte o lies in the atom of lane m, which ends at `end`
                total += write_round(a, str.obase, str.lim, lane, ei, total, [&](unsigned o, uint64_t, unsigned m, unsigned end, unsigned *out, unsigned *mask) {
                    const unsigned pk = lane_read(pack, m);                    // (garbage where o >= T: not used)
                    const bool second = ((pk >> 17) & 1u) && o + 1 == end;     // a two-byte atom's second byte
                    *out = second ? (pk >> 8) & 0xFFu : pk & 0xFFu;
                    *mask = second ? 0u : ((pk >> 16) & 1u) ? 3u : 2u;
                });
            }
            cur = nxt;
            nxt = after;
            k0 += 64;
        } while (k0 < n);
        if (!WRITE) close_sizes(a, s, lane, total, refuse, claimed, conts);
    }
}

}  // namespace bl

hipError_t launch_bytelevel(const ByteLevelLaunch &p, hipStream_t stream) {
    return txt::launch_split(bl::bytelevel_kernel<false>, bl::bytelevel_kernel<true>, p, stream);
}

}  // namespace dpt
