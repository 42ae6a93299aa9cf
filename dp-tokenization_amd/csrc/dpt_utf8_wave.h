// dpt_utf8_wave.h -- the walk the text-to-split kernels share (dpt_pretok.hip, dpt_bytelevel.hip): one wave per string
// in a grid-stride loop, a string's bytes 64 to a round with one lane per byte and the round after it already in
// registers, a sizes pass that sums and refuses and a write pass that produces every round's output 64 bytes at a
// time.  A kernel file states its splitter's rule -- what a byte becomes and when a string is refused -- and its
// launch arguments; everything here is the same for every rule.  Both launch structs carry the members named below
// (text, str_off, n_str, write, out_len, pre_status, out_text, out_off, cut_mask).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_internal.h"
#include "dpt_wave.h"

namespace dpt {
namespace txt {

constexpr unsigned WAVES = 4;        // strings per block of 256 threads
constexpr unsigned NOBYTE = 0x100;   // a lane past the string's end

__device__ __forceinline__ unsigned byte_load(const uint8_t *__restrict__ text, uint64_t base, uint64_t n, uint64_t k0, unsigned lane) {
    const uint64_t p = k0 + lane;
    return p < n ? (unsigned)text[base + p] : NOBYTE;
}

// the byte j lanes further on: this round's register, or the next round's
__device__ __forceinline__ unsigned ahead(unsigned cur, unsigned nxt, unsigned lane, unsigned j) {
    const unsigned src = lane + j;
    const unsigned a = lane_read(cur, src & 63u), b = lane_read(nxt, src & 63u);
    return src < 64u ? a : b;
}

// The character the lead byte b (>= 0xC0) opens with the bytes b1, b2, b3 behind it (NOBYTE past the string's end):
// its length and, in *cp, its code point -- or 0 when it opens no well-formed character (0xC0, 0xC1, 0xF5.., a
// missing continuation byte, an overlong form, a surrogate, a value above U+10FFFF).
__device__ __forceinline__ unsigned utf8_lead(unsigned b, unsigned b1, unsigned b2, unsigned b3, unsigned *cp) {
    auto is_cont = [](unsigned x) { return (x & 0x1C0u) == 0x80u; };   // (0x100 is not one)
    unsigned len = 0;
    if (b >= 0xC2u && b < 0xE0u) {
        if (is_cont(b1)) len = 2, *cp = (b & 0x1Fu) << 6 | (b1 & 0x3Fu);
    } else if (b >= 0xE0u && b < 0xF0u) {
        const bool second = b == 0xE0u ? b1 >= 0xA0u : b == 0xEDu ? b1 <= 0x9Fu : true;   // no overlong, no surrogate
        if (is_cont(b1) && second && is_cont(b2)) len = 3, *cp = (b & 0x0Fu) << 12 | (b1 & 0x3Fu) << 6 | (b2 & 0x3Fu);
    } else if (b >= 0xF0u && b < 0xF5u) {
        const bool second = b == 0xF0u ? b1 >= 0x90u : b == 0xF4u ? b1 <= 0x8Fu : true;   // no overlong, at most U+10FFFF
        if (is_cont(b1) && second && is_cont(b2) && is_cont(b3))
            len = 4, *cp = (b & 0x07u) << 18 | (b1 & 0x3Fu) << 12 | (b2 & 0x3Fu) << 6 | (b3 & 0x3Fu);
    }
    return len;
}

// The lanes of a round whose inclusive scan value ei is at or below o: output byte o lies in the item of lane
// scan_owner(ei, o).  A 6-step binary search over ds_bpermute reads; at most 63.
__device__ __forceinline__ unsigned scan_owner(unsigned ei, unsigned o) {
    unsigned m = 0;
#pragma unroll
    for (unsigned step = 32; step; step >>= 1)
        if (lane_read(ei, m + step - 1) <= o) m += step;
    return m;
}

// One string of a launch: its text is text[base .. base + n), its output range out_text / cut_mask[obase .. obase +
// lim) (write alone).
struct Str {
    uint64_t base, n, obase, lim;
};

// The string s of a launch whose first string starts at so0.  (The write pass skips a string the sizes pass refused
// before it comes here, on pre_status[s] in the kernel: that test inside this function measured +2 VGPRs.)
template <bool WRITE, typename Launch>
__device__ __forceinline__ Str open_string(const Launch &a, uint64_t s, uint64_t so0) {
    uint64_t obase = 0, lim = 0;
    if (WRITE) {
        obase = a.out_off[s] - a.out_off[0];
        lim = a.out_off[s + 1] - a.out_off[s];
    }
    const uint64_t base = a.str_off[s] - so0;
    const uint64_t n = a.str_off[s + 1] - a.str_off[s];
    return Str{base, n, obase, lim};
}

// The write pass's part of one round of a string whose output range is obase, lim (a Str's, passed as two values:
// as a Str the kernels' register counts changed).  ei = the inclusive scan of the lanes' output lengths (whatever goes
// out before the first lane's added to every value), total = the output bytes of the rounds before.  The round's
// T = ei[63] bytes go out 64 at a time: output byte o belongs to lane o mod 64, which asks the rule for it --
// rule(o, g, m, end, &out, &mask) with g = total + o the byte's index in the string's form, m = scan_owner(ei, o) and
// end = ei[m] (at o >= T it names some lane and the answer is not used) -- and stores it below the string's limit.
// One store instruction covers 64 consecutive bytes of text and one 64 of cut mask, whatever the lengths are.
// Returns T.
template <typename Launch, typename Rule>
__device__ __forceinline__ unsigned write_round(const Launch &a, uint64_t obase, uint64_t lim, unsigned lane, unsigned ei, uint64_t total, Rule rule) {
    const unsigned T = (unsigned)__builtin_amdgcn_readlane((int)ei, 63);
    for (unsigned it = 0; it < T; it += 64) {
        const unsigned o = it + lane;
        const unsigned m = scan_owner(ei, o);
        const unsigned end = lane_read(ei, m);
        const uint64_t g = total + o;
        unsigned out, mask;
        rule(o, g, m, end, &out, &mask);
        if (o < T && g < lim) {
            a.out_text[obase + g] = (uint8_t)out;
            a.cut_mask[obase + g] = (uint8_t)mask;
        }
    }
    return T;
}

// The sizes pass's end for one string: a stray continuation byte (the leads claimed other than the string holds) and
// a form of 2^32 bytes or more are refused as well, and lane 0 stores the length and the status.
template <typename Launch>
__device__ __forceinline__ void close_sizes(const Launch &a, uint64_t s, unsigned lane, uint64_t total, bool refuse, uint64_t claimed, uint64_t conts) {
    refuse |= claimed != conts;
    refuse |= total >= (1ull << 32);
    if (lane == 0) {
        a.out_len[s] = refuse ? 0 : total;
        a.pre_status[s] = refuse ? DPT_PRETOK_NEEDS_HOST : DPT_STATUS_OK;
    }
}

// The sizes or the write kernel of a splitter over p's strings.
template <typename Launch>
hipError_t launch_split(void (*sizes)(Launch), void (*write)(Launch), const Launch &p, hipStream_t stream) {
    if (p.n_str == 0) return hipSuccess;
    hipLaunchKernelGGL(p.write ? write : sizes, dim3(wave_per_string_blocks(p.n_str, WAVES)), dim3(WAVES * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace txt
}  // namespace dpt
