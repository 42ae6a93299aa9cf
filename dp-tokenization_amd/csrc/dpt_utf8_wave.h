// dpt_utf8_wave.h -- a string's bytes 64 to a round with one lane per byte, a lane's view of the bytes that follow
// it, and the well-formed UTF-8 character a lead byte opens: dpt_pretok.hip's helpers under names of their own, for
// dpt_bytelevel.hip.  (dpt_pretok.hip keeps its copies: taking them from here changed its generated code.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpt {
namespace txt {

constexpr unsigned NOBYTE = 0x100;   // a lane past the string's end

__device__ __forceinline__ unsigned lane_read(unsigned v, unsigned src) {
    return (unsigned)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
}

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

}  // namespace txt
}  // namespace dpt
