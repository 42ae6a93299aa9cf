// dpt_decode.hip -- ids back to bytes on the device (dpt_decode_sizes, dpt_decode, dpt_roundtrip).
//
// A decode table (dpt_detok.cpp) gives every id an {offset, length} entry into a blob of decoded pieces, so
// a string's decode is the concatenation of its ids' pieces.  One wave per string, 64 ids per round,
// everything in registers: lane k loads the entry of id k0 + k (one 8-byte load), an inclusive wave scan of
// the lengths gives every piece's end within the round, and the round's T bytes are produced 64 at a time:
// output byte o belongs to lane o mod 64, which finds its piece by a 6-step binary search over the scan
// values (ds_bpermute reads of the other lanes' registers, as dpt_spans.hip) and loads
// blob[entry.off + (o - piece start)].  Consecutive lanes hold consecutive output bytes, so one store
// instruction covers 64 consecutive bytes whatever the pieces' lengths are; a piece longer than 64 bytes just
// takes more of these steps.  The three kernels share the walk and differ in what a step does with its byte:
//   sizes      nothing: the lengths are summed, one entry load per id and one wave reduction per round
//   decode     stores it at out[out_off[s] - out_off[0] + position]
//   roundtrip  compares it with text[str_off[s] - str_off[0] + position]; a ballot gives the first difference,
//              and the string stops there
// Rows are loaded ahead of their use (the ids two rounds, the entries one).  No LDS, no workspace, no atomics.
// The only stores are out_len[s] / dec_status[s] / rt[s] / first_diff[s] and, in decode, bytes at positions
// below out_off[s + 1] - out_off[s] of the string's own output range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_internal.h"
#include "dpt_wave.h"

namespace dpt {
namespace dec {

constexpr unsigned WAVES = 4;   // strings per block of 256 threads

__device__ __forceinline__ bool any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

// The id of token k0 + lane (0 past the string's last token: nothing is loaded), and its table entry:
// {0, 0} past the last token, {0, DETOK_NONE} for an id outside the table -- checked before the load.
__device__ __forceinline__ int32_t id_load(const int32_t *__restrict__ ids, uint64_t ib, uint64_t ntok, uint64_t k0, unsigned lane) {
    const uint64_t k = k0 + lane;
    return k < ntok ? ids[ib + k] : 0;
}
__device__ __forceinline__ uint2 entry_load(const DecodeLaunch &a, int32_t id, uint64_t ntok, uint64_t k0, unsigned lane) {
    if (k0 + lane >= ntok) return make_uint2(0u, 0u);
    const int64_t d = (int64_t)id - (int64_t)a.id_min;
    if (d < 0 || d >= (int64_t)a.n_tab) return make_uint2(0u, DETOK_NONE);
    return a.tab[d];
}

template <int KIND>
__global__ void __launch_bounds__(WAVES * 64) decode_kernel(DecodeLaunch a) {
    const unsigned lane = lane_id();
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES + uni(threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
    const uint64_t io0 = a.id_off[0];
    const bool strip_flag = (a.flags & DPT_DECODE_STRIP_SPACE) != 0;
    for (uint64_t s = wave; s < a.n_str; s += n_waves) {
        const int32_t st = a.status ? a.status[s] : 0;
        if (st != 0) {   // a failed string has no ids: nothing but its status
            if (lane == 0) {
                if (KIND == DECODE_SIZES) a.out_len[s] = 0;
                else a.result[s] = st;
            }
            continue;
        }
        const uint64_t ib = a.id_off[s] - io0;
        const uint64_t ntok = a.id_off[s + 1] - a.id_off[s];
        // the other side: the string's output range (decode) or its text (roundtrip)
        uint64_t base = 0, lim = 0;
        if (KIND == DECODE_BYTES) {
            base = a.out_off[s] - a.out_off[0];
            lim = a.out_off[s + 1] - a.out_off[s];
        } else if (KIND == DECODE_ROUNDTRIP) {
            base = a.str_off[s] - a.str_off[0];
            lim = a.str_off[s + 1] - a.str_off[s];
        }
        int32_t id_next = id_load(a.ids, ib, ntok, 0, lane);
        uint2 e_next = entry_load(a, id_next, ntok, 0, lane);
        id_next = id_load(a.ids, ib, ntok, 64, lane);
        uint64_t total = 0;        // decoded bytes of the rounds before this one, the stripped ' ' included
        uint32_t strip = 0;        // 1: the string's first decoded byte is a ' ' that is dropped
        bool bad = false;          // an id without a piece
        bool differs = false;      // roundtrip: a difference was found, at fd
        uint64_t fd = 0;
        for (uint64_t k0 = 0; k0 < ntok; k0 += 64) {
            const uint2 e = e_next;
            e_next = entry_load(a, id_next, ntok, k0 + 64, lane);
            id_next = id_load(a.ids, ib, ntok, k0 + 128, lane);
            // the pieces before the first id without one still count (a difference in them is a difference)
            const uint64_t none = ballot(e.y == DETOK_NONE);
            const unsigned n_ok = none ? (unsigned)__builtin_ctzll(none) : 64u;
            bad = none != 0;
            const uint32_t len = lane < n_ok ? e.y : 0u;
            const uint32_t ei = wave_incl_scan_add(len);   // (64 pieces of at most 65535 bytes)
            const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)ei, 63);
            if (KIND == DECODE_SIZES) {
                // the first decoded byte decides the strip: the first piece of the string that is not empty
                if (strip_flag && total == 0 && T != 0) {
                    const unsigned first = (unsigned)__builtin_ctzll(ballot(len != 0u));
                    const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)e.x, (int)first);
                    strip = a.blob[off] == 0x20u;
                }
            } else {
                for (uint32_t it = 0; it < T; it += 64) {
                    const uint32_t o = it + lane;
                    // m = the pieces of this round that end at or before o: byte o lies in piece m
                    uint32_t m = 0;
#pragma unroll
                    for (unsigned step = 32; step; step >>= 1)
                        if (lane_read(ei, m + step - 1) <= o) m += step;
                    // (m <= 63; at o >= T, where no byte is, it names some piece that is not read)
                    const uint32_t end = lane_read(ei, m), plen = lane_read(len, m), poff = lane_read(e.x, m);
                    const bool have = o < T;
                    unsigned b = 0;
                    if (have) b = a.blob[poff + (o - (end - plen))];
                    if (strip_flag && total == 0 && it == 0)
                        strip = (unsigned)__builtin_amdgcn_readlane((int)b, 0) == 0x20u;
                    const uint64_t g = total + o;          // the byte's index in the string's decode
                    const uint64_t p = g - strip;          // ... and its position on the other side
                    const bool live = have && g >= strip;
                    if (KIND == DECODE_BYTES) {
                        if (live && p < lim) a.out[base + p] = (uint8_t)b;
                    } else {
                        const uint64_t diff = ballot(live && p < lim && a.text[base + p] != (uint8_t)b);
                        if (diff) {
                            differs = true;
                            fd = total + it + (unsigned)__builtin_ctzll(diff) - strip;
                            break;
                        }
                        if (total + it + 64 - strip > lim && total + T - strip > lim) {   // decoded past the text's end
                            differs = true;
                            fd = lim;
                            break;
                        }
                    }
                }
            }
            total += T;
            if (bad || differs) break;
        }
        const uint64_t dlen = total - strip;
        if (lane == 0) {
            if (KIND == DECODE_SIZES) {
                a.out_len[s] = dlen;
            } else if (KIND == DECODE_BYTES) {
                a.result[s] = bad || dlen != lim ? DPT_STATUS_INTERNAL : DPT_STATUS_OK;
            } else {
                if (!differs && !bad && dlen != lim) {   // one side is a prefix of the other
                    differs = true;
                    fd = dlen < lim ? dlen : lim;
                }
                a.result[s] = differs ? DPT_RT_DIFFERS : bad ? DPT_STATUS_INTERNAL : DPT_RT_EQUAL;
                if (differs && a.first_diff) a.first_diff[s] = (uint32_t)fd;
            }
        }
    }
}

}  // namespace dec

hipError_t launch_decode(const DecodeLaunch &p, hipStream_t stream) {
    if (p.n_str == 0) return hipSuccess;
    const unsigned blocks = wave_per_string_blocks(p.n_str, dec::WAVES);
    if (p.kind == DECODE_SIZES) hipLaunchKernelGGL(dec::decode_kernel<DECODE_SIZES>, dim3(blocks), dim3(dec::WAVES * 64), 0, stream, p);
    else if (p.kind == DECODE_BYTES) hipLaunchKernelGGL(dec::decode_kernel<DECODE_BYTES>, dim3(blocks), dim3(dec::WAVES * 64), 0, stream, p);
    else hipLaunchKernelGGL(dec::decode_kernel<DECODE_ROUNDTRIP>, dim3(blocks), dim3(dec::WAVES * 64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpt
