// dpt_wave.h -- the wave primitives every kernel file uses (64-lane wavefronts, GFX9 DPP).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpt {

__device__ __forceinline__ unsigned lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ unsigned uni(unsigned x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// the value of lane `src` (< 64, per lane)
__device__ __forceinline__ unsigned lane_read(unsigned v, unsigned src) {
    return (unsigned)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
}

// inclusive add-scan over 64 lanes (GFX9 DPP: row_shr 1/2/4/8, row_bcast 15/31)
__device__ __forceinline__ unsigned wave_incl_scan_add(unsigned v) {
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xF, 0xF, true);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xA, 0xF, false); // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xC, 0xF, false); // row_bcast:31
    return v;
}

// lane l receives x[l-1]; lane 0 receives `in` (wave_shr:1)
__device__ __forceinline__ unsigned wave_shift_in(unsigned x, unsigned in) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)in, (int)x, 0x138, 0xF, 0xF, false);
}

// ---- what the tokenize kernels (dpt_kernels.hip and its dpt_tok_*.h) use on top of those

// inclusive max-scan over 64 lanes (values >= 0; the same DPP steps as the add scan)
__device__ __forceinline__ unsigned wave_incl_scan_max(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0u, v, 0x111, 0xF, 0xF, true));  // row_shr:1
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0u, v, 0x112, 0xF, 0xF, true));  // row_shr:2
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0u, v, 0x114, 0xF, 0xF, true));  // row_shr:4
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0u, v, 0x118, 0xF, 0xF, true));  // row_shr:8
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0u, v, 0x142, 0xA, 0xF, false)); // row_bcast:15
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0u, v, 0x143, 0xC, 0xF, false)); // row_bcast:31
    return v;
}

// min within each row of 16 lanes, result in every lane of the row
// (mov_dpp with bound_ctrl lets hipcc fold each step into one v_min_u32_dpp)
__device__ __forceinline__ unsigned row_min_u32(unsigned v) {
    v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true));  // row_half_mirror
    v = min(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true));  // row_mirror
    return v;
}

// min over 64 lanes, result uniform (SGPR)
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = row_min_u32(v);
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false)); // row_bcast:15
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false)); // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false));
    return __builtin_amdgcn_readlane(v, 63);
}

// lane l receives x[l-1]; the first lane of each row receives `in` (row_shr:1; the wave's: wave_shift_in)
__device__ __forceinline__ unsigned row_shift_in(unsigned x, unsigned in) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)in, (int)x, 0x111, 0xF, 0xF, false);
}

// Lane-group shifts for lane-mode B: lane l of a group of LW lanes receives x of lane l + K (gshl) / l - K (gshr),
// `fill` past the group's edge.  LW = 16: one DPP row op (row_shl / row_shr:K); LW = 64 (one string across the
// wave, the one-string kernel): ds_bpermute.
template <int LW, unsigned K>
__device__ __forceinline__ unsigned gshl(unsigned x, unsigned fill) {
    if constexpr (LW == 16) {
        return (unsigned)__builtin_amdgcn_update_dpp((int)fill, (int)x, 0x100 | K, 0xF, 0xF, false);
    } else {
        const unsigned l = lane_id();
        const unsigned v = (unsigned)__builtin_amdgcn_ds_bpermute((int)(((l + K) & 63u) << 2), (int)x);
        return l + K < 64u ? v : fill;
    }
}
template <int LW, unsigned K>
__device__ __forceinline__ unsigned gshr(unsigned x, unsigned fill) {
    if constexpr (LW == 16) {
        return (unsigned)__builtin_amdgcn_update_dpp((int)fill, (int)x, 0x110 | K, 0xF, 0xF, false);
    } else {
        const unsigned l = lane_id();
        const unsigned v = (unsigned)__builtin_amdgcn_ds_bpermute((int)(((l - K) & 63u) << 2), (int)x);
        return l >= K ? v : fill;
    }
}

// x behind an empty asm (no instruction): the optimizer cannot see through it, so a select on a loaded value is not
// turned back into an exec-mask branch (a load that only one side of a select needs is sunk under a branch of its own)
__device__ __forceinline__ unsigned opaque(unsigned x) {
    asm("" : "+v"(x));
    return x;
}
// max over the 64 lanes, wave-uniform (an SGPR): row_shr maxima, then the rows' last lanes
__device__ __forceinline__ unsigned wave_umax(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true));
    return uni(max(max((unsigned)__builtin_amdgcn_readlane((int)v, 15), (unsigned)__builtin_amdgcn_readlane((int)v, 31)),
                   max((unsigned)__builtin_amdgcn_readlane((int)v, 47), (unsigned)__builtin_amdgcn_readlane((int)v, 63))));
}

// 64-bit inclusive add-scan over the wave (ds_bpermute shifts)
__device__ __forceinline__ uint64_t wave_incl_scan_add64(uint64_t v, unsigned lane) {
#pragma unroll
    for (unsigned k = 1; k < 64; k <<= 1) {
        const int src = (int)((lane >= k ? lane - k : lane) << 2);
        const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)(unsigned)v);
        const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)(unsigned)(v >> 32));
        v += lane >= k ? (((uint64_t)hi << 32) | lo) : 0ull;
    }
    return v;
}

__device__ __forceinline__ uint64_t uni64(uint64_t x) {
    return ((uint64_t)uni((unsigned)(x >> 32)) << 32) | uni((unsigned)x);
}

// lowest set bit (v_ffbl_b32: 0xFFFFFFFF for 0, no select needed where 0 cannot matter)
__device__ __forceinline__ unsigned ffbl(unsigned x) {
    unsigned r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace dpt
