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

}  // namespace dpt
