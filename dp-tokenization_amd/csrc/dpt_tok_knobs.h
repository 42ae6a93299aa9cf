// dpt_tok_knobs.h -- every compile-time option of the dpt_kernels.hip unit: the numeric tunables (a -D changes a size,
// never which code exists) and the diagnostic switches.  Read by dpt_kernels.hip and by A/B builds
// (make variant DEFS=-D..., tools/build_sed.sh).  The decided boolean A/B knobs are gone with their losing sides:
// DESIGN.md §9 keeps their numbers.
#pragma once
#include "dpt_internal.h"

namespace dpt {

// ------------------------------------------------------------------ numeric tunables
//   name            default  what it sizes                                                    measured (run tags: DESIGN.md §9)
//   DPT_BULK_U         4     C2's bulk pass: tokens per lane per round (their lookups before   r03 (every round's lookups first
//                            their stores)                                                     spilled: cfg2 -4.1 %)
//   DPT_HP_U           2     C2's hash pass: token rounds of 64 per iteration (loads before    r03 (1 or 4 rounds slower)
//                            stores)
//   DPT_A0_R2_MIN     24     A0's third-byte round: taken when at least this many lanes of    r05ae
//                            the slot have a walk past two plain bytes
//   DPT_WPE16          6     waves per SIMD asked of the 256-byte 16-lane kernels (<= 80       r03e
//                            VGPRs each); LDS (22 waves per CU) then binds -- 96 VGPRs / 5
//                            waves: no scratch spills, cfg2 -1.9 %
//   DPT_WPE64          6     the same for the 256-byte 64-lane kernel: BLOOM 17.4 -> 19.8      r03aa, r03ac
//                            GB/s against no cap (95 VGPRs, 20 waves; 7 or 8 spill more)
//   DPT_WPC_LO        20     small calls: the persistent grid's fewest resident waves per CU   profiles/r06_ab.log (r06c, r06o)
//                            (launch_tok)
//   DPT_WPC_GRAN     512     LDS allocation granule (bytes) that caps the resident waves per   profiles/r06_ab.log (r06b)
//                            CU (launch_tok)
//   A_REFILL          32     phase A: idle lanes needed before a batched refill                1 / 8 / 16 / 32 within 2 %
//   A_REFILL64        32     the same for the 64-lane kernels                                  8 / 1: neutral / -0.5 %, r03aa
//   NPART             16     first-pass work partitions (<= NPART_MAX)                         round 2 (one counter bound the kernel:
//                                                                                              TokPass::body)
#ifndef DPT_BULK_U
#define DPT_BULK_U 4
#endif
#ifndef DPT_HP_U
#define DPT_HP_U 2
#endif
#ifndef DPT_A0_R2_MIN
#define DPT_A0_R2_MIN 24
#endif
constexpr int A0_R2_MIN = DPT_A0_R2_MIN;
#ifndef DPT_WPE16
#define DPT_WPE16 6
#endif
constexpr int WPE16 = DPT_WPE16;
#ifndef DPT_WPE64
#define DPT_WPE64 6
#endif
constexpr int WPE64 = DPT_WPE64;
#ifndef DPT_WPC_LO
#define DPT_WPC_LO 20
#endif
#ifndef DPT_WPC_GRAN
#define DPT_WPC_GRAN 512
#endif
constexpr unsigned A_REFILL = 32;
constexpr unsigned A_REFILL64 = 32;
constexpr unsigned NPART = 16;
static_assert(NPART >= 1 && NPART <= NPART_MAX, "NPART");

// ------------------------------------------------------------------ diagnostics: wrong results by design
// (never in the product build; DPT_STAMPS and DPT_WSTAMPS are plain -D switches, read in dpt_tok_lds.h)
#ifndef DPT_STOP     // diagnostic builds only (wrong results): 1 = prep only, 21 = + A0, 2 = + A, 25 / 26 / 27 =
                     // + lane-mode B's cut points / recurrence / transfer scan + fix-up, 3 = + B/C0/C1
#define DPT_STOP 9
#endif
#ifndef DPT_DIAG_PREP   // diagnostic builds only (cfg2-shaped input): 1 = static claims (no counter atomics),
#define DPT_DIAG_PREP 0  // 2 = offsets computed as 256 s (no str_off loads), 3 = both, 4 = a second dependent claim
#endif                   // atomic, 8 = no batch-sum atomics (wrong CSR offsets) -- the refill chain's and the atomics' cost
#ifndef DPT_C2STOP   // diagnostic builds only (wrong results): C2 stops after its bulk pass (1) / hash pass (2)
#define DPT_C2STOP 0
#endif
#define DPT_RUN_B (DPT_STOP >= 3 && DPT_STOP != 21)
#define DPT_RUN_C2 (DPT_STOP == 9)

}  // namespace dpt
