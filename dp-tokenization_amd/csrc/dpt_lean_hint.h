// The host's side of the lean route's hint (dpt_objects.h dpt_ctx::lean_host; DESIGN.md 4, "the lean pass"): pure, no HIP.
#pragma once
#include <stdint.h>

namespace dpt {

constexpr uint32_t LEAN_RETRY = 8;   // hint off: every LEAN_RETRY-th call launches the lean kernel (its probe) again

// Plans one call: hint_off is the mirror word as read now (possibly a call stale), skipped the context's count of calls
// planned without the lean launch since the hint went off.  Returns true when this call runs without the lean launch.
inline bool lean_plan_skip(uint32_t hint_off, uint32_t &skipped) {
    if (!hint_off) {
        skipped = 0;
        return false;
    }
    skipped++;
    return skipped % LEAN_RETRY != 0;
}

}  // namespace dpt
