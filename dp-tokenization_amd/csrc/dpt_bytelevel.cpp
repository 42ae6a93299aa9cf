// dpt_bytelevel.cpp -- the byte-level split's separator table (include/dpt.h dpt_bytelevel_create): its host builder,
// the object that holds its device copy, and the argument checks of the two device calls whose kernels are in
// dpt_bytelevel.hip.  The rule itself is stated in the header.
//
// build_bytelevel_tables calls no HIP function: testable without a device (dpt_debug_bytelevel_table,
// tests/test_bytelevel_tables.py; tests/bytelevel_ref.py restates the rule).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "dpt_objects.h"

namespace dpt {

const char *build_bytelevel_tables(const uint32_t *sep_cps, uint32_t n_sep, ByteLevelTables *out) try {
    if (!sep_cps) return "null separator list";
    if (n_sep == 0 || n_sep > DPT_BYTELEVEL_MAX_SEPARATORS) return "0 or more than DPT_BYTELEVEL_MAX_SEPARATORS separators";
    ByteLevelTables &t = *out;
    t.ascii[0] = t.ascii[1] = 0;
    t.high.clear();
    for (uint32_t k = 0; k < n_sep; k++) {
        const uint32_t cp = sep_cps[k];
        if (cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu)) return "a separator that is not a Unicode scalar value";
        if (cp < 0x80u) t.ascii[cp >> 6] |= 1ull << (cp & 63u);
        else t.high.push_back(cp);
    }
    if (!((t.ascii[0] >> 0x20) & 1u)) return "U+0020 is not among the separators";
    std::sort(t.high.begin(), t.high.end());
    t.high.erase(std::unique(t.high.begin(), t.high.end()), t.high.end());
    t.n_sep = (uint32_t)(__builtin_popcountll(t.ascii[0]) + __builtin_popcountll(t.ascii[1]) + t.high.size());
    return nullptr;
} catch (const std::bad_alloc &) {
    return "out of host memory";
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_debug_bytelevel_table(const uint32_t *sep_cps, uint32_t n_sep, int which, void *out, uint64_t cap, uint64_t *size) {
    if (!size) return fail(DPT_E_ARG, "null size");
    if (which < 0 || which >= 3) return fail(DPT_E_ARG, "no such table");
    ByteLevelTables t;
    if (const char *err = build_bytelevel_tables(sep_cps, n_sep, &t)) return fail(DPT_E_ARG, err);
    const int64_t scalars[DPT_BYTELEVEL_SCALAR_INTS] = {t.n_sep, (int64_t)t.high.size()};
    const void *src[] = {t.ascii, t.high.data(), scalars};
    const uint64_t len[] = {sizeof(t.ascii), t.high.size() * 4, sizeof(scalars)};
    return debug_table_out(src[which], len[which], out, cap, size);
}

int dpt_bytelevel_create(const uint32_t *sep_cps, uint32_t n_sep, int device, dpt_bytelevel **out) {
    if (!out) return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    ByteLevelTables t;
    if (const char *err = build_bytelevel_tables(sep_cps, n_sep, &t)) return fail(DPT_E_ARG, err);
    if (const int rc = check_device_and_table(device, nullptr, 0)) return rc;
    DeviceGuard g(device);
    dpt_bytelevel *p = new (std::nothrow) dpt_bytelevel();
    if (!p) return fail(DPT_E_ARG, "out of host memory");
    p->device = device; p->n_high = (uint32_t)t.high.size(); p->ascii[0] = t.ascii[0]; p->ascii[1] = t.ascii[1];
    const hipError_t e = upload(&p->d_high, t.high);
    if (e != hipSuccess) {
        dpt_bytelevel_destroy(p);
        return hip_fail(e, "separator table upload");
    }
    *out = p;
    return DPT_OK;
}

int dpt_bytelevel_destroy(dpt_bytelevel *p) {
    if (!p) return DPT_OK;
    DeviceGuard g(p->device);
    (void)hipFree(p->d_high);
    delete p;
    return DPT_OK;
}

// The table's part of a launch, and the launch.
static int bytelevel_launch(const dpt_bytelevel *t, ByteLevelLaunch p, void *hip_stream) {
    p.ascii_sep[0] = t->ascii[0]; p.ascii_sep[1] = t->ascii[1]; p.high = t->d_high; p.n_high = t->n_high;
    DeviceGuard g(t->device);
    const hipError_t e = launch_bytelevel(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "byte-level split launch");
    return DPT_OK;
}

int dpt_bytelevel_sizes(const dpt_bytelevel *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str, uint64_t *out_len,
                        int32_t *pre_status, void *hip_stream) {
    return split_call(p, "null bytelevel", bytelevel_launch, false, text, str_off, n_str, out_len, pre_status, nullptr, nullptr, nullptr,
                      hip_stream);
}

int dpt_bytelevel_write(const dpt_bytelevel *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str,
                        const int32_t *pre_status, uint8_t *out_text, const uint64_t *out_off, uint8_t *cut_mask,
                        void *hip_stream) {
    return split_call(p, "null bytelevel", bytelevel_launch, true, text, str_off, n_str, nullptr, const_cast<int32_t *>(pre_status),
                      out_text, out_off, cut_mask, hip_stream);
}

}  // extern "C"
