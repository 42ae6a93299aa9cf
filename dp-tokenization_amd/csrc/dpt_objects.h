// dpt_objects.h -- what the two halves of the C-ABI share: the objects behind its handles, error reporting, and
// the one encode call both run (dpt_api.cpp: the objects, the workspace and the device-pointer calls;
// dpt_host.cpp: the host-buffer calls and their staging).
#pragma once
#include <string>
#include <vector>

#include "dpt_internal.h"

struct dpt_vocab : dpt::VocabScalars {
    int device = 0;
    int2 *d_slots = nullptr;
    int32_t *d_ids = nullptr;
    int16_t *d_pair16 = nullptr;      // C2's pair-id table (dpt::PAIR16_N int16), then phase A0's byte-pair table (65536 uint2), then the token hash
    int4 *d_slots4 = nullptr;         // {base | TERM, check, id, child filter} for the lane kernel
    // dpt_token_spans: byte length per id - id_min (0: no token has this id); null when the ids are too
    // sparse for a dense table or two tokens of different length share an id (the spans calls: DPT_E_VOCAB)
    uint16_t *d_tok_len = nullptr;
};

// The device copy of a decode table (dpt_detok.cpp build_detok_tables).
struct dpt_detok {
    int device = 0;
    uint2 *d_tab = nullptr;     // {offset in the blob, length | dpt::DETOK_NONE} per id - id_min
    uint8_t *d_blob = nullptr;  // the decoded pieces (never null: an empty blob is one byte)
    int32_t id_min = 0;
    uint32_t n_tab = 0;
};

// The device copy of a pre-tokenization table (dpt_pretok.cpp build_pretok_tables), and what of it travels with the
// kernel arguments.
struct dpt_pretok {
    int device = 0;
    uint32_t *d_bmp = nullptr;      // dpt::PRETOK_BMP_WORDS
    uint32_t *d_astral = nullptr;   // n_astral known code points from U+10000 up (null: none)
    uint8_t *d_lit = nullptr;       // the literal block: 8 words, n_lit + 1 offsets, the bytes
    uint8_t *d_prefix = nullptr;    // the BOS piece, then U+2581
    uint32_t n_astral = 0, n_lit = 0, bos_len = 0;
    bool runs_ok = true;
    uint64_t ascii_known[2] = {0, 0};
    uint64_t lit_first[4] = {0, 0, 0, 0};
};

// The device copy of a byte-level split's separator table (dpt_bytelevel.cpp build_bytelevel_tables): the separators
// below U+0080 travel with the kernel arguments.
struct dpt_bytelevel {
    int device = 0;
    uint32_t *d_high = nullptr;     // n_high separators from U+0080 up, ascending (null: none)
    uint32_t n_high = 0;
    uint64_t ascii[2] = {0, 0};
};

// The device copy of a BPE pair table (dpt_bpe.cpp build_bpe_tables; the format is in dpt_bpe_table.h).
struct dpt_bpe {
    int device = 0;
    uint4 *d_entries = nullptr;     // 2 * n_buckets entries {left, right, merged, rank}
    uint32_t n_buckets = 0, seed = 0;
};

struct dpt_ctx {
    int device = 0;
    // workspace of the device path (ensure_workspace)
    int32_t *staging32 = nullptr;     // ids staged as int32 (vocabularies with an id outside 0..32767)
    uint64_t cap32 = 0;
    int16_t *staging16 = nullptr;     // ids staged as int16 (vocabularies with ids16)
    uint64_t cap16 = 0;
    uint8_t *arena = nullptr;         // the unbounded pass's scratch, 20 bytes per input byte it holds
    uint64_t arena_cap = 0;           // input bytes
    bool arena_reserved = false;      // dpt_ctx_reserve_vocab set it: the encode path does not resize it
    uint64_t *counts = nullptr;
    uint32_t *retry_list = nullptr;
    uint64_t cap_str = 0;
    dpt::CounterBlock *ctr = nullptr; // the counter block (dpt::CTR_ALLOC_BYTES)
    uint8_t *wsl_scratch = nullptr;   // word lists of the 256-byte pass (dpt::wsl_scratch_bytes)
    uint4 *pend = nullptr;            // pending residual tokens of the 256-byte pass (dpt::pend_scratch_bytes)
    // two parity regions R0, R1 of batch lines (dpt::BS_LINE u64 per 256-string batch: its sum in the
    // first), then the batch prefixes of the scan path (cap_batches u64): the call of parity P uses R_P
    // and -- fold calls -- zeroes R_(1-P) for the next one (the parity flips); between calls R_parity
    // is all zero.  See dpt_internal.h fin_fold and BS_LINE.
    unsigned long long *flags = nullptr;
    uint64_t cap_batches = 0;
    int flag_parity = 0;
    unsigned max_blocks = 0;
    // host paths (dpt_host.cpp Stager alone touches them): one device buffer in and one out (dpt_host_layout.h), each
    // mirrored by a pinned host buffer so every copy is one async DMA
    uint8_t *d_in = nullptr, *p_in = nullptr, *d_out = nullptr, *p_out = nullptr;
    uint8_t *pd_in = nullptr, *pd_out = nullptr;   // p_in / p_out as the device addresses them (zero-copy calls), or null
    uint64_t cap_in = 0, cap_pin_in = 0, cap_out = 0, cap_pin_out = 0;
    // dpt_ctx_set_histogram: folded into the next encode's finish pass
    int64_t *hist = nullptr;
    uint32_t hist_bins = 0;
    bool hist_overwrite = false;
    // profiling
    bool profile = false;
    std::vector<hipEvent_t> events;   // groups of 4 per call
    uint64_t launches = 0;
    // test-only (dpt_ctx_debug_counter_bias): every call starts the unbounded pass's arena counter and the
    // far-pair counter at this value, the arena and far pointers passed down shifted by it
    uint64_t counter_bias = 0;
    // The lean route's hint as the host sees it (dpt_internal.h LeanWord): lean_host[0] mirrors LEAN_OFF -- the lean
    // kernels store it to this pinned word as well -- and is read without a synchronise when a call is planned: while it
    // says "off" only every LEAN_RETRY-th call launches the lean kernel (whose probe may turn the hint on again), the
    // others run the general kernel alone, as before the lean route.  A stale read costs one call the better route.
    uint32_t *lean_host = nullptr, *lean_host_dev = nullptr;
    uint32_t lean_skipped = 0;   // calls planned without the lean launch since the hint went off
    bool debug_no_lean = false;  // test-only (dpt_ctx_debug_no_lean): no call of this context takes the lean route
};

namespace dpt {

// (the thread's message itself lives in dpt_api.cpp: set_last_error)
inline int fail(int code, const std::string &msg) { return set_last_error(msg), code; }
inline int hip_fail(hipError_t e, const char *what) { return fail(DPT_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// A host table as a fresh device buffer (an empty table: none, *d stays null).
template <typename D, typename T>
hipError_t upload(D **d, const std::vector<T> &h) {
    if (h.empty()) return hipSuccess;
    const hipError_t e = hipMalloc((void **)d, h.size() * sizeof(T));
    return e != hipSuccess ? e : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// Every *_create call (n_tok = 0: no table): a device of this index exists and the token table's offsets ascend.  (dpt_api.cpp)
int check_device_and_table(int device, const uint64_t *tok_off, uint32_t n_tok);

// What the sizes call (write = false: out_len, pre_status) and the write call (pre_status, out_text, out_off, cut_mask)
// of a splitter share, dpt_pretok_* and dpt_bytelevel_* alike: the null checks, the launch's common fields, and
// the launch itself, which adds the table's part -- launch(t, a, hip_stream).
template <typename Launch, typename Obj>
int split_call(const Obj *t, const char *null_obj, int (*launch)(const Obj *, Launch, void *), bool write, const uint8_t *text,
               const uint64_t *str_off, uint64_t n_str, uint64_t *out_len, int32_t *pre_status, uint8_t *out_text,
               const uint64_t *out_off, uint8_t *cut_mask, void *hip_stream) {
    if (!t) return fail(DPT_E_ARG, null_obj);
    if (!text || !str_off) return fail(DPT_E_ARG, "null text / str_off");
    if (!write && (!out_len || !pre_status)) return fail(DPT_E_ARG, "null out_len / pre_status");
    if (write && (!pre_status || !out_text || !out_off || !cut_mask)) return fail(DPT_E_ARG, "null pre_status / out_text / out_off / cut_mask");
    if (n_str == 0) return DPT_OK;
    Launch a{};
    a.write = write; a.text = text; a.str_off = str_off; a.n_str = n_str; a.out_len = out_len; a.pre_status = pre_status;
    a.out_text = out_text; a.out_off = out_off; a.cut_mask = cut_mask;
    return launch(t, a, hip_stream);
}

// Device buffer of at least `need` elements: exact on first allocation, +25 % when it grows.  A buffer that
// already holds `need` is left where it is.
template <typename T>
hipError_t grow(T **p, uint64_t *cap, uint64_t need) {
    if (need <= *cap && *p) return hipSuccess;
    uint64_t n = need < 64 ? 64 : need;
    if (*cap) n += n / 4;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e == hipSuccess) *cap = n;
    return e;
}

// What an encode call and a host-path call both name (a member left at its default is absent): the argument
// list the five encode entry points share, the rest by name.
struct CsrCall {
    int mode_flags = DPT_MODE_RAW;   // DPT_MODE_* | DPT_FLAG_*
    const uint8_t *text = nullptr, *cut_mask = nullptr;
    const uint64_t *str_off = nullptr;
    uint64_t n_bytes = 0, n_str = 0, ids_cap = 0, far_cap = 0;
    int32_t *ids = nullptr, *status = nullptr, *capped_len = nullptr;
    uint64_t *id_off = nullptr, *edges = nullptr, *far = nullptr;   // dpt_dp_host*: the per-atom-end masks, far_cap far edge pairs
    void set(int mode_flags_, const uint8_t *text_, uint64_t n_bytes_, const uint64_t *str_off_, const uint8_t *cut_mask_,
             uint64_t n_str_, int32_t *status_, int32_t *capped_len_, int32_t *ids_ = nullptr, uint64_t ids_cap_ = 0) {
        mode_flags = mode_flags_; text = text_; n_bytes = n_bytes_; str_off = str_off_; cut_mask = cut_mask_; n_str = n_str_;
        status = status_; capped_len = capped_len_; ids = ids_; ids_cap = ids_cap_;
    }
};
// One encode call as its caller sees it (encode_impl): DEVICE pointers.
struct EncodeRequest : CsrCall {
    hipStream_t stream = nullptr;
    uint64_t *padded_counts = nullptr;   // dpt_encode_padded: the caller's counts (id_off is not used)
    bool dev_call = false;               // dpt_encode itself: it alone takes an armed histogram (dpt_ctx_set_histogram_ex)
    uint64_t *ctr_snap = nullptr;        // host path: where the counter block's reset copies its first 64 bytes
    bool no_fallback = false;            // host path: no string needs the 2048-byte or unbounded pass
};

// dpt_api.cpp
int ensure_workspace(dpt_ctx *c, const dpt_vocab *v, uint64_t n_bytes, uint64_t n_str, uint64_t long_bytes, bool staging = true);
int encode_impl(dpt_ctx *c, const dpt_vocab *v, const EncodeRequest &r);
// A spans / decode launch from its caller's arguments (v null: without the vocabulary's part; decode_check adds
// the table's), and the argument checks the device and the host form of a call share.
SpansLaunch spans_args(const dpt_vocab *v, int mode, const uint8_t *text, const uint64_t *str_off, const uint8_t *cut_mask,
                       uint64_t n_str, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint32_t *tok_end,
                       uint32_t *tok_word, int32_t *span_status);
int spans_check(const SpansLaunch &p, const dpt_vocab *v, uint64_t n_bytes);
extern const char *const NO_TOK_LEN;   // the spans calls' DPT_E_VOCAB message
DecodeLaunch decode_args(int kind, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str);
int decode_check(DecodeLaunch *p, const dpt_detok *d, int flags);

}  // namespace dpt
