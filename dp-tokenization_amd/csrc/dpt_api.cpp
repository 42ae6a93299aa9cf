// dpt_api.cpp -- the C-ABI declared in include/dpt.h.
//
// Owns: the device copy of the vocabulary (dpt_vocab: the upload of dpt_vocab.cpp's build_vocab_tables) and of
// a decode table (dpt_detok: dpt_detok.cpp's build_detok_tables),
// per-stream workspaces (dpt_ctx), argument checking, the host-buffer convenience paths and their staging,
// and the event-based kernel timing used by bench.py.  No C++ exception crosses the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dpt.h"
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

static uint64_t flag_words(uint64_t cap_batches) { return cap_batches * (2 * dpt::BS_LINE + 1); }
// The regions of a call of this parity (dpt_ctx::flags below): its own batch lines, the other parity's
// (which it zeroes) and the batch prefixes behind both.
static void flag_regions(unsigned long long *flags, uint64_t cap_batches, int parity, dpt::EncodeLaunch *p) {
    const uint64_t rl = cap_batches * dpt::BS_LINE;
    p->flags = flags + (parity ? rl : 0); p->zero_other = flags + (parity ? 0 : rl); p->zero_n = cap_batches;
    p->bpre = flags + 2 * rl;
}

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
    // host paths (stage_host): one device buffer in and one out (EncodeLayout, SpansLayout), each mirrored
    // by a pinned host buffer so every copy is one async DMA
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
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(DPT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

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

// Device buffer of at least `need` elements: exact on first allocation, +25 % when it grows.
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

// Pinned host buffer likewise (4096 bytes at least); *pd, its address as the device sees it, is cleared when it moves.
hipError_t grow_pinned(uint8_t **p, uint8_t **pd, uint64_t *cap, uint64_t need) {
    if (need <= *cap && *p) return hipSuccess;
    uint64_t n = need < 4096 ? 4096 : need + (*cap ? need / 4 : 0);
    if (*p) (void)hipHostFree(*p);
    *p = *pd = nullptr;
    *cap = 0;
    hipError_t e = hipHostMalloc((void **)p, n, hipHostMallocDefault);
    if (e == hipSuccess) *cap = n;
    return e;
}

// Input bytes the unbounded pass can hold per call when the caller does not say: every string for
// small batches, 1/32 of the batch for large ones (20 bytes of arena per held byte: 5/8 of the
// batch's size); the host path grows it on overflow, dpt_ctx_reserve_vocab sets it.
uint64_t default_long_bytes(uint64_t n_bytes) {
    const uint64_t floor = 4ull << 20;
    uint64_t lb = n_bytes / 32;
    if (lb < floor) lb = floor;
    return lb < n_bytes ? lb : n_bytes;
}

constexpr uint64_t ARENA_PER_BYTE = 20;   // uint4 rec + int32 stg (dpt_long.hip)

// v == nullptr: both staging widths (the vocabulary is not known yet); staging = false: no staging
// (dpt_encode_padded writes the ids into the caller's buffer)
int ensure_workspace(dpt_ctx *c, const dpt_vocab *v, uint64_t n_bytes, uint64_t n_str, uint64_t long_bytes,
                     bool staging = true) {
    hipError_t e;
    bool fresh = false;   // zeroed buffers were (re)allocated
    const bool need16 = staging && (!v || v->ids16), need32 = staging && (!v || !v->ids16);
    // (+8 elements: the finish pass reads staged ids as whole dwords, up to 2 elements past the last)
    if (need16 && (e = grow(&c->staging16, &c->cap16, n_bytes + 8)) != hipSuccess) return hip_fail(e, "hipMalloc(staging16)");
    if (need32 && (e = grow(&c->staging32, &c->cap32, n_bytes + 8)) != hipSuccess) return hip_fail(e, "hipMalloc(staging32)");
    // long_bytes = 0 (the encode path): the default size, unless the caller reserved the arena -- a
    // reserved arena is left alone, so a reserved call never reallocates (capture-safe, dpt.h)
    const uint64_t lb = long_bytes ? long_bytes : default_long_bytes(n_bytes);
    if (!c->arena || (lb > c->arena_cap && (long_bytes || !c->arena_reserved))) {
        uint64_t cap = c->arena_cap ? c->arena_cap * ARENA_PER_BYTE : 0;
        if ((e = grow(&c->arena, &cap, lb * ARENA_PER_BYTE)) != hipSuccess) return hip_fail(e, "hipMalloc(arena)");
        c->arena_cap = cap / ARENA_PER_BYTE;
    }
    if (n_str > c->cap_str || !c->counts) {
        uint64_t cap = c->cap_str, cap2 = dpt::N_RETRY_LISTS * c->cap_str;
        e = grow(&c->counts, &cap, n_str);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(counts)");
        e = grow(&c->retry_list, &cap2, dpt::N_RETRY_LISTS * n_str);   // (dpt::RetryList)
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(retry_list)");
        cap2 /= dpt::N_RETRY_LISTS;
        c->cap_str = cap < cap2 ? cap : cap2;
    }
    const uint64_t nbat = (n_str + dpt::FIN_BATCH - 1) / dpt::FIN_BATCH;
    if (nbat > c->cap_batches || !c->flags) {
        // (+25 % on growth; the regions start at zero and every call leaves the next one's zeroed)
        uint64_t capb = nbat > 1 ? nbat : 1;
        if (c->cap_batches) capb += capb / 4;
        if (c->flags) (void)hipFree(c->flags);
        c->flags = nullptr;
        c->cap_batches = 0;
        c->flag_parity = 0;
        if ((e = hipMalloc((void **)&c->flags, flag_words(capb) * sizeof(unsigned long long))) != hipSuccess) return hip_fail(e, "hipMalloc(flags)");
        if ((e = hipMemset(c->flags, 0, flag_words(capb) * sizeof(unsigned long long))) != hipSuccess) return hip_fail(e, "hipMemset(flags)");
        c->cap_batches = capb;
        fresh = true;
    }
    if (!c->wsl_scratch) {
        e = hipMalloc((void **)&c->wsl_scratch, dpt::wsl_scratch_bytes(c->max_blocks));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(wsl_scratch)");
    }
    if (!c->pend) {
        e = hipMalloc((void **)&c->pend, dpt::pend_scratch_bytes(c->max_blocks));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(pend)");
    }
    if (!c->ctr) {
        // zeroed once here; every call's finish kernel resets it for the next call
        e = hipMalloc((void **)&c->ctr, dpt::CTR_ALLOC_BYTES);
        if (e == hipSuccess) e = hipMemset(c->ctr, 0, dpt::CTR_ALLOC_BYTES);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(ctr)");
        fresh = true;
    }
    // the zero state every later call relies on must be in place before a call on any stream (a
    // non-blocking stream is not ordered after the null stream's memsets); allocations only
    if (fresh && (e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "hipDeviceSynchronize(zeroed workspace)");
    return DPT_OK;
}

// First-pass kernel: 16-lane rows (4 strings per wave) when every token has <= 16 code points,
// else 64-lane rows.  DPT_KERNEL=rows64 forces the 64-lane kernel (tests run it on the 32k vocab).
int kernel_variant(uint32_t max_cp) {
    int v = max_cp <= 16 ? dpt::KERNEL_ROWS16 : dpt::KERNEL_ROWS64;
    if (const char *e = getenv("DPT_KERNEL"))
        if (!strcmp(e, "rows64")) v = dpt::KERNEL_ROWS64;
    return v;
}

// What an encode call and a host-path call both name (a member left at its default is absent).
struct CsrCall {
    int mode_flags = DPT_MODE_RAW;   // DPT_MODE_* | DPT_FLAG_*
    const uint8_t *text = nullptr, *cut_mask = nullptr;
    const uint64_t *str_off = nullptr;
    uint64_t n_bytes = 0, n_str = 0, ids_cap = 0, far_cap = 0;
    int32_t *ids = nullptr, *status = nullptr, *capped_len = nullptr;
    uint64_t *id_off = nullptr, *edges = nullptr, *far = nullptr;   // dpt_dp_host*: the per-atom-end masks, far_cap far edge pairs
};
// One encode call as its caller sees it (encode_impl): DEVICE pointers.
struct EncodeRequest : CsrCall {
    hipStream_t stream = nullptr;
    uint64_t *padded_counts = nullptr;   // dpt_encode_padded: the caller's counts (id_off is not used)
    bool dev_call = false;               // dpt_encode itself: it alone takes an armed histogram (dpt_ctx_set_histogram_ex)
    uint64_t *ctr_snap = nullptr;        // host path: where the counter block's reset copies its first 64 bytes
    bool no_fallback = false;            // host path: no string needs the 2048-byte or unbounded pass
};
// One host-path call (encode_host): HOST pointers.
struct HostRequest : CsrCall {
    uint64_t *n_far = nullptr;   // dpt_dp_host_far: the far edge pairs found
    int depth = 0;               // 1: the rerun of the strings an arena overflow left out (it may not overflow again)
};

uint64_t al8(uint64_t x) { return (x + 7) & ~7ull; }
template <typename T>
T *at(uint8_t *buf, uint64_t off) { return reinterpret_cast<T *>(buf + off); }

// The encode host path's buffers, as byte offsets (text and id_off sit at 0):
struct EncodeLayout {
    uint64_t in_off, in_cut, in_bytes;   // in:  text | offsets rebased to 0 (the device view is self-contained) | cut mask
    uint64_t st, capped, ctr, ids, edges, far, out_bytes;   // out: id_off | status | capped | counters | ids | edges | far edge pairs
    EncodeLayout(uint64_t n_bytes, uint64_t n_str, bool with_edges, uint64_t far_pairs) {
        in_off = al8(n_bytes + 1); in_cut = in_off + 8 * (n_str + 1); in_bytes = in_cut + al8(n_bytes + 1);
        st = 8 * (n_str + 1); capped = st + al8(4 * n_str + 4); ctr = capped + al8(4 * n_str + 4);
        ids = ctr + sizeof(dpt::CounterBlock); edges = ids + al8(4 * (n_bytes + 1));
        far = edges + (with_edges ? 8 * (n_bytes + 1) : 0); out_bytes = far + 16 * far_pairs;
    }
};
// The spans host path's (str_off and tok_end sit at 0):
struct SpansLayout {
    uint64_t in_idoff, in_ids, in_st, in_text, in_cut, in_bytes;   // in:  str_off and id_off rebased to 0 | ids | status | text | cut mask
    uint64_t word, ss, out_bytes;                                  // out: tok_end | tok_word | span_status
    SpansLayout(uint64_t n_bytes, uint64_t n_str, uint64_t n_tok, bool cut, bool with_word) {
        in_idoff = 8 * (n_str + 1); in_ids = 2 * in_idoff; in_st = in_ids + al8(4 * n_tok + 4);
        in_text = in_st + al8(4 * n_str); in_cut = in_text + al8(n_bytes + 1); in_bytes = in_cut + (cut ? al8(n_bytes + 1) : 0);
        word = al8(4 * n_tok + 4); ss = with_word ? 2 * word : word; out_bytes = ss + al8(4 * n_str);
    }
};

// The decode host path's (id_off sits at 0; the sizes pass has out_len alone in the out buffer, the decode
// pass dec_status and the bytes):
struct DecodeLayout {
    uint64_t in_outoff, in_ids, in_st, in_bytes;   // in:  id_off rebased to 0 | out_off | ids | status
    uint64_t len_bytes, bytes;                     // out: out_len (sizes pass); dec_status | the decoded bytes (decode pass)
    DecodeLayout(uint64_t n_str, uint64_t n_tok) {
        in_outoff = 8 * (n_str + 1); in_ids = 2 * in_outoff; in_st = in_ids + al8(4 * n_tok + 4);
        in_bytes = in_st + al8(4 * n_str + 4);
        len_bytes = 8 * n_str; bytes = al8(4 * n_str + 4);
    }
};
// The round trip's (id_off and rt sit at 0):
struct RoundtripLayout {
    uint64_t in_stroff, in_ids, in_st, in_text, in_bytes;   // in:  id_off and str_off rebased to 0 | ids | status | text
    uint64_t fd, out_bytes;                                 // out: rt | first_diff
    RoundtripLayout(uint64_t n_bytes, uint64_t n_str, uint64_t n_tok) {
        in_stroff = 8 * (n_str + 1); in_ids = 2 * in_stroff; in_st = in_ids + al8(4 * n_tok + 4);
        in_text = in_st + al8(4 * n_str + 4); in_bytes = in_text + al8(n_bytes + 1);
        fd = al8(4 * n_str + 4); out_bytes = 2 * fd;
    }
};

// Both host paths' staging: the device buffers and their pinned mirrors hold in_bytes / out_bytes.  A
// zero-copy address (pd_in / pd_out) is valid or null: grow_pinned clears it when its pinned buffer moves,
// the zero-copy call (encode_host_impl) looks it up when it needs it.
int stage_host(dpt_ctx *c, uint64_t in_bytes, uint64_t out_bytes) {
    hipError_t e;
    if ((e = grow(&c->d_in, &c->cap_in, in_bytes)) != hipSuccess) return hip_fail(e, "hipMalloc(host-path in)");
    if ((e = grow(&c->d_out, &c->cap_out, out_bytes)) != hipSuccess) return hip_fail(e, "hipMalloc(host-path out)");
    if ((e = grow_pinned(&c->p_in, &c->pd_in, &c->cap_pin_in, in_bytes)) != hipSuccess) return hip_fail(e, "hipHostMalloc(in)");
    if ((e = grow_pinned(&c->p_out, &c->pd_out, &c->cap_pin_out, out_bytes)) != hipSuccess) return hip_fail(e, "hipHostMalloc(out)");
    return DPT_OK;
}

// The kernels take string lengths as 32-bit values (dpt.h): offsets must be monotone and every
// string shorter than 4 GiB, or a wrapped length would read past the text.  id_off (nullable, the spans path): monotone.
int check_str_off(const uint64_t *str_off, uint64_t n_str, uint64_t n_bytes, const uint64_t *id_off = nullptr) {
    if (str_off[n_str] - str_off[0] != n_bytes) return fail(DPT_E_ARG, "n_bytes != str_off[n_str]-str_off[0]");
    for (uint64_t i = 0; i < n_str; i++) {
        if (str_off[i + 1] < str_off[i]) return fail(DPT_E_ARG, "str_off not monotone");
        if (str_off[i + 1] - str_off[i] >= (1ull << 32)) return fail(DPT_E_ARG, "a string of 4 GiB or more");
        if (id_off && id_off[i + 1] < id_off[i]) return fail(DPT_E_ARG, "id_off not monotone");
    }
    return DPT_OK;
}

// The vocabulary's part of an encode launch.
void launch_vocab(const dpt_vocab *v, dpt::EncodeLaunch *p) {
    p->slots = v->d_slots; p->slot_ids = v->d_ids; p->slots4 = v->d_slots4; p->pair16 = v->d_pair16;
    p->n_slots = v->stats.n_slots; p->root_base = v->root_base;
    p->ws_node = v->ws_node; p->ws_base = v->ws_base; p->ws_id = v->ws_id;
}

// A host table as a fresh device buffer (an empty table: none, *d stays null).
template <typename D, typename T>
hipError_t upload(D **d, const std::vector<T> &h) {
    if (h.empty()) return hipSuccess;
    const hipError_t e = hipMalloc((void **)d, h.size() * sizeof(T));
    return e != hipSuccess ? e : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// dpt_vocab_destroy, and dpt_vocab_create's exit after a failed upload
void vocab_free(dpt_vocab *v) {
    DeviceGuard g(v->device);
    for (void *p : {(void *)v->d_slots, (void *)v->d_ids, (void *)v->d_slots4, (void *)v->d_pair16, (void *)v->d_tok_len})
        (void)hipFree(p);
    delete v;
}

}  // namespace

namespace dpt {
void set_last_error(const std::string &msg) { g_err = msg; }   // (dpt_rccl.cpp, dpt_vocab.cpp)
}

extern "C" {

const char *dpt_last_error(void) { return g_err.c_str(); }

int dpt_abi_version(void) { return DPT_ABI_VERSION; }

int dpt_vocab_create(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok,
                     int device, dpt_vocab **out) {
    if (!out || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0])) return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DPT_E_NODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(DPT_E_ARG, "bad device index");
    for (uint32_t t = 0; t < n_tok; t++)
        if (tok_off[t + 1] < tok_off[t]) return fail(DPT_E_ARG, "tok_off not monotone");
    // every table, on the host; then the upload
    dpt::VocabTables t;
    if (const char *err = dpt::build_vocab_tables(utf8_blob, tok_off, ids, n_tok, &t)) return fail(DPT_E_VOCAB, err);
    DeviceGuard g(device);
    hipError_t e = dpt::kernel_init();
    if (e != hipSuccess) return hip_fail(e, "kernel_init");
    dpt_vocab *v = new (std::nothrow) dpt_vocab();
    if (!v) return fail(DPT_E_ARG, "out of host memory");
    static_cast<dpt::VocabScalars &>(*v) = t;
    v->device = device;
    e = upload(&v->d_slots, t.slots);
    if (e == hipSuccess) e = upload(&v->d_slots4, t.slots4);
    if (e == hipSuccess) e = upload(&v->d_ids, t.slot_ids);
    if (e == hipSuccess) e = upload(&v->d_pair16, t.pair);
    if (e == hipSuccess) e = upload(&v->d_tok_len, t.tok_len);
    if (e != hipSuccess) {
        vocab_free(v);
        return hip_fail(e, "vocab upload");
    }
    *out = v;
    return DPT_OK;
}

int dpt_vocab_destroy(dpt_vocab *v) {
    if (v) vocab_free(v);
    return DPT_OK;
}

int dpt_vocab_stats_get(const dpt_vocab *v, dpt_vocab_stats *out) {
    if (!v || !out) return fail(DPT_E_ARG, "null argument");
    *out = v->stats;
    return DPT_OK;
}

int dpt_ctx_create(int device, dpt_ctx **out) {
    if (!out) return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DPT_E_NODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(DPT_E_ARG, "bad device index");
    dpt_ctx *c = new (std::nothrow) dpt_ctx();
    if (!c) return fail(DPT_E_ARG, "out of host memory");
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->max_blocks = (unsigned)prop.multiProcessorCount * 64u;
    if (c->max_blocks == 0) c->max_blocks = 256u * 64u;
    *out = c;
    return DPT_OK;
}

int dpt_ctx_destroy(dpt_ctx *c) {
    if (!c) return DPT_OK;
    DeviceGuard g(c->device);
    void *ps[] = {c->staging32, c->staging16, c->arena, c->counts, c->retry_list, c->ctr, c->wsl_scratch,
                  c->pend, c->flags, c->d_in, c->d_out};
    for (void *p : ps)
        if (p) (void)hipFree(p);
    if (c->p_in) (void)hipHostFree(c->p_in);
    if (c->p_out) (void)hipHostFree(c->p_out);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    delete c;
    return DPT_OK;
}

int dpt_ctx_reserve(dpt_ctx *c, uint64_t n_bytes, uint64_t n_str) {
    return dpt_ctx_reserve_vocab(c, nullptr, n_bytes, n_str, 0);
}

int dpt_ctx_reserve_vocab(dpt_ctx *c, const dpt_vocab *v, uint64_t n_bytes, uint64_t n_str, uint64_t long_bytes) {
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if (v && v->device != c->device) return fail(DPT_E_ARG, "ctx and vocab on different devices");
    DeviceGuard g(c->device);
    const int rc = ensure_workspace(c, v, n_bytes, n_str, long_bytes);
    if (rc == DPT_OK && long_bytes) c->arena_reserved = true;
    return rc;
}

int dpt_ctx_workspace_bytes(const dpt_ctx *c, uint64_t *device_path, uint64_t *host_path) {
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if (device_path)
        *device_path = c->cap16 * 2 + c->cap32 * 4 + c->arena_cap * ARENA_PER_BYTE + c->cap_str * (8 + dpt::N_RETRY_LISTS * 4) +
                       flag_words(c->cap_batches) * 8 + (c->wsl_scratch ? dpt::wsl_scratch_bytes(c->max_blocks) : 0) +
                       (c->pend ? dpt::pend_scratch_bytes(c->max_blocks) : 0) +
                       (c->ctr ? dpt::CTR_ALLOC_BYTES : 0);
    if (host_path) *host_path = c->cap_in + c->cap_out;
    return DPT_OK;
}

int dpt_ctx_long_need(dpt_ctx *c, uint64_t *need, uint64_t *cap) {
    if (!c || !need) return fail(DPT_E_ARG, "null argument");
    *need = 0;
    if (cap) *cap = c->arena_cap;
    if (!c->ctr) return DPT_OK;
    DeviceGuard g(c->device);
    hipError_t e = hipMemcpy(need, &c->ctr->last_need, sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "D2H arena counter");
    *need = *need >= c->counter_bias ? *need - c->counter_bias : 0;   // (0 after an empty call)
    return DPT_OK;
}

int dpt_ctx_debug_counter_bias(dpt_ctx *c, uint64_t bias) {
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if (bias >= (1ull << 62)) return fail(DPT_E_ARG, "counter bias too large");
    c->counter_bias = bias;
    return DPT_OK;
}

static int encode_impl(dpt_ctx *c, const dpt_vocab *v, const EncodeRequest &r) {
    const int mode = r.mode_flags & DPT_MODE_MASK;
    const uint64_t n_bytes = r.n_bytes, n_str = r.n_str;
    if (!c || !v) return fail(DPT_E_ARG, "null ctx or vocab");
    // the armed histogram is this call's whatever happens below (one call only, failed ones included)
    int64_t *hist = r.dev_call ? c->hist : nullptr;
    const uint32_t hist_bins = c->hist_bins;
    const bool hist_overwrite = c->hist_overwrite;
    if (r.dev_call) { c->hist = nullptr; c->hist_overwrite = false; }
    if (mode != DPT_MODE_RAW && mode != DPT_MODE_PRESPLIT && mode != DPT_MODE_ATOMS) return fail(DPT_E_ARG, "bad mode");
    if (r.mode_flags & ~(DPT_MODE_MASK | DPT_FLAG_UNCAPPED | DPT_FLAG_LEN_ONLY)) return fail(DPT_E_ARG, "bad flags");
    const bool padded = r.padded_counts != nullptr;
    if (!r.str_off || (!r.id_off && !padded) || (n_str && !r.status)) return fail(DPT_E_ARG, "null output/offsets");
    if (n_bytes && (!r.text || !r.ids)) return fail(DPT_E_ARG, "null text/ids");
    if (mode != DPT_MODE_RAW && n_bytes && !r.cut_mask) return fail(DPT_E_ARG, "PRESPLIT/ATOMS need cut_mask");
    if (r.ids_cap < n_bytes) return fail(DPT_E_CAP, "ids_cap must be >= n_bytes");
    if (n_str > 0x7FFFFFFFull) return fail(DPT_E_ARG, "too many strings for one call (max 2^31-1)");
    if (c->device != v->device) return fail(DPT_E_ARG, "ctx and vocab on different devices");
    DeviceGuard g(c->device);
    if (const int rc = ensure_workspace(c, v, n_bytes, n_str, 0, !padded)) return rc;
    const hipStream_t st = r.stream;
    dpt::EncodeLaunch p;
    // the caller's view
    p.mode = r.mode_flags; p.text = r.text; p.str_off = r.str_off; p.cut_mask = r.cut_mask; p.n_str = n_str; p.n_bytes = n_bytes;
    p.ids = r.ids; p.id_off = r.id_off; p.status = r.status; p.capped = r.capped_len;
    p.edges = r.edges; p.far = r.edges ? r.far : nullptr; p.far_cap = r.far_cap;
    p.ctr_snap = r.ctr_snap; p.no_fallback = r.no_fallback; p.padded = padded;
    p.hist = hist; p.hist_bins = hist_bins; p.hist_overwrite = hist_overwrite;
    // the workspace; int16 staging when every id fits in 0..32767 (half the staging traffic)
    p.staging = c->staging32; p.staging16 = v->ids16 ? c->staging16 : nullptr; p.counts = c->counts;
    p.retry_list = c->retry_list; p.ctr = c->ctr; p.wsl_scratch = c->wsl_scratch; p.pend = c->pend;
    p.max_blocks = c->max_blocks; p.arena = c->arena; p.arena_cap = c->arena_cap; p.counter_bias = c->counter_bias;
    flag_regions(c->flags, c->cap_batches, c->flag_parity, &p);
    // padded: the ids go straight to their final place (int32), the counts to the caller's array
    if (padded) { p.staging = r.ids; p.staging16 = nullptr; p.counts = r.padded_counts; }
    // the vocabulary
    launch_vocab(v, &p);
    p.long_span = v->stats.max_cp > 64 ? 1 : 0;
    p.max_tok_bytes = v->stats.max_bytes;
    p.variant = kernel_variant(v->stats.max_cp);
    // (a per-string dp_tokenize call: one launch instead of two -- the finish kernel was 5 us of its 43)
    p.solo = !dpt::launch_knobs().no_solo && r.no_fallback && n_str == 1 && !padded && !r.edges && !hist && !c->profile && r.ctr_snap;
    if (c->counter_bias && n_str) {
        // test-only: the arena and far-pair counters start this call at the bias (the previous call's reset
        // left them 0), so the kernels' offsets have a low word >= 2^31 without a 40-GiB arena; the far
        // list is passed down shifted by as many pairs
        const uint64_t b = c->counter_bias;
        for (uint64_t *w : {&c->ctr->arena_used, &c->ctr->far_pairs}) {
            uint32_t *const lo = reinterpret_cast<uint32_t *>(w);
            hipError_t e0 = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lo), (int)(uint32_t)b, 1, st);
            if (e0 == hipSuccess) e0 = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lo + 1), (int)(uint32_t)(b >> 32), 1, st);
            if (e0 != hipSuccess) return hip_fail(e0, "counter bias");
        }
        if (p.far) {
            p.far = reinterpret_cast<uint64_t *>(reinterpret_cast<uintptr_t>(p.far) - 16 * b);
            p.far_cap = r.far_cap + b;
        }
    }
    hipEvent_t ev[2], *evp = nullptr;
    if (c->profile) {
        for (int k = 0; k < 2; k++) {
            hipError_t e = hipEventCreate(&ev[k]);
            if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
            c->events.push_back(ev[k]);
        }
        evp = ev;
        c->launches++;
    }
    hipError_t e = dpt::launch_encode(p, st, evp);
    if (e != hipSuccess) {
        (void)hipMemsetAsync(c->ctr, 0, dpt::CTR_ALLOC_BYTES, st);   // the scan kernel did not reset them
        (void)hipMemsetAsync(c->flags, 0, flag_words(c->cap_batches) * sizeof(unsigned long long), st);   // nor zero the batch lines
        c->flag_parity = 0;
        return hip_fail(e, "encode launch");
    }
    if (!padded && dpt::fin_fold(n_str)) c->flag_parity ^= 1;   // the finish pass zeroed the other region
    return DPT_OK;
}

int dpt_encode(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
               const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap,
               uint64_t *id_off, int32_t *status, int32_t *capped_len, void *hip_stream) {
    if (mode & ~DPT_MODE_MASK) return fail(DPT_E_ARG, "flags are for dpt_dp_host");
    EncodeRequest r;
    r.mode_flags = mode; r.text = text; r.n_bytes = n_bytes; r.str_off = str_off; r.cut_mask = cut_mask; r.n_str = n_str;
    r.ids = ids; r.ids_cap = ids_cap; r.id_off = id_off; r.status = status; r.capped_len = capped_len;
    r.stream = (hipStream_t)hip_stream; r.dev_call = true;
    return encode_impl(c, v, r);
}

int dpt_encode_padded(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                      const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap,
                      uint64_t *counts, int32_t *status, int32_t *capped_len, void *hip_stream) {
    if (mode & ~DPT_MODE_MASK) return fail(DPT_E_ARG, "flags are for dpt_dp_host");
    if (!counts) return fail(DPT_E_ARG, "null counts");
    EncodeRequest r;
    r.mode_flags = mode; r.text = text; r.n_bytes = n_bytes; r.str_off = str_off; r.cut_mask = cut_mask; r.n_str = n_str;
    r.ids = ids; r.ids_cap = ids_cap; r.padded_counts = counts; r.status = status; r.capped_len = capped_len;
    r.stream = (hipStream_t)hip_stream;
    return encode_impl(c, v, r);
}

// Host path calls up to this many input bytes check whether any string needs the fallback passes.
constexpr uint64_t NO_FALLBACK_CHECK_BYTES = 16384;

// True when no string of a RAW / PRESPLIT call can leave the first pass (dpt_kernels.hip tokenize_kernel):
// every word fits its window of dpt::SMALL_CH bytes (consecutive word starts -- byte 0, then ' ' in RAW mode
// or a cut byte on a non-continuation byte in PRESPLIT mode -- at most that far apart, the last one at most
// that far before the string's end) and every atom (a code point: a byte and its continuation bytes) has at
// most 4 bytes.  (Vocabularies with tokens of more than 64 code points are not checked: the caller.)
static bool no_fallback_needed(int mode, const uint8_t *text, const uint64_t *str_off, const uint8_t *cut,
                               uint64_t n_str) {
    if (mode != DPT_MODE_RAW && mode != DPT_MODE_PRESPLIT) return false;
    const uint64_t base = str_off[0];
    for (uint64_t i = 0; i < n_str; i++) {
        const uint64_t a = str_off[i] - base, b = str_off[i + 1] - base;
        uint64_t ws = a;        // the current word's start
        unsigned cont = 0;      // continuation bytes after the current atom's first byte
        for (uint64_t k = a; k < b; k++) {
            const uint8_t x = text[k];
            const bool is_cont = k > a && (x & 0xC0) == 0x80;   // (the string's first byte starts an atom)
            cont = is_cont ? cont + 1 : 0;
            if (cont > 3) return false;   // an atom of over 4 bytes
            const bool wstart = k > a && (mode == DPT_MODE_RAW ? x == ' ' : (cut[k] != 0 && !is_cont));
            if (wstart) {
                if (k - ws > dpt::SMALL_CH) return false;
                ws = k;
            }
        }
        if (b - ws > dpt::SMALL_CH) return false;
    }
    return true;
}

// One call through the staging buffers.  *overflow: the unbounded pass's arena was too small for some
// strings (status 3) and has been grown since: they alone run again (rerun_too_long).
static int encode_host_impl(dpt_ctx *c, const dpt_vocab *v, const HostRequest &r, bool *overflow) {
    const uint64_t n_bytes = r.n_bytes, n_str = r.n_str;
    *overflow = false;
    // host arguments first (checkable without a device)
    if (!r.str_off || !r.id_off || (n_str && !r.status)) return fail(DPT_E_ARG, "null output/offsets");
    if (n_bytes && (!r.text || !r.ids)) return fail(DPT_E_ARG, "null text/ids");
    if (r.ids_cap < n_bytes) return fail(DPT_E_CAP, "ids_cap must be >= n_bytes");
    int rc;
    hipError_t e;
    if ((rc = check_str_off(r.str_off, n_str, n_bytes))) return rc;
    if (!c || !v) return fail(DPT_E_ARG, "null ctx or vocab");
    DeviceGuard g(c->device);
    const bool cut = (r.mode_flags & DPT_MODE_MASK) != DPT_MODE_RAW && n_bytes;
    if (cut && !r.cut_mask) return fail(DPT_E_ARG, "PRESPLIT/ATOMS need cut_mask");
    const bool want_far = r.edges && r.far;
    const EncodeLayout L(n_bytes, n_str, r.edges != nullptr, want_far ? r.far_cap : 0);
    if ((rc = stage_host(c, L.in_bytes, L.out_bytes))) return rc;
    if (n_bytes) memcpy(c->p_in, r.text, n_bytes);
    uint64_t *off = at<uint64_t>(c->p_in, L.in_off);
    for (uint64_t i = 0; i <= n_str; i++) off[i] = r.str_off[i] - r.str_off[0];
    if (cut) memcpy(c->p_in + L.in_cut, r.cut_mask, n_bytes);
    const hipStream_t st = 0;
    const uint64_t *p_idoff = at<const uint64_t>(c->p_out, 0);
    const dpt::CounterBlock *p_ctr = at<const dpt::CounterBlock>(c->p_out, L.ctr);   // the call's counters (their reset's snapshot)
    // small batches: everything in one copy (ids up to the n_bytes bound); large: the head, then the ids.
    // The counter block's first 64 bytes ride in d_out's counter slot (the finish pass's reset copies
    // them there), so one copy brings them back.
    const bool one_copy = 4 * n_bytes <= (4ull << 20);
    // Small calls skip the 2048-byte and unbounded passes' dispatches when no string can need them
    // (no_fallback_needed): a per-string dp_tokenize call's launch chain loses two of its four kernels.
    const bool no_fb = n_bytes <= NO_FALLBACK_CHECK_BYTES && !r.edges && v->stats.max_cp <= 64 &&
                       no_fallback_needed(r.mode_flags & DPT_MODE_MASK, r.text, r.str_off, cut ? r.cut_mask : nullptr, n_str);
    // the call on one pair of buffers, as the device addresses them
    auto request = [&](uint8_t *in, uint8_t *out) {
        EncodeRequest q;
        q.mode_flags = r.mode_flags; q.n_bytes = n_bytes; q.n_str = n_str; q.ids_cap = n_bytes ? n_bytes : 1;
        q.text = in; q.str_off = at<const uint64_t>(in, L.in_off); q.cut_mask = cut ? in + L.in_cut : nullptr;
        q.id_off = at<uint64_t>(out, 0); q.status = at<int32_t>(out, L.st); q.capped_len = at<int32_t>(out, L.capped);
        q.ctr_snap = at<uint64_t>(out, L.ctr); q.ids = at<int32_t>(out, L.ids);
        q.stream = st;
        q.no_fallback = no_fb;
        return q;
    };
    // One string with no fallback pass (a per-string dp_tokenize call): zero-copy -- its lone wave
    // (EncodeLaunch::solo) reads the text from and writes the outputs to the pinned host buffers, so the
    // call is one launch and a sync (two copies and their gaps less)
    if (no_fb && n_str == 1 && !r.edges && !c->profile && !dpt::launch_knobs().no_solo) {
        if (!c->pd_in && (e = hipHostGetDevicePointer((void **)&c->pd_in, c->p_in, 0)) != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer");
        if (!c->pd_out && (e = hipHostGetDevicePointer((void **)&c->pd_out, c->p_out, 0)) != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer");
        if ((rc = encode_impl(c, v, request(c->pd_in, c->pd_out)))) return rc;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
        const uint64_t total = p_idoff[1];
        if (total > r.ids_cap || total > n_bytes) return fail(DPT_E_CAP, "ids overflow");
        r.id_off[0] = 0; r.id_off[1] = total;
        r.status[0] = *at<const int32_t>(c->p_out, L.st);
        if (r.capped_len) r.capped_len[0] = *at<const int32_t>(c->p_out, L.capped);
        if (total) memcpy(r.ids, c->p_out + L.ids, 4 * total);
        return DPT_OK;
    }
    EncodeRequest q = request(c->d_in, c->d_out);
    q.edges = r.edges ? at<uint64_t>(c->d_out, L.edges) : nullptr;
    q.far = want_far ? at<uint64_t>(c->d_out, L.far) : nullptr;
    q.far_cap = r.far_cap;
    if ((e = hipMemcpyAsync(c->d_in, c->p_in, L.in_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e, "H2D");
    for (int attempt = 0;; attempt++) {
        if ((rc = encode_impl(c, v, q))) return rc;
        if ((e = hipMemcpyAsync(c->p_out, c->d_out, one_copy ? L.out_bytes : L.ids, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(e, "D2H");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
        // the call's claimed bytes (finish_kernel), less the test-only dpt_ctx_debug_counter_bias
        const uint64_t used = n_str ? p_ctr->last_need - c->counter_bias : 0;
        if (used > n_bytes) return fail(DPT_E_HIP, "unbounded pass counter out of range");   // never expected
        if (used <= c->arena_cap) break;
        // the unbounded pass's arena was too small for the strings routed to it (those strings got
        // status 3): grow it to what the pass claimed and run the call again
        if (attempt > 0 || r.depth > 0) return fail(DPT_E_ARG, "unbounded pass arena overflow after growth");
        if ((rc = ensure_workspace(c, v, n_bytes, n_str, used))) return rc;
        // without edge outputs only the strings the arena could not hold run again (a sub-batch,
        // spliced in by the caller); edge-recording calls (one string each from the drop-ins) rerun whole
        if (!r.edges) {
            *overflow = true;
            break;
        }
    }
    const uint64_t total = p_idoff[n_str];
    if (total > r.ids_cap) return fail(DPT_E_CAP, "ids overflow");
    uint64_t nf = 0;
    if (want_far) {
        nf = n_str ? p_ctr->last_far - c->counter_bias : 0;   // the call's far edge pairs (finish_kernel)
        if (r.n_far) *r.n_far = nf;
        if (nf > r.far_cap) return fail(DPT_E_CAP, "far edge list overflow (*n_far holds the pairs needed)");
    }
    if (!one_copy) {
        if (total && (e = hipMemcpyAsync(c->p_out + L.ids, q.ids, 4 * total, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(e, "D2H ids");
        if (r.edges && n_bytes &&
            (e = hipMemcpyAsync(c->p_out + L.edges, q.edges, 8 * n_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(e, "D2H edges");
        if (nf && (e = hipMemcpyAsync(c->p_out + L.far, q.far, 16 * nf, hipMemcpyDeviceToHost, st)) != hipSuccess)
            return hip_fail(e, "D2H far edges");
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
    }
    memcpy(r.id_off, c->p_out, 8 * (n_str + 1));
    if (n_str) memcpy(r.status, c->p_out + L.st, 4 * n_str);
    if (r.capped_len && n_str) memcpy(r.capped_len, c->p_out + L.capped, 4 * n_str);
    if (total) memcpy(r.ids, c->p_out + L.ids, 4 * total);
    if (r.edges && n_bytes) memcpy(r.edges, c->p_out + L.edges, 8 * n_bytes);
    if (nf) memcpy(r.far, c->p_out + L.far, 16 * nf);
    return DPT_OK;
}

// After an arena overflow (the arena has since grown to what the pass claimed): the strings with
// status DPT_STATUS_TOO_LONG -- exactly those the unbounded pass could not hold -- as one sub-batch,
// their results spliced into the caller's CSR arrays.
static int rerun_too_long(dpt_ctx *c, const dpt_vocab *v, const HostRequest &r) {
    const uint64_t n_str = r.n_str;
    std::vector<uint64_t> sel;
    for (uint64_t i = 0; i < n_str; i++)
        if (r.status[i] == DPT_STATUS_TOO_LONG) sel.push_back(i);
    if (sel.empty()) return DPT_OK;
    const uint64_t k = sel.size();
    std::vector<uint64_t> soff(k + 1, 0);
    for (uint64_t q = 0; q < k; q++) soff[q + 1] = soff[q] + (r.str_off[sel[q] + 1] - r.str_off[sel[q]]);
    const uint64_t sb = soff[k];
    const bool cut = (r.mode_flags & DPT_MODE_MASK) != DPT_MODE_RAW;
    std::vector<uint8_t> stext(sb ? sb : 1), scut(cut && sb ? sb : 1);
    for (uint64_t q = 0; q < k; q++) {
        const uint64_t a = r.str_off[sel[q]] - r.str_off[0], n = soff[q + 1] - soff[q];
        if (n) memcpy(stext.data() + soff[q], r.text + a, n);
        if (cut && n) memcpy(scut.data() + soff[q], r.cut_mask + a, n);
    }
    std::vector<int32_t> sids(sb ? sb : 1), sst(k), scap(k);
    std::vector<uint64_t> sidoff(k + 1);
    HostRequest s;
    s.mode_flags = r.mode_flags; s.text = stext.data(); s.n_bytes = sb; s.str_off = soff.data(); s.cut_mask = cut ? scut.data() : nullptr;
    s.n_str = k; s.ids = sids.data(); s.ids_cap = sb ? sb : 1; s.id_off = sidoff.data(); s.status = sst.data();
    s.capped_len = r.capped_len ? scap.data() : nullptr;
    s.depth = 1;
    bool again;   // (never set: a rerun that overflows fails)
    const int rc = encode_host_impl(c, v, s, &again);
    if (rc) return rc;
    // splice: the overflowed strings had no ids; rebuild the CSR arrays around their new ones
    const uint64_t total = r.id_off[n_str] + sidoff[k];
    if (total > r.ids_cap) return fail(DPT_E_CAP, "ids overflow");
    std::vector<int32_t> old(r.ids, r.ids + r.id_off[n_str]);
    std::vector<uint64_t> old_off(r.id_off, r.id_off + n_str + 1);
    uint64_t o = 0, q = 0;
    for (uint64_t i = 0; i < n_str; i++) {
        r.id_off[i] = o;
        if (q < k && sel[q] == i) {
            const uint64_t n = sidoff[q + 1] - sidoff[q];
            if (n) memcpy(r.ids + o, sids.data() + sidoff[q], 4 * n);
            o += n;
            r.status[i] = sst[q];
            if (r.capped_len) r.capped_len[i] = scap[q];
            q++;
        } else {
            const uint64_t n = old_off[i + 1] - old_off[i];
            if (n) memcpy(r.ids + o, old.data() + old_off[i], 4 * n);
            o += n;
        }
    }
    r.id_off[n_str] = o;
    return DPT_OK;
}

static int encode_host(dpt_ctx *c, const dpt_vocab *v, const HostRequest &r) {
    bool overflow;
    const int rc = encode_host_impl(c, v, r, &overflow);
    return rc || !overflow ? rc : rerun_too_long(c, v, r);
}

int dpt_encode_host(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                    const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap,
                    uint64_t *id_off, int32_t *status, int32_t *capped_len) {
    if (mode & ~DPT_MODE_MASK) return fail(DPT_E_ARG, "flags are for dpt_dp_host");
    HostRequest r;
    r.mode_flags = mode; r.text = text; r.n_bytes = n_bytes; r.str_off = str_off; r.cut_mask = cut_mask; r.n_str = n_str;
    r.ids = ids; r.ids_cap = ids_cap; r.id_off = id_off; r.status = status; r.capped_len = capped_len;
    return encode_host(c, v, r);
}

// dpt_dp_host*'s common part: r holds the caller's arguments, the lengths (nullable) as capped_len.  No ids.
static int dp_host(dpt_ctx *c, const dpt_vocab *v, HostRequest r) {
    if (!(r.mode_flags & (DPT_FLAG_UNCAPPED | DPT_FLAG_LEN_ONLY))) r.mode_flags |= DPT_FLAG_LEN_ONLY;
    std::vector<uint64_t> id_off(r.n_str + 1);
    std::vector<int32_t> len_tmp(r.capped_len ? 0 : r.n_str + 1);
    int32_t dummy_ids[1];
    r.ids = dummy_ids; r.ids_cap = r.n_bytes ? r.n_bytes : 1; r.id_off = id_off.data();
    if (!r.capped_len) r.capped_len = len_tmp.data();
    return encode_host(c, v, r);
}

int dpt_dp_host(dpt_ctx *c, const dpt_vocab *v, int mode_flags, const uint8_t *text, uint64_t n_bytes,
                const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *status, int32_t *lengths,
                uint64_t *edges) {
    if (!lengths && !edges) return fail(DPT_E_ARG, "nothing to compute");
    HostRequest r;
    r.mode_flags = mode_flags; r.text = text; r.n_bytes = n_bytes; r.str_off = str_off; r.cut_mask = cut_mask; r.n_str = n_str;
    r.status = status; r.capped_len = lengths; r.edges = edges;
    return dp_host(c, v, r);
}

int dpt_dp_host_far(dpt_ctx *c, const dpt_vocab *v, int mode_flags, const uint8_t *text, uint64_t n_bytes,
                    const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *status, int32_t *lengths,
                    uint64_t *edges, uint64_t *far, uint64_t far_cap, uint64_t *n_far) {
    if (!edges || !n_far || (far_cap && !far)) return fail(DPT_E_ARG, "dpt_dp_host_far needs edges, far and n_far");
    *n_far = 0;
    uint64_t dummy_far[2];
    HostRequest r;
    r.mode_flags = mode_flags; r.text = text; r.n_bytes = n_bytes; r.str_off = str_off; r.cut_mask = cut_mask; r.n_str = n_str;
    r.status = status; r.capped_len = lengths; r.edges = edges;
    r.far = far ? far : dummy_far; r.far_cap = far_cap; r.n_far = n_far;
    return dp_host(c, v, r);
}

// Argument checks shared by the two spans entry points (no device is touched, v is not dereferenced
// before every pointer has been checked).
static int spans_check(const dpt::SpansLaunch &p, const dpt_vocab *v, uint64_t n_bytes) {
    if (!v) return fail(DPT_E_ARG, "null vocab");
    const struct { const void *ptr; const char *err; } need[] = {{p.str_off, "null str_off"}, {p.ids, "null ids"}, {p.id_off, "null id_off"},
        {p.status, "null status"}, {p.tok_end, "null tok_end"}, {p.span_status, "null span_status"}};
    for (const auto &n : need)
        if (!n.ptr) return fail(DPT_E_ARG, n.err);
    if (p.mode != DPT_MODE_RAW && p.mode != DPT_MODE_PRESPLIT && p.mode != DPT_MODE_ATOMS) return fail(DPT_E_ARG, "bad mode");
    if (p.mode != DPT_MODE_RAW && !p.cut_mask) return fail(DPT_E_ARG, "PRESPLIT/ATOMS need cut_mask");
    if (n_bytes && !p.text) return fail(DPT_E_ARG, "null text");
    return DPT_OK;
}

static const char *const NO_TOK_LEN = "vocabulary has no dense per-id token lengths (sparse ids, or one id on tokens of different length)";

int dpt_token_spans(const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes, const uint64_t *str_off,
                    const uint8_t *cut_mask, uint64_t n_str, const int32_t *ids, const uint64_t *id_off,
                    const int32_t *status, uint32_t *tok_end, uint32_t *tok_word, int32_t *span_status, void *hip_stream) {
    dpt::SpansLaunch p;
    p.mode = mode; p.text = text; p.str_off = str_off; p.cut_mask = cut_mask; p.n_str = n_str;
    p.ids = ids; p.id_off = id_off; p.status = status; p.tok_end = tok_end; p.tok_word = tok_word; p.span_status = span_status;
    if (const int rc = spans_check(p, v, n_bytes)) return rc;
    if (!v->d_tok_len) return fail(DPT_E_VOCAB, NO_TOK_LEN);
    p.tok_len = v->d_tok_len; p.id_min = v->id_min; p.n_tab = v->n_tab;
    DeviceGuard g(v->device);
    const hipError_t e = dpt::launch_spans(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "spans launch");
    return DPT_OK;
}

int dpt_token_spans_host(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                         const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, const int32_t *ids,
                         const uint64_t *id_off, const int32_t *status, uint32_t *tok_end, uint32_t *tok_word,
                         int32_t *span_status) {
    // host arguments first (checkable without a device)
    dpt::SpansLaunch p;
    p.mode = mode; p.text = text; p.str_off = str_off; p.cut_mask = cut_mask; p.n_str = n_str;
    p.ids = ids; p.id_off = id_off; p.status = status; p.tok_end = tok_end; p.tok_word = tok_word; p.span_status = span_status;
    int rc = spans_check(p, v, n_bytes);
    if (rc) return rc;
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if ((rc = check_str_off(str_off, n_str, n_bytes, id_off))) return rc;
    if (c->device != v->device) return fail(DPT_E_ARG, "ctx and vocab on different devices");
    if (!v->d_tok_len) return fail(DPT_E_VOCAB, NO_TOK_LEN);
    if (n_str == 0) return DPT_OK;
    const uint64_t n_tok = id_off[n_str] - id_off[0];
    const bool cut = mode != DPT_MODE_RAW;
    DeviceGuard g(c->device);
    hipError_t e;
    const SpansLayout L(n_bytes, n_str, n_tok, cut, tok_word != nullptr);
    if ((rc = stage_host(c, L.in_bytes, L.out_bytes))) return rc;
    uint64_t *so = at<uint64_t>(c->p_in, 0), *io = at<uint64_t>(c->p_in, L.in_idoff);
    for (uint64_t i = 0; i <= n_str; i++) {
        so[i] = str_off[i] - str_off[0];
        io[i] = id_off[i] - id_off[0];
    }
    if (n_tok) memcpy(c->p_in + L.in_ids, ids, 4 * n_tok);
    memcpy(c->p_in + L.in_st, status, 4 * n_str);
    if (n_bytes) memcpy(c->p_in + L.in_text, text, n_bytes);
    if (cut && n_bytes) memcpy(c->p_in + L.in_cut, cut_mask, n_bytes);
    // the same call on the device buffers
    p.text = c->d_in + L.in_text; p.str_off = at<const uint64_t>(c->d_in, 0); p.cut_mask = cut ? c->d_in + L.in_cut : nullptr;
    p.ids = at<const int32_t>(c->d_in, L.in_ids); p.id_off = at<const uint64_t>(c->d_in, L.in_idoff);
    p.status = at<const int32_t>(c->d_in, L.in_st); p.tok_end = at<uint32_t>(c->d_out, 0);
    p.tok_word = tok_word ? at<uint32_t>(c->d_out, L.word) : nullptr; p.span_status = at<int32_t>(c->d_out, L.ss);
    p.tok_len = v->d_tok_len; p.id_min = v->id_min; p.n_tab = v->n_tab;
    const hipStream_t st = 0;
    if ((e = hipMemcpyAsync(c->d_in, c->p_in, L.in_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e, "H2D");
    if ((e = dpt::launch_spans(p, st)) != hipSuccess) return hip_fail(e, "spans launch");
    if ((e = hipMemcpyAsync(c->p_out, c->d_out, L.out_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "D2H");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
    if (n_tok) memcpy(tok_end, c->p_out, 4 * n_tok);
    if (n_tok && tok_word) memcpy(tok_word, c->p_out + L.word, 4 * n_tok);
    memcpy(span_status, c->p_out + L.ss, 4 * n_str);
    return DPT_OK;
}

int dpt_detok_create(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok, int rule,
                     const int32_t *skip_ids, uint32_t n_skip, int device, dpt_detok **out) {
    if (!out || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0]) || (n_skip && !skip_ids))
        return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    if (rule < DPT_DETOK_PIECES || rule > DPT_DETOK_BYTELEVEL) return fail(DPT_E_ARG, "no such decode rule");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DPT_E_NODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(DPT_E_ARG, "bad device index");
    for (uint32_t t = 0; t < n_tok; t++)
        if (tok_off[t + 1] < tok_off[t]) return fail(DPT_E_ARG, "tok_off not monotone");
    dpt::DetokTables t;
    if (const char *err = dpt::build_detok_tables(utf8_blob, tok_off, ids, n_tok, rule, skip_ids, n_skip, &t)) return fail(DPT_E_VOCAB, err);
    if (t.blob.empty()) t.blob.push_back(0);
    DeviceGuard g(device);
    dpt_detok *d = new (std::nothrow) dpt_detok();
    if (!d) return fail(DPT_E_ARG, "out of host memory");
    d->device = device; d->id_min = t.id_min; d->n_tab = t.n_tab;
    hipError_t e = upload(&d->d_tab, t.tab);
    if (e == hipSuccess) e = upload(&d->d_blob, t.blob);
    if (e != hipSuccess) {
        dpt_detok_destroy(d);
        return hip_fail(e, "decode table upload");
    }
    *out = d;
    return DPT_OK;
}

int dpt_detok_destroy(dpt_detok *d) {
    if (!d) return DPT_OK;
    DeviceGuard g(d->device);
    (void)hipFree(d->d_tab);
    (void)hipFree(d->d_blob);
    delete d;
    return DPT_OK;
}

// Argument checks shared by the decode entry points (no device is touched, d is not dereferenced before every
// pointer has been checked), and the table's part of a launch.
static int decode_check(dpt::DecodeLaunch *p, const dpt_detok *d, int flags) {
    if (!d) return fail(DPT_E_ARG, "null detok");
    if (!p->id_off) return fail(DPT_E_ARG, "null id_off");
    if (flags & ~DPT_DECODE_STRIP_SPACE) return fail(DPT_E_ARG, "bad decode flags");
    if (p->kind == dpt::DECODE_SIZES && !p->out_len) return fail(DPT_E_ARG, "null out_len");
    if (p->kind == dpt::DECODE_BYTES && !p->out_off) return fail(DPT_E_ARG, "null out_off");
    if (p->kind == dpt::DECODE_BYTES && !p->result) return fail(DPT_E_ARG, "null dec_status");
    if (p->kind == dpt::DECODE_ROUNDTRIP && !p->str_off) return fail(DPT_E_ARG, "null str_off");
    if (p->kind == dpt::DECODE_ROUNDTRIP && !p->result) return fail(DPT_E_ARG, "null rt");
    p->flags = flags; p->tab = d->d_tab; p->blob = d->d_blob; p->id_min = d->id_min; p->n_tab = d->n_tab;
    return DPT_OK;
}

static int decode_launch(const dpt::DecodeLaunch &p, const dpt_detok *d, void *hip_stream) {
    DeviceGuard g(d->device);
    const hipError_t e = dpt::launch_decode(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "decode launch");
    return DPT_OK;
}

int dpt_decode_sizes(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str,
                     int flags, uint64_t *out_len, void *hip_stream) {
    dpt::DecodeLaunch p{};
    p.kind = dpt::DECODE_SIZES; p.ids = ids; p.id_off = id_off; p.status = status; p.n_str = n_str; p.out_len = out_len;
    if (const int rc = decode_check(&p, d, flags)) return rc;
    return decode_launch(p, d, hip_stream);
}

int dpt_decode(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str,
               int flags, uint8_t *out, const uint64_t *out_off, int32_t *dec_status, void *hip_stream) {
    dpt::DecodeLaunch p{};
    p.kind = dpt::DECODE_BYTES; p.ids = ids; p.id_off = id_off; p.status = status; p.n_str = n_str;
    p.out = out; p.out_off = out_off; p.result = dec_status;
    if (const int rc = decode_check(&p, d, flags)) return rc;
    return decode_launch(p, d, hip_stream);
}

int dpt_roundtrip(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                  const uint8_t *text, const uint64_t *str_off, uint64_t n_str, int flags, int32_t *rt,
                  uint32_t *first_diff, void *hip_stream) {
    dpt::DecodeLaunch p{};
    p.kind = dpt::DECODE_ROUNDTRIP; p.ids = ids; p.id_off = id_off; p.status = status; p.n_str = n_str;
    p.text = text; p.str_off = str_off; p.result = rt; p.first_diff = first_diff;
    if (const int rc = decode_check(&p, d, flags)) return rc;
    return decode_launch(p, d, hip_stream);
}

// the decode host paths' offsets (nullable str_off): monotone
static int check_decode_off(const uint64_t *id_off, const uint64_t *str_off, uint64_t n_str) {
    for (uint64_t i = 0; i < n_str; i++) {
        if (id_off[i + 1] < id_off[i]) return fail(DPT_E_ARG, "id_off not monotone");
        if (str_off && str_off[i + 1] < str_off[i]) return fail(DPT_E_ARG, "str_off not monotone");
        if (str_off && str_off[i + 1] - str_off[i] >= (1ull << 32)) return fail(DPT_E_ARG, "a string of 4 GiB or more");
    }
    return DPT_OK;
}

int dpt_decode_host(dpt_ctx *c, const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                    uint64_t n_str, int flags, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *dec_status) {
    // host arguments first (checkable without a device)
    dpt::DecodeLaunch p{};
    p.kind = dpt::DECODE_BYTES; p.ids = ids; p.id_off = id_off; p.status = status; p.n_str = n_str;
    p.out = out; p.out_off = out_off; p.result = dec_status;
    int rc = decode_check(&p, d, flags);
    if (rc) return rc;
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if ((rc = check_decode_off(id_off, nullptr, n_str))) return rc;
    const uint64_t n_tok = id_off[n_str] - id_off[0];
    if ((n_tok && !ids) || (out_cap && !out)) return fail(DPT_E_ARG, "null argument");
    if (c->device != d->device) return fail(DPT_E_ARG, "ctx and detok on different devices");
    out_off[0] = 0;
    if (n_str == 0) return DPT_OK;
    DeviceGuard g(c->device);
    hipError_t e;
    const DecodeLayout L(n_str, n_tok);
    if ((rc = stage_host(c, L.in_bytes, L.len_bytes))) return rc;
    uint64_t *io = at<uint64_t>(c->p_in, 0);
    for (uint64_t i = 0; i <= n_str; i++) io[i] = id_off[i] - id_off[0];
    if (n_tok) memcpy(c->p_in + L.in_ids, ids, 4 * n_tok);
    if (status) memcpy(c->p_in + L.in_st, status, 4 * n_str);
    // the sizes, then their prefix sum on the host
    p.kind = dpt::DECODE_SIZES;
    p.ids = at<const int32_t>(c->d_in, L.in_ids); p.id_off = at<const uint64_t>(c->d_in, 0);
    p.status = status ? at<const int32_t>(c->d_in, L.in_st) : nullptr; p.out_len = at<uint64_t>(c->d_out, 0);
    const hipStream_t st = 0;
    if ((e = hipMemcpyAsync(c->d_in, c->p_in, L.in_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e, "H2D");
    if ((e = dpt::launch_decode(p, st)) != hipSuccess) return hip_fail(e, "decode sizes launch");
    if ((e = hipMemcpyAsync(c->p_out, c->d_out, L.len_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "D2H");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
    const uint64_t *len = at<const uint64_t>(c->p_out, 0);
    for (uint64_t i = 0; i < n_str; i++) out_off[i + 1] = out_off[i] + len[i];
    const uint64_t decoded = out_off[n_str];
    if (decoded > out_cap) return fail(DPT_E_CAP, "decoded bytes do not fit out_cap (the need is out_off[n_str])");
    // the bytes (the in buffer keeps its size, so it stays where it is; the out buffer may move)
    if ((rc = stage_host(c, L.in_bytes, L.bytes + al8(decoded + 1)))) return rc;
    uint64_t *oo = at<uint64_t>(c->p_in, L.in_outoff);
    memcpy(oo, out_off, 8 * (n_str + 1));
    p.kind = dpt::DECODE_BYTES;
    p.out = c->d_out + L.bytes; p.out_off = at<const uint64_t>(c->d_in, L.in_outoff); p.result = at<int32_t>(c->d_out, 0);
    if ((e = hipMemcpyAsync(c->d_in + L.in_outoff, oo, 8 * (n_str + 1), hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e, "H2D");
    if ((e = dpt::launch_decode(p, st)) != hipSuccess) return hip_fail(e, "decode launch");
    if ((e = hipMemcpyAsync(c->p_out, c->d_out, L.bytes + decoded, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "D2H");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
    memcpy(dec_status, c->p_out, 4 * n_str);
    if (decoded) memcpy(out, c->p_out + L.bytes, decoded);
    return DPT_OK;
}

int dpt_roundtrip_host(dpt_ctx *c, const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                       const uint8_t *text, const uint64_t *str_off, uint64_t n_str, int flags, int32_t *rt,
                       uint32_t *first_diff) {
    dpt::DecodeLaunch p{};
    p.kind = dpt::DECODE_ROUNDTRIP; p.ids = ids; p.id_off = id_off; p.status = status; p.n_str = n_str;
    p.text = text; p.str_off = str_off; p.result = rt; p.first_diff = first_diff;
    int rc = decode_check(&p, d, flags);
    if (rc) return rc;
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if ((rc = check_decode_off(id_off, str_off, n_str))) return rc;
    const uint64_t n_tok = id_off[n_str] - id_off[0], n_bytes = str_off[n_str] - str_off[0];
    if ((n_tok && !ids) || (n_bytes && !text)) return fail(DPT_E_ARG, "null argument");
    if (c->device != d->device) return fail(DPT_E_ARG, "ctx and detok on different devices");
    if (n_str == 0) return DPT_OK;
    DeviceGuard g(c->device);
    hipError_t e;
    const RoundtripLayout L(n_bytes, n_str, n_tok);
    if ((rc = stage_host(c, L.in_bytes, L.out_bytes))) return rc;
    uint64_t *io = at<uint64_t>(c->p_in, 0), *so = at<uint64_t>(c->p_in, L.in_stroff);
    for (uint64_t i = 0; i <= n_str; i++) {
        io[i] = id_off[i] - id_off[0];
        so[i] = str_off[i] - str_off[0];
    }
    if (n_tok) memcpy(c->p_in + L.in_ids, ids, 4 * n_tok);
    if (status) memcpy(c->p_in + L.in_st, status, 4 * n_str);
    if (n_bytes) memcpy(c->p_in + L.in_text, text, n_bytes);
    // the same call on the device buffers
    p.ids = at<const int32_t>(c->d_in, L.in_ids); p.id_off = at<const uint64_t>(c->d_in, 0);
    p.status = status ? at<const int32_t>(c->d_in, L.in_st) : nullptr;
    p.text = c->d_in + L.in_text; p.str_off = at<const uint64_t>(c->d_in, L.in_stroff);
    p.result = at<int32_t>(c->d_out, 0); p.first_diff = at<uint32_t>(c->d_out, L.fd);
    const hipStream_t st = 0;
    if ((e = hipMemcpyAsync(c->d_in, c->p_in, L.in_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e, "H2D");
    if ((e = dpt::launch_decode(p, st)) != hipSuccess) return hip_fail(e, "roundtrip launch");
    if ((e = hipMemcpyAsync(c->p_out, c->d_out, L.out_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "D2H");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "sync");
    memcpy(rt, c->p_out, 4 * n_str);
    if (first_diff) {   // (written only where the verdict is DPT_RT_DIFFERS, as the device call does)
        const uint32_t *fd = at<const uint32_t>(c->p_out, L.fd);
        for (uint64_t i = 0; i < n_str; i++)
            if (rt[i] == DPT_RT_DIFFERS) first_diff[i] = fd[i];
    }
    return DPT_OK;
}

int dpt_token_histogram(const uint64_t *id_off, const int32_t *status, uint64_t n_str, int64_t *hist, uint32_t n_bins,
                        void *hip_stream) {
    if (!id_off || !hist || (n_str && !status) || n_bins < 2 || n_bins > DPT_HIST_MAX_BINS)
        return fail(DPT_E_ARG, "bad histogram arguments (2 <= n_bins <= DPT_HIST_MAX_BINS)");
    hipError_t e = dpt::launch_histogram(id_off, status, n_str, hist, n_bins, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "histogram launch");
    return DPT_OK;
}

int dpt_ctx_set_histogram_ex(dpt_ctx *c, int64_t *hist, uint32_t n_bins, int flags) {
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if (hist && (n_bins < 2 || n_bins > DPT_HIST_MAX_BINS)) return fail(DPT_E_ARG, "n_bins outside 2..DPT_HIST_MAX_BINS");
    if (flags & ~DPT_HIST_OVERWRITE) return fail(DPT_E_ARG, "unknown histogram flags");
    c->hist = hist;
    c->hist_bins = hist ? n_bins : 0;
    c->hist_overwrite = hist && (flags & DPT_HIST_OVERWRITE);
    return DPT_OK;
}

int dpt_ctx_set_histogram(dpt_ctx *c, int64_t *hist, uint32_t n_bins) { return dpt_ctx_set_histogram_ex(c, hist, n_bins, 0); }

int dpt_ctx_profile(dpt_ctx *c, int enable) {
    if (!c) return fail(DPT_E_ARG, "null ctx");
    c->profile = enable != 0;
    return DPT_OK;
}

int dpt_ctx_profile_read(dpt_ctx *c, double *ms, uint64_t *launches) {
    if (!c || !ms) return fail(DPT_E_ARG, "null argument");
    DeviceGuard g(c->device);
    ms[0] = 0.0;
    ms[1] = ms[2] = -1.0;   // not timed: one event pair per call (every event record costs the stream ~6 us)
    for (size_t k = 0; k + 1 < c->events.size(); k += 2) {
        hipError_t e = hipEventSynchronize(c->events[k + 1]);
        if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
        float t = 0.f;
        e = hipEventElapsedTime(&t, c->events[k], c->events[k + 1]);
        if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
        ms[0] += t;
    }
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    c->events.clear();
    if (launches) *launches = c->launches;
    c->launches = 0;
    return DPT_OK;
}

}  // extern "C"
