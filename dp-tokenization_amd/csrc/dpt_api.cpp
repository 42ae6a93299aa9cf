// dpt_api.cpp -- the C-ABI declared in include/dpt.h, less its host-buffer calls (dpt_host.cpp).
//
// Owns: the device copy of the vocabulary (dpt_vocab: the upload of dpt_vocab.cpp's build_vocab_tables) and of
// a decode table (dpt_detok: dpt_detok.cpp's build_detok_tables),
// per-stream workspaces (dpt_ctx), argument checking, the one encode call every entry point runs (encode_impl),
// and the event-based kernel timing used by bench.py.  No C++ exception crosses the ABI.
#include <stdlib.h>
#include <string.h>

#include "dpt_objects.h"

using namespace dpt;

static uint64_t flag_words(uint64_t cap_batches) { return cap_batches * (2 * dpt::BS_LINE + 1); }
// The regions of a call of this parity (dpt_ctx::flags below): its own batch lines, the other parity's
// (which it zeroes) and the batch prefixes behind both.
static void flag_regions(unsigned long long *flags, uint64_t cap_batches, int parity, dpt::EncodeLaunch *p) {
    const uint64_t rl = cap_batches * dpt::BS_LINE;
    p->flags = flags + (parity ? rl : 0); p->zero_other = flags + (parity ? 0 : rl); p->zero_n = cap_batches;
    p->bpre = flags + 2 * rl;
}

namespace {

thread_local std::string g_err;

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

}  // namespace

// v == nullptr: both staging widths (the vocabulary is not known yet); staging = false: no staging
// (dpt_encode_padded writes the ids into the caller's buffer)
int dpt::ensure_workspace(dpt_ctx *c, const dpt_vocab *v, uint64_t n_bytes, uint64_t n_str, uint64_t long_bytes, bool staging) {
    hipError_t e;
    bool fresh = false;   // zeroed buffers were (re)allocated
    const bool need16 = staging && (!v || v->ids16), need32 = staging && (!v || !v->ids16);
    // (+8 elements: the finish pass reads staged ids as whole dwords, up to 2 elements past the last)
    if (need16 && (e = grow(&c->staging16, &c->cap16, n_bytes + 8)) != hipSuccess) return hip_fail(e, "hipMalloc(staging16)");
    if (need32 && (e = grow(&c->staging32, &c->cap32, n_bytes + 8)) != hipSuccess) return hip_fail(e, "hipMalloc(staging32)");
    // long_bytes = 0 (the encode path): the default size, unless the caller reserved the arena -- a
    // reserved arena is left alone, so a reserved call never reallocates (dpt.h)
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
        if (!c->lean_host) {   // the hint's host mirror (dpt_objects.h)
            e = hipHostMalloc((void **)&c->lean_host, 64, hipHostMallocMapped);
            if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&c->lean_host_dev, c->lean_host, 0);
            if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(lean hint)");
            c->lean_host[0] = 0;
        }
        fresh = true;
    }
    // the zero state every later call relies on must be in place before a call on any stream (a
    // non-blocking stream is not ordered after the null stream's memsets); allocations only
    if (fresh && (e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "hipDeviceSynchronize(zeroed workspace)");
    return DPT_OK;
}

namespace {

// First-pass kernel: 16-lane rows (4 strings per wave) when every token has <= 16 code points,
// else 64-lane rows.  DPT_KERNEL=rows64 forces the 64-lane kernel (tests run it on the 32k vocab).
int kernel_variant(uint32_t max_cp) {
    int v = max_cp <= 16 ? dpt::KERNEL_ROWS16 : dpt::KERNEL_ROWS64;
    if (const char *e = getenv("DPT_KERNEL"))
        if (!strcmp(e, "rows64")) v = dpt::KERNEL_ROWS64;
    return v;
}

// The vocabulary's part of an encode launch.
void launch_vocab(const dpt_vocab *v, dpt::EncodeLaunch *p) {
    p->slots = v->d_slots; p->slot_ids = v->d_ids; p->slots4 = v->d_slots4; p->pair16 = v->d_pair16;
    p->n_slots = v->stats.n_slots; p->root_base = v->root_base;
    p->ws_node = v->ws_node; p->ws_base = v->ws_base; p->ws_id = v->ws_id;
}

// dpt_vocab_destroy, and dpt_vocab_create's exit after a failed upload
void vocab_free(dpt_vocab *v) {
    DeviceGuard g(v->device);
    for (void *p : {(void *)v->d_slots, (void *)v->d_ids, (void *)v->d_slots4, (void *)v->d_pair16, (void *)v->d_tok_len})
        (void)hipFree(p);
    delete v;
}

}  // namespace

// (dpt_internal.h)  The environment is read on every call, as kernel_variant reads DPT_KERNEL.
unsigned dpt::wave_per_string_blocks(uint64_t n_str, unsigned waves) {
    const uint64_t want = (n_str + waves - 1) / waves;
    uint64_t blocks = want < (1ull << 20) ? want : (1ull << 20);
    if (const char *e = getenv("DPT_WAVE_GRID_BLOCKS")) {
        char *end = nullptr;
        const long long cap = strtoll(e, &end, 10);
        if (end != e && *end == '\0' && cap > 0 && (uint64_t)cap < blocks) blocks = (uint64_t)cap;
    }
    return (unsigned)blocks;
}

namespace dpt {
void set_last_error(const std::string &msg) { g_err = msg; }   // (dpt_rccl.cpp, dpt_vocab.cpp)

int check_device_and_table(int device, const uint64_t *tok_off, uint32_t n_tok) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DPT_E_NODEV, "no HIP device");
    if (device < 0 || device >= ndev) return fail(DPT_E_ARG, "bad device index");
    for (uint32_t t = 0; t < n_tok; t++)
        if (tok_off[t + 1] < tok_off[t]) return fail(DPT_E_ARG, "tok_off not monotone");
    return DPT_OK;
}
}

int dpt::encode_impl(dpt_ctx *c, const dpt_vocab *v, const EncodeRequest &r) {
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
    p.lean_mirror = c->lean_host_dev;
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
    // (only the calls the lean route is for count towards the retry: on a context of mixed calls the probe would else
    // fall on a call that launches no lean kernel)
    if (c->debug_no_lean)
        p.lean_skip = true;
    else if (dpt::lean_eligible(p))
        p.lean_skip = dpt::lean_plan_skip(c->lean_host ? *static_cast<volatile uint32_t *>(c->lean_host) : 0u, c->lean_skipped);
    hipError_t e = dpt::launch_encode(p, st, evp);
    if (e != hipSuccess) {
        (void)hipMemsetAsync(c->ctr, 0, dpt::CTR_ALLOC_BYTES, st);   // the scan kernel did not reset them
        if (c->lean_host) c->lean_host[0] = 0;
        (void)hipMemsetAsync(c->flags, 0, flag_words(c->cap_batches) * sizeof(unsigned long long), st);   // nor zero the batch lines
        c->flag_parity = 0;
        return hip_fail(e, "encode launch");
    }
    if (!padded && dpt::fin_fold(n_str)) c->flag_parity ^= 1;   // the finish pass zeroed the other region
    return DPT_OK;
}

SpansLaunch dpt::spans_args(const dpt_vocab *v, int mode, const uint8_t *text, const uint64_t *str_off, const uint8_t *cut_mask,
                            uint64_t n_str, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint32_t *tok_end,
                            uint32_t *tok_word, int32_t *span_status) {
    SpansLaunch p{};
    p.mode = mode; p.text = text; p.str_off = str_off; p.cut_mask = cut_mask; p.n_str = n_str;
    p.ids = ids; p.id_off = id_off; p.status = status; p.tok_end = tok_end; p.tok_word = tok_word; p.span_status = span_status;
    if (v) { p.tok_len = v->d_tok_len; p.id_min = v->id_min; p.n_tab = v->n_tab; }
    return p;
}

// Argument checks shared by the two spans entry points (no device is touched, v is not dereferenced
// before every pointer has been checked).
int dpt::spans_check(const SpansLaunch &p, const dpt_vocab *v, uint64_t n_bytes) {
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

const char *const dpt::NO_TOK_LEN = "vocabulary has no dense per-id token lengths (sparse ids, or one id on tokens of different length)";

DecodeLaunch dpt::decode_args(int kind, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str) {
    DecodeLaunch p{};
    p.kind = kind; p.ids = ids; p.id_off = id_off; p.status = status; p.n_str = n_str;
    return p;
}

// Argument checks shared by the decode entry points (no device is touched, d is not dereferenced before every
// pointer has been checked), and the table's part of a launch.
int dpt::decode_check(DecodeLaunch *p, const dpt_detok *d, int flags) {
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

// The option checks of dpt_collate and dpt_collate_pair and the launch members both have (Opts: either call's options).
// ``specials``: the flags that each put one special into a row, ``words`` their names; ``others``: the call's other flags.
// Returns 0 with *r filled, or the error.
constexpr uint32_t COLLATE_SIDES = DPT_COLLATE_PAD_LEFT | DPT_COLLATE_TRUNC_LEFT | DPT_COLLATE_I64;   // (flags of both calls)
template <class Opts>
static int collate_rows(dpt::CollateRows *r, const Opts *opts, uint32_t specials, const char *words, uint32_t others, uint64_t n_str,
                        void *input_ids, void *mask, void *labels, uint32_t *lengths) {
    const uint32_t row_len = opts->row_len, n_special = (uint32_t)__builtin_popcount(opts->flags & specials);
    if (opts->flags & ~(specials | others)) return fail(DPT_E_ARG, "unknown bits in opts->flags");
    if (row_len == 0) return fail(DPT_E_ARG, "opts->row_len is 0");
    if (row_len < n_special) return fail(DPT_E_ARG, std::string("opts->row_len holds fewer elements than the ") + words + " asked for");
    if (row_len > (1u << 31)) return fail(DPT_E_ARG, "opts->row_len over 2^31");
    if (opts->row_stride && opts->row_stride < row_len) return fail(DPT_E_ARG, "opts->row_stride under row_len");
    *r = {n_str, row_len, opts->row_stride ? opts->row_stride : row_len, opts->pad_id, opts->bos_id, opts->eos_id, opts->ignore_id,
          opts->flags, input_ids, mask, labels, lengths};
    return DPT_OK;
}

extern "C" {

const char *dpt_last_error(void) { return g_err.c_str(); }

int dpt_abi_version(void) { return DPT_ABI_VERSION; }

int dpt_vocab_create(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok,
                     int device, dpt_vocab **out) {
    if (!out || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0])) return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    if (const int rc = check_device_and_table(device, tok_off, n_tok)) return rc;
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
    if (const int rc = check_device_and_table(device, nullptr, 0)) return rc;
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
    if (c->lean_host) (void)hipHostFree(c->lean_host);
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

int dpt_ctx_debug_no_lean(dpt_ctx *c, int on) {
    if (!c) return fail(DPT_E_ARG, "null ctx");
    c->debug_no_lean = on != 0;
    return DPT_OK;
}

int dpt_ctx_debug_lean_words(dpt_ctx *c, uint32_t out[4]) {
    if (!c || !out) return fail(DPT_E_ARG, "null argument");
    for (int k = 0; k < 4; k++) out[k] = 0;
    if (!c->ctr) return DPT_OK;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(out, reinterpret_cast<const uint8_t *>(c->ctr) + dpt::PART_CTR_OFFSET + dpt::LEAN_LINE * dpt::PART_STRIDE * 4,
                      3 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    out[3] = c->lean_skipped;
    return e == hipSuccess ? DPT_OK : hip_fail(e, "lean words");
}

int dpt_debug_wave_grid(uint64_t n_str, uint32_t waves, uint32_t *blocks) {
    if (!blocks || waves == 0) return fail(DPT_E_ARG, "bad wave grid arguments");
    *blocks = dpt::wave_per_string_blocks(n_str, waves);
    return DPT_OK;
}

int dpt_encode(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
               const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap,
               uint64_t *id_off, int32_t *status, int32_t *capped_len, void *hip_stream) {
    if (mode & ~DPT_MODE_MASK) return fail(DPT_E_ARG, "flags are for dpt_dp_host");
    EncodeRequest r;
    r.set(mode, text, n_bytes, str_off, cut_mask, n_str, status, capped_len, ids, ids_cap);
    r.id_off = id_off; r.stream = (hipStream_t)hip_stream; r.dev_call = true;
    return encode_impl(c, v, r);
}

int dpt_encode_padded(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                      const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap,
                      uint64_t *counts, int32_t *status, int32_t *capped_len, void *hip_stream) {
    if (mode & ~DPT_MODE_MASK) return fail(DPT_E_ARG, "flags are for dpt_dp_host");
    if (!counts) return fail(DPT_E_ARG, "null counts");
    EncodeRequest r;
    r.set(mode, text, n_bytes, str_off, cut_mask, n_str, status, capped_len, ids, ids_cap);
    r.padded_counts = counts; r.stream = (hipStream_t)hip_stream;
    return encode_impl(c, v, r);
}

int dpt_token_spans(const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes, const uint64_t *str_off,
                    const uint8_t *cut_mask, uint64_t n_str, const int32_t *ids, const uint64_t *id_off,
                    const int32_t *status, uint32_t *tok_end, uint32_t *tok_word, int32_t *span_status, void *hip_stream) {
    const dpt::SpansLaunch p = spans_args(v, mode, text, str_off, cut_mask, n_str, ids, id_off, status, tok_end, tok_word, span_status);
    if (const int rc = spans_check(p, v, n_bytes)) return rc;
    if (!v->d_tok_len) return fail(DPT_E_VOCAB, NO_TOK_LEN);
    DeviceGuard g(v->device);
    const hipError_t e = dpt::launch_spans(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "spans launch");
    return DPT_OK;
}

int dpt_bpe_encode(const dpt_bpe *b, const dpt_vocab *v, const uint8_t *text, uint64_t n_bytes, const uint64_t *str_off,
                   const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap, uint64_t *counts, int32_t *status,
                   uint32_t *tok_word, void *hip_stream) {
    if (!b || !v) return fail(DPT_E_ARG, "null bpe / vocab");
    if (!str_off || !counts || !status) return fail(DPT_E_ARG, "null str_off / counts / status");
    if (n_bytes && (!text || !cut_mask || !ids)) return fail(DPT_E_ARG, "null text / cut_mask / ids");
    if (ids_cap < n_bytes) return fail(DPT_E_ARG, "ids_cap < n_bytes");
    if (b->device != v->device) return fail(DPT_E_ARG, "pair table and vocabulary on different devices");
    if (n_str == 0) return DPT_OK;
    dpt::BpeLaunch p{};
    p.text = text; p.str_off = str_off; p.cut_mask = cut_mask; p.n_str = n_str; p.ids = ids; p.counts = counts;
    p.status = status; p.tok_word = tok_word;
    p.entries = b->d_entries; p.header = dpt::BpeHeader{b->n_buckets, b->seed};
    p.slots4 = v->d_slots4; p.n_slots = v->stats.n_slots; p.root_base = v->root_base;
    DeviceGuard g(v->device);
    const hipError_t e = dpt::launch_bpe(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "bpe launch");
    return DPT_OK;
}

int dpt_detok_create(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok, int rule,
                     const int32_t *skip_ids, uint32_t n_skip, int device, dpt_detok **out) {
    if (!out || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0]) || (n_skip && !skip_ids))
        return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    if (rule < DPT_DETOK_PIECES || rule > DPT_DETOK_BYTELEVEL) return fail(DPT_E_ARG, "no such decode rule");
    if (const int rc = check_device_and_table(device, tok_off, n_tok)) return rc;
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

int dpt_decode_sizes(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str,
                     int flags, uint64_t *out_len, void *hip_stream) {
    dpt::DecodeLaunch p = decode_args(dpt::DECODE_SIZES, ids, id_off, status, n_str);
    p.out_len = out_len;
    if (const int rc = decode_check(&p, d, flags)) return rc;
    return decode_launch(p, d, hip_stream);
}

int dpt_decode(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str,
               int flags, uint8_t *out, const uint64_t *out_off, int32_t *dec_status, void *hip_stream) {
    dpt::DecodeLaunch p = decode_args(dpt::DECODE_BYTES, ids, id_off, status, n_str);
    p.out = out; p.out_off = out_off; p.result = dec_status;
    if (const int rc = decode_check(&p, d, flags)) return rc;
    return decode_launch(p, d, hip_stream);
}

int dpt_roundtrip(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                  const uint8_t *text, const uint64_t *str_off, uint64_t n_str, int flags, int32_t *rt,
                  uint32_t *first_diff, void *hip_stream) {
    dpt::DecodeLaunch p = decode_args(dpt::DECODE_ROUNDTRIP, ids, id_off, status, n_str);
    p.text = text; p.str_off = str_off; p.result = rt; p.first_diff = first_diff;
    if (const int rc = decode_check(&p, d, flags)) return rc;
    return decode_launch(p, d, hip_stream);
}

int dpt_token_histogram(const uint64_t *id_off, const int32_t *status, uint64_t n_str, int64_t *hist, uint32_t n_bins,
                        void *hip_stream) {
    if (!id_off || !hist || (n_str && !status) || n_bins < 2 || n_bins > DPT_HIST_MAX_BINS)
        return fail(DPT_E_ARG, "bad histogram arguments (2 <= n_bins <= DPT_HIST_MAX_BINS)");
    hipError_t e = dpt::launch_histogram(id_off, status, n_str, hist, n_bins, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "histogram launch");
    return DPT_OK;
}

int dpt_collate(const int32_t *ids, const uint64_t *off, const uint64_t *counts, const int32_t *status, uint64_t n_str,
                const dpt_collate_opts *opts, void *input_ids, void *attention_mask, void *labels, uint32_t *lengths,
                void *hip_stream) {
    if (!ids) return fail(DPT_E_ARG, "null ids");
    if (!off) return fail(DPT_E_ARG, "null off");
    if (!opts) return fail(DPT_E_ARG, "null opts");
    if (!input_ids) return fail(DPT_E_ARG, "null input_ids");
    dpt::CollateLaunch p{};
    if (const int rc = collate_rows(&p.r, opts, DPT_COLLATE_BOS | DPT_COLLATE_EOS, "BOS / EOS", COLLATE_SIDES, n_str, input_ids,
                                    attention_mask, labels, lengths))
        return rc;
    if (n_str == 0) return DPT_OK;
    p.src = {ids, off, counts, status};
    const hipError_t e = dpt::launch_collate(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "collate launch");
    return DPT_OK;
}

int dpt_collate_pair(const dpt_collate_side *a, const dpt_collate_side *b, uint64_t n_str, const dpt_collate_pair_opts *opts,
                     void *input_ids, void *attention_mask, void *labels, void *token_type_ids, uint32_t *lengths,
                     uint32_t *b_start, void *hip_stream) {
    if (!a) return fail(DPT_E_ARG, "null a");
    if (!b) return fail(DPT_E_ARG, "null b");
    if (!a->ids) return fail(DPT_E_ARG, "null a->ids");
    if (!a->off) return fail(DPT_E_ARG, "null a->off");
    if (!b->ids) return fail(DPT_E_ARG, "null b->ids");
    if (!b->off) return fail(DPT_E_ARG, "null b->off");
    if (!opts) return fail(DPT_E_ARG, "null opts");
    if (!input_ids) return fail(DPT_E_ARG, "null input_ids");
    dpt::CollatePairLaunch p{};
    if (const int rc = collate_rows(&p.r, opts, DPT_COLLATE_BOS | DPT_COLLATE_SEP | DPT_COLLATE_EOS, "BOS / SEP / EOS",
                                    COLLATE_SIDES | DPT_COLLATE_MASK_A | DPT_COLLATE_TRIM_A_FIRST, n_str, input_ids, attention_mask,
                                    labels, lengths))
        return rc;
    if (n_str == 0) return DPT_OK;
    p.a = {a->ids, a->off, a->counts, a->status};
    p.b = {b->ids, b->off, b->counts, b->status};
    p.sep_id = opts->sep_id; p.max_a = opts->max_a; p.max_b = opts->max_b;
    p.token_type = token_type_ids; p.b_start = b_start;
    const hipError_t e = dpt::launch_collate_pair(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "collate pair launch");
    return DPT_OK;
}

// The option and size checks of the packing calls: collate's, with DPT_COLLATE_PAD_LEFT unknown here.
constexpr uint32_t PACK_OTHERS = DPT_COLLATE_TRUNC_LEFT | DPT_COLLATE_I64 | DPT_PACK_MASK_FIRST;
static int pack_rows(dpt::CollateRows *r, const dpt_pack_opts *opts, uint64_t n_str, void *input_ids, void *labels) {
    if (const int rc = collate_rows(r, opts, DPT_COLLATE_BOS | DPT_COLLATE_EOS, "BOS / EOS", PACK_OTHERS, n_str, input_ids, nullptr, labels,
                                    nullptr))
        return rc;
    if (n_str >= (1ull << 31)) return fail(DPT_E_ARG, "n_str over 2^31 - 1");
    return DPT_OK;
}

int dpt_pack_sizes(const uint64_t *off, const uint64_t *counts, const int32_t *status, uint64_t n_str, const dpt_pack_opts *opts,
                   uint32_t *lengths, void *hip_stream) {
    if (!off) return fail(DPT_E_ARG, "null off");
    if (!opts) return fail(DPT_E_ARG, "null opts");
    if (!lengths) return fail(DPT_E_ARG, "null lengths");
    dpt::CollateRows r{};
    if (const int rc = pack_rows(&r, opts, n_str, nullptr, nullptr)) return rc;
    const uint32_t n_special = (uint32_t)__builtin_popcount(opts->flags & (DPT_COLLATE_BOS | DPT_COLLATE_EOS));
    const hipError_t e = dpt::launch_pack_sizes({nullptr, off, counts, status}, (uint32_t)n_str, r.row_len - n_special, n_special, lengths,
                                                (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "pack sizes launch");
    return DPT_OK;
}

int dpt_pack_plan_workspace(uint64_t n_str, uint64_t *bytes) {
    if (!bytes) return fail(DPT_E_ARG, "null bytes");
    if (n_str >= (1ull << 31)) return fail(DPT_E_ARG, "n_str over 2^31 - 1");
    *bytes = dpt::pack_plan_workspace_bytes(n_str);
    return DPT_OK;
}

int dpt_pack_plan(const uint64_t *tok_off, uint64_t n_str, uint32_t row_len, uint64_t row_cap, uint32_t *str_row, uint32_t *str_col,
                  uint32_t *row_first, uint32_t *row_fill, uint64_t *n_rows, void *ws, uint64_t ws_bytes, void *hip_stream) {
    if (!tok_off) return fail(DPT_E_ARG, "null tok_off");
    if (!n_rows) return fail(DPT_E_ARG, "null n_rows");
    if (row_len == 0) return fail(DPT_E_ARG, "row_len is 0");
    if (row_len > (1u << 31)) return fail(DPT_E_ARG, "row_len over 2^31");
    if (n_str >= (1ull << 31)) return fail(DPT_E_ARG, "n_str over 2^31 - 1");
    if (row_cap >= (1ull << 31)) return fail(DPT_E_ARG, "row_cap over 2^31 - 1");
    if (n_str && !ws) return fail(DPT_E_ARG, "null ws");
    if ((uintptr_t)ws % 4) return fail(DPT_E_ARG, "ws is not 4-byte aligned");
    if (ws_bytes < dpt::pack_plan_workspace_bytes(n_str)) return fail(DPT_E_CAP, "ws_bytes under dpt_pack_plan_workspace(n_str)");
    const dpt::PackPlanLaunch p{tok_off, (uint32_t)n_str, row_len, (uint32_t)row_cap, str_row, str_col, row_first, row_fill, n_rows, ws};
    const hipError_t e = dpt::launch_pack_plan(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "pack plan launch");
    return DPT_OK;
}

int dpt_pack_write(const dpt_collate_side *side, uint64_t n_str, const uint64_t *tok_off, const uint32_t *row_first,
                   const uint64_t *n_rows, uint64_t row_cap, const dpt_pack_opts *opts, void *input_ids, void *position_ids,
                   void *segment_ids, void *labels, void *hip_stream) {
    if (!side) return fail(DPT_E_ARG, "null side");
    if (!side->ids) return fail(DPT_E_ARG, "null side->ids");
    if (!side->off) return fail(DPT_E_ARG, "null side->off");
    if (!tok_off) return fail(DPT_E_ARG, "null tok_off");
    if (!row_first) return fail(DPT_E_ARG, "null row_first");
    if (!n_rows) return fail(DPT_E_ARG, "null n_rows");
    if (!opts) return fail(DPT_E_ARG, "null opts");
    if (!input_ids) return fail(DPT_E_ARG, "null input_ids");
    dpt::PackWriteLaunch p{};
    if (const int rc = pack_rows(&p.r, opts, n_str, input_ids, labels)) return rc;
    if (row_cap >= (1ull << 31)) return fail(DPT_E_ARG, "row_cap over 2^31 - 1");
    p.src = {side->ids, side->off, side->counts, side->status};
    p.tok_off = tok_off; p.row_first = row_first; p.n_rows = n_rows; p.row_cap = row_cap;
    p.position_ids = position_ids; p.segment_ids = segment_ids;
    const hipError_t e = dpt::launch_pack_write(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "pack write launch");
    return DPT_OK;
}

int dpt_debug_pack_geometry(uint32_t *strings_per_block, uint32_t *grid_cap) {
    if (!strings_per_block || !grid_cap) return fail(DPT_E_ARG, "null argument");
    *strings_per_block = dpt::PACK_BLOCK_STRINGS;
    *grid_cap = dpt::PACK_GRID_CAP;
    return DPT_OK;
}

// The checks both word-compare calls make of their sides, flags and n_str; 0 with p's common members filled.
static int words_args(dpt::WordsLaunch *p, const dpt_word_side *a, const dpt_word_side *b, uint64_t n_str, int flags,
                      int32_t *wc_status) {
    if (!a) return fail(DPT_E_ARG, "null a");
    if (!b) return fail(DPT_E_ARG, "null b");
    if (!a->off) return fail(DPT_E_ARG, "null a->off");
    if (!a->tok_word) return fail(DPT_E_ARG, "null a->tok_word");
    if (!b->off) return fail(DPT_E_ARG, "null b->off");
    if (!b->tok_word) return fail(DPT_E_ARG, "null b->tok_word");
    if (flags == 0 || (flags & ~(DPT_WORDS_LESS | DPT_WORDS_GREATER))) return fail(DPT_E_ARG, "flags: DPT_WORDS_LESS and / or DPT_WORDS_GREATER");
    if (n_str >= (1ull << 31)) return fail(DPT_E_ARG, "n_str over 2^31 - 1");
    if (!wc_status) return fail(DPT_E_ARG, "null wc_status");
    p->a = *a; p->b = *b; p->n_str = n_str; p->flags = flags; p->wc_status = wc_status;
    return DPT_OK;
}

static int words_launch(const dpt::WordsLaunch &p, void *hip_stream) {
    if (p.n_str == 0) return DPT_OK;
    const hipError_t e = dpt::launch_words(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "word compare launch");
    return DPT_OK;
}

int dpt_word_compare_sizes(const dpt_word_side *a, const dpt_word_side *b, uint64_t n_str, int flags, uint32_t *n_words,
                           uint32_t *n_sel, uint32_t *len_a, uint32_t *len_b, int32_t *wc_status, void *hip_stream) {
    dpt::WordsLaunch p{};
    if (const int rc = words_args(&p, a, b, n_str, flags, wc_status)) return rc;
    if (!n_words) return fail(DPT_E_ARG, "null n_words");
    if (!n_sel) return fail(DPT_E_ARG, "null n_sel");
    p.write = false;
    p.n_words = n_words; p.n_sel = n_sel; p.len_a = len_a; p.len_b = len_b;
    return words_launch(p, hip_stream);
}

int dpt_word_compare_write(const dpt_word_side *a, const dpt_word_side *b, uint64_t n_str, int flags, const uint64_t *word_off,
                           uint32_t *cnt_a, uint32_t *cnt_b, const uint64_t *sel_off, uint32_t *sel_str, uint32_t *sel_word,
                           uint32_t *sel_begin, uint32_t *sel_end, uint32_t *sel_a_first, uint32_t *sel_a_count,
                           uint32_t *sel_b_first, uint32_t *sel_b_count, int32_t *wc_status, void *hip_stream) {
    dpt::WordsLaunch p{};
    if (const int rc = words_args(&p, a, b, n_str, flags, wc_status)) return rc;
    const int n_word_args = (word_off != nullptr) + (cnt_a != nullptr) + (cnt_b != nullptr);
    if (n_word_args != 0 && n_word_args != 3) return fail(DPT_E_ARG, "word_off, cnt_a and cnt_b go together");
    const bool any_sel = sel_str || sel_word || sel_begin || sel_end || sel_a_first || sel_a_count || sel_b_first || sel_b_count;
    if (any_sel && !sel_off) return fail(DPT_E_ARG, "null sel_off");
    if ((sel_begin || sel_end) && !a->tok_end) return fail(DPT_E_ARG, "sel_begin / sel_end need a->tok_end");
    p.write = true;
    p.word_off = word_off; p.cnt_a = cnt_a; p.cnt_b = cnt_b;
    p.sel_off = sel_off; p.sel_str = sel_str; p.sel_word = sel_word; p.sel_begin = sel_begin; p.sel_end = sel_end;
    p.sel_a_first = sel_a_first; p.sel_a_count = sel_a_count; p.sel_b_first = sel_b_first; p.sel_b_count = sel_b_count;
    return words_launch(p, hip_stream);
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
