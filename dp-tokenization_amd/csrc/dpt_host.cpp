// dpt_host.cpp -- the calls of include/dpt.h that take HOST pointers: each checks its arguments, stages them in
// the ctx's pinned and device buffers (Stager; the arrays' places: dpt_host_layout.h), runs the device call
// on the staged copy, brings the results back and synchronises.
#include <string.h>

#include "dpt_host_layout.h"
#include "dpt_objects.h"

using namespace dpt;

namespace {

// Pinned host buffer of at least `need` bytes (4096 at least, +25 % when it grows); *pd, its address as the
// device sees it, is cleared when it moves.
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

// One host-buffer call's use of its ctx's staging: a device buffer and its pinned mirror per side, every copy
// one async DMA on the null stream.  The contract the calls rely on:
//  - stage() may be called again in the middle of a call with another layout (dpt_decode_host, once it knows
//    the decoded size).  A side whose size does not grow does not move and keeps its contents; one that grows
//    may move, and then holds nothing: views of it taken before are stale.
//  - A zero-copy address (dpt_ctx::pd_in / pd_out) is valid or null: stage() clears it when its pinned buffer
//    moves, zero_copy() looks it up again then and only then.
struct Stager {
    dpt_ctx *c;
    HostLayout L{};
    hipStream_t st = nullptr;
    int stage(const HostLayout &l) {
        hipError_t e;
        L = l;
        if ((e = grow(&c->d_in, &c->cap_in, L.in.bytes)) != hipSuccess) return hip_fail(e, "hipMalloc(host-path in)");
        if ((e = grow(&c->d_out, &c->cap_out, L.out.bytes)) != hipSuccess) return hip_fail(e, "hipMalloc(host-path out)");
        if ((e = grow_pinned(&c->p_in, &c->pd_in, &c->cap_pin_in, L.in.bytes)) != hipSuccess) return hip_fail(e, "hipHostMalloc(in)");
        if ((e = grow_pinned(&c->p_out, &c->pd_out, &c->cap_pin_out, L.out.bytes)) != hipSuccess) return hip_fail(e, "hipHostMalloc(out)");
        return DPT_OK;
    }
    // Segment s of a side as T[] in the buffer at `base` (null for an absent segment): the pinned host buffer,
    // the device buffer, or -- a zero-copy call -- the pinned buffer as the device addresses it.
    template <typename T> static T *at(uint8_t *base, const HostSide &side, int s) {
        return side.seg[s].payload + side.seg[s].slack ? reinterpret_cast<T *>(base + side.seg[s].offset) : nullptr;
    }
    template <typename T> T *host_in(int s) const { return at<T>(c->p_in, L.in, s); }
    template <typename T> const T *dev_in(int s) const { return at<const T>(c->d_in, L.in, s); }
    template <typename T> const T *host_out(int s) const { return at<const T>(c->p_out, L.out, s); }
    template <typename T> T *dev_out(int s) const { return at<T>(c->d_out, L.out, s); }
    // fill the in side: n bytes of an array (null or empty: nothing), or n_str + 1 offsets rebased to 0 (the
    // device view is self-contained); read the out side after sync(): n bytes of segment s (dst null: not wanted)
    void put(int s, const void *src, uint64_t n) const { if (src && n) memcpy(host_in<uint8_t>(s), src, n); }
    void rebase(int s, const uint64_t *off, uint64_t n_str) const {
        for (uint64_t i = 0; i <= n_str; i++) host_in<uint64_t>(s)[i] = off[i] - off[0];
    }
    void get(void *dst, int s, uint64_t n) const { if (dst && n) memcpy(dst, host_out<uint8_t>(s), n); }
    // the copies: the whole in side or one segment of it up; the out side's first bytes or n bytes of a segment down
    int done(hipError_t e, const char *what) const { return e != hipSuccess ? hip_fail(e, what) : DPT_OK; }   // (a launch's result too)
    int copy(uint8_t *dst, const uint8_t *src, uint64_t off, uint64_t n, hipMemcpyKind kind, const char *what) const {
        return n ? done(hipMemcpyAsync(dst + off, src + off, n, kind, st), what) : DPT_OK;
    }
    int upload() const { return copy(c->d_in, c->p_in, 0, L.in.bytes, hipMemcpyHostToDevice, "H2D"); }
    int upload(int s) const { return copy(c->d_in, c->p_in, L.in.seg[s].offset, L.in.seg[s].payload, hipMemcpyHostToDevice, "H2D"); }
    int download(uint64_t prefix) const { return copy(c->p_out, c->d_out, 0, prefix, hipMemcpyDeviceToHost, "D2H"); }
    int download(int s, uint64_t n, const char *what = "D2H") const { return copy(c->p_out, c->d_out, L.out.seg[s].offset, n, hipMemcpyDeviceToHost, what); }
    int sync() const { return done(hipStreamSynchronize(st), "sync"); }
    // the pinned buffers as the device addresses them
    int zero_copy(uint8_t **in, uint8_t **out) const {
        hipError_t e;
        if (!c->pd_in && (e = hipHostGetDevicePointer((void **)&c->pd_in, c->p_in, 0)) != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer");
        if (!c->pd_out && (e = hipHostGetDevicePointer((void **)&c->pd_out, c->p_out, 0)) != hipSuccess) return hip_fail(e, "hipHostGetDevicePointer");
        *in = c->pd_in; *out = c->pd_out;
        return DPT_OK;
    }
};

// The kernels take string lengths as 32-bit values (dpt.h): offsets must be monotone and every string shorter
// than 4 GiB, or a wrapped length would read past the text.  n_bytes (nullable): what str_off must span.
// id_off (nullable): monotone.  id_first: its message comes first (the decode calls).
int check_offsets(const uint64_t *str_off, uint64_t n_str, const uint64_t *n_bytes, const uint64_t *id_off, bool id_first = false) {
    if (n_bytes && str_off[n_str] - str_off[0] != *n_bytes) return fail(DPT_E_ARG, "n_bytes != str_off[n_str]-str_off[0]");
    for (uint64_t i = 0; i < n_str; i++) {
        if (id_first && id_off[i + 1] < id_off[i]) return fail(DPT_E_ARG, "id_off not monotone");
        if (str_off && str_off[i + 1] < str_off[i]) return fail(DPT_E_ARG, "str_off not monotone");
        if (str_off && str_off[i + 1] - str_off[i] >= (1ull << 32)) return fail(DPT_E_ARG, "a string of 4 GiB or more");
        if (!id_first && id_off && id_off[i + 1] < id_off[i]) return fail(DPT_E_ARG, "id_off not monotone");
    }
    return DPT_OK;
}

// One host-path call (encode_host): HOST pointers.
struct HostRequest : CsrCall {
    uint64_t *n_far = nullptr;   // dpt_dp_host_far: the far edge pairs found
    int depth = 0;               // 1: the rerun of the strings an arena overflow left out (it may not overflow again)
};

// Host path calls up to this many input bytes check whether any string needs the fallback passes.
constexpr uint64_t NO_FALLBACK_CHECK_BYTES = 16384;

// True when no string of a RAW / PRESPLIT call can leave the first pass (dpt_kernels.hip tokenize_kernel):
// every word fits its window of dpt::SMALL_CH bytes (consecutive word starts -- byte 0, then ' ' in RAW mode
// or a cut byte on a non-continuation byte in PRESPLIT mode -- at most that far apart, the last one at most
// that far before the string's end) and every atom (a code point: a byte and its continuation bytes) has at
// most 4 bytes.  (Vocabularies with tokens of more than 64 code points are not checked: the caller.)
bool no_fallback_needed(int mode, const uint8_t *text, const uint64_t *str_off, const uint8_t *cut, uint64_t n_str) {
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
int encode_host_impl(dpt_ctx *c, const dpt_vocab *v, const HostRequest &r, bool *overflow) {
    const uint64_t n_bytes = r.n_bytes, n_str = r.n_str;
    *overflow = false;
    // host arguments first (checkable without a device)
    if (!r.str_off || !r.id_off || (n_str && !r.status)) return fail(DPT_E_ARG, "null output/offsets");
    if (n_bytes && (!r.text || !r.ids)) return fail(DPT_E_ARG, "null text/ids");
    if (r.ids_cap < n_bytes) return fail(DPT_E_CAP, "ids_cap must be >= n_bytes");
    int rc;
    if ((rc = check_offsets(r.str_off, n_str, &n_bytes, nullptr))) return rc;
    if (!c || !v) return fail(DPT_E_ARG, "null ctx or vocab");
    DeviceGuard g(c->device);
    const bool cut = (r.mode_flags & DPT_MODE_MASK) != DPT_MODE_RAW && n_bytes;
    if (cut && !r.cut_mask) return fail(DPT_E_ARG, "PRESPLIT/ATOMS need cut_mask");
    const bool want_far = r.edges && r.far;
    Stager s{c};
    if ((rc = s.stage(encode_layout(n_bytes, n_str, cut, r.edges != nullptr, want_far ? r.far_cap : 0)))) return rc;
    s.put(ENC_TEXT, r.text, n_bytes); s.rebase(ENC_STR_OFF, r.str_off, n_str);
    if (cut) s.put(ENC_CUT, r.cut_mask, n_bytes);
    const uint64_t *p_idoff = s.host_out<uint64_t>(ENC_ID_OFF);
    const dpt::CounterBlock *p_ctr = s.host_out<dpt::CounterBlock>(ENC_CTR);   // the call's counters (their reset's snapshot)
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
        const HostLayout &l = s.L;
        q.set(r.mode_flags, in, n_bytes, s.at<const uint64_t>(in, l.in, ENC_STR_OFF), s.at<const uint8_t>(in, l.in, ENC_CUT), n_str,
              s.at<int32_t>(out, l.out, ENC_STATUS), s.at<int32_t>(out, l.out, ENC_CAPPED), s.at<int32_t>(out, l.out, ENC_IDS), n_bytes ? n_bytes : 1);
        q.id_off = s.at<uint64_t>(out, l.out, ENC_ID_OFF); q.ctr_snap = s.at<uint64_t>(out, l.out, ENC_CTR);
        q.edges = s.at<uint64_t>(out, l.out, ENC_EDGES); q.far_cap = r.far_cap;
        q.far = want_far ? reinterpret_cast<uint64_t *>(out + s.L.out.seg[ENC_FAR].offset) : nullptr;   // (far_cap 0: the count alone)
        q.stream = s.st; q.no_fallback = no_fb;
        return q;
    };
    // One string with no fallback pass (a per-string dp_tokenize call): zero-copy -- its lone wave
    // (EncodeLaunch::solo) reads the text from and writes the outputs to the pinned host buffers, so the
    // call is one launch and a sync (two copies and their gaps less)
    if (no_fb && n_str == 1 && !r.edges && !c->profile && !dpt::launch_knobs().no_solo) {
        uint8_t *in, *out;
        if ((rc = s.zero_copy(&in, &out)) || (rc = encode_impl(c, v, request(in, out))) || (rc = s.sync())) return rc;
        const uint64_t total = p_idoff[1];
        if (total > r.ids_cap || total > n_bytes) return fail(DPT_E_CAP, "ids overflow");
        r.id_off[0] = 0; r.id_off[1] = total;
        s.get(r.status, ENC_STATUS, 4); s.get(r.capped_len, ENC_CAPPED, 4); s.get(r.ids, ENC_IDS, 4 * total);
        return DPT_OK;
    }
    const EncodeRequest q = request(c->d_in, c->d_out);
    if ((rc = s.upload())) return rc;
    for (int attempt = 0;; attempt++) {
        if ((rc = encode_impl(c, v, q)) || (rc = s.download(one_copy ? s.L.out.bytes : s.L.out.seg[ENC_IDS].offset)) || (rc = s.sync())) return rc;
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
    const uint64_t edge_bytes = r.edges ? 8 * n_bytes : 0;
    if (!one_copy && ((rc = s.download(ENC_IDS, 4 * total, "D2H ids")) || (rc = s.download(ENC_EDGES, edge_bytes, "D2H edges")) ||
                      (rc = s.download(ENC_FAR, 16 * nf, "D2H far edges")) || (rc = s.sync())))
        return rc;
    s.get(r.id_off, ENC_ID_OFF, 8 * (n_str + 1)); s.get(r.status, ENC_STATUS, 4 * n_str); s.get(r.capped_len, ENC_CAPPED, 4 * n_str);
    s.get(r.ids, ENC_IDS, 4 * total); s.get(r.edges, ENC_EDGES, edge_bytes); s.get(r.far, ENC_FAR, 16 * nf);
    return DPT_OK;
}

// After an arena overflow (the arena has since grown to what the pass claimed): the strings with
// status DPT_STATUS_TOO_LONG -- exactly those the unbounded pass could not hold -- as one sub-batch,
// their results spliced into the caller's CSR arrays.
int rerun_too_long(dpt_ctx *c, const dpt_vocab *v, const HostRequest &r) {
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
    s.set(r.mode_flags, stext.data(), sb, soff.data(), cut ? scut.data() : nullptr, k, sst.data(),
          r.capped_len ? scap.data() : nullptr, sids.data(), sb ? sb : 1);
    s.id_off = sidoff.data();
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

int encode_host(dpt_ctx *c, const dpt_vocab *v, const HostRequest &r) {
    bool overflow;
    const int rc = encode_host_impl(c, v, r, &overflow);
    return rc || !overflow ? rc : rerun_too_long(c, v, r);
}

// dpt_dp_host*'s common part: r holds the caller's arguments, the lengths (nullable) as capped_len.  No ids.
int dp_host(dpt_ctx *c, const dpt_vocab *v, HostRequest r) {
    if (!(r.mode_flags & (DPT_FLAG_UNCAPPED | DPT_FLAG_LEN_ONLY))) r.mode_flags |= DPT_FLAG_LEN_ONLY;
    std::vector<uint64_t> id_off(r.n_str + 1);
    std::vector<int32_t> len_tmp(r.capped_len ? 0 : r.n_str + 1);
    int32_t dummy_ids[1];
    r.ids = dummy_ids; r.ids_cap = r.n_bytes ? r.n_bytes : 1; r.id_off = id_off.data();
    if (!r.capped_len) r.capped_len = len_tmp.data();
    return encode_host(c, v, r);
}

}  // namespace

extern "C" {

int dpt_encode_host(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                    const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap,
                    uint64_t *id_off, int32_t *status, int32_t *capped_len) {
    if (mode & ~DPT_MODE_MASK) return fail(DPT_E_ARG, "flags are for dpt_dp_host");
    HostRequest r;
    r.set(mode, text, n_bytes, str_off, cut_mask, n_str, status, capped_len, ids, ids_cap);
    r.id_off = id_off;
    return encode_host(c, v, r);
}

int dpt_dp_host(dpt_ctx *c, const dpt_vocab *v, int mode_flags, const uint8_t *text, uint64_t n_bytes,
                const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *status, int32_t *lengths,
                uint64_t *edges) {
    if (!lengths && !edges) return fail(DPT_E_ARG, "nothing to compute");
    HostRequest r;
    r.set(mode_flags, text, n_bytes, str_off, cut_mask, n_str, status, lengths);
    r.edges = edges;
    return dp_host(c, v, r);
}

int dpt_dp_host_far(dpt_ctx *c, const dpt_vocab *v, int mode_flags, const uint8_t *text, uint64_t n_bytes,
                    const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *status, int32_t *lengths,
                    uint64_t *edges, uint64_t *far, uint64_t far_cap, uint64_t *n_far) {
    if (!edges || !n_far || (far_cap && !far)) return fail(DPT_E_ARG, "dpt_dp_host_far needs edges, far and n_far");
    *n_far = 0;
    uint64_t dummy_far[2];
    HostRequest r;
    r.set(mode_flags, text, n_bytes, str_off, cut_mask, n_str, status, lengths);
    r.edges = edges; r.far = far ? far : dummy_far; r.far_cap = far_cap; r.n_far = n_far;
    return dp_host(c, v, r);
}

int dpt_token_spans_host(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                         const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, const int32_t *ids,
                         const uint64_t *id_off, const int32_t *status, uint32_t *tok_end, uint32_t *tok_word,
                         int32_t *span_status) {
    // host arguments first (checkable without a device)
    int rc = spans_check(spans_args(v, mode, text, str_off, cut_mask, n_str, ids, id_off, status, tok_end, tok_word, span_status), v, n_bytes);
    if (rc) return rc;
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if ((rc = check_offsets(str_off, n_str, &n_bytes, id_off))) return rc;
    if (c->device != v->device) return fail(DPT_E_ARG, "ctx and vocab on different devices");
    if (!v->d_tok_len) return fail(DPT_E_VOCAB, NO_TOK_LEN);
    if (n_str == 0) return DPT_OK;
    const uint64_t n_tok = id_off[n_str] - id_off[0];
    DeviceGuard g(c->device);
    Stager s{c};
    if ((rc = s.stage(spans_layout(n_bytes, n_str, n_tok, mode != DPT_MODE_RAW, tok_word != nullptr)))) return rc;
    s.rebase(SP_STR_OFF, str_off, n_str); s.rebase(SP_ID_OFF, id_off, n_str);
    s.put(SP_IDS, ids, 4 * n_tok); s.put(SP_STATUS, status, 4 * n_str); s.put(SP_TEXT, text, n_bytes);
    if (mode != DPT_MODE_RAW) s.put(SP_CUT, cut_mask, n_bytes);
    // the same call on the device buffers
    const dpt::SpansLaunch p = spans_args(v, mode, s.dev_in<uint8_t>(SP_TEXT), s.dev_in<uint64_t>(SP_STR_OFF), s.dev_in<uint8_t>(SP_CUT), n_str,
                                          s.dev_in<int32_t>(SP_IDS), s.dev_in<uint64_t>(SP_ID_OFF), s.dev_in<int32_t>(SP_STATUS),
                                          s.dev_out<uint32_t>(SP_TOK_END), s.dev_out<uint32_t>(SP_TOK_WORD), s.dev_out<int32_t>(SP_SPAN_STATUS));
    if ((rc = s.upload()) || (rc = s.done(dpt::launch_spans(p, s.st), "spans launch")) || (rc = s.download(s.L.out.bytes)) || (rc = s.sync())) return rc;
    s.get(tok_end, SP_TOK_END, 4 * n_tok); s.get(tok_word, SP_TOK_WORD, 4 * n_tok); s.get(span_status, SP_SPAN_STATUS, 4 * n_str);
    return DPT_OK;
}

int dpt_decode_host(dpt_ctx *c, const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                    uint64_t n_str, int flags, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *dec_status) {
    // host arguments first (checkable without a device)
    dpt::DecodeLaunch p = decode_args(dpt::DECODE_BYTES, ids, id_off, status, n_str);
    p.out = out; p.out_off = out_off; p.result = dec_status;
    int rc = decode_check(&p, d, flags);
    if (rc) return rc;
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if ((rc = check_offsets(nullptr, n_str, nullptr, id_off, true))) return rc;
    const uint64_t n_tok = id_off[n_str] - id_off[0];
    if ((n_tok && !ids) || (out_cap && !out)) return fail(DPT_E_ARG, "null argument");
    if (c->device != d->device) return fail(DPT_E_ARG, "ctx and detok on different devices");
    out_off[0] = 0;
    if (n_str == 0) return DPT_OK;
    DeviceGuard g(c->device);
    Stager s{c};
    if ((rc = s.stage(decode_layout(n_str, n_tok, 0)))) return rc;
    s.rebase(DEC_ID_OFF, id_off, n_str); s.put(DEC_IDS, ids, 4 * n_tok); s.put(DEC_STATUS, status, 4 * n_str);
    // the sizes, then their prefix sum on the host
    p.kind = dpt::DECODE_SIZES; p.ids = s.dev_in<int32_t>(DEC_IDS); p.id_off = s.dev_in<uint64_t>(DEC_ID_OFF);
    p.status = status ? s.dev_in<int32_t>(DEC_STATUS) : nullptr; p.out_len = s.dev_out<uint64_t>(DEC_OUT_LEN);
    if ((rc = s.upload()) || (rc = s.done(dpt::launch_decode(p, s.st), "decode sizes launch")) || (rc = s.download(DEC_OUT_LEN, 8 * n_str)) || (rc = s.sync())) return rc;
    const uint64_t *len = s.host_out<uint64_t>(DEC_OUT_LEN);
    for (uint64_t i = 0; i < n_str; i++) out_off[i + 1] = out_off[i] + len[i];
    const uint64_t decoded = out_off[n_str];
    if (decoded > out_cap) return fail(DPT_E_CAP, "decoded bytes do not fit out_cap (the need is out_off[n_str])");
    // the bytes: the in side keeps its size, so it stays where it is with the ids in it; the out side may move
    if ((rc = s.stage(decode_layout(n_str, n_tok, decoded)))) return rc;
    s.put(DEC_OUT_OFF, out_off, 8 * (n_str + 1));
    p.kind = dpt::DECODE_BYTES; p.out = s.dev_out<uint8_t>(DEC_BYTES); p.out_off = s.dev_in<uint64_t>(DEC_OUT_OFF); p.result = s.dev_out<int32_t>(DEC_RESULT);
    if ((rc = s.upload(DEC_OUT_OFF)) || (rc = s.done(dpt::launch_decode(p, s.st), "decode launch")) ||
        (rc = s.download(s.L.out.seg[DEC_BYTES].offset + decoded)) || (rc = s.sync()))
        return rc;
    s.get(dec_status, DEC_RESULT, 4 * n_str); s.get(out, DEC_BYTES, decoded);
    return DPT_OK;
}

int dpt_roundtrip_host(dpt_ctx *c, const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                       const uint8_t *text, const uint64_t *str_off, uint64_t n_str, int flags, int32_t *rt,
                       uint32_t *first_diff) {
    dpt::DecodeLaunch p = decode_args(dpt::DECODE_ROUNDTRIP, ids, id_off, status, n_str);
    p.text = text; p.str_off = str_off; p.result = rt; p.first_diff = first_diff;
    int rc = decode_check(&p, d, flags);
    if (rc) return rc;
    if (!c) return fail(DPT_E_ARG, "null ctx");
    if ((rc = check_offsets(str_off, n_str, nullptr, id_off, true))) return rc;
    const uint64_t n_tok = id_off[n_str] - id_off[0], n_bytes = str_off[n_str] - str_off[0];
    if ((n_tok && !ids) || (n_bytes && !text)) return fail(DPT_E_ARG, "null argument");
    if (c->device != d->device) return fail(DPT_E_ARG, "ctx and detok on different devices");
    if (n_str == 0) return DPT_OK;
    DeviceGuard g(c->device);
    Stager s{c};
    if ((rc = s.stage(roundtrip_layout(n_bytes, n_str, n_tok)))) return rc;
    s.rebase(RT_ID_OFF, id_off, n_str); s.rebase(RT_STR_OFF, str_off, n_str);
    s.put(RT_IDS, ids, 4 * n_tok); s.put(RT_STATUS, status, 4 * n_str); s.put(RT_TEXT, text, n_bytes);
    // the same call on the device buffers
    p.ids = s.dev_in<int32_t>(RT_IDS); p.id_off = s.dev_in<uint64_t>(RT_ID_OFF); p.status = status ? s.dev_in<int32_t>(RT_STATUS) : nullptr;
    p.text = s.dev_in<uint8_t>(RT_TEXT); p.str_off = s.dev_in<uint64_t>(RT_STR_OFF);
    p.result = s.dev_out<int32_t>(RT_RESULT); p.first_diff = s.dev_out<uint32_t>(RT_FIRST_DIFF);
    if ((rc = s.upload()) || (rc = s.done(dpt::launch_decode(p, s.st), "roundtrip launch")) || (rc = s.download(s.L.out.bytes)) || (rc = s.sync())) return rc;
    s.get(rt, RT_RESULT, 4 * n_str);
    const uint32_t *fd = s.host_out<uint32_t>(RT_FIRST_DIFF);
    for (uint64_t i = 0; first_diff && i < n_str; i++)   // (written only where the verdict is DPT_RT_DIFFERS, as the device call does)
        if (rt[i] == DPT_RT_DIFFERS) first_diff[i] = fd[i];
    return DPT_OK;
}

int dpt_debug_host_layout(int call, uint64_t n_bytes, uint64_t n_str, uint64_t n_tok, int flags, uint64_t far_pairs, uint64_t *out) {
    if (!out || call < 0 || call > 3 || (flags & ~7)) return fail(DPT_E_ARG, "bad host layout arguments");
    const bool cut = flags & 1, word = flags & 2, edges = flags & 4;
    const HostLayout l = call == 0 ? encode_layout(n_bytes, n_str, cut, edges, far_pairs) : call == 1 ? spans_layout(n_bytes, n_str, n_tok, cut, word)
                       : call == 2 ? decode_layout(n_str, n_tok, n_bytes) : roundtrip_layout(n_bytes, n_str, n_tok);
    memset(out, 0, DPT_HOST_LAYOUT_INTS * sizeof(uint64_t));
    for (const HostSide *sd : {&l.in, &l.out}) {
        *out++ = sd->n; *out++ = sd->bytes;
        memcpy(out, sd->seg, sd->n * sizeof(Segment));
        out += 3 * HOST_MAX_SEG;
    }
    return DPT_OK;
}

}  // extern "C"
