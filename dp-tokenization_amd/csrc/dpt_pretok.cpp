// dpt_pretok.cpp -- the pre-tokenization table (include/dpt.h dpt_pretok_create): its host builder, the object that
// holds its device copy, and the argument checks of the two device calls whose kernels are in dpt_pretok.hip.  The
// table is what those kernels need to know of a vocabulary to write llama mode's pre-split text themselves -- which
// characters are a piece of their own (every other character becomes its byte pieces), whether a run of spaces is
// safe, the BOS piece, and the literal strings a tokenizer object treats specially.  The rule itself is stated in the
// header.
//
// build_pretok_tables calls no HIP function: testable without a device (dpt_debug_pretok_table,
// tests/test_pretok_tables.py; tests/pretok_ref.py restates the rules).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>

#include "dpt_objects.h"

namespace dpt {

namespace {

const uint8_t WS[3] = {0xE2, 0x96, 0x81};   // U+2581

// The code point of p[0..len) when it is exactly one well-formed UTF-8 character, else -1.
int64_t one_char(const uint8_t *p, size_t len) {
    if (len == 1) return p[0] < 0x80 ? p[0] : -1;
    auto cont = [&](size_t k) { return (p[k] & 0xC0) == 0x80; };
    if (len == 2) return p[0] >= 0xC2 && p[0] <= 0xDF && cont(1) ? ((p[0] & 0x1F) << 6) | (p[1] & 0x3F) : -1;
    if (len == 3) {
        if ((p[0] & 0xF0) != 0xE0 || !cont(1) || !cont(2)) return -1;
        const int64_t cp = ((p[0] & 0x0F) << 12) | ((p[1] & 0x3F) << 6) | (p[2] & 0x3F);
        return cp >= 0x800 && !(cp >= 0xD800 && cp <= 0xDFFF) ? cp : -1;
    }
    if (len == 4) {
        if ((p[0] & 0xF8) != 0xF0 || !cont(1) || !cont(2) || !cont(3)) return -1;
        const int64_t cp = ((int64_t)(p[0] & 0x07) << 18) | ((p[1] & 0x3F) << 12) | ((p[2] & 0x3F) << 6) | (p[3] & 0x3F);
        return cp >= 0x10000 && cp <= 0x10FFFF ? cp : -1;
    }
    return -1;
}

bool ws_at(const uint8_t *p, size_t len, size_t k) { return k + 3 <= len && memcmp(p + k, WS, 3) == 0; }

}  // namespace

const char *build_pretok_tables(const uint8_t *blob, const uint64_t *off, uint32_t n, const uint8_t *bos, uint32_t bos_len,
                                const uint8_t *lit_blob, const uint64_t *lit_off, uint32_t n_lit, PretokTables *out,
                                int *code) try {
    *code = DPT_E_ARG;
    if (n_lit > DPT_PRETOK_MAX_LITERALS) return "more than DPT_PRETOK_MAX_LITERALS literals";
    if (bos_len > DPT_PRETOK_MAX_BOS) return "BOS piece longer than DPT_PRETOK_MAX_BOS bytes";
    for (uint32_t k = 0; k < n_lit; k++) {
        if (lit_off[k + 1] < lit_off[k]) return "lit_off not monotone";
        const uint64_t len = lit_off[k + 1] - lit_off[k];
        if (len < 1 || len > DPT_PRETOK_MAX_LITERAL_BYTES) return "a literal of 0 or more than DPT_PRETOK_MAX_LITERAL_BYTES bytes";
    }
    *code = DPT_E_VOCAB;
    PretokTables &t = *out;
    t.bmp.assign(PRETOK_BMP_WORDS, 0u);
    t.astral.clear();
    t.runs_ok = true;
    t.n_known = 0;
    std::unordered_set<std::string> have;
    have.reserve(n);
    for (uint32_t k = 0; k < n; k++) {
        const size_t len = (size_t)(off[k + 1] - off[k]);
        if (len == 0) continue;
        const uint8_t *p = blob + (off[k] - off[0]);
        if (!have.emplace(reinterpret_cast<const char *>(p), len).second) continue;
        bool all_ws = len % 3 == 0;
        for (size_t j = 0; all_ws && j < len; j += 3) all_ws = ws_at(p, len, j);
        if (all_ws && len >= 6) t.runs_ok = false;
        if (!all_ws)
            for (size_t j = 1; j + 3 <= len; j++)
                if (ws_at(p, len, j)) return "a piece holds U+2581 after its first character";
        const int64_t cp = one_char(p, len);
        if (cp < 0) continue;
        t.n_known++;
        if (cp < 0x10000) t.bmp[(size_t)cp >> 5] |= 1u << (cp & 31);
        else t.astral.push_back((uint32_t)cp);
    }
    std::sort(t.astral.begin(), t.astral.end());
    for (unsigned b = 0; b < 256; b++) {
        static const char HEX[] = "0123456789ABCDEF";
        const char piece[6] = {'<', '0', 'x', HEX[b >> 4], HEX[b & 15], '>'};
        if (!have.count(std::string(piece, 6))) return "a byte piece <0xNN> is missing";
    }
    if (bos_len && !have.count(std::string(reinterpret_cast<const char *>(bos), bos_len))) return "the BOS piece is not in the vocabulary";
    t.bos_len = bos_len;
    t.prefix.assign(bos, bos + bos_len);
    t.prefix.insert(t.prefix.end(), WS, WS + 3);
    t.n_lit = n_lit;
    std::vector<uint32_t> head(8 + n_lit + 1, 0u);
    for (uint32_t k = 0; k < n_lit; k++) {
        const uint8_t first = lit_blob[lit_off[k] - lit_off[0]];
        head[first >> 5] |= 1u << (first & 31);
        head[8 + k + 1] = (uint32_t)(lit_off[k + 1] - lit_off[0]);
    }
    t.lit.resize(head.size() * 4);
    memcpy(t.lit.data(), head.data(), t.lit.size());
    if (n_lit) t.lit.insert(t.lit.end(), lit_blob, lit_blob + (lit_off[n_lit] - lit_off[0]));
    *code = DPT_OK;
    return nullptr;
} catch (const std::bad_alloc &) {
    *code = DPT_E_ARG;
    return "out of host memory";
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_debug_pretok_table(const uint8_t *utf8_blob, const uint64_t *tok_off, uint32_t n_tok, const uint8_t *bos_piece,
                           uint32_t bos_len, const uint8_t *lit_blob, const uint64_t *lit_off, uint32_t n_lit, int which,
                           void *out, uint64_t cap, uint64_t *size) {
    if (!size || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0]) || (bos_len && !bos_piece) ||
        (n_lit && (!lit_blob || !lit_off)))
        return fail(DPT_E_ARG, "null argument");
    for (uint32_t t = 0; t < n_tok; t++)
        if (tok_off[t + 1] < tok_off[t]) return fail(DPT_E_ARG, "tok_off not monotone");
    if (which < 0 || which >= 5) return fail(DPT_E_ARG, "no such table");
    PretokTables t;
    int code = DPT_OK;
    if (const char *err = build_pretok_tables(utf8_blob, tok_off, n_tok, bos_piece, bos_len, lit_blob, lit_off, n_lit, &t, &code))
        return fail(code, err);
    const int64_t scalars[DPT_PRETOK_SCALAR_INTS] = {t.runs_ok ? 1 : 0, t.n_known, t.n_lit, t.bos_len};
    const void *src[] = {t.bmp.data(), t.astral.data(), t.lit.data(), t.prefix.data(), scalars};
    const uint64_t len[] = {t.bmp.size() * 4, t.astral.size() * 4, t.lit.size(), t.prefix.size(), sizeof(scalars)};
    return debug_table_out(src[which], len[which], out, cap, size);
}

int dpt_pretok_create(const uint8_t *utf8_blob, const uint64_t *tok_off, uint32_t n_tok, const uint8_t *bos_piece,
                      uint32_t bos_len, const uint8_t *lit_blob, const uint64_t *lit_off, uint32_t n_lit, int device,
                      dpt_pretok **out) {
    if (!out || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0]) || (bos_len && !bos_piece) ||
        (n_lit && (!lit_blob || !lit_off)))
        return fail(DPT_E_ARG, "null argument");
    *out = nullptr;
    if (const int rc = check_device_and_table(device, tok_off, n_tok)) return rc;
    PretokTables t;
    int code = DPT_OK;
    if (const char *err = build_pretok_tables(utf8_blob, tok_off, n_tok, bos_piece, bos_len, lit_blob, lit_off, n_lit, &t, &code))
        return fail(code, err);
    DeviceGuard g(device);
    dpt_pretok *p = new (std::nothrow) dpt_pretok();
    if (!p) return fail(DPT_E_ARG, "out of host memory");
    p->device = device; p->n_astral = (uint32_t)t.astral.size(); p->n_lit = t.n_lit; p->bos_len = t.bos_len; p->runs_ok = t.runs_ok;
    uint32_t first[8];
    memcpy(first, t.lit.data(), sizeof(first));
    for (int k = 0; k < 2; k++) p->ascii_known[k] = t.bmp[2 * k] | (uint64_t)t.bmp[2 * k + 1] << 32;
    for (int k = 0; k < 4; k++) p->lit_first[k] = first[2 * k] | (uint64_t)first[2 * k + 1] << 32;
    hipError_t e = upload(&p->d_bmp, t.bmp);
    if (e == hipSuccess) e = upload(&p->d_astral, t.astral);
    if (e == hipSuccess) e = upload(&p->d_lit, t.lit);
    if (e == hipSuccess) e = upload(&p->d_prefix, t.prefix);
    if (e != hipSuccess) {
        dpt_pretok_destroy(p);
        return hip_fail(e, "pre-tokenization table upload");
    }
    *out = p;
    return DPT_OK;
}

int dpt_pretok_destroy(dpt_pretok *p) {
    if (!p) return DPT_OK;
    DeviceGuard g(p->device);
    for (void *d : {(void *)p->d_bmp, (void *)p->d_astral, (void *)p->d_lit, (void *)p->d_prefix}) (void)hipFree(d);
    delete p;
    return DPT_OK;
}

// The table's part of a launch, and the launch.
static int pretok_launch(const dpt_pretok *t, PretokLaunch p, void *hip_stream) {
    p.bmp = t->d_bmp; p.astral = t->d_astral; p.n_astral = t->n_astral;
    p.lit_off = reinterpret_cast<const uint32_t *>(t->d_lit) + 8;
    p.lit_bytes = t->d_lit + 4 * (8 + t->n_lit + 1);
    p.n_lit = t->n_lit; p.prefix = t->d_prefix; p.bos_len = t->bos_len; p.runs_ok = t->runs_ok;
    for (int k = 0; k < 2; k++) p.ascii_known[k] = t->ascii_known[k];
    for (int k = 0; k < 4; k++) p.lit_first[k] = t->lit_first[k];
    DeviceGuard g(t->device);
    const hipError_t e = launch_pretok(p, (hipStream_t)hip_stream);
    if (e != hipSuccess) return hip_fail(e, "pre-tokenization launch");
    return DPT_OK;
}

int dpt_pretok_sizes(const dpt_pretok *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str, uint64_t *out_len,
                     int32_t *pre_status, void *hip_stream) {
    return split_call(p, "null pretok", pretok_launch, false, text, str_off, n_str, out_len, pre_status, nullptr, nullptr, nullptr, hip_stream);
}

int dpt_pretok_write(const dpt_pretok *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str,
                     const int32_t *pre_status, uint8_t *out_text, const uint64_t *out_off, uint8_t *cut_mask,
                     void *hip_stream) {
    return split_call(p, "null pretok", pretok_launch, true, text, str_off, n_str, nullptr, const_cast<int32_t *>(pre_status), out_text,
                      out_off, cut_mask, hip_stream);
}

static int pretok_launch_atoms(const dpt_pretok *t, PretokLaunch p, void *hip_stream) {
    p.atoms = true;
    return pretok_launch(t, p, hip_stream);
}

int dpt_pretok_write_atoms(const dpt_pretok *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str,
                           const int32_t *pre_status, uint8_t *out_text, const uint64_t *out_off, uint8_t *cut_mask,
                           void *hip_stream) {
    return split_call(p, "null pretok", pretok_launch_atoms, true, text, str_off, n_str, nullptr, const_cast<int32_t *>(pre_status),
                      out_text, out_off, cut_mask, hip_stream);
}

}  // extern "C"
