// dpt_detok.cpp -- host builder of the decode table (include/dpt.h dpt_detok_create): what every id of a
// vocabulary decodes to under one rule -- the tokenizer's own decode (reference packages/tokenizer_utils.py:82-84,
// :176-179: llama_tokenizer.decode / bloom_tokenizer.decode), as one {offset, length} entry per id and a blob
// of decoded pieces that the kernels of dpt_decode.hip stream from L2.
//
// No HIP call: testable without a device (dpt_debug_detok_table, tests/test_detok_tables.py; tests/decode_ref.py
// restates the rules).  dpt_api.cpp uploads the bytes and owns the device copy.
#include <stdint.h>
#include <string.h>

#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "dpt_internal.h"

namespace dpt {

namespace {

// The GPT-2 / ByteLevel bytes-to-unicode alphabet, inverted: the byte of code point cp, -1 outside the
// alphabet.  The printable Latin-1 bytes 0x21..0x7E, 0xA1..0xAC and 0xAE..0xFF stand for themselves; the
// other 68 bytes are the code points 0x100.. in byte order.
struct ByteLevelAlphabet {
    int16_t byte_of[0x100 + 68];
    ByteLevelAlphabet() {
        unsigned n = 0;
        for (unsigned b = 0; b < 256; b++) {
            const bool printable = (b >= 0x21 && b <= 0x7E) || (b >= 0xA1 && b <= 0xAC) || b >= 0xAE;
            byte_of[b] = printable ? (int16_t)b : (int16_t)-1;
            if (!printable) byte_of[0x100 + n++] = (int16_t)b;
        }
    }
    int get(uint32_t cp) const { return cp < 0x100 + 68 ? byte_of[cp] : -1; }
};

bool is_hex_upper(uint8_t c) { return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'F'); }
unsigned hex_val(uint8_t c) { return c <= '9' ? c - '0' : c - 'A' + 10u; }

// One token's decoded bytes, appended to out.
void decode_piece(const uint8_t *p, size_t len, int rule, std::vector<uint8_t> &out) {
    if (rule == DPT_DETOK_SP) {
        if (len == 6 && p[0] == '<' && p[1] == '0' && p[2] == 'x' && is_hex_upper(p[3]) && is_hex_upper(p[4]) && p[5] == '>') {
            out.push_back((uint8_t)(hex_val(p[3]) * 16 + hex_val(p[4])));
            return;
        }
        for (size_t k = 0; k < len;) {
            if (k + 2 < len && p[k] == 0xE2 && p[k + 1] == 0x96 && p[k + 2] == 0x81) {   // U+2581
                out.push_back(' ');
                k += 3;
            } else {
                out.push_back(p[k++]);
            }
        }
        return;
    }
    if (rule == DPT_DETOK_BYTELEVEL) {
        static const ByteLevelAlphabet alphabet;
        // the alphabet's code points have one or two UTF-8 bytes (at most U+0143); anything else, malformed
        // bytes included, keeps the token verbatim
        const size_t mark = out.size();
        bool ok = true;
        for (size_t k = 0; k < len && ok;) {
            uint32_t cp;
            if (p[k] < 0x80) {
                cp = p[k++];
            } else if ((p[k] & 0xE0) == 0xC0 && p[k] >= 0xC2 && k + 1 < len && (p[k + 1] & 0xC0) == 0x80) {
                cp = ((uint32_t)(p[k] & 0x1F) << 6) | (p[k + 1] & 0x3F);
                k += 2;
            } else {
                ok = false;
                break;
            }
            const int b = alphabet.get(cp);
            if (b < 0) ok = false;
            else out.push_back((uint8_t)b);
        }
        if (ok) return;
        out.resize(mark);
    }
    out.insert(out.end(), p, p + len);   // DPT_DETOK_PIECES
}

}  // namespace

const char *build_detok_tables(const uint8_t *blob, const uint64_t *off, const int32_t *ids, uint32_t n, int rule,
                               const int32_t *skip_ids, uint32_t n_skip, DetokTables *out) try {
    if (rule != DPT_DETOK_PIECES && rule != DPT_DETOK_SP && rule != DPT_DETOK_BYTELEVEL) return "no such decode rule";
    // the entries that count, as in dpt_vocab_create: non-empty, and of entries with equal bytes the last
    std::unordered_map<std::string, uint32_t> last;
    last.reserve(n);
    for (uint32_t t = 0; t < n; t++) {
        const uint64_t len = off[t + 1] - off[t];
        if (len == 0) continue;
        if (len > 0xFFFF) return "token longer than 65535 bytes";
        last[std::string(reinterpret_cast<const char *>(blob + (off[t] - off[0])), (size_t)len)] = t;
    }
    auto counts = [&](uint32_t t) {
        const uint64_t len = off[t + 1] - off[t];
        if (len == 0) return false;
        return last.find(std::string(reinterpret_cast<const char *>(blob + (off[t] - off[0])), (size_t)len))->second == t;
    };
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    auto widen = [&](int32_t id) {
        lo = id < lo ? id : lo;
        hi = id > hi ? id : hi;
    };
    for (uint32_t t = 0; t < n; t++)
        if (counts(t)) widen(ids ? ids[t] : (int32_t)t);
    for (uint32_t k = 0; k < n_skip; k++) widen(skip_ids[k]);
    if (lo > hi) return "no tokens";
    const uint64_t span = (uint64_t)(hi - lo) + 1;
    if (span > 8 * (uint64_t)last.size() + 65536) return "ids too sparse for a dense decode table";
    // the token of every id: of two tokens on one id the later wins; a skipped id has none to decode
    std::vector<int64_t> tok_of((size_t)span, -1);
    for (uint32_t t = 0; t < n; t++)
        if (counts(t)) tok_of[(size_t)((ids ? ids[t] : (int32_t)t) - lo)] = t;
    std::vector<uint8_t> skipped((size_t)span, 0);
    for (uint32_t k = 0; k < n_skip; k++) skipped[(size_t)(skip_ids[k] - lo)] = 1;
    DetokTables &d = *out;
    d.tab.assign((size_t)span, make_uint2(0u, DETOK_NONE));
    d.blob.clear();
    d.longest = 0;
    for (uint64_t i = 0; i < span; i++) {
        if (skipped[i]) {
            d.tab[i] = make_uint2((uint32_t)d.blob.size(), 0u);
            continue;
        }
        if (tok_of[i] < 0) continue;
        const size_t start = d.blob.size();
        decode_piece(blob + (off[tok_of[i]] - off[0]), (size_t)(off[tok_of[i] + 1] - off[tok_of[i]]), rule, d.blob);
        if (d.blob.size() >= (1ull << 32)) return "decoded pieces of 4 GiB or more";
        const uint32_t len = (uint32_t)(d.blob.size() - start);   // (never longer than the token: at most 65535)
        d.tab[i] = make_uint2((uint32_t)start, len);
        if (len > d.longest) d.longest = len;
    }
    d.id_min = (int32_t)lo;
    d.n_tab = (uint32_t)span;
    return nullptr;
} catch (const std::bad_alloc &) {
    return "out of host memory";
}

}  // namespace dpt

extern "C" int dpt_debug_detok_table(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok,
                                     int rule, const int32_t *skip_ids, uint32_t n_skip, int which, void *out, uint64_t cap,
                                     uint64_t *size) {
    auto fail = [](int code, const char *msg) { dpt::set_last_error(msg); return code; };
    if (!size || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0]) || (n_skip && !skip_ids))
        return fail(DPT_E_ARG, "null argument");
    for (uint32_t t = 0; t < n_tok; t++)
        if (tok_off[t + 1] < tok_off[t]) return fail(DPT_E_ARG, "tok_off not monotone");
    if (rule < DPT_DETOK_PIECES || rule > DPT_DETOK_BYTELEVEL) return fail(DPT_E_ARG, "no such decode rule");
    dpt::DetokTables t;
    if (const char *err = dpt::build_detok_tables(utf8_blob, tok_off, ids, n_tok, rule, skip_ids, n_skip, &t)) return fail(DPT_E_VOCAB, err);
    const int64_t scalars[DPT_DETOK_SCALAR_INTS] = {t.id_min, t.n_tab, (int64_t)t.blob.size(), t.longest};
    const void *src[] = {t.tab.data(), t.blob.data(), scalars};
    const uint64_t len[] = {t.tab.size() * sizeof(uint2), t.blob.size(), sizeof(scalars)};
    if (which < 0 || which >= 3) return fail(DPT_E_ARG, "no such table");
    return dpt::debug_table_out(src[which], len[which], out, cap, size);
}
