// dpt_vocab.cpp -- host packer: the vocabulary key set (reference
// packages/tokenizer_utils.py:53-57, `vocab = set(llama_tokenizer.get_vocab())`)
// becomes a byte-level double-array trie that the kernels walk from L2.
//
// Owns: every device table of a vocabulary as host bytes (build_vocab_tables: trie, root and byte-pair tables,
// token hash, per-id token lengths, scalars).  No HIP call: testable without a device (dpt_debug_vocab_table,
// tests/test_vocab_tables.py).  dpt_api.cpp uploads the bytes and owns the device copy.
//
//   slot t of a node reached by byte b from parent p:  t = base[p] + b, check[t] == p
//   base[t] carries bit 31 when a token ends at t (id[t] is that token's id) and bit 30 when
//   the node has no children (a walk that reaches it is over without another lookup).
//
// Placement is first-fit over free slots (a find-next-free forest with path
// compression), breadth-first from the root, so hot short prefixes sit in the
// first few KB of the table.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "dpt_internal.h"

namespace dpt {

namespace {

struct Node {
    uint32_t first_child = 0;   // 0 = none (node 0 is the root, never a child)
    uint32_t next_sibling = 0;
    int32_t id = -1;
    uint8_t label = 0;
};

struct FreeFinder {
    std::vector<uint32_t> parent;  // parent[x] = x if free, else a larger candidate
    explicit FreeFinder(size_t n) { grow(n); }
    void grow(size_t n) {
        size_t o = parent.size();
        if (n <= o) return;
        parent.resize(n);
        for (size_t i = o; i < n; i++) parent[i] = (uint32_t)i;
    }
    uint32_t find(uint32_t x) {
        grow((size_t)x + 1024);
        uint32_t r = x;
        while (parent[r] != r) {
            r = parent[r];
            grow((size_t)r + 1024);
        }
        while (parent[x] != r) {
            uint32_t nx = parent[x];
            parent[x] = r;
            x = nx;
        }
        return r;
    }
    void take(uint32_t x) {
        grow((size_t)x + 1025);
        parent[x] = x + 1;
    }
};

constexpr int32_t TERM = (int32_t)0x80000000, LEAF = 0x40000000, BASE_MASK = 0x3FFFFFFF;

// slot t ends a token (a TERM slot always carries an id >= 0: build_double_array; the root, check -2, never does)
bool is_tok(const DoubleArray &da, uint32_t t) { return da.check[t] >= 0 && (da.base[t] & TERM) && da.id[t] >= 0; }

// C2's token hash table (dpt_internal.h TokHashHeader + buckets of two {fp, id}) over the tokens of at
// most TOKHASH_MAX_BYTES_LONG bytes, as uint32 words; {0, 0, 0, 0} (max_probe 0: no table) if no seed gives
// every token an unambiguous lookup.  For a token of the last vocabulary entry of equal bytes wins,
// like the trie (build_double_array).
std::vector<uint32_t> build_token_hash(const uint8_t *blob, const uint64_t *off, const int32_t *ids, uint32_t n) {
    struct Key { uint32_t w[TOKHASH_MAX_BYTES_LONG / 4]; uint32_t len; int32_t id; };
    std::vector<Key> keys;
    keys.reserve(n);
    // entries of equal bytes: one key, the last entry's id (dict semantics, as the trie) --
    // two keys of one byte string would share a fingerprint and no seed could build the table
    std::unordered_map<std::string, size_t> seen;
    seen.reserve(n);
    for (uint32_t t = 0; t < n; t++) {
        const uint64_t len = off[t + 1] - off[t];
        if (len == 0 || len > TOKHASH_MAX_BYTES_LONG) continue;
        const int32_t id = ids ? ids[t] : (int32_t)t;
        const auto ins = seen.emplace(std::string(reinterpret_cast<const char *>(blob + (off[t] - off[0])), (size_t)len), keys.size());
        if (!ins.second) {
            keys[ins.first->second].id = id;
            continue;
        }
        Key k;
        memset(k.w, 0, sizeof(k.w));
        k.len = (uint32_t)len;
        k.id = id;
        memcpy(k.w, blob + (off[t] - off[0]), len);   // little-endian dwords, zero past the token
        keys.push_back(k);
    }
    auto khash = [](const Key &k, uint32_t seed, uint32_t &h, uint32_t &fp) {
        const unsigned nd = k.len <= 16 ? 4u : (k.len + 3u) / 4u;
        TokHashState a = tokhash_start(k.len, seed);
        for (unsigned q = 0; q < nd; q++) a = tokhash_step(a, k.w[q], q);
        tokhash_end(a, h, fp);
    };
    std::vector<uint32_t> none(4, 0u);
    if (keys.empty()) return none;
    uint32_t nb = 1;
    while (nb < keys.size()) nb <<= 1;   // buckets of two entries: load <= 1/2
    const uint32_t mask = nb - 1;
    std::vector<uint32_t> H(keys.size()), F(keys.size());
    for (uint32_t seed = 0x2545F491u, tries = 0; tries < 8; tries++, seed = seed * 0x9E3779B9u + 0x7F4A7C15u) {
        for (size_t q = 0; q < keys.size(); q++) {
            khash(keys[q], seed, H[q], F[q]);
            H[q] &= mask;
        }
        std::vector<uint32_t> tab(4 + (size_t)nb * 4, 0u);
        uint32_t *bk = tab.data() + 4;
        std::vector<int32_t> who((size_t)nb * 2, -1);   // key per entry
        auto put = [&](uint32_t b, unsigned e, int32_t q) {
            bk[4 * (size_t)b + 2 * e] = F[q];
            bk[4 * (size_t)b + 2 * e + 1] = (uint32_t)keys[q].id;
            who[2 * (size_t)b + e] = q;
        };
        // cuckoo placement: a key takes a free entry of its two buckets, else evicts one (a pseudo-random
        // walk) and the evicted key moves to its other bucket
        bool bad = false;
        uint32_t rng = seed | 1u;
        for (size_t q0 = 0; q0 < keys.size() && !bad; q0++) {
            int32_t cur = (int32_t)q0;
            uint32_t b = H[q0];
            bool placed = false;
            for (int kick = 0; kick < 2000 && !placed; kick++) {
                const uint32_t b2 = tokhash_alt(b, F[cur], mask);
                const uint32_t cand[4][2] = {{b, 0}, {b, 1}, {b2, 0}, {b2, 1}};
                for (const auto &c : cand)
                    if (!placed && who[2 * (size_t)c[0] + c[1]] < 0) { put(c[0], c[1], cur); placed = true; }
                if (placed) break;
                rng = rng * 1664525u + 1013904223u;
                const uint32_t vb = (rng >> 16) & 1u ? b2 : b;
                const unsigned ve = (rng >> 17) & 1u;
                const int32_t victim = who[2 * (size_t)vb + ve];
                put(vb, ve, cur);
                cur = victim;
                b = tokhash_alt(vb, F[cur], mask);   // the victim's other bucket
            }
            bad = !placed;
        }
        if (bad) continue;
        // every key's lookup (the first entry of its fingerprint in bucket h, then in its partner) is its own
        for (size_t q = 0; q < keys.size() && !bad; q++) {
            const uint32_t b1 = H[q], b2 = tokhash_alt(b1, F[q], mask);
            const uint32_t cand[4][2] = {{b1, 0}, {b1, 1}, {b2, 0}, {b2, 1}};
            bool found = false;
            for (const auto &c : cand) {
                if (found || bk[4 * (size_t)c[0] + 2 * c[1]] != F[q]) continue;
                found = true;
                bad = who[2 * (size_t)c[0] + c[1]] != (int32_t)q;
            }
            bad = bad || !found;
        }
        if (bad) continue;
        tab[0] = mask;
        tab[1] = 2;   // a lookup visits two buckets
        tab[2] = seed;
        return tab;
    }
    return none;
}

// dpt_token_spans' table: tab[id - id_min] = the byte length of the token with that id, 0 where no token
// has it -- over the tokens the trie holds (a later duplicate's id replaced the earlier one's there), a
// token's length being its node's depth.  False (no table) when the id range is too sparse to hold
// densely or two tokens of different length share an id.
bool build_tok_len(const DoubleArray &da, std::vector<uint16_t> &tab, int32_t &id_min) {
    int32_t lo = INT32_MAX, hi = INT32_MIN;
    uint64_t n = 0;
    for (uint32_t t = 1; t < da.stats.n_slots; t++) {
        if (!is_tok(da, t)) continue;
        lo = da.id[t] < lo ? da.id[t] : lo;
        hi = da.id[t] > hi ? da.id[t] : hi;
        n++;
    }
    if (!n) return false;
    const uint64_t span = (uint64_t)((int64_t)hi - (int64_t)lo) + 1;
    if (span > 8 * n + 65536) return false;
    tab.assign((size_t)span, (uint16_t)0);
    for (uint32_t t = 1; t < da.stats.n_slots; t++) {
        if (!is_tok(da, t)) continue;
        uint32_t depth = 0;
        for (int32_t q = (int32_t)t; q > 0; q = da.check[q]) depth++;   // (slot 0 is the root; tokens have at most 65535 bytes)
        uint16_t &e = tab[(size_t)(da.id[t] - lo)];
        if (e && e != depth) return false;
        e = (uint16_t)depth;
    }
    id_min = lo;
    return true;
}

template <typename T>
size_t bytes_of(const std::vector<T> &v) { return v.size() * sizeof(T); }

}  // namespace

const char *build_double_array(const uint8_t *blob, const uint64_t *off, const int32_t *ids, uint32_t n,
                               DoubleArray *out) {
    std::vector<Node> nodes(1);
    uint32_t max_bytes = 0, max_cp = 0, n_tok = 0;
    for (uint32_t t = 0; t < n; t++) {
        const uint8_t *p = blob + (off[t] - off[0]);
        const uint64_t len = off[t + 1] - off[t];
        if (len == 0) continue;
        if (len > 0xFFFF) return "token longer than 65535 bytes";
        uint32_t cur = 0;
        uint32_t cp = 0;
        for (uint64_t k = 0; k < len; k++) {
            const uint8_t b = p[k];
            cp += (b & 0xC0) != 0x80;
            uint32_t c = nodes[cur].first_child, prev = 0;
            while (c && nodes[c].label < b) { prev = c; c = nodes[c].next_sibling; }
            if (!c || nodes[c].label != b) {
                Node nn;
                nn.label = b;
                nn.next_sibling = c;
                nodes.push_back(nn);
                const uint32_t ni = (uint32_t)nodes.size() - 1;
                if (prev) nodes[prev].next_sibling = ni;
                else nodes[cur].first_child = ni;
                c = ni;
            }
            cur = c;
        }
        if (nodes[cur].id < 0) n_tok++;
        nodes[cur].id = ids ? ids[t] : (int32_t)t;   // later duplicates win (dict semantics)
        if (len > max_bytes) max_bytes = (uint32_t)len;
        if (cp > max_cp) max_cp = cp;
    }

    // breadth-first placement
    std::vector<int32_t> &base = out->base, &check = out->check, &tid = out->id;
    base.assign(1024, 0);
    check.assign(1024, -1);
    tid.assign(1024, -1);
    auto ensure = [&](size_t n) {
        if (n > base.size()) {
            size_t m = std::max(n, base.size() * 2);
            base.resize(m, 0);
            check.resize(m, -1);
            tid.resize(m, -1);
        }
    };
    FreeFinder ff(1 << 16);
    ff.take(0);                       // root occupies slot 0
    check[0] = -2;
    std::vector<std::pair<uint32_t, uint32_t>> queue;  // (trie node, slot)
    queue.reserve(nodes.size());
    queue.push_back({0u, 0u});
    uint32_t max_slot = 0;
    std::vector<uint8_t> labels;
    std::vector<uint32_t> kids;
    for (size_t qi = 0; qi < queue.size(); qi++) {
        const uint32_t nd = queue[qi].first, slot = queue[qi].second;
        if (nodes[nd].id >= 0) tid[slot] = nodes[nd].id;
        labels.clear();
        kids.clear();
        for (uint32_t c = nodes[nd].first_child; c; c = nodes[c].next_sibling) {
            labels.push_back(nodes[c].label);
            kids.push_back(c);
        }
        if (labels.empty()) { base[slot] = LEAF; continue; }
        // smallest b >= 0 with every b+label free
        uint32_t x = labels[0];
        uint32_t b;
        for (;;) {
            const uint32_t f = ff.find(x);
            b = f - labels[0];
            bool ok = true;
            for (size_t k = 1; k < labels.size(); k++) {
                const uint32_t t = b + labels[k];
                if (ff.find(t) != t) { ok = false; break; }
            }
            if (ok) break;
            x = f + 1;
        }
        base[slot] = (int32_t)b;
        for (size_t k = 0; k < labels.size(); k++) {
            const uint32_t t = b + labels[k];
            ff.take(t);
            ensure((size_t)t + 1);
            check[t] = (int32_t)slot;
            if (t > max_slot) max_slot = t;
            queue.push_back({kids[k], t});
        }
        if (b > 0x3FFFFF00u) return "double array too large";
    }
    // mark terminals; the arrays end 256 slots past the last node (a lookup of any byte stays inside)
    const uint32_t n_slots = max_slot + 1 + 256;
    base.resize(n_slots, 0);
    check.resize(n_slots, -1);
    tid.resize(n_slots, -1);
    for (uint32_t t = 0; t < n_slots; t++)
        if (tid[t] >= 0) base[t] |= TERM;

    out->stats.n_slots = n_slots; out->stats.n_nodes = (uint32_t)nodes.size(); out->stats.n_tokens = n_tok;
    out->stats.max_bytes = max_bytes; out->stats.max_cp = max_cp;
    out->root_base = base[0] & BASE_MASK;
    return nullptr;
}

const char *build_vocab_tables(const uint8_t *blob, const uint64_t *off, const int32_t *ids, uint32_t n, VocabTables *out) try {
    DoubleArray da;
    if (const char *err = build_double_array(blob, off, ids, n, &da)) return err;
    VocabTables &v = *out;
    const uint32_t ns = da.stats.n_slots;
    // slots, then the two-byte root table: entry b0 << 8 | b1 describes the walk from the root over
    // bytes b0 b1 -- .x = base word of the node reached (0 if none), .y = that node's slot (0 if
    // none) | 1 << 30 if b0 is a root child | 1 << 31 if b0 alone is a token.  Phase A's first
    // lookup of every walk consumes two bytes through it.
    // slots4: {base, check, id, child filter} per slot, then the root table again as
    // {.x, .y, id of the node reached (-1 if none), child filter of the node reached} -- phase A of tokenize_kernel reads only these
    // (a filter bit per possible next byte, child_bit: a walk whose next byte has no bit ends
    // without the failing lookup), and its id serves C2's one-lookup tokens of two bytes
    v.slots.resize((size_t)ns + 65536);
    v.slots4.resize((size_t)ns + 65536);
    std::vector<uint32_t> filt(ns, 0u);
    // C2's one-lookup tokens (int16 vocabularies): pair16[b0 << 8 | b1] = id of the two-byte token
    // b0 b1, pair16[65536 + b0] = id of the one-byte token b0, -1 where none -- the ids the root table
    // and the root children give (slots4), in a 128-KB int16 table whose printable-ASCII part (24 KB
    // of lines) stays in a CU's L1 where the 16-B root-table entries (144 KB) do not
    std::vector<int16_t> pair16(PAIR16_N, (int16_t)-1);
    // phase A0 (byte-parallel first lookups of pure-ASCII windows) needs only flags and the child
    // filter of the root-table entry: a0[b0 << 8 | b1] = {b0 is a root child | b0 is a token << 1 |
    // node b0 b1 exists << 2 | it ends a token << 3 | it is a leaf << 4, its child filter} -- 8 B
    // instead of the 16-B slots4 entry, so twice the entries per L1/L2 line
    std::vector<uint2> a0((size_t)65536, make_uint2(0u, 0u));
    for (uint32_t t = 0; t < ns; t++) {
        const int32_t p = da.check[t];
        if (p >= 0 && (uint32_t)p < ns) {
            const uint32_t b = t - (uint32_t)(da.base[p] & BASE_MASK);
            if (b < 256) filt[p] |= 1u << child_bit(b);
        }
    }
    for (uint32_t t = 0; t < ns; t++) {
        v.slots[t] = make_int2(da.base[t], da.check[t]);
        v.slots4[t] = make_int4(da.base[t], da.check[t], da.id[t], (int32_t)filt[t]);
    }
    for (uint32_t b0 = 0; b0 < 256; b0++) {
        const uint32_t s1 = (uint32_t)da.root_base + b0;
        const bool e1 = s1 < ns && da.check[s1] == 0;
        const bool term1 = e1 && (da.base[s1] & TERM);
        const bool leaf1 = e1 && (da.base[s1] & LEAF);
        const uint32_t base1 = e1 ? (uint32_t)(da.base[s1] & BASE_MASK) : 0u;
        for (uint32_t b1 = 0; b1 < 256; b1++) {
            const uint32_t s2 = base1 + b1;
            const bool e2 = e1 && !leaf1 && s2 < ns && da.check[s2] == (int32_t)s1;
            const uint32_t y = (e2 ? s2 : 0u) | (e1 ? 0x40000000u : 0u) | (term1 ? 0x80000000u : 0u);
            v.slots[(size_t)ns + (b0 << 8) + b1] = make_int2(e2 ? da.base[s2] : 0, (int32_t)y);
            v.slots4[(size_t)ns + (b0 << 8) + b1] = make_int4(e2 ? da.base[s2] : 0, (int32_t)y, e2 ? da.id[s2] : -1,
                                                              e2 ? (int32_t)filt[s2] : 0);
            pair16[(b0 << 8) + b1] = (int16_t)(e2 ? da.id[s2] : -1);
            a0[(b0 << 8) + b1] = make_uint2((e1 ? 1u : 0u) | (term1 ? 2u : 0u) | (e2 ? 4u : 0u) |
                                                (e2 && (da.base[s2] & TERM) ? 8u : 0u) | (e2 && (da.base[s2] & LEAF) ? 16u : 0u),
                                            e2 ? filt[s2] : 0u);
        }
        pair16[65536 + b0] = (int16_t)(e1 ? da.id[s1] : -1);
        // a raw '\n' after b0 is "<0x0A>": A0 looks (b0, '\n') up as it reads and finds (b0, '<')'s entry
        a0[(b0 << 8) + '\n'] = a0[(b0 << 8) + '<'];
    }
    // C2's token hash table (dpt_internal.h): header + buckets, after a0
    std::vector<uint32_t> th = build_token_hash(blob, off, ids, n);
    if (th[1]) {   // the header's last word: 1 + the id of "<0x0A>" (a '\n' atom's expansion; last duplicate wins), 0 = none
        for (uint32_t t = 0; t < n; t++) {
            const uint64_t o = off[t] - off[0], len = off[t + 1] - off[t];
            const int32_t id = ids ? ids[t] : (int32_t)t;
            if (len == 6 && !memcmp(blob + o, "<0x0A>", 6)) th[3] = id >= 0 ? (uint32_t)id + 1u : 0u;
        }
    }
    // one allocation, one kernel pointer (SGPRs are what the hot kernel spills): pair16, then a0, then the hash
    static_assert(PAIR16_N * sizeof(int16_t) + 65536 * sizeof(uint2) == TOKHASH_OFFSET, "pair block layout");
    v.pair.resize(TOKHASH_OFFSET + bytes_of(th));
    memcpy(v.pair.data(), pair16.data(), bytes_of(pair16));
    memcpy(v.pair.data() + bytes_of(pair16), a0.data(), bytes_of(a0));
    memcpy(v.pair.data() + TOKHASH_OFFSET, th.data(), bytes_of(th));
    v.hash_buckets = th[1] ? th[0] + 1 : 0; v.hash_probe = th[1];
    if (build_tok_len(da, v.tok_len, v.id_min)) v.n_tab = (uint32_t)v.tok_len.size();
    else v.tok_len.clear();
    v.root_base = da.root_base;
    // the node after '▁' (E2 96 81): the pending-token walks start word-start tokens there
    int32_t node = 0;
    for (uint32_t c : {0xE2u, 0x96u, 0x81u}) {
        const uint32_t t = (uint32_t)(da.base[node] & BASE_MASK) + c;
        if (t >= ns || da.check[t] != node) { node = -1; break; }
        node = (int32_t)t;
    }
    v.ws_node = node;
    v.ws_base = node >= 0 ? (da.base[node] & BASE_MASK) : 0;
    v.ws_id = node >= 0 ? da.id[node] : -1;
    v.ids16 = true;
    for (uint32_t t = 0; t < ns && v.ids16; t++) v.ids16 = !is_tok(da, t) || da.id[t] <= 32767;
    v.stats = da.stats;
    v.stats.hash_max_probe = v.hash_probe; v.stats.hash_buckets = v.hash_buckets;
    v.slot_ids = std::move(da.id);
    // (the pair block counts up to TOKHASH_OFFSET: the figure has never included the token hash)
    v.stats.device_bytes = bytes_of(v.slots) + bytes_of(v.slot_ids) + bytes_of(v.slots4) + TOKHASH_OFFSET + bytes_of(v.tok_len);
    return nullptr;
} catch (const std::bad_alloc &) {
    return "out of host memory";
}

}  // namespace dpt

extern "C" int dpt_debug_vocab_table(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok,
                                     int which, void *out, uint64_t cap, uint64_t *size) {
    auto fail = [](int code, const char *msg) { dpt::set_last_error(msg); return code; };
    if (!size || !tok_off || (!utf8_blob && n_tok && tok_off[n_tok] != tok_off[0])) return fail(DPT_E_ARG, "null argument");
    for (uint32_t t = 0; t < n_tok; t++)
        if (tok_off[t + 1] < tok_off[t]) return fail(DPT_E_ARG, "tok_off not monotone");
    dpt::VocabTables t;
    if (const char *err = dpt::build_vocab_tables(utf8_blob, tok_off, ids, n_tok, &t)) return fail(DPT_E_VOCAB, err);
    const int32_t scalars[DPT_VOCAB_SCALAR_INTS] = {
        t.root_base, t.ws_node, t.ws_base, t.ws_id, t.ids16, t.id_min, (int32_t)t.n_tab, (int32_t)t.hash_buckets,
        (int32_t)t.hash_probe, (int32_t)t.stats.n_tokens, (int32_t)t.stats.n_nodes, (int32_t)t.stats.n_slots,
        (int32_t)t.stats.max_bytes, (int32_t)t.stats.max_cp, (int32_t)(uint32_t)t.stats.device_bytes,
        (int32_t)(t.stats.device_bytes >> 32)};
    const void *src[] = {t.slots.data(), t.slot_ids.data(), t.slots4.data(), t.pair.data(), t.tok_len.data(), scalars};
    const uint64_t len[] = {dpt::bytes_of(t.slots), dpt::bytes_of(t.slot_ids), dpt::bytes_of(t.slots4), dpt::bytes_of(t.pair),
                            dpt::bytes_of(t.tok_len), sizeof(scalars)};
    if (which < 0 || which >= 6) return fail(DPT_E_ARG, "no such table");
    return dpt::debug_table_out(src[which], len[which], out, cap, size);
}
