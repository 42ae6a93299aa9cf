// Internal interface between the C-ABI (dpt_api.cpp), the host table builders (dpt_vocab.cpp, dpt_detok.cpp,
// dpt_pretok.cpp, dpt_bytelevel.cpp, dpt_bpe.cpp) and the kernels (the dpt_kernels.hip unit -- that file with
// dpt_long.hip and dpt_tok_*.h -- and dpt_spans.hip, dpt_decode.hip, dpt_collate.hip, dpt_pretok.hip,
// dpt_bytelevel.hip, dpt_bpe.hip, dpt_words.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dpt.h"
#include "dpt_bpe_table.h"
#include "dpt_lean_hint.h"

namespace dpt {

// window bytes of the windowed passes
constexpr int SMALL_CH = 256;   // the first pass's window
constexpr int MID_CH = 512;     // the 512-byte pass's (PRESPLIT / ATOMS calls of 16-lane vocabularies)
constexpr int BIG_CH = 2048;    // the 2048-byte pass's

// The first 64 bytes of the counter block (CTR_ALLOC_BYTES; from byte PART_CTR_OFFSET the first pass's
// partition counters and their used-up mask).  Zeroed once at allocation, then reset for the next call
// (reset_counters, dpt_kernels.hip) by the batch scan or the finish pass -- or, in a one-string host-path
// call, by the lone wave of the first pass.  The host path reads these 64 bytes back (EncodeLaunch::ctr_snap).
struct CounterBlock {
    uint32_t retry_count;       // strings on the 2048-byte pass's list (first pass); the 512-byte pass's input
    uint32_t big_done;          // 2048-byte blocks done (fallback_kernel)
    uint32_t big_work;          // the 2048-byte pass's work counter
    uint32_t long_count;        // strings on the unbounded pass's list
    uint32_t long_work;         // the unbounded pass's work counter
    uint32_t mid_work;          // the 512-byte pass's work counter (mid_kernel)
    uint32_t ticket;            // fallback_kernel's block ticket
    uint32_t mid_retry_count;   // the 2048-byte pass's list count when the 512-byte pass ran
    uint64_t arena_used;        // the unbounded pass's claimed arena bytes
    uint64_t last_need;         // ... of the last call (dpt_ctx_long_need)
    uint64_t far_pairs;         // far edge pairs found
    uint64_t last_far;          // ... by the last call (dpt_dp_host_far)
};
// (the kernels address the block, partition counters included, as uint32 words)
inline uint32_t *ctr_words(CounterBlock *c) { return reinterpret_cast<uint32_t *>(c); }
static_assert(sizeof(CounterBlock) == 64, "counter block");
static_assert(offsetof(CounterBlock, last_need) == 40 && offsetof(CounterBlock, last_far) == 56, "host read-back");

// EncodeLaunch::retry_list holds three lists of up to n_str string indices each
enum RetryList {
    LIST_BIG = 0,             // the 2048-byte pass's, filled by the first pass (the 512-byte pass's input when it runs)
    LIST_LONG = 1,            // the unbounded pass's
    LIST_BIG_AFTER_MID = 2,   // the 2048-byte pass's when the 512-byte pass ran: what that pass could not hold
    N_RETRY_LISTS = 3
};

struct EncodeLaunch {
    int mode;                // DPT_MODE_* | DPT_FLAG_*
    uint64_t *edges;         // nullable: per atom end E(i)&reachable masks (n_bytes entries)
    uint64_t *far;           // nullable (with edges): optimal predecessors more than 64 atoms back, as
    uint64_t far_cap;        //   (end index, back distance) pairs -- far_cap pairs; the count is in the counter block
    const uint8_t *text;
    const uint64_t *str_off;
    const uint8_t *cut_mask;
    uint64_t n_str;
    int32_t *ids;
    uint64_t *id_off;
    int32_t *status;
    int32_t *capped;
    // workspace
    int32_t *staging;
    int16_t *staging16;      // non-null: ids staged as int16 here instead (every vocabulary id in 0..32767)
    uint64_t *counts;
    uint32_t *retry_list;    // N_RETRY_LISTS x n_str string indices (retry_list_of below)
    CounterBlock *ctr;       // the counter block (CTR_ALLOC_BYTES)
    uint8_t *wsl_scratch;    // max_blocks x wsl_scratch_bytes(1) bytes
    int long_span;           // vocabulary tokens longer than 64 code points: words over 64 atoms -> unbounded pass
    uint32_t max_tok_bytes;  // longest vocabulary token, bytes
    unsigned long long *flags;   // the batch lines (BS_LINE below): per FIN_BATCH-string batch, the sum of its counts,
                                 //   added by the tokenize passes as strings finish; zeroed for the next call
    unsigned long long *bpre;    // per batch (dense): its exclusive id prefix (batch_scan_kernel)
    unsigned long long *zero_other;   // fold calls: the other parity's batch lines, zeroed for the next call ...
    uint64_t zero_n;             // ... (batches)
    uint64_t *ctr_snap;          // nullable (host path): the counter block's first 64 bytes, copied here by its reset
    bool no_fallback;            // the host checked that no string needs the 2048-byte or unbounded pass: skip them
    uint64_t n_bytes = 0;        // the call's input bytes
    bool solo;                   // one-string host-path call without fallbacks, histogram, edges or profiling: the first
                                 //   pass writes the CSR arrays itself (ids at 0.., id_off = {0, count}) and resets
                                 //   the counter block (its snapshot to ctr_snap); nothing else is launched
    unsigned max_blocks;
    int variant;             // KERNEL_* below
    bool padded;             // dpt_encode_padded: staging = the caller's ids, counts = the caller's; no finish pass
    uint4 *pend;             // 16-lane first pass: each wave's pending residual tokens (pend_scratch_bytes)
    int64_t *hist;           // nullable: the token-count histogram to add to in the finish pass (dpt_ctx_set_histogram)
    uint32_t hist_bins;
    bool hist_overwrite;     // DPT_HIST_OVERWRITE: the call's histogram replaces hist (zeroed on the device first)
    uint8_t *arena;          // the unbounded pass's scratch: 20 bytes per input byte of the strings it takes
    uint64_t arena_cap;      // input bytes the arena holds
    uint64_t counter_bias;   // test-only (dpt_ctx_debug_counter_bias): the arena and far-pair counters start at it
    bool lean_skip = false;        // no lean launch: the context's hint is off and this is not a retry call, or the
                                   //   context's test switch (dpt_ctx_debug_no_lean)
    uint32_t *lean_mirror = nullptr;   // nullable: the pinned host word the lean kernels mirror LEAN_OFF to
    // vocabulary
    const int2 *slots;
    const int32_t *slot_ids;
    const int16_t *pair16;   // ids of the one- and two-byte tokens (PAIR16_N int16), then phase A0's byte-pair flags
                             //   + child filters (65536 uint2) -- dpt_vocab.cpp build_vocab_tables
    const int4 *slots4;      // {base | TERM<<31 | LEAF<<30, check, id, child filter}
    uint32_t n_slots;
    int32_t root_base;
    int32_t ws_node, ws_base, ws_id;   // the trie node after U+2581, its base word and id (-1: none)
};

// first-pass work partitions (dpt_kernels.hip, TokPass::body): up to NPART_MAX counters, one per
// PART_STRIDE uint32 (a 256-byte line each), from byte PART_CTR_OFFSET of the counter block, then the
// used-up mask; the counter block is CTR_ALLOC_BYTES long (the host path copies its first 64 bytes)
constexpr unsigned NPART_MAX = 32;
// entries of the pair-id table (65536 byte pairs + 256 single bytes, int16; a multiple of 4 so the
// A0 table after it is 8-byte aligned)
constexpr unsigned PAIR16_N = 65536 + 256;
// strings per finish batch (the batch arrays are sized one per 64 strings, two arrays)
constexpr unsigned FIN_BATCH = 256;
constexpr unsigned PART_STRIDE = 64;   // (counters 4 KB apart measured the same, r05i)
// Calls of 2..FIN_FOLD_MAX batches run no batch_scan_kernel: each finish block sums the batch sums
// before its own batch (<= FIN_FOLD_MAX / FIN_THREADS loads per thread), zeroes the OTHER array for
// the next call (the two arrays swap roles: dpt_ctx's flag parity) and block 0 resets the counter
// block.  Saves a launch (~5 us) on the strong-scaling shard sizes (125k..500k strings).
#ifndef FIN_FOLD_MAX_DEF
#define FIN_FOLD_MAX_DEF 2048   // A/B knob (both the API and the kernels must see the same value)
#endif
constexpr unsigned FIN_FOLD_MAX = FIN_FOLD_MAX_DEF;
__host__ __device__ inline bool fin_fold(uint64_t n_str) {
    const uint64_t nb = (n_str + FIN_BATCH - 1) / FIN_BATCH;
    return nb > 1 && nb <= FIN_FOLD_MAX;
}
constexpr unsigned FIN_MAX_BINS = 1024;   // histogram bins the finish pass folds in (more: the separate pass)

// Batch lines (EncodeLaunch::flags): one 128-byte line per batch, so the strings finishing in
// neighbouring batches -- the first pass's partitions run through the batches side by side -- add to
// different lines (16 batches' sums in one line serialised the adds: +0.05 ms at cfg2, +11 % at 125k
// strings, profiles/r04d_ab.log).  u64 [0]: the count sum -- one atomic add per finished string.
constexpr unsigned BS_LINE = 16;
constexpr size_t PART_CTR_OFFSET = 256;
constexpr size_t CTR_ALLOC_BYTES = PART_CTR_OFFSET + (NPART_MAX + 1) * PART_STRIDE * 4;
// The lean route's words (raw calls of 16-lane vocabularies, dpt_kernels.hip): the line after the used-up mask's
// (the first pass uses 16 partition lines and the mask's of the NPART_MAX + 1 allocated).  Zero at allocation and
// never reset between calls: they are the context's memory of its last calls' text.
constexpr unsigned LEAN_LINE = 17;
enum LeanWord {
    LEAN_OFF = 0,        // the hint: nonzero = the lean waves claim nothing.  Set by a lean wave that deferred too many of its
                         //   strings; cleared by the probe (the lean launch's first wave, when it finds the hint off: the
                         //   batch's first strings through prep and phase A, unclaimed, nothing written) when none of them
                         //   would have been deferred
    LEAN_DEFERRED = 1,   // the strings the last lean launch deferred (written by the general launch; the tests read it)
    LEAN_PROBES = 2,     // probes made so far (the tests read it)
};
static_assert(LEAN_LINE > 16 && LEAN_LINE <= NPART_MAX, "the lean words' line: past the mask's, inside the block");

// child filter bit of next byte b (slots4[].w, host and device): XOR with b >> 5 permutes the
// low five bits inside each 32-byte block, so the 26 lowercase letters get distinct bits
__host__ __device__ inline unsigned child_bit(unsigned b) { return (b ^ (b >> 5)) & 31u; }

// Token hash table (C2's one-lookup ids for tokens of 3..16 expanded bytes; build_vocab_tables puts
// it after the A0 table in the pair16 allocation).  Key: the token's bytes as four little-endian
// dwords, zero past its length, plus the length.  Buckets of two {fp, id} entries (fp != 0; 0 marks a
// free entry), two choices per key (cuckoo placement, round 5): bucket h & mask or its partner
// tokhash_alt(h & mask, fp).  The kernels load a key's home bucket first and its partner only when the
// key is not in its home bucket (one more load round for the wave, never a chain; loading both
// at once for every key measured slower on cfg2 / cfg5, round 5 r05aj, and is gone) -- a lookup never
// walks a probe chain (with linear probing 5.7 % of cfg4's hashed tokens were not in their home bucket,
// and almost every 64-token round ran the serial probe loop for some lane).  The builder checks that the first entry carrying a key's
// fp among its two buckets (in the kernel's order) is its own (else it re-seeds): a span the DP
// selected is a vocabulary token by construction (phase A matched it), so the lookup needs no key
// compare.
constexpr unsigned TOKHASH_MAX_BYTES = 16;        // the 16-lane kernels' keys (four dwords)
constexpr unsigned TOKHASH_MAX_BYTES_LONG = 64;   // the table's tokens; the 64-lane kernels hash keys this long
constexpr size_t TOKHASH_OFFSET = PAIR16_N * sizeof(int16_t) + 65536 * 8;   // bytes into the pair16 allocation
struct TokHashHeader {
    uint32_t mask;        // buckets - 1 (a power of two)
    uint32_t max_probe;   // buckets a lookup visits: 2 (its two choices); 0: no table -- the walkers resolve every token
    uint32_t seed;
    uint32_t nl_id1;      // 1 + the id of "<0x0A>" (0: none): raw mode's one-atom '\n' tokens take it without a lookup
};
// The key is max(4, ceil(len / 4)) little-endian dwords w_k of the token's bytes, zero past its
// length, mixed into one 64-bit state (lo, hi) by one 32 x 32 -> 64 multiply-add per dword (round 5;
// the two murmur/xxHash-style 32-bit chains before cost ~48 VALU per key, ~3 % of cfg4's first pass):
//   start  lo = seed ^ len, hi = seed * G;   per dword  (hi:lo) = (w_k ^ lo) * K[k] + hi;
//   end    (hi:lo) = (lo ^ C) * K[16] + hi,  h = lo ^ hi (the bucket is h & mask), fp = hi | 1.
// The product's high half mixes every bit of (w ^ lo) and is added into the next step's low half, so
// byte-level vocabularies' keys whose differences sit in the top bytes of two dwords do not cancel (a
// linear sum of w_k * K[k] mod 2^32 failed every seed on the 250,680-token BLOOM vocabulary).  (h, fp)
// carry the whole 64-bit state: a fingerprint derived from h alone (round 2) left 32 bits per key and
// ~7 full collisions among the BLOOM keys.
constexpr uint32_t TOKHASH_K[17] = {
    0xFB13EED5u, 0xE031651Bu, 0xD57B9AE9u, 0xF49344BFu, 0xB7A058D5u, 0xB4BC663Du, 0xE3606AA1u, 0x829E9285u, 0x9D183F11u,
    0xF3C85069u, 0xAEAD8A81u, 0xC9C1030Bu, 0xC71547B7u, 0xF78B48A3u, 0xB5FE207Fu, 0xEA0A7265u, 0xC71BEEC7u};
struct TokHashState {
    uint32_t lo, hi;
};
__host__ __device__ inline TokHashState tokhash_start(uint32_t len, uint32_t seed) {
    return {seed ^ len, seed * 0x9E3779B9u};
}
__host__ __device__ inline TokHashState tokhash_step(TokHashState s, uint32_t w, unsigned k) {
    const uint64_t t = (uint64_t)(w ^ s.lo) * TOKHASH_K[k] + s.hi;
    return {(uint32_t)t, (uint32_t)(t >> 32)};
}
__host__ __device__ inline void tokhash_end(TokHashState s, uint32_t &h, uint32_t &fp) {
    const uint64_t t = (uint64_t)(s.lo ^ 0x5BD1E995u) * TOKHASH_K[16] + s.hi;
    h = (uint32_t)t ^ (uint32_t)(t >> 32);
    fp = (uint32_t)(t >> 32) | 1u;
}
// the partner of bucket b for a key of fingerprint fp (an involution: from either bucket, the other)
__host__ __device__ inline uint32_t tokhash_alt(uint32_t b, uint32_t fp, uint32_t mask) { return (b ^ (fp >> 8)) & mask; }
// four-dword keys (tokens of at most 16 bytes)
__host__ __device__ inline void tokhash(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t len, uint32_t seed,
                                        uint32_t &h, uint32_t &fp) {
    TokHashState s = tokhash_start(len, seed);
    s = tokhash_step(s, w0, 0);
    s = tokhash_step(s, w1, 1);
    s = tokhash_step(s, w2, 2);
    s = tokhash_step(s, w3, 3);
    tokhash_end(s, h, fp);
}

// kernel variants for the first pass (the 2048-byte window pass always follows for retries)
constexpr int KERNEL_ROWS16 = 1;  // 4 strings per wave in 16-lane DPP rows, LDS windows (max_cp <= 16)
constexpr int KERNEL_ROWS64 = 2;  // 1 string per wave, 64-lane DPP (max_cp <= 64)

inline uint32_t *retry_list_of(const EncodeLaunch &p, RetryList which) { return p.retry_list + (uint64_t)which * p.n_str; }

// A/B knobs, read from the environment once per process (launch_knobs); each is off / at its default
// when its variable is unset
struct LaunchKnobs {
    bool generic_ps;      // DPT_GENERIC_PS: plain PRESPLIT / ATOMS calls through the runtime-mode kernels
    bool generic_raw;     // DPT_GENERIC_RAW: plain RAW calls through the generic 16-lane kernel (r06i: cfg2 +9 %, cfg4 +7 %)
    bool no_solo_wave;    // DPT_NO_SOLO_WAVE: solo calls on the four-string 16-lane kernels
    bool no_solo;         // DPT_NO_SOLO: no one-string calls at all (dpt_api.cpp)
    bool no_mid;          // DPT_NO_MID: the 512-byte pass off
    bool no_small_wpc;    // DPT_NO_SMALL_WPC: the small-call wave rule off (launch_tok)
    bool no_lean;         // DPT_NO_LEAN: plain RAW calls without the lean launch -- the general kernel alone, as before it
                          //   (per call: EncodeLaunch::lean_skip)
    int fb_big_per_cu;    // DPT_FB_BIG_PER_CU: 2048-byte blocks per CU of non-raw calls (3; <= 0: the small grid)
    int waves_per_cu;     // DPT_WAVES_PER_CU: the first pass's resident waves per CU (0: by occupancy)
};
const LaunchKnobs &launch_knobs();

hipError_t launch_encode(const EncodeLaunch &p, hipStream_t stream, hipEvent_t ev[2]);
// launch_encode's plan for p takes the lean route unless the hint or DPT_NO_LEAN says otherwise (pure: no HIP call)
bool lean_eligible(const EncodeLaunch &p);
size_t wsl_scratch_bytes(unsigned max_blocks);
size_t pend_scratch_bytes(unsigned max_blocks);
hipError_t launch_histogram(const uint64_t *id_off, const int32_t *status, uint64_t n_str, int64_t *hist,
                            uint32_t n_bins, hipStream_t stream);
// The grid of a one-wave-per-string kernel with `waves` waves to a block: a wave for every string, up to 2^20 blocks
// (more strings: the waves stride).  DPT_WAVE_GRID_BLOCKS=<n> caps it at n blocks, read per call (dpt_api.cpp; tests
// run many trips of the stride on small batches with it); unset, empty, not a number or <= 0: no cap.
unsigned wave_per_string_blocks(uint64_t n_str, unsigned waves);
// token spans of an encoded batch (dpt_spans.hip; include/dpt.h dpt_token_spans): every pointer a device pointer
struct SpansLaunch {
    int mode;
    const uint8_t *text;
    const uint64_t *str_off;
    const uint8_t *cut_mask;
    uint64_t n_str;
    const int32_t *ids;
    const uint64_t *id_off;
    const int32_t *status;
    uint32_t *tok_end;
    uint32_t *tok_word;        // nullable
    int32_t *span_status;
    const uint16_t *tok_len;   // the vocabulary's byte length per id - id_min (0: no token has this id)
    int32_t id_min;
    uint32_t n_tab;            // entries of tok_len
};
hipError_t launch_spans(const SpansLaunch &p, hipStream_t stream);
hipError_t kernel_init();

// Decode table of a vocabulary (dpt_detok.cpp build_detok_tables; include/dpt.h dpt_detok_create): what
// every id decodes to under one rule, as host bytes exactly as dpt_detok_create uploads them.
//   tab[id - id_min] = {.x = the piece's offset in blob, .y = its length in bytes (0: a skipped id or a
//   piece that decodes to nothing), or DETOK_NONE for an id no token has (.x = 0)}
//   blob = the pieces in id order, back to back
constexpr uint32_t DETOK_NONE = 0x80000000u;
struct DetokTables {
    std::vector<uint2> tab;
    std::vector<uint8_t> blob;
    int32_t id_min = 0;
    uint32_t n_tab = 0;
    uint32_t longest = 0;   // the longest decoded piece, bytes
};
// returns 0 or an error message; calls no HIP function
const char *build_detok_tables(const uint8_t *blob, const uint64_t *off, const int32_t *ids, uint32_t n, int rule,
                               const int32_t *skip_ids, uint32_t n_skip, DetokTables *out);

// One launch of the decode kernels (dpt_decode.hip; include/dpt.h dpt_decode_sizes, dpt_decode, dpt_roundtrip):
// every pointer a device pointer.
enum DecodeKind { DECODE_SIZES = 0, DECODE_BYTES = 1, DECODE_ROUNDTRIP = 2 };
struct DecodeLaunch {
    int kind;                  // DecodeKind
    int flags;                 // DPT_DECODE_*
    const int32_t *ids;
    const uint64_t *id_off;
    const int32_t *status;     // nullable: all 0
    uint64_t n_str;
    // the table
    const uint2 *tab;
    const uint8_t *blob;
    int32_t id_min;
    uint32_t n_tab;
    // DECODE_SIZES
    uint64_t *out_len;
    // DECODE_BYTES
    uint8_t *out;
    const uint64_t *out_off;
    // DECODE_ROUNDTRIP
    const uint8_t *text;
    const uint64_t *str_off;
    uint32_t *first_diff;      // nullable
    // DECODE_BYTES: dec_status, DECODE_ROUNDTRIP: rt
    int32_t *result;
};
hipError_t launch_decode(const DecodeLaunch &p, hipStream_t stream);

// The launches of the collate kernel (dpt_collate.hip; include/dpt.h dpt_collate, dpt_collate_pair): every pointer a
// device pointer, the options already checked (row_len >= the specials asked for, row_stride >= row_len, known flags).
struct CollateSide {           // one source: the ids of an encoded batch
    const int32_t *ids;
    const uint64_t *off;       // n_str + 1
    const uint64_t *counts;    // nullable: the token counts come from off
    const int32_t *status;     // nullable: all 0
};
struct CollateRows {           // the rows and the outputs every launch has
    uint64_t n_str;
    uint32_t row_len;
    uint64_t row_stride;       // elements, >= row_len
    int32_t pad_id, bos_id, eos_id, ignore_id;
    uint32_t flags;            // DPT_COLLATE_*
    void *input_ids;           // int32, or int64 with DPT_COLLATE_I64 (and every other row output)
    void *mask;                // nullable
    void *labels;              // nullable
    uint32_t *lengths;         // nullable
};
struct CollateLaunch {
    CollateSide src;
    CollateRows r;
};
hipError_t launch_collate(const CollateLaunch &p, hipStream_t stream);

struct CollatePairLaunch {     // rows of two segments
    CollateSide a, b;
    CollateRows r;
    int32_t sep_id;
    uint32_t max_a, max_b;     // per-side caps, 0: none
    void *token_type;          // nullable
    uint32_t *b_start;         // nullable
};
hipError_t launch_collate_pair(const CollatePairLaunch &p, hipStream_t stream);

// The launches of the packing kernels (dpt_packing.hip; include/dpt.h dpt_pack_sizes, dpt_pack_plan, dpt_pack_write):
// every pointer a device pointer, the arguments already checked (n_str, row_cap < 2^31, the options as collate's).
constexpr uint32_t PACK_BLOCK_STRINGS = 1024;   // B: the strings of one plan block
constexpr uint32_t PACK_GRID_CAP = 512;         // the plan's blocks at most (two of B threads per CU); more chunks: they stride
uint64_t pack_plan_workspace_bytes(uint64_t n_str);
hipError_t launch_pack_sizes(const CollateSide &src, uint32_t n_str, uint32_t room, uint32_t n_special, uint32_t *lengths, hipStream_t stream);
struct PackPlanLaunch {
    const uint64_t *tok_off;   // n_str + 1
    uint32_t n_str;
    uint32_t row_len;
    uint32_t row_cap;
    uint32_t *str_row, *str_col;       // nullable, n_str each
    uint32_t *row_first, *row_fill;    // nullable, row_cap + 1 and row_cap
    uint64_t *n_rows;
    void *ws;                  // pack_plan_workspace_bytes(n_str)
};
hipError_t launch_pack_plan(const PackPlanLaunch &p, hipStream_t stream);
struct PackWriteLaunch {
    CollateSide src;
    CollateRows r;             // (mask, lengths unused; flags: DPT_COLLATE_* and DPT_PACK_MASK_FIRST)
    const uint64_t *tok_off;   // n_str + 1
    const uint32_t *row_first; // row_cap + 1
    const uint64_t *n_rows;
    uint64_t row_cap;
    void *position_ids;        // nullable
    void *segment_ids;         // nullable
};
hipError_t launch_pack_write(const PackWriteLaunch &p, hipStream_t stream);

// One launch of the per-word comparison kernel (dpt_words.hip; include/dpt.h dpt_word_compare_sizes,
// dpt_word_compare_write): every pointer a device pointer, the arguments already checked.
struct WordsLaunch {
    bool write;                  // false: the sizes pass
    dpt_word_side a, b;
    uint64_t n_str;
    int flags;                   // DPT_WORDS_LESS | DPT_WORDS_GREATER
    // sizes
    uint32_t *n_words, *n_sel;
    uint32_t *len_a, *len_b;     // nullable
    // write
    const uint64_t *word_off;    // nullable with cnt_a / cnt_b
    uint32_t *cnt_a, *cnt_b;
    const uint64_t *sel_off;     // nullable when every sel_* is
    uint32_t *sel_str, *sel_word, *sel_begin, *sel_end;           // nullable, each
    uint32_t *sel_a_first, *sel_a_count, *sel_b_first, *sel_b_count;
    // both
    int32_t *wc_status;
};
hipError_t launch_words(const WordsLaunch &p, hipStream_t stream);

// Pre-tokenization table of a vocabulary (dpt_pretok.cpp build_pretok_tables; include/dpt.h dpt_pretok_create), as
// host bytes exactly as dpt_pretok_create uploads them.
constexpr uint32_t PRETOK_BMP_WORDS = 2048;   // the known set below U+10000, one bit per code point
struct PretokTables {
    std::vector<uint32_t> bmp;      // PRETOK_BMP_WORDS: bit cp & 31 of word cp >> 5
    std::vector<uint32_t> astral;   // the known code points from U+10000 up, ascending
    std::vector<uint8_t> lit;       // 8 uint32 (the literals' first bytes as a bitmap) | n_lit + 1 uint32 offsets | bytes
    std::vector<uint8_t> prefix;    // the BOS piece, then U+2581
    bool runs_ok = true;
    uint32_t n_known = 0, n_lit = 0, bos_len = 0;
};
// returns 0 or an error message (*code: DPT_E_ARG or DPT_E_VOCAB); calls no HIP function
const char *build_pretok_tables(const uint8_t *blob, const uint64_t *off, uint32_t n, const uint8_t *bos, uint32_t bos_len,
                                const uint8_t *lit_blob, const uint64_t *lit_off, uint32_t n_lit, PretokTables *out, int *code);

// One launch of the pre-tokenization kernels (dpt_pretok.hip; include/dpt.h dpt_pretok_sizes, dpt_pretok_write):
// every pointer a device pointer.
struct PretokLaunch {
    bool write;                  // false: the sizes pass
    bool atoms;                  // write: the mask is an ATOMS mask (dpt_pretok_write_atoms)
    const uint8_t *text;
    const uint64_t *str_off;
    uint64_t n_str;
    // the table
    const uint32_t *bmp;
    const uint32_t *astral;      // n_astral entries (null when 0)
    uint32_t n_astral;
    uint64_t lit_first[4];       // the literals' first bytes as a bitmap
    const uint32_t *lit_off;     // n_lit + 1
    const uint8_t *lit_bytes;
    uint32_t n_lit;
    const uint8_t *prefix;       // bos_len + 3 bytes
    uint32_t bos_len;
    bool runs_ok;
    uint64_t ascii_known[2];     // bmp's first four words: the known code points below U+0080
    // sizes
    uint64_t *out_len;
    int32_t *pre_status;         // written by sizes, read by write
    // write
    uint8_t *out_text;
    const uint64_t *out_off;
    uint8_t *cut_mask;
};
hipError_t launch_pretok(const PretokLaunch &p, hipStream_t stream);

// Separator table of a byte-level split (dpt_bytelevel.cpp build_bytelevel_tables; include/dpt.h dpt_bytelevel_create),
// as dpt_bytelevel_create keeps and uploads it.
struct ByteLevelTables {
    uint64_t ascii[2] = {0, 0};     // the separators below U+0080: bit cp & 63 of word cp >> 6
    std::vector<uint32_t> high;     // the separators from U+0080 up, ascending, each once
    uint32_t n_sep = 0;             // distinct separators
};
// returns 0 or an error message (DPT_E_ARG); calls no HIP function
const char *build_bytelevel_tables(const uint32_t *sep_cps, uint32_t n_sep, ByteLevelTables *out);

// One launch of the byte-level split kernels (dpt_bytelevel.hip; include/dpt.h dpt_bytelevel_sizes,
// dpt_bytelevel_write): every pointer a device pointer.
struct ByteLevelLaunch {
    bool write;                  // false: the sizes pass
    const uint8_t *text;
    const uint64_t *str_off;
    uint64_t n_str;
    // the table (read by write alone: the sizes do not depend on the separators)
    uint64_t ascii_sep[2];
    const uint32_t *high;        // n_high entries, ascending (null when 0)
    uint32_t n_high;
    // sizes
    uint64_t *out_len;
    int32_t *pre_status;         // written by sizes, read by write
    // write
    uint8_t *out_text;
    const uint64_t *out_off;
    uint8_t *cut_mask;
};
hipError_t launch_bytelevel(const ByteLevelLaunch &p, hipStream_t stream);

// Pair table of a greedy BPE merge (dpt_bpe.cpp build_bpe_tables; include/dpt.h dpt_bpe_create), as host bytes
// exactly as dpt_bpe_create uploads them (dpt_bpe_table.h has the format and the probe).
struct BpeTables {
    BpeHeader header{0, 0};
    std::vector<uint4> entries;     // 2 * header.n_buckets
};
// returns 0 or an error message (DPT_E_ARG); calls no HIP function
const char *build_bpe_tables(const int32_t *left, const int32_t *right, const int32_t *merged, const uint32_t *rank,
                             uint64_t n_pairs, BpeTables *out);

// One launch of the merge kernel (dpt_bpe.hip; include/dpt.h dpt_bpe_encode): every pointer a device pointer.
struct BpeLaunch {
    const uint8_t *text;
    const uint64_t *str_off;
    const uint8_t *cut_mask;
    uint64_t n_str;
    int32_t *ids;
    uint64_t *counts;
    int32_t *status;
    uint32_t *tok_word;          // nullable
    // the pair table
    const uint4 *entries;
    BpeHeader header;
    // the vocabulary's trie (slots4: {base | TERM | LEAF, check, id, child filter})
    const int4 *slots4;
    uint32_t n_slots;
    int32_t root_base;
};
hipError_t launch_bpe(const BpeLaunch &p, hipStream_t stream);

// host double-array trie over token bytes (dpt_vocab.cpp)
struct DoubleArray {
    // slot t: base[t] (| TERM bit 31 when a token ends here, | LEAF bit 30 when no child), check[t] = parent slot (-1 free)
    std::vector<int32_t> base, check, id;   // stats.n_slots each
    dpt_vocab_stats stats{};                // n_tokens, n_nodes, n_slots, max_bytes, max_cp
    int32_t root_base = 0;
};

// returns 0 or an error message
const char *build_double_array(const uint8_t *blob, const uint64_t *off, const int32_t *ids, uint32_t n,
                               DoubleArray *out);

// What the kernels need to know of a vocabulary besides its tables (dpt_vocab holds a copy).
struct VocabScalars {
    int32_t root_base = 0;
    int32_t ws_node = -1, ws_base = 0, ws_id = -1;   // the trie node after U+2581 (-1: no such path)
    bool ids16 = false;               // every id in 0..32767: ids are staged as int16 (half the staging traffic)
    uint32_t hash_buckets = 0, hash_probe = 0;   // C2's token hash table (0: none)
    int32_t id_min = 0;               // tok_len's first id
    uint32_t n_tab = 0;               // its entries (0: no table)
    dpt_vocab_stats stats{};
};
// Every device table of a vocabulary as host bytes, exactly as dpt_vocab_create uploads them
// (build_vocab_tables, dpt_vocab.cpp; the formats are described there).
struct VocabTables : VocabScalars {
    std::vector<int2> slots;          // n_slots {base, check}, then the two-byte root table (65536 entries)
    std::vector<int32_t> slot_ids;    // n_slots
    std::vector<int4> slots4;         // {base, check, id, child filter} per slot, then the root table again
    std::vector<uint8_t> pair;        // pair16 (PAIR16_N int16) | a0 (65536 uint2) | from TOKHASH_OFFSET: hash header + buckets
    std::vector<uint16_t> tok_len;    // byte length per id - id_min; empty: no dense table (the spans calls: DPT_E_VOCAB)
};
// returns 0 or an error message; calls no HIP function
const char *build_vocab_tables(const uint8_t *blob, const uint64_t *off, const int32_t *ids, uint32_t n, VocabTables *out);
void set_last_error(const std::string &msg);   // (dpt_api.cpp)

// The end of every dpt_debug_*_table call, the table chosen: its size, and its bytes when `out` is given and holds them.
inline int debug_table_out(const void *src, uint64_t len, void *out, uint64_t cap, uint64_t *size) {
    *size = len;
    if (out && cap < len) return set_last_error("table does not fit"), DPT_E_CAP;
    if (out && len) memcpy(out, src, len);
    return DPT_OK;
}

}  // namespace dpt
