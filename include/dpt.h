/*
 * dpt.h -- C-ABI of the MI355X shortest-tokenization engine (libdpt.so).
 *
 * Drop-in boundary for the reference's DP segmentation path.  The reference has
 * no FFI (pure Python); these entry points are what its Python
 * call surface binds through ctypes (dp-tokenization_amd/dptok/_lib.py):
 *
 *   dpt_vocab_create  <- dp_tokenize_llama's vocabulary capture,
 *                        reference packages/tokenizer_utils.py:53-57
 *                        (t2i = get_vocab(); vocab = set(t2i))
 *   dpt_encode        <- the dp_tokenize closure's per-word loop,
 *                        reference packages/tokenizer_utils.py:66-80, which calls
 *                        compute_shortest_tokenizations (packages/dp_tokenize.py:6-70)
 *                        and obtain_longest_token (packages/dp_tokenize.py:72-84)
 *                        for every word produced by pretokenize_raw
 *                        (packages/tokenizer_utils.py:33-50, DPT_MODE_RAW) or by
 *                        pretokenize_with_llama + merge_tokens
 *                        (packages/tokenizer_utils.py:7-31, DPT_MODE_PRESPLIT)
 *   dpt_pretok_sizes, dpt_pretok_write <- pretokenize_with_llama + merge_tokens themselves
 *                        (packages/tokenizer_utils.py:7-31) for the strings whose words are a per-character
 *                        function of the text: DPT_MODE_PRESPLIT input made on the device
 *   dpt_bytelevel_sizes, dpt_bytelevel_write <- the BLOOM adapter's pre_tokenize_str + per-character atoms
 *                        (packages/tokenizer_utils.py:155-162): DPT_MODE_ATOMS input made on the device
 *   dpt_bpe_encode     <- the other side of both drivers' comparison, the tokenizer's own ids:
 *                        len(llama_tokenizer.encode(x)), reference main_analyze_s2orc.py:272, :282, and
 *                        len(bloom_tokenizer.encode(x)), main_biomed_translation.py:74 (dpt_pretok_write_atoms or
 *                        dpt_bytelevel_write make its input)
 *   dpt_token_histogram <- the length comparison of the S2ORC probe,
 *                        reference main_analyze_s2orc.py:269-297 (len(dp_tokenize(x)))
 *   dpt_token_spans    <- the probe's per-word comparison, reference main_analyze_s2orc.py:275-290
 *                        (dp_tokenize on every pre-token, to tell which words the DP shortened)
 *   dpt_decode, dpt_roundtrip <- the decode_dp_tokenization closure, reference packages/tokenizer_utils.py:82-84,
 *                        :176-179, and the caller's round-trip assert, main_analyze_s2orc.py:84-87
 *   dpt_collate        <- llama_preprocessing_function's model inputs, reference main_analyze_s2orc.py:61-93
 *                        (input_ids, attention_mask = [1] * len(ids), truncation; the collator's padding)
 *   dpt_collate_pair   <- the BLOOM translation driver's model inputs, reference main_biomed_translation.py:138-145
 *                        (a source and a target per example) and :104-124 (the collator: source ids + target ids,
 *                        right-padded, returned as input_ids and labels)
 *   dpt_hist_allreduce <- SURVEY.md §8(b)/(e): the one collective of a sharded corpus (the
 *                        reference is single-process, llama_s2orc.sh:10; no call site there)
 *
 * Conventions: plain pointers and sizes, no C++ exceptions cross this boundary,
 * every function returns an int (0 = DPT_OK, < 0 = error; message in
 * dpt_last_error(), thread-local).  Device-pointer calls are stream-ordered and
 * never synchronise.  A dpt_vocab is immutable after creation and may be shared
 * by threads and streams; a dpt_ctx (workspace) must be used by one stream at a
 * time.
 */
#ifndef DPT_H
#define DPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPT_ABI_VERSION 6

/* return codes */
#define DPT_OK 0
#define DPT_E_ARG (-1)      /* bad argument (null pointer, size) */
#define DPT_E_HIP (-2)      /* HIP runtime error */
#define DPT_E_VOCAB (-3)    /* vocabulary not supported (e.g. a token longer than 65535 bytes) */
#define DPT_E_CAP (-4)      /* output capacity too small */
#define DPT_E_NODEV (-5)    /* no HIP device */
#define DPT_E_RCCL (-6)     /* RCCL missing (librccl.so.1 not loadable) or an RCCL call failed (ABI 6) */

/* modes (low 4 bits) */
#define DPT_MODE_RAW 0      /* pretokenize_raw semantics (tokenizer_utils.py:33-50) */
#define DPT_MODE_PRESPLIT 1 /* words start where cut_mask != 0; atoms = code points (llama mode) */
#define DPT_MODE_ATOMS 2    /* caller-defined atoms: cut_mask bit 1 = an atom starts, bit 0 = a word
                               starts (compute_shortest_tokenizations over an arbitrary atom list) */
#define DPT_MODE_MASK 0x0F
/* flags (dpt_dp_host only) */
#define DPT_FLAG_UNCAPPED 0x10 /* inf-initialised DP (inspect_tokenizer.py:77-86): lengths only */
#define DPT_FLAG_LEN_ONLY 0x20 /* capped DP lengths (dp_tokenize.py:70 len_dp[-1]), no ids */

/* per-string status (the reference's exceptions) */
#define DPT_STATUS_OK 0
#define DPT_STATUS_NO_TOKENIZATION 1 /* reference: ipdb.set_trace / ValueError (dp_tokenize.py:84) */
#define DPT_STATUS_EMPTY_WORD 2      /* reference: IndexError (dp_tokenize.py:49) */
#define DPT_STATUS_TOO_LONG 3        /* words, atoms and tokens of any length are exact (the windowed kernels
                                        hand what they cannot hold to the unbounded pass); dpt_encode returns
                                        3 only for a string the unbounded pass's arena could not hold in that
                                        call (dpt_ctx_long_need / dpt_ctx_reserve_vocab); dpt_encode_host and
                                        dpt_dp_host grow the arena and rerun, so they never do */
#define DPT_STATUS_INTERNAL 4        /* engine invariant violated (never expected) */
/* (5 = DPT_RT_DIFFERS, dpt_roundtrip's rt; 6 = DPT_PRETOK_NEEDS_HOST, dpt_pretok_sizes' pre_status) */

typedef struct dpt_vocab dpt_vocab;
typedef struct dpt_ctx dpt_ctx;

typedef struct {
    uint32_t n_tokens;     /* entries accepted (non-empty, duplicates collapsed) */
    uint32_t n_nodes;      /* byte-trie nodes */
    uint32_t n_slots;      /* double-array slots (incl. 256 padding) */
    uint32_t max_bytes;    /* longest token, UTF-8 bytes */
    uint32_t max_cp;       /* longest token, code points */
    uint64_t device_bytes; /* device memory held by the vocab */
    uint32_t hash_max_probe;   /* C2's token hash table (ABI 2): buckets a lookup may visit (2: a key's
                                  two choices, round 5); 0 = no table (every selected token is then
                                  re-walked in the trie) */
    uint32_t hash_buckets;     /* its buckets of two entries (0 = no table) */
} dpt_vocab_stats;

const char *dpt_last_error(void);
int dpt_abi_version(void);

/*
 * Build a vocabulary from n_tok UTF-8 strings: token t is
 * utf8_blob[tok_off[t] .. tok_off[t+1]), its id is ids[t] (or t if ids == NULL).
 * Later duplicates win (dict semantics); empty strings are ignored.  The library
 * copies everything, builds a byte double-array trie on the host and uploads it
 * to `device`.
 */
int dpt_vocab_create(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids,
                     uint32_t n_tok, int device, dpt_vocab **out);
int dpt_vocab_destroy(dpt_vocab *v);
int dpt_vocab_stats_get(const dpt_vocab *v, dpt_vocab_stats *out);

/* Workspace on `device` (grows on demand; after dpt_ctx_reserve* a call of at most the reserved size
 * allocates nothing and does not synchronise).  NOT capture-safe: dpt_encode keeps host state in step
 * with every call (which of two batch-sum regions a call of 257..524288 strings uses, the armed
 * histogram, profiling events), and a replayed graph does not see the host -- its second launch would
 * write wrong id_off and misplaced ids.  Do not record dpt_encode / dpt_encode_padded into a HIP graph
 * (hipStreamBeginCapture, torch.cuda.graph); DESIGN.md section 8 has the details.
 * Device-path workspace per call of n_bytes / n_str: the staged ids (2 bytes per input byte when
 * every vocabulary id is in 0..32767, else 4), 16 bytes per string, and the unbounded pass's arena
 * (20 bytes per input byte it holds; by default max(4 MiB, n_bytes/32) input bytes, at most n_bytes). */
int dpt_ctx_create(int device, dpt_ctx **out);
int dpt_ctx_destroy(dpt_ctx *c);
int dpt_ctx_reserve(dpt_ctx *c, uint64_t n_bytes, uint64_t n_str);   /* both staging widths */
/* Reserve for vocabulary v's staging width (v may be NULL: both) and an unbounded-pass arena holding
 * long_bytes input bytes of long-word strings per call (0: the default above; n_bytes: every string). */
int dpt_ctx_reserve_vocab(dpt_ctx *c, const dpt_vocab *v, uint64_t n_bytes, uint64_t n_str, uint64_t long_bytes);
/* Device bytes held: the device-path workspace and the host path's staging buffers. */
int dpt_ctx_workspace_bytes(const dpt_ctx *c, uint64_t *device_path, uint64_t *host_path);
/* After the ctx's last dpt_encode has completed (synchronise its stream first): the input bytes of the
 * strings its unbounded pass took (*need) and the arena's capacity (*cap).  need > cap: the strings that
 * did not fit have status DPT_STATUS_TOO_LONG -- reserve long_bytes >= need and call again. */
int dpt_ctx_long_need(dpt_ctx *c, uint64_t *need, uint64_t *cap);

/*
 * Tokenize n_str strings, CSR-packed: string s is text[str_off[s]-str_off[0] .. str_off[s+1]-str_off[0]),
 * n_bytes = str_off[n_str] - str_off[0] (passed explicitly so the host never reads device memory).
 * ALL pointers are DEVICE pointers on the ctx's device.  Outputs:
 *   ids[id_off[s] .. id_off[s+1])  token ids of string s (none when status[s] != 0)
 *   id_off[0..n_str]               id_off[0] = 0
 *   status[s]                      DPT_STATUS_*
 *   capped_len[s] (nullable)       sum over words of the reference's len_dp[-1] (dp_tokenize.py:70), -1 if unknown
 * ids_cap must be >= n_bytes (a string never yields more ids than bytes).
 * cut_mask (n_bytes bytes, PRESPLIT and ATOMS only): PRESPLIT: != 0 where a word starts (byte 0 of
 * every string always starts one); ATOMS: bit 1 where an atom starts, bit 0 where a word starts.
 * str_off must be monotone (str_off[s] <= str_off[s+1]) and every string < 4 GiB: the device path
 * cannot check device-resident offsets (an offset that goes backwards reads past the text);
 * dpt_encode_host / dpt_dp_host check both and fail with DPT_E_ARG.
 * Limits: every string < 4 GiB, n_str < 2^31; RAW / PRESPLIT text is UTF-8 (code points are the
 * atoms).  No limit on word, atom or token length: words over 256 bytes take a 2048-byte window
 * pass, longer words (and atoms over 8 bytes, or words over 64 atoms when the vocabulary has
 * tokens over 64 code points) an unbounded one-wave-per-string pass (dpt_long.hip).
 * Stream-ordered on hip_stream (hipStream_t, NULL = default stream); no host synchronisation.
 */
int dpt_encode(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
               const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids,
               uint64_t ids_cap, uint64_t *id_off, int32_t *status, int32_t *capped_len,
               void *hip_stream);

/*
 * dpt_encode without the CSR packing: the ids of string s stay at the string's own byte offset,
 * ids[str_off[s]-str_off[0] + k] for k < counts[s] (uint64 per string; 0 when status[s] != 0) --
 * the layout the tokenize passes write, so the finish pass (offsets + compaction, about 11 % of a
 * cfg2 call) does not run.  For callers that consume per-string id lists -- the dp_tokenize
 * closure's List[int] per string (reference packages/tokenizer_utils.py:66-80) -- rather than
 * one packed array.  Same arguments, limits and stream semantics as dpt_encode; ids_cap >= n_bytes.
 */
int dpt_encode_padded(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                      const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids,
                      uint64_t ids_cap, uint64_t *counts, int32_t *status, int32_t *capped_len,
                      void *hip_stream);

/* Same with HOST pointers: copies in, runs, copies out, synchronises. */
int dpt_encode_host(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                    const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids,
                    uint64_t ids_cap, uint64_t *id_off, int32_t *status, int32_t *capped_len);

/*
 * DP by-products without ids (HOST pointers; synchronises).  mode_flags = DPT_MODE_* |
 * DPT_FLAG_LEN_ONLY (capped len_dp[-1] per string, summed over words) or DPT_FLAG_UNCAPPED
 * (minimum token count, 65535 per word that has no tokenization).  status[s] as dpt_encode.
 * edges (nullable, n_bytes entries): for string s and atom end i (1-based atom index within
 * the string) edges[str_off[s]-str_off[0] + i - 1] has bit d set iff atom i-1-d .. i-1 is a
 * token, cost[i-1-d] + 1 == cost[i] and i-1-d is reachable -- the reference's
 * segment_index_dp[i-1] restricted to reachable starts (dp_tokenize.py:40-46), from which the
 * host enumerates every shortest tokenization in the reference's DFS order.  Reachable: a path of
 * tokens leads from the word's start to the atom boundary (the start itself is), under the capped and
 * the uncapped DP alike; cost is the DP's own (capped: min(atoms since the word's start, ...)), so
 * an unreachable end has an empty mask, and under the cap a reachable start may appear whose capped
 * cost no path attains -- a dead end for the walk, as in the reference.  Entries of edges that are no
 * atom end of a string (the tail of a string whose atoms have several bytes, a string of status 2) are
 * unspecified.
 */
int dpt_dp_host(dpt_ctx *c, const dpt_vocab *v, int mode_flags, const uint8_t *text, uint64_t n_bytes,
                const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *status,
                int32_t *lengths, uint64_t *edges);
/*
 * dpt_dp_host with edges, without the 64-atom limit of the masks: an optimal reachable predecessor
 * more than 64 atoms back (a token of more than 64 atoms -- vocabularies with tokens of more than 64
 * code points) is listed in far[] as the pair far[2k] = the edges[] index of the end (str_off[s] -
 * str_off[0] + i - 1), far[2k+1] = the back distance d >= 64 (start i-1-d), in no particular order,
 * instead of status 3.  far_cap counts pairs; *n_far = the pairs found.  Returns DPT_E_CAP (and the
 * needed *n_far) when they do not fit: call again with far_cap >= *n_far.  Replaces the status 3 of
 * reference dp_tokenize.py:40-46's unbounded segment_index_dp (no span limit there).
 */
int dpt_dp_host_far(dpt_ctx *c, const dpt_vocab *v, int mode_flags, const uint8_t *text, uint64_t n_bytes,
                    const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *status,
                    int32_t *lengths, uint64_t *edges, uint64_t *far, uint64_t far_cap, uint64_t *n_far);

/*
 * Token-count histogram (device pointers): hist[0..n_bins) counts strings by
 * #ids (last bin = overflow), then hist[n_bins+0] = total ids, hist[n_bins+1] =
 * total strings, hist[n_bins+2+k] = strings with status k (k = 0..4).
 * hist must hold n_bins + 8 int64 and is ACCUMULATED into (zero it first).  2 <= n_bins <= DPT_HIST_MAX_BINS
 * (the bins are counted in LDS).
 */
#define DPT_HIST_MAX_BINS 16384
int dpt_token_histogram(const uint64_t *id_off, const int32_t *status, uint64_t n_str,
                        int64_t *hist, uint32_t n_bins, void *hip_stream);

/*
 * Token byte spans and word indices of an encoded batch: which part of the input each id covers -- the
 * offset_mapping / word_ids of the tokenizers the reference sits beside, and what the S2ORC probe's
 * per-word comparison (reference main_analyze_s2orc.py:269-293) re-tokenizes every word for.
 * Added within ABI 6 (DPT_ABI_VERSION unchanged): a binding that may meet an older libdpt.so probes for
 * the symbol.
 *
 * text, n_bytes, str_off, cut_mask, n_str and mode are dpt_encode's arguments (same conventions:
 * str_off[0] need not be 0, text and cut_mask correspond to str_off[0], no alignment needed); ids,
 * id_off and status are what dpt_encode wrote for them.  Token k of string s is
 * ids[id_off[s] - id_off[0] + k]; tok_end and tok_word (nullable) use the same index.  Per string s:
 *   span_status[s] = status[s] when status[s] != 0 (nothing else is written for s); else 0 and
 *   tok_end[k]   the byte offset within the string, in the caller's text, where token k ends (token k
 *                starts at tok_end[k-1], token 0 at 0; the last token ends at the string's length)
 *   tok_word[k]  the 0-based index, within the string, of the word token k lies in.  A word starts at
 *                offset 0 and -- RAW -- at every ' ' after offset 0, -- PRESPLIT -- where cut_mask != 0,
 *                -- ATOMS -- where cut_mask & 1
 * A DP tokenization tiles the atom-expanded string, so the ends follow from the ids' byte lengths: with
 * E_k the summed length of tokens 0..k, tok_end[k] is the offset p whose expanded offset x(p) is E_k --
 * x(p) = p in PRESPLIT / ATOMS; RAW: x(0) = 0, x(p) = 3 + p + 2 * (the ' ' in [1, p)) + 5 * (the '\n' in
 * [1, p)) (pretokenize_raw, reference tokenizer_utils.py:33-50: byte 0 literal behind the word mark).
 * Ids that do not tile their string -- an id no token has, an E_k no offset attains, a last E_k that is
 * not x(length) -- give span_status[s] = DPT_STATUS_INTERNAL and unspecified tok_end / tok_word for s
 * alone; every store stays inside the string's own [id_off[s], id_off[s+1]) whatever the ids hold.
 * Strings < 4 GiB, str_off and id_off monotone (dpt_token_spans cannot check device-resident offsets).
 * DPT_E_VOCAB for a vocabulary without a dense per-id length table: ids spread over more than
 * 8 * n_tokens + 65536 values, or two tokens of different byte length on one id.
 *
 * dpt_token_spans: DEVICE pointers on the vocabulary's device; stream-ordered on hip_stream, never
 * synchronises, allocates nothing and needs no dpt_ctx: any number of calls may be in flight on one vocab.
 */
int dpt_token_spans(const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes, const uint64_t *str_off,
                    const uint8_t *cut_mask, uint64_t n_str, const int32_t *ids, const uint64_t *id_off,
                    const int32_t *status, uint32_t *tok_end, uint32_t *tok_word, int32_t *span_status, void *hip_stream);
/* Same with HOST pointers: copies in through the ctx's host-path staging (grows on demand), runs, copies
 * out, synchronises.  Checks that both offset arrays are monotone and every string is under 4 GiB. */
int dpt_token_spans_host(dpt_ctx *c, const dpt_vocab *v, int mode, const uint8_t *text, uint64_t n_bytes,
                         const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, const int32_t *ids,
                         const uint64_t *id_off, const int32_t *status, uint32_t *tok_end, uint32_t *tok_word,
                         int32_t *span_status);

/*
 * Decode: ids back to bytes, and the round-trip check of an encoded batch -- the second closure of the
 * reference's factories, decode_dp_tokenization (reference packages/tokenizer_utils.py:82-84, :176-179: the
 * tokenizer's own decode), and the assert its caller runs on every example, decode_dp_tokenization(
 * dp_tokenize(abstract)) == abstract (reference main_analyze_s2orc.py:84-87).  Added within ABI 6
 * (DPT_ABI_VERSION unchanged): a binding that may meet an older libdpt.so probes for the symbols.
 *
 * A dpt_detok is the decode table of a vocabulary under one rule: what every id decodes to.  It is built
 * from dpt_vocab_create's first four arguments (later duplicates win, empty strings are ignored, as there;
 * of two tokens on one id the later one wins), a rule and the ids that decode to nothing:
 *   DPT_DETOK_PIECES     the token's bytes as they are: a string's decode is its atom-expanded text, for
 *                        PRESPLIT / ATOMS ids exactly the text that was encoded
 *   DPT_DETOK_SP         SentencePiece's decode: every U+2581 (E2 96 81) becomes ' '; a token that is exactly
 *                        <0xNN> (6 bytes, two upper-case hex digits) becomes the byte NN.  The output is
 *                        bytes: no UTF-8 validation or repair
 *   DPT_DETOK_BYTELEVEL  every code point of the token goes back through the GPT-2 / ByteLevel
 *                        bytes-to-unicode alphabet (256 code points: the printable Latin-1 bytes 21..7E,
 *                        A1..AC, AE..FF stand for themselves, the other 68 bytes are U+0100.. in byte
 *                        order); a token with a code point outside the alphabet keeps its UTF-8 bytes
 *   skip_ids[0..n_skip)  decode to nothing under every rule (BOS and the like)
 * DPT_E_VOCAB when the ids (skip ids included) are spread over more than 8 * n_tokens + 65536 values: the
 * table is dense, one 8-byte entry per id.  Immutable after creation; may be shared by threads and streams.
 *
 * ids, id_off and status are what dpt_encode wrote (or any ids in that layout): token k of string s is
 * ids[id_off[s] - id_off[0] + k]; id_off[0] need not be 0.  status is nullable: all 0.  A string with
 * status[s] != 0 has no ids: it decodes to nothing, and the only thing written for it is that status
 * (dec_status[s], rt[s]; out_len[s] = 0).  flags: DPT_DECODE_STRIP_SPACE drops the string's first decoded
 * byte when it is ' ' (SentencePiece's dummy prefix, the word mark of RAW mode's first character).
 *   dpt_decode_sizes  out_len[s] = the decoded bytes of string s (the caller's prefix sum gives out_off)
 *   dpt_decode        the bytes of string s at out[out_off[s] - out_off[0] ..]; out_off[0] need not be 0, no
 *                     alignment is assumed.  dec_status[s] = 0, or DPT_STATUS_INTERNAL when an id of s lies
 *                     outside the table or no token has it, or when the decode does not fill
 *                     [out_off[s], out_off[s+1]) exactly; such a string's bytes (and its out_len) are
 *                     unspecified, every other string is exact, and every store stays inside the string's own
 *                     output range whatever the ids hold
 *   dpt_roundtrip     compares the decode of string s with text[str_off[s] - str_off[0] ..) without writing
 *                     it: rt[s] = DPT_RT_EQUAL or DPT_RT_DIFFERS, and first_diff[s] (nullable; written only
 *                     when rt[s] = DPT_RT_DIFFERS) = the first differing byte offset -- the shorter length
 *                     when one side is a prefix of the other.  An id without a token gives
 *                     DPT_STATUS_INTERNAL unless the bytes decoded before it already differ
 * DEVICE pointers on the table's device; stream-ordered on hip_stream, never synchronise, allocate nothing
 * and need no dpt_ctx: any number of calls may be in flight on one dpt_detok.  Strings and their decodes
 * < 4 GiB; id_off, str_off and out_off monotone (the device calls cannot check device-resident offsets).
 */
typedef struct dpt_detok dpt_detok;
#define DPT_DETOK_PIECES 0
#define DPT_DETOK_SP 1
#define DPT_DETOK_BYTELEVEL 2
#define DPT_DECODE_STRIP_SPACE 1
#define DPT_RT_EQUAL 0
#define DPT_RT_DIFFERS 5
int dpt_detok_create(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok, int rule,
                     const int32_t *skip_ids, uint32_t n_skip, int device, dpt_detok **out);
int dpt_detok_destroy(dpt_detok *d);
int dpt_decode_sizes(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str,
                     int flags, uint64_t *out_len, void *hip_stream);
int dpt_decode(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status, uint64_t n_str,
               int flags, uint8_t *out, const uint64_t *out_off, int32_t *dec_status, void *hip_stream);
int dpt_roundtrip(const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                  const uint8_t *text, const uint64_t *str_off, uint64_t n_str, int flags, int32_t *rt,
                  uint32_t *first_diff, void *hip_stream);
/* Same with HOST pointers: copy in through the ctx's host-path staging (grows on demand), run, copy out,
 * synchronise; both check that the offset arrays are monotone (DPT_E_ARG).  dpt_decode_host runs the sizes,
 * fills out_off[0..n_str] with their prefix sum from 0 -- always -- and, when out_off[n_str] > out_cap,
 * returns DPT_E_CAP having written no bytes: the caller reads the need from out_off and calls again. */
int dpt_decode_host(dpt_ctx *c, const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                    uint64_t n_str, int flags, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *dec_status);
int dpt_roundtrip_host(dpt_ctx *c, const dpt_detok *d, const int32_t *ids, const uint64_t *id_off, const int32_t *status,
                       const uint8_t *text, const uint64_t *str_off, uint64_t n_str, int flags, int32_t *rt,
                       uint32_t *first_diff);
/* TEST-ONLY, needs no device.  The bytes dpt_detok_create would upload for these arguments, built on the host
 * (tests/decode_ref.py holds a model of the format).  which: 0 the entries (n_tab pairs of uint32: the piece's
 * offset in the blob, its length -- 0 for a skipped id -- or 0x80000000 for an id no token has), 1 the blob
 * (the decoded pieces in id order), 2 DPT_DETOK_SCALAR_INTS int64: id_min, n_tab, blob bytes, longest decoded
 * piece.  *size = the table's bytes, always; it is copied to out (nullable) when cap >= *size, else DPT_E_CAP. */
#define DPT_DETOK_SCALAR_INTS 4
int dpt_debug_detok_table(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok, int rule,
                          const int32_t *skip_ids, uint32_t n_skip, int which, void *out, uint64_t cap, uint64_t *size);

/*
 * Model-input batches: the ids of an encoded batch as padded [n_str, row_len] rows -- what the reference's
 * llama_preprocessing_function hands the Trainer (main_analyze_s2orc.py:61-93: input_ids, attention_mask =
 * [1] * len(ids), truncation to max_length) after the collator has padded the batch.  Added within ABI 6
 * (DPT_ABI_VERSION unchanged): a binding that may meet an older libdpt.so probes for the symbol.
 *
 * ids (int32), off (uint64, n_str + 1 entries, off[0] need not be 0), counts (nullable, uint64 per string) and
 * status (nullable: all 0) describe the batch: string s has the tokens t[k] = ids[off[s] - off[0] + k] for
 * k < n, with n = off[s+1] - off[s] when counts == NULL (dpt_encode's layout, off = id_off) and n = counts[s]
 * otherwise (dpt_encode_padded's layout, off = str_off).  With L = row_len and n_special = the number of
 * DPT_COLLATE_BOS / DPT_COLLATE_EOS set, a string with status[s] == 0 gives
 *   keep = min(n, L - n_special) tokens: the first keep, or with DPT_COLLATE_TRUNC_LEFT the last keep
 *   seq  = [bos_id] + kept + [eos_id] (the specials survive truncation), len = keep + n_special
 *   input_ids row s:  seq in [0, len) and pad_id in [len, L); with DPT_COLLATE_PAD_LEFT pad_id in [0, L - len)
 *                     and seq in [L - len, L)
 *   attention_mask:   1 where the row holds seq, 0 where it holds pad_id
 *   labels:           the row of input_ids with ignore_id where the mask is 0
 *   lengths[s] = len  (an empty string gives its specials only)
 * and a string with status[s] != 0 a row of pad_id, mask 0, labels ignore_id and lengths[s] = 0, whatever its
 * off range or count holds.  Ids pass through unvalidated.  Row s starts at element s * row_stride of each of
 * input_ids, attention_mask and labels (row_stride 0: row_len; else >= row_len); their elements are int32, or
 * with DPT_COLLATE_I64 int64 (sign-extended).  attention_mask, labels and lengths are nullable.  Elements
 * [row_len, row_stride) of a row and everything outside the n_str rows are never written.  Outputs must not
 * overlap inputs and need their element's alignment only (4 or 8 bytes).
 * DPT_E_ARG, before any device work: null ids, off, opts or input_ids; row_len 0 or < n_special; row_stride
 * non-zero and < row_len; unknown flags.  n_str == 0 launches nothing.
 * DEVICE pointers on the current device; stream-ordered on hip_stream, never synchronises, allocates nothing
 * and needs no dpt_ctx and no vocabulary: any number of calls may be in flight.  No host-buffer form (the
 * product is a device tensor).  off monotone, row_len <= 2^31, n_str * row_stride < 2^63.
 */
#define DPT_COLLATE_BOS 1
#define DPT_COLLATE_EOS 2
#define DPT_COLLATE_PAD_LEFT 4
#define DPT_COLLATE_TRUNC_LEFT 8
#define DPT_COLLATE_I64 16
typedef struct {
    uint32_t row_len;      /* L: elements per row */
    uint64_t row_stride;   /* elements between row starts (0: row_len) */
    int32_t pad_id;
    int32_t bos_id;        /* read with DPT_COLLATE_BOS */
    int32_t eos_id;        /* read with DPT_COLLATE_EOS */
    int32_t ignore_id;     /* labels at pad positions (e.g. -100) */
    uint32_t flags;        /* DPT_COLLATE_* */
} dpt_collate_opts;
int dpt_collate(const int32_t *ids, const uint64_t *off, const uint64_t *counts, const int32_t *status,
                uint64_t n_str, const dpt_collate_opts *opts, void *input_ids, void *attention_mask,
                void *labels, uint32_t *lengths, void *hip_stream);

/*
 * Source + target model-input batches: rows of two segments -- what the reference's BLOOM translation driver
 * feeds its model.  There apply_tokenizer (main_biomed_translation.py:138-145) tokenizes a source and a target per
 * example, and ShortcutDataCollatorForSeq2Seq (:104-124) builds each row as the source ids followed by the target
 * ids, right-pads the batch with the pad id and returns that tensor as both input_ids and labels.  Added within
 * ABI 6 (DPT_ABI_VERSION unchanged): a binding that may meet an older libdpt.so probes for the symbol.
 *
 * Each side (a: the source, b: the target) is described like the first four arguments of the one-sequence call
 * above, independently of the other: ids (int32), off (uint64, n_str + 1 entries, off[0] need not be 0 and ids
 * corresponds to it), counts (nullable; NULL: off is an id_off and n = off[s+1] - off[s], else off is a str_off
 * and n = counts[s]) and status (nullable: all 0).  Both sides may point into the buffers of one encode, e.g. the
 * sources at strings [0, n) and the targets at [n, 2n) of one padded encode.  With L = row_len, n_special = the
 * number of DPT_COLLATE_BOS / DPT_COLLATE_SEP / DPT_COLLATE_EOS set, room = L - n_special and nA, nB the two token
 * counts, a row s whose statuses are both 0 gives
 *   caps      cA = max_a ? min(nA, max_a) : nA, and cB from max_b likewise
 *   overflow  over = max(0, cA + cB - room); B gives up tokens first: dB = min(over, cB), dA = over - dB; with
 *             DPT_COLLATE_TRIM_A_FIRST A does: dA = min(over, cA), dB = over - dA
 *   kept      kA = cA - dA, kB = cB - dB; a side keeps its first k tokens, or with DPT_COLLATE_TRUNC_LEFT the
 *             last k of its n
 *   seq  = [bos_id] + A_kept + [sep_id] + B_kept + [eos_id] (the specials survive truncation),
 *   len  = kA + kB + n_special
 *   input_ids, attention_mask: as in the one-sequence call (padding side, row_stride, element width, sign extension)
 *   labels:           the row of input_ids with ignore_id at pad positions; with DPT_COLLATE_MASK_A ignore_id also
 *                     on the bos, every A token and the sep (the loss is on B and the eos only)
 *   token_type_ids:   0 on bos / A / sep and on pad, 1 on B and eos (same element type)
 *   lengths[s] = len
 *   b_start[s] = the row column of B's first position: start + bos + kA + sep, with start = L - len under
 *                DPT_COLLATE_PAD_LEFT and 0 otherwise; written when kB = 0 too
 * and a row where either status is non-zero is all pad_id, mask 0, labels ignore_id, type 0, lengths[s] = 0 and
 * b_start[s] = 0, whatever its off ranges or counts hold: no id of it is read.  Ids pass through unvalidated.
 * attention_mask, labels, token_type_ids, lengths and b_start are nullable.  Elements [row_len, row_stride) of a row
 * and everything outside the n_str rows are never written.  Outputs must not overlap inputs and need their
 * element's alignment only.
 * DPT_E_ARG, before any device work (also with n_str == 0): null a, b, a->ids, a->off, b->ids, b->off, opts or
 * input_ids; row_len 0, < n_special or > 2^31; row_stride non-zero and < row_len; unknown flags.  n_str == 0
 * launches nothing.
 * DEVICE pointers on the current device; stream-ordered on hip_stream, never synchronises, allocates nothing and
 * needs no dpt_ctx and no vocabulary: any number of calls may be in flight.  No host-buffer form.  The
 * reference's collator is the case without specials, right padding, ignore_id = pad_id (its labels are the
 * padded input_ids themselves) and DPT_COLLATE_I64.
 */
typedef struct {            /* one side of the pair */
    const int32_t *ids;
    const uint64_t *off;
    const uint64_t *counts; /* nullable */
    const int32_t *status;  /* nullable */
} dpt_collate_side;
#define DPT_COLLATE_SEP 32          /* sep_id between the sides */
#define DPT_COLLATE_MASK_A 64       /* labels = ignore_id on bos + A + sep */
#define DPT_COLLATE_TRIM_A_FIRST 128
typedef struct {
    uint32_t row_len;      /* L: elements per row */
    uint64_t row_stride;   /* elements between row starts (0: row_len) */
    int32_t pad_id;
    int32_t bos_id;        /* read with DPT_COLLATE_BOS */
    int32_t sep_id;        /* read with DPT_COLLATE_SEP */
    int32_t eos_id;        /* read with DPT_COLLATE_EOS */
    int32_t ignore_id;
    uint32_t max_a, max_b; /* per-side caps, 0 = none */
    uint32_t flags;        /* DPT_COLLATE_* (BOS, EOS, PAD_LEFT, TRUNC_LEFT, I64 as above) */
} dpt_collate_pair_opts;
int dpt_collate_pair(const dpt_collate_side *a, const dpt_collate_side *b, uint64_t n_str,
                     const dpt_collate_pair_opts *opts, void *input_ids, void *attention_mask, void *labels,
                     void *token_type_ids, uint32_t *lengths, uint32_t *b_start, void *hip_stream);

/*
 * Sequence packing: consecutive strings of an encoded batch packed into rows of L = row_len tokens, in order and
 * greedily, no sequence split -- the rows a training loop makes of dpt_collate's one-row-per-string output when most
 * of that is padding (S2ORC abstracts of a few hundred tokens against max_length = 2048, reference
 * main_analyze_s2orc.py:68, :209).  Added within ABI 6 (DPT_ABI_VERSION unchanged): a binding that may meet an older
 * libdpt.so probes for the symbols.  Three calls, in the dpt_decode_sizes -> dpt_decode pattern (the prefix sum
 * between them is the caller's):
 *
 * 1. dpt_pack_sizes: lengths[s] (uint32) of every string, exactly dpt_collate's lengths: with the source described by
 *    (off, counts, status) as there, n_special = the number of DPT_COLLATE_BOS / DPT_COLLATE_EOS set,
 *      len[s] = 0 when status[s] != 0, else min(n, L - n_special) + n_special          (so len[s] <= L)
 *    The caller takes the exclusive prefix sum of lengths into tok_off (uint64, n_str + 1 entries; tok_off[0] need
 *    not be 0).
 * 2. dpt_pack_plan: the placement, from tok_off alone (no ids, no vocabulary: any lengths <= row_len pack this way).
 *    A string with len[s] == 0 -- a failed string, an empty string without specials -- is never placed.  The others:
 *      r = -1; fill = L + 1
 *      for s in 0..n_str-1, len[s] > 0:
 *          if fill + len[s] > L: r += 1; fill = 0; row_first[r] = s
 *          str_row[s] = r; str_col[s] = fill; fill += len[s]
 *      n_rows = r + 1
 *    str_row[s] = DPT_PACK_NONE and str_col[s] = 0 for an unplaced string; row_fill[r] = the tokens of row r;
 *    row_first[r] = n_str for n_rows <= r <= row_cap and row_fill[r] = 0 for n_rows <= r < row_cap.  str_row, str_col
 *    (uint32, n_str entries), row_first (uint32, row_cap + 1 entries) and row_fill (uint32, row_cap entries) are
 *    nullable; entries of rows >= row_cap (row_first: > row_cap) are not written, and *n_rows (uint64, on the device)
 *    always reports the need, also above row_cap.  ws: dpt_pack_plan_workspace(n_str) bytes of the caller's device
 *    memory, 4-byte aligned (at most 16 bytes per string plus a constant; nullable when n_str == 0); DPT_E_CAP when
 *    ws_bytes is smaller.
 * 3. dpt_pack_write: the rows r < min(n_rows, row_cap), elements and row_stride as in dpt_collate:
 *      input_ids:     the sequences [bos_id] + kept + [eos_id] of the row's placed strings, back to back from column
 *                     0, pad_id in the rest; kept = the first len - n_special tokens, or with DPT_COLLATE_TRUNC_LEFT
 *                     the last
 *      position_ids:  the position inside its own sequence, from 0; 0 at pad
 *      segment_ids:   s - row_first[r] + 1 on every position of string s, 0 at pad (distinct per sequence of a row;
 *                     the attention mask is segment_ids != 0)
 *      labels:        the id inside a sequence, ignore_id at pad; with DPT_PACK_MASK_FIRST ignore_id also on position
 *                     0 of every sequence (the token no earlier token of its own sequence predicts)
 *    Rows [n_rows, row_cap) are all pad: 0, 0 and ignore_id.  Rows >= row_cap, elements [row_len, row_stride) of a row
 *    and everything outside the arrays are never written.  side describes the source as dpt_collate's first four
 *    arguments do; tok_off, row_first and n_rows are the plan's.  position_ids, segment_ids and labels are nullable.
 *
 * DPT_E_ARG, before any device work (also with n_str == 0): a null required pointer (sizes: off, opts, lengths; plan:
 * tok_off, n_rows, and ws when n_str > 0; write: side, side->ids, side->off, tok_off, row_first, n_rows, opts,
 * input_ids); row_len 0, < n_special or > 2^31; row_stride non-zero and < row_len; unknown flags or
 * DPT_COLLATE_PAD_LEFT; n_str >= 2^31; row_cap >= 2^31.
 * All three take DEVICE pointers on the current device, are stream-ordered on hip_stream, never synchronise, allocate
 * nothing and need no dpt_ctx.  n_str == 0 launches nothing: the plan then still sets *n_rows = 0, row_first[0..row_cap]
 * = 0 and row_fill = 0 (stream-ordered fills), the write leaves every row as it is.
 * tok_off and row_first are the caller's data: whatever they hold, every store lands inside the arrays as sized
 * above, an id is loaded only from inside its string's own token range, and every loop has a bound fixed before it
 * starts; a tok_off that is no prefix sum of lengths <= row_len gives unspecified values, never a fault or a hang.
 */
#define DPT_PACK_MASK_FIRST 256     /* labels = ignore_id on position 0 of every sequence */
#define DPT_PACK_NONE 0xFFFFFFFFu   /* str_row of a string that is not placed */
typedef dpt_collate_opts dpt_pack_opts;   /* flags: DPT_COLLATE_BOS, _EOS, _TRUNC_LEFT, _I64 and DPT_PACK_MASK_FIRST */
int dpt_pack_sizes(const uint64_t *off, const uint64_t *counts, const int32_t *status, uint64_t n_str,
                   const dpt_pack_opts *opts, uint32_t *lengths, void *hip_stream);
int dpt_pack_plan_workspace(uint64_t n_str, uint64_t *bytes);
int dpt_pack_plan(const uint64_t *tok_off, uint64_t n_str, uint32_t row_len, uint64_t row_cap, uint32_t *str_row,
                  uint32_t *str_col, uint32_t *row_first, uint32_t *row_fill, uint64_t *n_rows, void *ws,
                  uint64_t ws_bytes, void *hip_stream);
int dpt_pack_write(const dpt_collate_side *side, uint64_t n_str, const uint64_t *tok_off, const uint32_t *row_first,
                   const uint64_t *n_rows, uint64_t row_cap, const dpt_pack_opts *opts, void *input_ids,
                   void *position_ids, void *segment_ids, void *labels, void *hip_stream);
/* TEST-ONLY, needs no device: the strings one block of the plan takes (B) and the plan's grid cap (more than
 * grid_cap * B strings: the blocks stride), so tests take their edge sizes from the library. */
int dpt_debug_pack_geometry(uint32_t *strings_per_block, uint32_t *grid_cap);

/*
 * Llama-mode pre-tokenization on the device: text in, DPT_MODE_PRESPLIT input (text + cut mask) out -- what the
 * reference's default pre-tokenizer, pretokenize_with_llama + merge_tokens (packages/tokenizer_utils.py:7-31,
 * selected at :52, main_analyze_s2orc.py:74, :256), keeps of SentencePiece's output: the concatenation of the pieces
 * and which pieces start with U+2581.  For a Llama-style model (identity normaliser, dummy prefix, byte fallback, no
 * whitespace folding) both are a per-character function of the text, except on a few input classes where the merge
 * order or the tokenizer object decides; those strings are marked DPT_PRETOK_NEEDS_HOST and left to the caller's host
 * tokenizer.  Added within ABI 6 (DPT_ABI_VERSION unchanged): a binding that may meet an older libdpt.so probes for
 * the symbols.
 *
 * A dpt_pretok is the table of one vocabulary (dpt_vocab_create's first three arguments; empty strings are ignored):
 *   known     the code points that are a one-character piece
 *   runs_ok   no piece of two or more characters consists of U+2581 only
 * with the BOS piece (bos_len 0: no BOS word; at most DPT_PRETOK_MAX_BOS bytes) and n_lit literal strings -- the
 * tokenizer's special and added tokens, which its encode matches in the text before the model runs: literal k is
 * lit_blob[lit_off[k] - lit_off[0] .. lit_off[k+1] - lit_off[0]), at most DPT_PRETOK_MAX_LITERALS of 1 ..
 * DPT_PRETOK_MAX_LITERAL_BYTES bytes each.  DPT_E_ARG beyond those limits.  DPT_E_VOCAB when one of the byte pieces
 * <0x00> .. <0xFF> is missing, when a piece holds U+2581 after its first character and is not U+2581 only (the
 * word starts would depend on the merges), or when the BOS piece is not in the vocabulary.  Immutable after creation;
 * may be shared by threads and streams.
 *
 * A string is certified (pre_status[s] = 0) unless
 *   - its first byte is ' ' (the tokenizer objects disagree about a leading space),
 *   - it holds U+2581 (indistinguishable from a space afterwards),
 *   - it holds one of the literals as a substring (the tokenizer object decides what they become),
 *   - it holds two consecutive spaces while !runs_ok (a multi-U+2581 piece would swallow word starts),
 *   - it is not well-formed UTF-8: a truncated sequence (at the string's end too: the next string's bytes never
 *     complete it), an overlong form, a surrogate, a value above U+10FFFF, a stray continuation byte,
 *   - its pre-split form would reach 4 GiB;
 * then pre_status[s] = DPT_PRETOK_NEEDS_HOST, out_len[s] = 0 and nothing is written for it.  On the recorded
 * SentencePiece cases (tests/golden/sp_llama_cases.json.gz: two tokenizer objects, 565 texts each) the rule certifies
 * 292 texts per tokenizer, all with the recorded words, and refuses every one of the 236 texts on which the two
 * tokenizer objects disagree.  The rule is pinned on that model only: a caller with another tokenizer checks it first
 * (the Python adapter runs a probe list through both at construction).
 * The pre-split form of a certified string: the BOS piece's bytes, one word; then, only when the text is not empty,
 * U+2581 opening a word; then per character: ' ' -> U+2581 opening a word, a known character -> its own bytes, any
 * other character -> <0xNN> (upper-case hex) for each of its UTF-8 bytes.  cut_mask is 1 at the first byte of the
 * output and at the first byte of every word-opening U+2581, 0 elsewhere.  An empty text gives the BOS word alone,
 * and nothing at all (length 0, status 0) without a BOS piece.
 *   dpt_pretok_sizes  out_len[s] (uint64) = the bytes of string s's pre-split form, pre_status[s] (int32) as above
 *   dpt_pretok_write  the form of string s at out_text[out_off[s] - out_off[0] ..] and its mask at the same index of
 *                     cut_mask; out_off (n_str + 1 entries; out_off[0] need not be 0) is the caller's prefix sum of
 *                     out_len, pre_status what the sizes pass wrote.  Every store stays inside the string's own
 *                     [out_off[s], out_off[s+1]) whatever the bytes hold
 * text and str_off as dpt_encode's (str_off[0] need not be 0, no alignment is assumed); no load goes beyond a
 * string's last byte.  DEVICE pointers on the table's device; stream-ordered on hip_stream, never synchronise,
 * allocate nothing and need no dpt_ctx: any number of calls may be in flight on one dpt_pretok.  DPT_E_ARG, before any
 * device work, for a null pointer; n_str == 0 launches nothing.  Strings < 4 GiB, str_off and out_off monotone (the
 * device calls cannot check device-resident offsets).  No host-buffer form: the product feeds dpt_encode on the device.
 */
typedef struct dpt_pretok dpt_pretok;
#define DPT_PRETOK_NEEDS_HOST 6   /* per-string value of pre_status */
#define DPT_PRETOK_MAX_LITERALS 32
#define DPT_PRETOK_MAX_LITERAL_BYTES 64
#define DPT_PRETOK_MAX_BOS 61
int dpt_pretok_create(const uint8_t *utf8_blob, const uint64_t *tok_off, uint32_t n_tok, const uint8_t *bos_piece,
                      uint32_t bos_len, const uint8_t *lit_blob, const uint64_t *lit_off, uint32_t n_lit, int device,
                      dpt_pretok **out);
int dpt_pretok_destroy(dpt_pretok *p);
int dpt_pretok_sizes(const dpt_pretok *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str, uint64_t *out_len,
                     int32_t *pre_status, void *hip_stream);
int dpt_pretok_write(const dpt_pretok *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str,
                     const int32_t *pre_status, uint8_t *out_text, const uint64_t *out_off, uint8_t *cut_mask,
                     void *hip_stream);
/* Added within ABI 6 (DPT_ABI_VERSION unchanged).  dpt_pretok_write with a DPT_MODE_ATOMS mask, the input of
 * dpt_bpe_encode: the same arguments, the same text, and cut_mask = 3 at the output's first byte and at the first
 * byte of every word-opening U+2581, 2 at the first byte of every other atom, 0 elsewhere.  The atoms are the BOS
 * piece (one atom), each U+2581, each character that is a piece of its own, and each <0xNN> group that byte fallback
 * produced (one atom of 6 bytes).  A literal "<0x41>" typed in the text is six one-character atoms: SentencePiece
 * keeps the two apart, because byte pieces never take part in merges, and the PRESPLIT form cannot. */
int dpt_pretok_write_atoms(const dpt_pretok *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str,
                           const int32_t *pre_status, uint8_t *out_text, const uint64_t *out_off, uint8_t *cut_mask,
                           void *hip_stream);
/* TEST-ONLY, needs no device.  The bytes dpt_pretok_create would upload for these arguments, built on the host
 * (tests/pretok_ref.py holds a model of the format).  which: 0 the known set below U+10000 as a bitmap (2048 uint32:
 * bit cp & 31 of word cp >> 5), 1 the known code points from U+10000 up (uint32, ascending), 2 the literal block
 * (8 uint32: the bitmap of the literals' first bytes; n_lit + 1 uint32: their offsets from 0; their bytes), 3 the
 * prefix (the BOS piece, then U+2581), 4 DPT_PRETOK_SCALAR_INTS int64: runs_ok, the number of known code points,
 * n_lit, bos_len.  *size = the table's bytes, always; it is copied to out (nullable) when cap >= *size, else DPT_E_CAP. */
#define DPT_PRETOK_SCALAR_INTS 4
int dpt_debug_pretok_table(const uint8_t *utf8_blob, const uint64_t *tok_off, uint32_t n_tok, const uint8_t *bos_piece,
                           uint32_t bos_len, const uint8_t *lit_blob, const uint64_t *lit_off, uint32_t n_lit, int which,
                           void *out, uint64_t cap, uint64_t *size);

/*
 * Byte-level pre-tokenization on the device: text in, DPT_MODE_ATOMS input (text + cut mask) out -- what the BLOOM
 * adapter (packages/tokenizer_utils.py dp_tokenize_bloom) builds on the host from the tokenizer's pre-tokenizer,
 * Sequence[Split(Regex(" ?[^(\s|[.,!?...])]+"), isolated), ByteLevel(add_prefix_space=False, use_regex=False)], and a
 * dictionary lookup per character.  Both halves are local functions of the text, so the rule is exact: only text
 * that is not well-formed UTF-8 is left to the caller's host path.  Added within ABI 6 (DPT_ABI_VERSION unchanged): a
 * binding that may meet an older libdpt.so probes for the symbols.
 *
 * A dpt_bytelevel is the separator set SEP of one split of the family "optional U+0020, then one or more
 * non-separators, isolated": n_sep (1 .. DPT_BYTELEVEL_MAX_SEPARATORS) Unicode scalar values, U+0020 among them,
 * duplicates collapse.  DPT_E_ARG for a null pointer, a count outside that range, a value that is not a scalar value
 * (a surrogate, above U+10FFFF) or a set without U+0020.  Immutable after creation; may be shared by threads and
 * streams.  BLOOM's set has 39 members (dptok/bytelevel.py BLOOM_SEPARATORS).
 *
 * Word starts, over the characters c[0..n) of a string: a space c[i] == U+0020 is ABSORBED when c[i+1] exists and
 * is not in SEP.  A word starts at i == 0, at an absorbed space, at a non-separator whose predecessor is a separator
 * that is not an absorbed space, and at a separator that is not absorbed and whose predecessor is a non-separator;
 * nowhere else.  Runs of unabsorbed separators form one word ("a  b" -> "a", " ", " b"); the empty string has none.
 * Atoms: every input byte is one atom, its GPT-2 bytes-to-unicode character (DPT_DETOK_BYTELEVEL's alphabet): bytes
 * 0x21 .. 0x7E stay one byte, every other byte becomes a two-byte UTF-8 character (U+00A1 .. U+0143).
 * The output is DPT_MODE_ATOMS input: the atoms' UTF-8, and a cut mask that is 3 at the first byte of a word's first
 * atom, 2 at the first byte of every other atom, 0 at an atom's second byte.
 *
 * pre_status[s] = 0 unless the string is not well-formed UTF-8 (the classes dpt_pretok_sizes refuses: a truncated
 * sequence -- at the string's end too: the next string's bytes never complete it --, an overlong form, a surrogate,
 * a value above U+10FFFF, a stray continuation byte) or its form would reach 4 GiB; then pre_status[s] =
 * DPT_PRETOK_NEEDS_HOST, out_len[s] = 0 and nothing is written for it.
 *   dpt_bytelevel_sizes  out_len[s] (uint64) = the bytes of string s's ATOMS form, pre_status[s] (int32) as above
 *   dpt_bytelevel_write  the form of string s at out_text[out_off[s] - out_off[0] ..] and its mask at the same index
 *                        of cut_mask; out_off (n_str + 1 entries; out_off[0] need not be 0) is the caller's prefix
 *                        sum of out_len, pre_status what the sizes pass wrote.  Every store stays inside the
 *                        string's own [out_off[s], out_off[s+1]) whatever the bytes hold
 * text and str_off as dpt_encode's (str_off[0] need not be 0, no alignment is assumed); no load goes beyond a
 * string's last byte.  DEVICE pointers on the table's device; stream-ordered on hip_stream, never synchronise,
 * allocate nothing and need no dpt_ctx: any number of calls may be in flight on one dpt_bytelevel.  DPT_E_ARG, before
 * any device work, for a null pointer; n_str == 0 launches nothing.  Strings < 4 GiB, str_off and out_off monotone.
 * No host-buffer form: the product feeds dpt_encode on the device.
 */
typedef struct dpt_bytelevel dpt_bytelevel;
#define DPT_BYTELEVEL_MAX_SEPARATORS 256
int dpt_bytelevel_create(const uint32_t *sep_cps, uint32_t n_sep, int device, dpt_bytelevel **out);
int dpt_bytelevel_destroy(dpt_bytelevel *p);
int dpt_bytelevel_sizes(const dpt_bytelevel *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str,
                        uint64_t *out_len, int32_t *pre_status, void *hip_stream);
int dpt_bytelevel_write(const dpt_bytelevel *p, const uint8_t *text, const uint64_t *str_off, uint64_t n_str,
                        const int32_t *pre_status, uint8_t *out_text, const uint64_t *out_off, uint8_t *cut_mask,
                        void *hip_stream);
/* TEST-ONLY, needs no device.  What dpt_bytelevel_create would keep and upload for these arguments, built on the
 * host (tests/bytelevel_ref.py holds a model of the format).  which: 0 the separators below U+0080 as a bitmap (2
 * uint64: bit cp & 63 of word cp >> 6), 1 the separators from U+0080 up (uint32, ascending, each once), 2
 * DPT_BYTELEVEL_SCALAR_INTS int64: the distinct separators, those from U+0080 up.  *size = the table's bytes, always;
 * it is copied to out (nullable) when cap >= *size, else DPT_E_CAP. */
#define DPT_BYTELEVEL_SCALAR_INTS 2
int dpt_debug_bytelevel_table(const uint32_t *sep_cps, uint32_t n_sep, int which, void *out, uint64_t cap,
                              uint64_t *size);

/*
 * The tokenizer's own encoding on the device.  Added within ABI 6 (DPT_ABI_VERSION unchanged).  The reference drivers
 * compare the shortest tokenization with the tokenizer's default one (main_analyze_s2orc.py:272, :282:
 * len(dp_tokenize(x)) against len(llama_tokenizer.encode(x)); main_biomed_translation.py:74 the same for BLOOM).  Both
 * defaults are greedy BPE merges over the words of atoms the device pre-tokenizers already produce, so one rule and one
 * table serve both: every atom becomes the id of the token with exactly its bytes, and within each word the symbols
 * merge until no adjacent pair is in the pair table, each step merging the adjacent pair of lowest (rank, position).
 * Nothing merges across a word start.  (Merging every local minimum of a word at once is NOT this rule: with (p,q)->P
 * at rank 0, (P,r)->Q at rank 1 and (r,s)->R at rank 2 the word p q r s gives [Q, s], not [P, R].)
 *
 * dpt_bpe_create: entry k says that the adjacent symbols left[k], right[k] may merge into merged[k]; the lowest rank
 * merges first, equal ranks on different pairs are allowed (the leftmost pair wins).  DPT_E_ARG for a null pointer,
 * n_pairs = 0 or >= 2^31, a negative id, a (left, right) key given twice, or the rank 0xFFFFFFFF (a miss's value).
 * The object is immutable and may be shared by threads and streams.  On the device it is a hash keyed by the 64-bit
 * pair with the value {merged, rank}: 32 bytes per pair (16-byte entries, load 0.5), two buckets per key and never a
 * probe chain.
 *
 * dpt_bpe_encode: text, n_bytes, str_off, cut_mask, n_str exactly as dpt_encode's DPT_MODE_ATOMS input (cut_mask bit 1
 * where an atom starts, bit 0 where a word starts; str_off[0] need not be 0; no alignment is assumed; strings < 4 GiB,
 * str_off monotone; a string's first byte opens a word whatever its mask says).  Output in dpt_encode_padded's layout,
 * so dpt_collate and the adapters read it as they read the DP's ids: ids[str_off[s] - str_off[0] + k] for
 * k < counts[s], tok_word (nullable) at the same index = the 0-based word of token k within the string; status[s] =
 * 0, or DPT_STATUS_NO_TOKENIZATION with counts[s] = 0 when some atom is no token of v (slots of such a string may
 * hold anything); an empty string gives count 0 and status 0.  ids_cap >= n_bytes is required.  Words of any length are
 * exact: words of up to 256 atoms merge in LDS, a longer word that does not fit there merges in place in the
 * string's own output slots (slow; no workspace).
 * DEVICE pointers on the device of b and v (the same one).  Stream-ordered on hip_stream, never synchronises,
 * allocates nothing and needs no dpt_ctx and no host state: any number of calls may be in flight.  Every store stays
 * inside the string's own [str_off[s], str_off[s+1]) slots of ids / tok_word and its own counts / status entry,
 * whatever the mask holds.  DPT_E_ARG, before any device work, for a null pointer (tok_word excepted) or
 * ids_cap < n_bytes; n_str == 0 launches nothing.
 */
typedef struct dpt_bpe dpt_bpe;
int dpt_bpe_create(const int32_t *left, const int32_t *right, const int32_t *merged, const uint32_t *rank,
                   uint64_t n_pairs, int device, dpt_bpe **out);
int dpt_bpe_destroy(dpt_bpe *b);
int dpt_bpe_encode(const dpt_bpe *b, const dpt_vocab *v, const uint8_t *text, uint64_t n_bytes,
                   const uint64_t *str_off, const uint8_t *cut_mask, uint64_t n_str, int32_t *ids, uint64_t ids_cap,
                   uint64_t *counts, int32_t *status, uint32_t *tok_word, void *hip_stream);
/* TEST-ONLY, needs no device.  Builds the bytes dpt_bpe_create would upload for its first five arguments and answers
 * the n_q queries (q_left[k], q_right[k]) from those bytes through the probe function the kernel runs:
 * out_merged[k], out_rank[k], or -1 and 0xFFFFFFFF for a pair that is not in the table.  DPT_E_ARG as
 * dpt_bpe_create, or for a null query / result array with n_q > 0. */
int dpt_debug_bpe_lookup(const int32_t *left, const int32_t *right, const int32_t *merged, const uint32_t *rank,
                         uint64_t n_pairs, const int32_t *q_left, const int32_t *q_right, uint64_t n_q,
                         int32_t *out_merged, uint32_t *out_rank);

/*
 * Two tokenizations of a batch compared word by word on the device.  Added within ABI 6 (DPT_ABI_VERSION unchanged).
 * The reference's S2ORC probe lists, for every abstract the shortest tokenization improves, the improved words and
 * their tokens on both sides (main_analyze_s2orc.py:277-290, the improved_tokens / worse_tokens columns of its
 * frame).  Both word-index streams are already on the device -- dpt_token_spans writes tok_word / tok_end for the DP
 * ids, dpt_bpe_encode tok_word for the default ids -- so the answer is a short list of records and only those leave
 * the GPU.  Two calls in the manner of dpt_decode_sizes -> dpt_decode: the sizes, the caller's two prefix sums, the
 * write.
 *
 * A side is one tokenization by word, in either layout, each side independently: off / counts / status as
 * dpt_collate_side's (counts NULL: off is an id_off and n = off[s+1] - off[s]; else off is a str_off and
 * n = counts[s]), tok_word and tok_end at off[s] - off[0] + k for token k < n of string s (n < 2^32; a side with
 * more is malformed).  The rule is defined on the values alone.  For string s and side X with the word values
 * w_0..w_{n-1}:
 *   validity   X is well-formed when n == 0, or w_0 == 0 and every w_k - w_{k-1} is 0 or 1; its word count W_X is
 *              then w_{n-1} + 1 (0 when n == 0), the count of word w the length of its run of equal values and
 *              first(w) the token index where the run starts.
 *   wc_status[s] = status_a[s] when non-zero, else status_b[s] when non-zero, else DPT_STATUS_INTERNAL when a side
 *              is malformed or W_a != W_b, else 0 (pre-tokenization values such as DPT_PRETOK_NEEDS_HOST pass
 *              through a side's status).
 *   len_a[s], len_b[s] (nullable) = that side's n when that side's own status is 0, else 0.
 *   n_words[s] = W_a and n_sel[s] = the words the flags select when wc_status[s] == 0, else both 0.  DPT_WORDS_LESS
 *              selects cnt_a(w) < cnt_b(w), DPT_WORDS_GREATER cnt_a(w) > cnt_b(w), both flags !=.
 * dpt_word_compare_write takes the exclusive prefix sums of n_words and n_sel as word_off and sel_off (n_str + 1
 * entries each; entry 0 need not be 0).  word_off, cnt_a and cnt_b are nullable together; the sel_* arrays are
 * nullable one by one, sel_off with all of them.  For a string of status 0:
 *   cnt_a, cnt_b at word_off[s] - word_off[0] + w = the two counts of word w;
 *   the selected words in ascending w at sel_off[s] - sel_off[0] + d: sel_str = s, sel_word = w, sel_a_first /
 *   sel_a_count / sel_b_first / sel_b_count = first(w) and the count on each side, token indices within the string
 *   (no id is read: the caller gathers them), sel_begin / sel_end = a->tok_end of the last token of word w - 1 (0
 *   for w = 0) and of word w: the word's bytes in the text dpt_token_spans was given (RAW's leading ' ' included).
 * Every store of write stays inside the string's own [word_off[s], word_off[s+1]) and [sel_off[s], sel_off[s+1]),
 * whatever the inputs hold; a string whose derived counts do not fill those ranges exactly gets
 * DPT_STATUS_INTERNAL and unspecified contents in its own ranges only; a string of non-zero status gets nothing
 * but the status.
 * DPT_E_ARG, before any device work (also with n_str == 0): null a, b, off or tok_word of a side, a null n_words,
 * n_sel or wc_status, word_off / cnt_a / cnt_b not all given or all null, a sel_* array without sel_off, sel_begin
 * or sel_end with a null a->tok_end, flags 0 or with unknown bits, n_str >= 2^31.  n_str == 0 launches nothing.
 * DEVICE pointers on the current device; stream-ordered on hip_stream, never synchronises, allocates nothing and
 * needs no dpt_ctx and no vocabulary: any number of calls may be in flight.  No host-buffer form.
 */
typedef struct {             /* one tokenization of the batch, by word */
    const uint64_t *off;      /* n_str + 1 entries; off[0] need not be 0, tok_word / tok_end correspond to it */
    const uint64_t *counts;   /* nullable, as dpt_collate_side: NULL -> n = off[s+1]-off[s]; else n = counts[s] */
    const int32_t  *status;   /* nullable: all 0 */
    const uint32_t *tok_word; /* word index of token k of string s at off[s]-off[0]+k */
    const uint32_t *tok_end;  /* nullable; side a's is read for the word byte spans */
} dpt_word_side;
#define DPT_WORDS_LESS    1   /* select the words with fewer tokens on a than on b */
#define DPT_WORDS_GREATER 2   /* ... with more */
int dpt_word_compare_sizes(const dpt_word_side *a, const dpt_word_side *b, uint64_t n_str, int flags,
                           uint32_t *n_words, uint32_t *n_sel, uint32_t *len_a, uint32_t *len_b,
                           int32_t *wc_status, void *hip_stream);
int dpt_word_compare_write(const dpt_word_side *a, const dpt_word_side *b, uint64_t n_str, int flags,
                           const uint64_t *word_off, uint32_t *cnt_a, uint32_t *cnt_b,
                           const uint64_t *sel_off, uint32_t *sel_str, uint32_t *sel_word,
                           uint32_t *sel_begin, uint32_t *sel_end,
                           uint32_t *sel_a_first, uint32_t *sel_a_count,
                           uint32_t *sel_b_first, uint32_t *sel_b_count,
                           int32_t *wc_status, void *hip_stream);

/*
 * Fold the token-count histogram of dpt_token_histogram into the NEXT dpt_encode call on this ctx
 * (dpt_encode only: dpt_encode_host, dpt_encode_padded and dpt_dp_host* leave it armed; a dpt_encode
 * that fails still consumes it)
 * (its finish pass: no separate launch, no re-read of the offsets and statuses): hist (device
 * pointer, n_bins + 8 int64, layout and accumulate semantics of dpt_token_histogram) is added to
 * once, stream-ordered with that call.  hist NULL cancels.  n_bins above 1024 uses the separate
 * histogram pass after the encode.  One call only: set it again for the next.
 */
int dpt_ctx_set_histogram(dpt_ctx *c, int64_t *hist, uint32_t n_bins);

/* As dpt_ctx_set_histogram; flags DPT_HIST_OVERWRITE: the call's histogram REPLACES hist's contents
 * (the device zeroes it in stream order first) -- a per-step histogram without a memset launch. */
#define DPT_HIST_OVERWRITE 1
int dpt_ctx_set_histogram_ex(dpt_ctx *c, int64_t *hist, uint32_t n_bins, int flags);

/* Per-ctx kernel timing with HIP events on the encode stream (for bench.py's roofline): one event
 * pair per call around the tokenize passes (first pass, 2048-byte pass, unbounded pass). */
int dpt_ctx_profile(dpt_ctx *c, int enable);
/* Sums over calls since the last read (synchronises on the recorded events):
 * ms[0] tokenize passes; ms[1], ms[2] = -1 (not timed); *launches = calls timed. */
int dpt_ctx_profile_read(dpt_ctx *c, double *ms, uint64_t *launches);

/* TEST-ONLY.  Every later call on c starts the unbounded pass's arena counter and the far-pair counter
 * at `bias` instead of 0, with the arena and far-list pointers the kernels get shifted back by as many
 * elements: results are unchanged, but the kernels' arena offsets and far-pair indices are >= bias.
 * With a bias whose low word is >= 2^31 this exercises the 64-bit uniform reassembly of those values
 * (two readfirstlane halves; an int low half sign-extends) without a 40-GiB arena
 * (tests/test_gpu_parity.py::test_long_pass_offsets_past_2g).  bias < 2^62; 0 turns it off. */
int dpt_ctx_debug_counter_bias(dpt_ctx *c, uint64_t bias);

/* TEST-ONLY, needs no device.  Added within ABI 6 (DPT_ABI_VERSION unchanged).  The kernels an encode call
 * with these properties launches (tests/test_launch_plan.py holds the table).  variant: 1 = 16-lane rows,
 * 2 = 64-lane; hist: 0 none, 1 add, 2 overwrite; knobs: bits 1 DPT_GENERIC_PS, 2 DPT_GENERIC_RAW,
 * 4 DPT_NO_SOLO_WAVE, 8 DPT_NO_MID.  out: [0..5] the first pass's lanes, WIDE, SW, RAW, SOLO, MC; [6..9] the
 * 512-byte pass runs, its SW, WIDE, MC; [10..13] the 2048-byte + unbounded launch runs, its WIDE, RAW, the
 * list the 2048-byte pass reads (0 / 2: the first / 512-byte pass's); [14] the tail: 0 memsets, 1 nothing
 * (solo), 2 reset_kernel, 3 scan + finish, 4 fold finish, 5 one-batch finish; [15] finish width in bits;
 * [16..19] the histogram is folded into the finish pass, stored by it, zeroed by (0 nobody, 1 the 2048-byte
 * pass, 2 the scan, 3 a memset), the separate pass follows.  DPT_E_ARG: a kernel it names does not exist.
 * One more knob: 16 DPT_NO_LEAN (it changes none of these ints: dpt_debug_launch_plan_lean). */
#define DPT_LAUNCH_PLAN_INTS 20
int dpt_debug_launch_plan(int variant, int mode_flags, int st16, int edges, int solo, int padded, int no_fallback,
                          int profiled, uint64_t n_str, int hist, uint32_t hist_bins, unsigned knobs, int32_t *out);
/* TEST-ONLY, needs no device.  *lean = 1 when such a call takes the lean route: the lean kernel, then the general
 * one fed the deferred strings, in the first pass's place (tests/test_launch_plan_lean.py). */
int dpt_debug_launch_plan_lean(int variant, int mode_flags, int st16, int edges, int solo, int padded, uint64_t n_str,
                               unsigned knobs, int32_t *lean);
/* TEST-ONLY.  The context's lean-route words after its last call (waits for the device): out[0] the hint (nonzero:
 * the lean waves claim nothing), out[1] the strings the last lean launch deferred, out[2] the probes made so far,
 * out[3] the calls planned without the lean launch since the hint went off (the host's side of it).  A context
 * that has made no call yet: zeros. */
int dpt_ctx_debug_lean_words(dpt_ctx *c, uint32_t out[4]);
/* TEST-ONLY.  on != 0: the context's calls run without the lean launch (as the whole process does with DPT_NO_LEAN set
 * when it starts), and do not count for the hint; 0: back to the plan's choice. */
int dpt_ctx_debug_no_lean(dpt_ctx *c, int on);

/* TEST-ONLY, needs no device.  Added within ABI 6 (DPT_ABI_VERSION unchanged).  The bytes dpt_vocab_create
 * would upload for this vocabulary (its first four arguments), built on the host
 * (tests/test_vocab_tables.py holds a model of the formats).  which: 0 slots (n_slots + 65536 int32 pairs),
 * 1 slot ids (n_slots int32), 2 slots4 (n_slots + 65536 x four int32), 3 the pair block (65536 + 256 int16 |
 * 65536 x two uint32 | hash header + buckets), 4 tok_len (uint16 per id - id_min; size 0: no table),
 * 5 DPT_VOCAB_SCALAR_INTS int32: root_base, ws_node, ws_base, ws_id, ids16, id_min, n_tab, hash_buckets,
 * hash_probe, n_tokens, n_nodes, n_slots, max_bytes, max_cp, device_bytes (low, high word).
 * *size = the table's bytes, always; it is copied to out (nullable) when cap >= *size, else DPT_E_CAP. */
#define DPT_VOCAB_SCALAR_INTS 16
int dpt_debug_vocab_table(const uint8_t *utf8_blob, const uint64_t *tok_off, const int32_t *ids, uint32_t n_tok,
                          int which, void *out, uint64_t cap, uint64_t *size);

/* TEST-ONLY, needs no device.  Added within ABI 6 (DPT_ABI_VERSION unchanged).  Where a host-buffer call keeps
 * its arrays in the ctx's staging buffers (tests/test_host_layout.py holds the rules).  call: 0 dpt_encode_host /
 * dpt_dp_host*, 1 dpt_token_spans_host, 2 dpt_decode_host (n_bytes: the decoded bytes; 0 for its sizes pass),
 * 3 dpt_roundtrip_host; flags: bits 1 a cut mask, 2 tok_word, 4 edges; far_pairs: the far edge list's room.
 * out: DPT_HOST_LAYOUT_INTS uint64 -- for the in side, then the out side: the number of segments, the side's
 * bytes, then DPT_HOST_LAYOUT_SEGS x {offset, payload bytes, slack bytes}, the segments in their order. */
#define DPT_HOST_LAYOUT_SEGS 7
#define DPT_HOST_LAYOUT_INTS (2 * (2 + 3 * DPT_HOST_LAYOUT_SEGS))
int dpt_debug_host_layout(int call, uint64_t n_bytes, uint64_t n_str, uint64_t n_tok, int flags, uint64_t far_pairs,
                          uint64_t *out);

/* TEST-ONLY, needs no device.  Added within ABI 6 (DPT_ABI_VERSION unchanged).  *blocks = the grid a
 * one-wave-per-string kernel with `waves` waves to a block (the decode, spans, pre-tokenization and byte-level
 * kernels: 4) gets for n_str strings under the current environment: min(ceil(n_str / waves), 2^20) blocks, so
 * that a wave takes a second string only in calls of more than waves * 2^20 strings -- and at most
 * DPT_WAVE_GRID_BLOCKS blocks when that variable holds a decimal number > 0 (read on every call; for tests that
 * run many trips of the waves' stride on small batches, tests/test_gpu_wave_stride.py). */
int dpt_debug_wave_grid(uint64_t n_str, uint32_t waves, uint32_t *blocks);

/*
 * Multi-GPU without torch (ABI 6; SURVEY.md §8(b) dpt_hist_allreduce, §8(e) "direct RCCL with a
 * file-store unique id").  One process per GPU: rank 0 calls dpt_rccl_get_unique_id and hands the
 * DPT_RCCL_ID_BYTES bytes to the other ranks by any means (a file, a socket, MPI); every rank then calls
 * dpt_rccl_comm_create with the same id (collective: it blocks until all `world` ranks have joined).
 * RCCL is loaded on first use (dlopen of librccl.so.1: the copy the process already holds -- e.g.
 * PyTorch-ROCm's -- else the one on the library path), so libdpt.so itself does not depend on it;
 * without it these calls return DPT_E_RCCL.
 */
#define DPT_RCCL_ID_BYTES 128
int dpt_rccl_get_unique_id(uint8_t *id_out);
int dpt_rccl_comm_create(const uint8_t *id, int world, int rank, int device, void **comm_out);
int dpt_rccl_comm_destroy(void *rccl_comm);
/*
 * Sum hist[0..n) (device pointer, int64; the dpt_token_histogram layout) over every rank of
 * rccl_comm, in place, stream-ordered on hip_stream (NULL = the default stream): one ncclAllReduce.
 * rccl_comm is an ncclComm_t -- from dpt_rccl_comm_create or the caller's own RCCL setup.
 */
int dpt_hist_allreduce(int64_t *hist, size_t n, void *rccl_comm, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DPT_H */
