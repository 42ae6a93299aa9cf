// dpt_tok_lds.h -- what a tokenize wave holds and is handed: the lane-group geometry (Group, Wfin), a wave's LDS
// layout (GroupLDS, SlotState, the strides), trie access (TrieView), the kernel arguments (EncodeArgs, KernArgs) and
// the diagnostic builds' stamp macros.  Read by dpt_kernels.hip: prep, TokPass and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace dpt {

// ------------------------------------------------------------------ group geometry

template <int G> struct Group;

// G = 16: four strings per wave, one per DPP row.  Per atom: {cpos, ~span mask} in one
// dword (after phase B the mask half of a word-end atom holds the word's final key, Wfin<16>,
// and in C1 the mask halves take the selected tokens); per end position i, one u16 `fin`:
// the back distances (minus one) of the largest reachable j in E(i) attaining G[i] (dg) and
// of the largest reachable j in E(i) (de), 4 bits each.  Both exist at every position of a
// valid word's selected path (Appendix A: a reachable i has a reachable j attaining its key),
// and C1 walks valid words only, so no "none" code is stored.
template <> struct Group<16> {
    using M = uint16_t;
    // smask: until phase B, the inverted END mask of end position i: bit d clear = atoms
    // i-1-d .. i-1 are a token (phase A clears the bits with LDS atomics)
    struct Rec { uint16_t cpos; uint16_t smask; };
    struct Fin { uint8_t v; };   // dg | de << 4
    static __device__ __forceinline__ unsigned dg(const Fin &x) { return x.v & 15u; }
    static __device__ __forceinline__ unsigned de(const Fin &x) { return (x.v >> 4) & 15u; }
};

// G = 64: one string per wave (vocabularies with tokens of 17..64 code points).
template <> struct Group<64> {
    using M = uint64_t;
    struct Rec { uint64_t smask; uint16_t cpos; uint16_t pad[3]; };
    struct Fin { uint32_t d; uint32_t w; };   // w: the final key (Wfin<64>)
    static __device__ __forceinline__ unsigned dg(const Fin &x) { return x.d & 127u; }
    static __device__ __forceinline__ unsigned de(const Fin &x) { return (x.d >> 8) & 127u; }
};

// ------------------------------------------------------------------ LDS layout

constexpr uint16_t CP_WS = 0x8000;        // cpos bit: atom starts a word
constexpr unsigned MAX_ATOM_BYTES = 8;    // expanded atom = one u64 (raw: '▁'+4-byte code point = 7)

// final state at a word end.  G = 16: 16 bits in the word-end atom's mask half:
// cost << 6 | invalid << 5 | 31-G, straight from the key (its bits 10..14 are constant 1s);
// cost 1023 = the uncapped DP's "inf" (0xFFFF, inspect_tokenizer.py:80), capped costs <= CH
template <int G> struct Wfin;
template <> struct Wfin<16> {
    using T = uint16_t;
    // one v_bfi: bits 5..15 from r >> 10, the rest from r (bits 16+ fall off in the u16)
    static __device__ __forceinline__ T pack(unsigned r) {
        unsigned o;
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(o) : "s"(0xFFE0u), "v"(r >> 10), "v"(r));
        return (T)o;
    }
    static __device__ __forceinline__ unsigned cost(T x) { return (x >> 6) == 1023u ? 0xFFFFu : (x >> 6); }
    static __device__ __forceinline__ bool invalid(T x) { return (x >> 5) & 1u; }
    static __device__ __forceinline__ unsigned gmax(T x) { return 31u - (x & 31u); }
};
template <> struct Wfin<64> {
    using T = uint32_t;   // the group-min key itself: cost<<16 | invalid<<15 | 0x7FFF-G
    static __device__ __forceinline__ T pack(unsigned r) { return r; }
    static __device__ __forceinline__ unsigned cost(T x) { return x >> 16; }
    static __device__ __forceinline__ bool invalid(T x) { return (x >> 15) & 1u; }
    static __device__ __forceinline__ unsigned gmax(T x) { return 0x7FFFu - (x & 0x7FFFu); }
};

// G = 64: rec[] as two arrays (span masks, code-point prefixes) -- 10 bytes per atom instead of the
// 16 of an aligned struct, so LDS per wave (5.2 KB) holds more resident waves than the 24 that 80
// VGPRs allow; rec[j] yields references to both fields, so the shared code reads L.rec[j].cpos alike
template <int NA> struct RecSoA {
    uint64_t sm[NA];
    uint16_t cp[NA];
    struct Ref { uint64_t &smask; uint16_t &cpos; };
    struct CRef { const uint64_t &smask; const uint16_t &cpos; };
    __device__ __forceinline__ Ref operator[](unsigned i) { return {sm[i], cp[i]}; }
    __device__ __forceinline__ CRef operator[](unsigned i) const { return {sm[i], cp[i]}; }
};

template <int CH, int G>
struct GroupLDS {
    using M = typename Group<G>::M;
    static constexpr int NA = CH + 2;            // atoms + sentinel
    // rec[j]: code-point prefix of atom j (| CP_WS at word starts and at the window end) and the
    //         span mask of tokens of 1..G atoms starting at j; after phase B the mask field holds
    //         the first atom of selected token j (tokens tile the window)
    std::conditional_t<(G == 64), RecSoA<NA>, typename Group<G>::Rec[NA]> rec;
    typename Group<G>::Fin fin[NA];   // per end position, see Group<G>
    // the final key of the word ending at atom e
    __device__ __forceinline__ typename Wfin<G>::T wkey(unsigned e) const {
        if constexpr (G == 16) return rec[e].smask;
        else return fin[e].w;
    }
    // CH = 256: u8, stored mod 256 -- offsets and word starts are < 256; the sentinels (wlen,
    // n_atoms <= 256) are recovered with modular differences (atom_len, word_end)
    using Idx = std::conditional_t<(CH <= 256), uint8_t, uint16_t>;
    // word -> first atom: in global scratch for 256-byte windows (WSLG; LDS is what limits the
    // resident waves there), in LDS for the 2048-byte pass
    static constexpr bool WSLG = CH <= 256;
    static constexpr int WSL_STRIDE = (NA + 15) & ~15;
    Idx aoff[NA];                   // atom -> byte offset in the window
    Idx wsl[WSLG ? 1 : NA];
    __device__ __forceinline__ unsigned atom_len(unsigned j) const { return (Idx)(aoff[j + 1] - aoff[j]); }
    // word w's first atom / its end (= the next word's first atom, or n_atoms)
    __device__ __forceinline__ unsigned word_start(const uint8_t *gw, unsigned w) const {
        if constexpr (WSLG) return gw[w];
        else return wsl[w];
    }
    __device__ __forceinline__ unsigned word_end(const uint8_t *gw, unsigned w) const {
        if constexpr (WSLG) return (((unsigned)gw[w + 1] + 255u) & 0xFFu) + 1u;
        else return wsl[w + 1];
    }
    __device__ __forceinline__ void set_word_start(uint8_t *gw, unsigned w, unsigned v) {
        if constexpr (WSLG) gw[w] = (uint8_t)v;
        else wsl[w] = (Idx)v;
    }
    // the window's input bytes (expanded on the fly); the dword reads of the last atoms run up to
    // 12 bytes past the end, into the next group or the slot states -- masked off, never used
    alignas(16) uint8_t bytes[CH];
    // G = 64, 256-byte windows, non-raw modes (no expansions: a token's bytes are the window's): per byte
    // position p <= wlen, byte[p] | BF_ATOM (an atom starts at p, or p == wlen) | BF_STOP (a word starts
    // at p, or p == wlen) -- phase A's byte-stream walker reads ONE u16 per trie step
    // (zero-length when unused: one spare byte here rounded the 16-lane group up 16 bytes -- 21 resident
    // waves per CU instead of 22, and the slots' bank interleaving off; the static_assert below holds it)
    static constexpr bool BSTREAM = G == 64 && CH == 256;
    uint16_t bf[BSTREAM ? CH + 2 : 0];
    // ... and per atom: 1 = it starts a word that is one vocabulary token (the whole-word shortcut)
    uint8_t scf[BSTREAM ? CH + 2 : 0];
};
constexpr unsigned BF_ATOM = 0x100u, BF_STOP = 0x200u;

// strings are < 4 GiB (dpt.h); abase: atoms of the string's earlier windows
// (48 bytes: LDS per slot is what bounds the resident waves)
struct SlotState {
    uint64_t sb;
    uint32_t s, slen, pos, ntok, capsum, wtok;
    uint32_t abase;
    uint16_t wlen, n_atoms, n_words;
    uint8_t active, status, inval, capb;   // capb: some atom of the window is not a token by itself (the cap can bind)
    uint8_t cpw;   // a '\u2581'-compressed PRESPLIT window (prep_window): raw mode's ASCII paths, no first-atom rule
    uint8_t pad;
};
static_assert(sizeof(SlotState) == 48, "slot state layout");

template <int CH, int G>
constexpr int group_lds_bytes() { return (int)((sizeof(GroupLDS<CH, G>) + 15) & ~size_t(15)); }

// A wave's LDS: per slot g its group's arrays, then its SlotState -- slot g at g * group_stride.  The
// 16-lane kernel's stride (1856 B = 464 dwords, 16 mod 32) puts the two DPP rows of a 32-lane LDS lane group
// (slots 0 / 1, 2 / 3) half a bank row apart: lane-mode B and C1 step through chunks 17 atoms apart, and
// two slots 452 dwords apart (the arrays back to back, then the slot states) made most of those reads
// 2-way bank conflicts; interleaved, the same bytes are conflict-free.
template <int CH, int G>
constexpr int group_stride() { return group_lds_bytes<CH, G>() + (int)sizeof(SlotState); }
static_assert(group_stride<256, 16>() == 1856, "16-lane group stride: 21 resident waves per CU (512-B LDS granule), slots 16 dwords mod 32 apart");
template <int CH, int G>
constexpr int block_lds_bytes() { return (64 / G) * group_stride<CH, G>(); }

// ------------------------------------------------------------------ trie access

struct TrieView {
    // .x = base | TERM<<31 | LEAF<<30, .y = check (parent slot, -1 free); followed by the 65536-entry
    // two-byte root table (entry b0 << 8 | b1 at slots[n_slots + ...], see dpt_api.cpp)
    const int2 *__restrict__ slots;
    const int32_t *__restrict__ ids;  // token id of a terminal slot
    const int4 *__restrict__ slots4;  // {base, check, id, 0}: C2's walks get the id with the last node
    int32_t root_base;
    uint32_t n_slots;
    // [b0 << 8 | b1]: id of the two-byte token, [65536 + b0]: of the one-byte one (-1: none); then, from
    // element PAIR16_N, A0's uint2 table [b0 << 8 | b1]: flags (root child b0, b0 a token, node b0 b1, its
    // TERM, LEAF) + that node's child filter
    const int16_t *__restrict__ pair16;
};

// Trie reads through buffer resources: 32-bit slot offsets (no 64-bit address arithmetic) and a
// range check that makes any index safe (out of range reads {0, 0}: a failed transition).
__device__ __forceinline__ int2 trie_slot(const TrieView &tv, int32_t t) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)tv.slots, (short)0, (int)((tv.n_slots + 65536u) * 8u), 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, (unsigned)t * 8u, 0, 0);
    return make_int2((int32_t)v[0], (int32_t)v[1]);
}
// phase A: {base, check, id, child filter} per slot, then the root table as {.x, .y, 0, child
// filter} (dpt_api.cpp), so one 16-byte load serves both
__device__ __forceinline__ int4 trie_slotA(const TrieView &tv, int32_t t) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)tv.slots4, (short)0, (int)((tv.n_slots + 65536u) * 16u), 0x00020000);
    return __builtin_bit_cast(int4, __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)t * 16u, 0, 0));
}
__device__ __forceinline__ int4 trie_slot4(const TrieView &tv, int32_t t) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)tv.slots4, (short)0, (int)(tv.n_slots * 16u), 0x00020000);
    return __builtin_bit_cast(int4, __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)t * 16u, 0, 0));
}

[[maybe_unused]] constexpr int32_t TERM_BIT = (int32_t)0x80000000;
[[maybe_unused]] constexpr int32_t LEAF_BIT = 0x40000000;  // no children (dpt_long.hip ends walks on it; this kernel uses the child filters)
constexpr int32_t BASE_MASK = 0x3FFFFFFF;

// ------------------------------------------------------------------ arguments

struct EncodeArgs {
    const uint8_t *text;
    const uint64_t *str_off;
    const uint8_t *cut_mask;    // PRESPLIT / ATOMS only
    uint64_t n_str;
    int32_t *staging;           // ids staged at (str_off[s]-str_off[0]) + k
    int16_t *staging16;         // non-null: the ids are staged here as int16 instead (half the bytes)
    uint64_t *counts;           // per string
    unsigned long long *bsum;   // nullable: the batch lines (dpt_internal.h BS_LINE): per FIN_BATCH strings, the sum of
                                //   their counts (atomics as strings finish)
    int32_t *status;
    int32_t *capped;            // nullable
    uint32_t *retry_list;       // strings for the 2048-byte pass
    uint32_t *retry_count;
    uint32_t *long_list;        // strings for the unbounded pass (dpt_long.hip)
    uint32_t *long_count;
    const uint32_t *work_list;  // 2048-byte pass: the retry list
    const uint32_t *work_count;
    uint32_t *work_next;        // 2048-byte pass: its work counter (zeroed per launch)
    uint32_t *part_ctr;         // first pass: NPART partition counters (PART_STRIDE apart), then the used-up mask
    uint8_t *wsl_scratch;       // word lists of the 256-byte pass: grid x NG x WSL_STRIDE bytes
    uint4 *pend;                // 16-lane first pass: per wave, 64 pending residual tokens (walk_pending)
    int32_t ws_node, ws_base, ws_id;   // the trie node after U+2581, its base word and id (-1: none)
    int long_span;              // the vocabulary has tokens longer than 64 code points
    uint64_t *edges;            // nullable: per atom end, the E(i) & reachable back-distance mask
    int mode;                   // DPT_MODE_* | DPT_FLAG_*
    unsigned long long *hist_zero;   // 2048-byte pass, fin_fold calls with DPT_HIST_OVERWRITE: the histogram to
    uint32_t n_hist;                 //   zero before the finish pass adds to it (the scan kernel's duty otherwise)
    uint64_t *id_off;
    int32_t *ids;
    // one-string host-path calls (EncodeLaunch::solo): the string's ids go straight to ids (staging =
    // ids, counts = id_off + 1) and the lone wave writes id_off[0] and resets the counter block (its
    // first 64 bytes to ctr_snap) -- no fallback, scan or finish launch follows
    int solo;
    uint64_t *ctr_snap;
};

#ifdef DPT_STAMPS
// diagnostic build only: cycles per phase summed over waves (never in the product build)
__device__ unsigned long long g_stamps[10];
// (the wave's stamps: the driver's, handed to the one phase that stamps inside itself, C2)
struct Stamps {
    unsigned long long acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long prev = __builtin_amdgcn_s_memtime();
};
#define STAMP(k) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); st.acc[k] += _t - st.prev; st.prev = _t; } while (0)
#define STAMP_FLUSH do { if (lane == 0) for (int _k = 0; _k < 10; _k++) atomicAdd(&g_stamps[_k], st.acc[_k]); } while (0)
#else
struct Stamps {};
#define STAMP(k)
#define STAMP_FLUSH
#endif
#ifdef DPT_WSTAMPS
// diagnostic build only (its own library, no phase stamps): the first pass's per-wave timeline (tools/wave_timeline.py): per wave (blockIdx), [0] its first
// instruction, [1 + k] the end of its k-th slot round (| the round's busy slots << 56), [WST_N - 1] its exit
// (| its rounds << 48); s_memrealtime (100 MHz, one clock for the whole chip)
constexpr unsigned WST_MAXW = 8192, WST_N = 128;
__device__ unsigned long long g_wst[WST_MAXW * WST_N];
#define WST_REC(k, v) do { if (!BIG && lane == 0 && bid < WST_MAXW && (unsigned)(k) < WST_N) g_wst[(size_t)bid * WST_N + (k)] = (v); } while (0)
#define WST_NOW() ((unsigned long long)__builtin_amdgcn_s_memrealtime())
#else
#define WST_REC(k, v)
#define WST_NOW() 0ull
#endif

// The kernel's arguments, as one struct at the start of the kernarg segment
struct KernArgs {
    EncodeArgs ea;
    TrieView tv;
};
typedef __attribute__((address_space(4))) const KernArgs ConstKernArgs;
// Arguments are read through the kernarg segment pointer, which KREFRESH makes opaque at every phase
// boundary: each phase then loads (s_load, scalar-cache hits) the few arguments it uses instead of
// the compiler keeping all ~30 of them in SGPRs across the whole loop -- the hot kernel sits at the
// SGPR limit and spills.
// (a field-wise copy: only the fields a use reads are loaded)
__device__ __forceinline__ TrieView tv_of(ConstKernArgs *kp) {
    TrieView t;
    t.slots = kp->tv.slots; t.ids = kp->tv.ids; t.slots4 = kp->tv.slots4;
    t.root_base = kp->tv.root_base; t.n_slots = kp->tv.n_slots; t.pair16 = kp->tv.pair16;
    return t;
}
// (the 16-lane instantiations: the 64-lane ones do not spill, and measured 1.7 % slower with it)
#define KREFRESH() do { if constexpr (G == 16) asm volatile("" : "+s"(kp)); } while (0)

}  // namespace dpt
