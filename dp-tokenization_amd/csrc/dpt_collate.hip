// dpt_collate.hip -- model-input batches from the ids of an encoded batch (dpt_collate, dpt_collate_pair).
//
// rows_kernel, a pure streaming pass: up to four [n_str, row_len] outputs are written (most of the traffic), each
// element is pad, a special or one id gathered from the string's own token range (include/dpt.h has the
// rules).  Threads are laid over the OUTPUT, flattened row-major, so every store instruction of a wave is a
// contiguous row segment (or the tail of one row and the head of the next) whatever the strings' lengths
// are, and a wave is not tied to a row: with row_len = 16 a wave covers four rows.
//
// The output is counted in units of V elements, V = 1 (the element path, any alignment) or 16 bytes' worth
// (4 x int32 / 2 x int64: one 16-byte store per output, taken when every output base, row_stride x width and
// row_len x width are multiples of 16, so a unit never leaves its row).  A block takes CHUNK consecutive
// units per round and strides over the chunks (the grid is capped at the resident blocks); a thread holds UNITS of
// them, THREADS apart, and issues the row loads (off, count, status) of all of them, then their id loads, then the
// stores, so UNITS x V id loads are in flight per thread.  Unit -> (row, column) needs a division by the row's units:
// the chunk's first row and column are kept incrementally across rounds (the grid's stride divided on the host), and
// inside a chunk the quotient is 0 or 1 for rows of at least CHUNK units and one 32 x 33-bit multiply by a host-made
// reciprocal for shorter ones (exact: the dividend stays under 2 x CHUNK).  Rows index in 64 bits.
// No LDS, no atomics, no workspace.
//
// What a row holds is the kernel's Rule: its launch struct, the units per thread, the per-call constants, a unit's
// row state (length, first column, source bases) and its loads, the value at a sequence position, which positions
// are in B and which carry a label, the fourth row output and what it stores per row beside lengths.
//   SingleRule (dpt_collate):      seq = [bos] kept [eos] from one source.
//   PairRule (dpt_collate_pair):   seq = [bos] A_kept [sep] B_kept [eos], each side with its own (ids, off, counts,
//                                  status); token_type_ids as the fourth output and b_start next to lengths.  A unit
//                                  carries two source bases, so it has its own units knob.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "dpt_internal.h"

namespace dpt {
namespace col {

constexpr unsigned THREADS = 256;
// A/B knobs (compile-time; make variant VSRC=dpt_collate.hip V=<tag> DEFS=..., then DPT_LIB=build/var_<tag>/libdpt.so):
// units per thread and round, non-temporal row stores, a fixed grid cap (0: the resident blocks).  Measured on
// cfg2: 8 units with non-temporal stores 3..12 % under 4 units with plain stores; 2 units
// slower than 4.
#ifndef DPT_COLLATE_UNITS
#define DPT_COLLATE_UNITS 8
#endif
#ifndef DPT_COLLATE_NT
#define DPT_COLLATE_NT 1
#endif
#ifndef DPT_COLLATE_BLOCKS
#define DPT_COLLATE_BLOCKS 0
#endif
// The pair rule's units per thread and round (make variant VSRC=dpt_collate.hip V=pu8 DEFS=-DDPT_COLLATE_PAIR_UNITS=8).
// Its row state is about twice the single rule's: 8 units take ~147 VGPRs (occupancy 3 waves per SIMD), 4 units ~81
// (5..6).  Measured on 1M pairs: 4 units 6 % under 8, 6 units between, 2 units 21 % over 4.
#ifndef DPT_COLLATE_PAIR_UNITS
#define DPT_COLLATE_PAIR_UNITS 4
#endif
constexpr unsigned MAX_BLOCKS_LIMIT = 4096;    // (blockIdx.x * CHUNK stays under 2^32 by far)
constexpr unsigned MAX_DEVICES = 64;

// how the flattened units map to rows (made on the host, launch)
struct Geometry {
    uint32_t lu;       // units per row
    uint32_t dr;       // the grid's stride (gridDim.x * CHUNK units) = dq rows + dr units
    uint64_t dq;
    uint64_t magic;    // ceil(2^32 / lu) for lu < CHUNK, else 0: the quotient is a compare
    uint64_t chunks;   // ceil(n_str * lu / CHUNK)
};

// the geometry of n_str rows of lu units under chunks of ``chunk`` units and at most max_blocks blocks -> the blocks
static unsigned make_geometry(Geometry &g, uint64_t n_str, uint32_t lu, unsigned chunk, unsigned max_blocks) {
    g.lu = lu;
    const uint64_t units = n_str * lu;
    g.chunks = (units + chunk - 1) / chunk;
    const unsigned blocks = (unsigned)(g.chunks < max_blocks ? g.chunks : max_blocks);
    const uint64_t stride = (uint64_t)blocks * chunk;
    g.dq = stride / lu;
    g.dr = (uint32_t)(stride % lu);
    g.magic = lu < chunk ? ((1ull << 32) + lu - 1) / lu : 0;
    return blocks;
}

template <typename T, int V>
using Vec = T __attribute__((ext_vector_type(V)));

template <typename T, int V>
__device__ __forceinline__ void store_unit(T *p, Vec<T, V> v) {
    if (DPT_COLLATE_NT) __builtin_nontemporal_store(v, reinterpret_cast<Vec<T, V> *>(p));
    else *reinterpret_cast<Vec<T, V> *>(p) = v;
}

// string ``row``'s offset, token count and status on one side (zeros for a unit past the last row)
__device__ __forceinline__ void load_side(const CollateSide &s, uint64_t row, bool live, uint64_t &o, uint64_t &n, int32_t &st) {
    o = 0, n = 0, st = 0;
    if (live) {
        o = s.off[row];
        n = s.counts ? s.counts[row] : s.off[row + 1] - o;
        if (s.status) st = s.status[row];
    }
}

// the per-call constants of both rules; ``seps``: the specials between bos and eos
struct Call {
    uint32_t flags, L, n_bos, n_special, room;
    __device__ Call(const CollateRows &r, uint32_t seps)
        : flags(r.flags), L(r.row_len), n_bos(has(DPT_COLLATE_BOS) ? 1u : 0u), n_special(n_bos + seps + (has(DPT_COLLATE_EOS) ? 1u : 0u)),
          room(L - n_special) {}   // (the host checked L >= n_special)
    __device__ __forceinline__ bool has(uint32_t flag) const { return (flags & flag) != 0; }
};

// The single rule (include/dpt.h dpt_collate): seq = [bos] kept [eos].
struct SingleRule {
    using Launch = CollateLaunch;
    static constexpr unsigned UNITS = DPT_COLLATE_UNITS;
    struct Call : col::Call {
        uint64_t off0;
        __device__ Call(const Launch &a) : col::Call(a.r, 0u), off0(a.src.off[0]) {}
    };
    struct Row {
        uint64_t src;           // ids index of sequence position 0 (the BOS's place when there is one)
        uint32_t len, start;    // the sequence's length (0: a failed string) and first column
    };
    static __device__ __forceinline__ Row load(const Launch &a, const Call &c, uint64_t row, bool live) {
        uint64_t o, n;
        int32_t st;
        load_side(a.src, row, live, o, n, st);
        const uint32_t keep = n < c.room ? (uint32_t)n : c.room;
        Row r;
        r.len = st != 0 ? 0u : keep + c.n_special;
        r.start = c.has(DPT_COLLATE_PAD_LEFT) ? c.L - r.len : 0u;
        // (the BOS's place as a 0 / 1 constant: with c.n_bos in this 64-bit sum <int64, 2> measured 1 % slower)
        r.src = o - c.off0 + (c.has(DPT_COLLATE_TRUNC_LEFT) ? n - keep : 0) - (c.has(DPT_COLLATE_BOS) ? 1u : 0u);
        return r;
    }
    // the value at sequence position p < r.len
    static __device__ __forceinline__ int32_t token(const Launch &a, const Call &c, const Row &r, uint32_t p) {
        if (c.has(DPT_COLLATE_BOS) && p == 0u) return a.r.bos_id;
        if (c.has(DPT_COLLATE_EOS) && p == r.len - 1u) return a.r.eos_id;
        return a.src.ids[r.src + p];
    }
    static __device__ __forceinline__ bool in_b(const Row &, uint32_t) { return false; }
    static __device__ __forceinline__ bool in_labels(const Call &, const Row &, uint32_t) { return true; }
    static __host__ __device__ void *extra(const Launch &) { return nullptr; }
    static __device__ __forceinline__ void per_row(const Launch &, const Row &, uint64_t) {}
};

// The pair rule (include/dpt.h dpt_collate_pair): seq = [bos] A_kept [sep] B_kept [eos].  The kept counts in closed
// form: the side that gives first keeps what the other leaves of the room, kA = min(cA, room) and kB = min(cB, room -
// kA) when B gives first (the sides swapped under TRIM_A_FIRST) -- the header's over / dA / dB arithmetic, which
// tests/test_collate_pair_ref.py checks exhaustively.  A unit's row state: bseq, the sequence position of B's first
// place (bos + kA + sep), splits the row into the A zone [0, bseq) and the B zone [bseq, len); FAILED (with len 0) marks
// a row one of whose statuses is non-zero.
struct PairRule {
    using Launch = CollatePairLaunch;
    static constexpr unsigned UNITS = DPT_COLLATE_PAIR_UNITS;
    static constexpr uint32_t FAILED = 0xFFFFFFFFu;   // (bseq <= row_len <= 2^31)
    struct Call : col::Call {
        uint32_t n_sep;
        uint64_t a_off0, b_off0;
        __device__ Call(const Launch &a)
            : col::Call(a.r, (a.r.flags & DPT_COLLATE_SEP) ? 1u : 0u), n_sep(has(DPT_COLLATE_SEP) ? 1u : 0u), a_off0(a.a.off[0]),
              b_off0(a.b.off[0]) {}
    };
    struct Row {
        uint64_t src_a, src_b;        // ids index of sequence position 0, per side
        uint32_t len, start, bseq;
    };
    static __device__ __forceinline__ Row load(const Launch &a, const Call &c, uint64_t row, bool live) {
        uint64_t oa, na, ob, nb;
        int32_t sta, stb;
        load_side(a.a, row, live, oa, na, sta);
        load_side(a.b, row, live, ob, nb, stb);
        const uint64_t ca = a.max_a && na > a.max_a ? a.max_a : na, cb = a.max_b && nb > a.max_b ? a.max_b : nb;
        uint32_t ka, kb;
        if (c.has(DPT_COLLATE_TRIM_A_FIRST)) {
            kb = cb < c.room ? (uint32_t)cb : c.room;
            ka = ca < c.room - kb ? (uint32_t)ca : c.room - kb;
        } else {
            ka = ca < c.room ? (uint32_t)ca : c.room;
            kb = cb < c.room - ka ? (uint32_t)cb : c.room - ka;
        }
        const bool failed = (sta | stb) != 0;
        Row r;
        r.bseq = failed ? FAILED : c.n_bos + ka + c.n_sep;
        r.len = failed ? 0u : ka + kb + c.n_special;
        r.start = c.has(DPT_COLLATE_PAD_LEFT) ? c.L - r.len : 0u;
        r.src_a = oa - c.a_off0 + (c.has(DPT_COLLATE_TRUNC_LEFT) ? na - ka : 0) - c.n_bos;
        r.src_b = ob - c.b_off0 + (c.has(DPT_COLLATE_TRUNC_LEFT) ? nb - kb : 0) - r.bseq;
        return r;
    }
    static __device__ __forceinline__ int32_t token(const Launch &a, const Call &c, const Row &r, uint32_t p) {
        const bool in_a = p < r.bseq;
        if (c.has(DPT_COLLATE_BOS) && p == 0u) return a.r.bos_id;
        if (c.has(DPT_COLLATE_SEP) && p + 1u == r.bseq) return a.sep_id;
        if (c.has(DPT_COLLATE_EOS) && p == r.len - 1u) return a.r.eos_id;
        return (in_a ? a.a.ids : a.b.ids)[(in_a ? r.src_a : r.src_b) + p];
    }
    static __device__ __forceinline__ bool in_b(const Row &r, uint32_t p) { return p >= r.bseq; }
    static __device__ __forceinline__ bool in_labels(const Call &c, const Row &r, uint32_t p) { return !c.has(DPT_COLLATE_MASK_A) || p >= r.bseq; }
    static __host__ __device__ void *extra(const Launch &a) { return a.token_type; }
    static __device__ __forceinline__ void per_row(const Launch &a, const Row &r, uint64_t row) {
        if (a.b_start) a.b_start[row] = r.bseq != FAILED ? r.start + r.bseq : 0u;
    }
};

template <typename T, int V, class Rule>
__global__ void __launch_bounds__(THREADS) rows_kernel(typename Rule::Launch a, Geometry g) {
    constexpr unsigned UNITS = Rule::UNITS, CHUNK = THREADS * UNITS;
    static_assert(2ull * CHUNK * CHUNK < (1ull << 32) && (uint64_t)MAX_BLOCKS_LIMIT * CHUNK < (1ull << 31), "32-bit unit arithmetic");
    const uint32_t LU = g.lu;
    const typename Rule::Call c(a);
    T *const out_ids = static_cast<T *>(a.r.input_ids);
    T *const out_mask = static_cast<T *>(a.r.mask);
    T *const out_lab = static_cast<T *>(a.r.labels);
    T *const out_extra = static_cast<T *>(Rule::extra(a));

    // the first unit of this block's chunk: row row0, unit r0 of it (blockIdx.x * CHUNK < 2^23)
    const uint32_t f0 = blockIdx.x * CHUNK;
    uint64_t row0 = f0 / LU;
    uint32_t r0 = f0 - (uint32_t)row0 * LU;
    for (uint64_t k = blockIdx.x; k < g.chunks; k += gridDim.x) {
        uint64_t row[UNITS];
        uint32_t col[UNITS];
        bool live[UNITS];
        typename Rule::Row rs[UNITS];
        // the rows' offsets, counts and statuses
#pragma unroll
        for (unsigned u = 0; u < UNITS; ++u) {
            const uint32_t x = r0 + threadIdx.x + u * THREADS;   // (< lu + CHUNK <= 2^31 + CHUNK)
            const uint32_t q = g.magic ? (uint32_t)(((uint64_t)x * g.magic) >> 32) : (x >= LU ? 1u : 0u);
            row[u] = row0 + q;
            col[u] = (x - q * LU) * (uint32_t)V;
            live[u] = row[u] < a.r.n_str;
            rs[u] = Rule::load(a, c, row[u], live[u]);
        }
        // the ids
        int32_t tok[UNITS][V];
#pragma unroll
        for (unsigned u = 0; u < UNITS; ++u) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t p = col[u] + (uint32_t)e - rs[u].start;   // position in the sequence (wraps: pad)
                tok[u][e] = live[u] && p < rs[u].len ? Rule::token(a, c, rs[u], p) : a.r.pad_id;
            }
        }
        // the stores
#pragma unroll
        for (unsigned u = 0; u < UNITS; ++u) {
            if (!live[u]) continue;
            Vec<T, V> vi, vm, vl, vx;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t p = col[u] + (uint32_t)e - rs[u].start;
                const bool in_seq = p < rs[u].len;
                vi[e] = (T)tok[u][e];
                vm[e] = in_seq ? (T)1 : (T)0;
                vl[e] = in_seq && Rule::in_labels(c, rs[u], p) ? (T)tok[u][e] : (T)a.r.ignore_id;
                vx[e] = in_seq && Rule::in_b(rs[u], p) ? (T)1 : (T)0;
            }
            const uint64_t at = row[u] * a.r.row_stride + col[u];
            store_unit<T, V>(out_ids + at, vi);
            if (out_mask) store_unit<T, V>(out_mask + at, vm);
            if (out_lab) store_unit<T, V>(out_lab + at, vl);
            if (out_extra) store_unit<T, V>(out_extra + at, vx);
            if (a.r.lengths && col[u] == 0u) a.r.lengths[row[u]] = rs[u].len;
            if (col[u] == 0u) Rule::per_row(a, rs[u], row[u]);
        }
        // the next chunk of this block
        row0 += g.dq;
        r0 += g.dr;
        if (r0 >= LU) {
            r0 -= LU;
            ++row0;
        }
    }
}

// The grid cap: the blocks that are resident at once (the occupancy the registers allow x the CUs; 5 x 256 on
// the MI355X).  More chunks than that: the blocks stride.  A cap of 1.6 x the resident blocks (2048) measured
// 8..12 % slower -- the second, partial wave of blocks runs on a part-empty chip -- and 0.8 x (1024) 2..6 %.
// Asked of the runtime once per kernel and device (a host-side query: no synchronisation, no device work).
template <typename K>
unsigned grid_cap(K kernel, unsigned *cache) {
    if (DPT_COLLATE_BLOCKS) return DPT_COLLATE_BLOCKS;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= (int)MAX_DEVICES) return 1280;
    if (!cache[dev]) {
        int per_cu = 0, cus = 0;
        const bool ok = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, THREADS, 0) == hipSuccess &&
                        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per_cu > 0 && cus > 0;
        const uint64_t n = ok ? (uint64_t)per_cu * (uint64_t)cus : 1280;
        cache[dev] = (unsigned)(n < MAX_BLOCKS_LIMIT ? n : MAX_BLOCKS_LIMIT);
    }
    return cache[dev];
}

template <typename T, int V, class Rule>
hipError_t launch(const typename Rule::Launch &p, hipStream_t stream) {
    static unsigned cache[MAX_DEVICES];   // (0: not asked yet; a race stores the same value twice)
    Geometry g;
    const unsigned blocks = make_geometry(g, p.r.n_str, p.r.row_len / (uint32_t)V, THREADS * Rule::UNITS,
                                          grid_cap(rows_kernel<T, V, Rule>, cache));
    hipLaunchKernelGGL((rows_kernel<T, V, Rule>), dim3(blocks), dim3(THREADS), 0, stream, p, g);
    return hipGetLastError();
}

// A/B knob (tools/collate_bench.py): DPT_COLLATE_NO_WIDE=1 sends every call through the element path
static bool no_wide() {
    static const bool v = [] {
        const char *e = getenv("DPT_COLLATE_NO_WIDE");
        return e && e[0] == '1';
    }();
    return v;
}

// the element width and the store path of one call
template <class Rule>
hipError_t launch_rows(const typename Rule::Launch &p, hipStream_t stream) {
    if (p.r.n_str == 0) return hipSuccess;
    const bool i64 = (p.r.flags & DPT_COLLATE_I64) != 0;
    const unsigned width = i64 ? 8 : 4, v = 16 / width;
    // the 16-byte path: a unit of v elements never leaves its row and every store is 16-byte aligned
    const uintptr_t bases = (uintptr_t)p.r.input_ids | (uintptr_t)p.r.mask | (uintptr_t)p.r.labels | (uintptr_t)Rule::extra(p);
    const bool wide = !no_wide() && bases % 16 == 0 && p.r.row_len % v == 0 && p.r.row_stride % v == 0;
    if (i64) return wide ? launch<int64_t, 2, Rule>(p, stream) : launch<int64_t, 1, Rule>(p, stream);
    return wide ? launch<int32_t, 4, Rule>(p, stream) : launch<int32_t, 1, Rule>(p, stream);
}

}  // namespace col

hipError_t launch_collate(const CollateLaunch &p, hipStream_t stream) { return col::launch_rows<col::SingleRule>(p, stream); }

hipError_t launch_collate_pair(const CollatePairLaunch &p, hipStream_t stream) { return col::launch_rows<col::PairRule>(p, stream); }

}  // namespace dpt
