// dpt_collate.hip -- model-input batches from the ids of an encoded batch (dpt_collate).
//
// A pure streaming pass: up to three [n_str, row_len] outputs are written (most of the traffic), each
// element is pad, a special or one id gathered from the string's own token range (include/dpt.h has the
// rule).  Threads are laid over the OUTPUT, flattened row-major, so every store instruction of a wave is a
// contiguous row segment (or the tail of one row and the head of the next) whatever the strings' lengths
// are, and a wave is not tied to a row: with row_len = 16 a wave covers four rows.
//
// The output is counted in units of V elements, V = 1 (the element path, any alignment) or 16 bytes' worth
// (4 x int32 / 2 x int64: one 16-byte store per output, taken when every output base, row_stride x width and
// row_len x width are multiples of 16, so a unit never leaves its row).  A block takes CHUNK consecutive
// units per round and strides over the chunks (the grid is capped at the resident blocks); a thread holds UNITS of them, THREADS apart, and issues the
// row loads (off, count, status) of all of them, then their id loads, then the stores, so UNITS x V id loads
// are in flight per thread.  Unit -> (row, column) needs a division by the row's units: the chunk's first
// row and column are kept incrementally across rounds (the grid's stride divided on the host), and inside a
// chunk the quotient is 0 or 1 for rows of at least CHUNK units and one 32 x 33-bit multiply by a host-made
// reciprocal for shorter ones (exact: the dividend stays under 2 x CHUNK).  Rows index in 64 bits.
// No LDS, no atomics, no workspace.
//
// collate_pair_kernel (dpt_collate_pair) is the same pass over rows of two segments -- [bos] A [sep] B [eos], each
// side with its own (ids, off, counts, status) -- with a fourth row output (token_type_ids) and b_start next to
// lengths.  Same geometry, stores and grid cap; a unit carries two source bases, so it has its own units knob.
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
// The pair kernel's units per thread and round (make variant VSRC=dpt_collate.hip V=pu8 DEFS=-DDPT_COLLATE_PAIR_UNITS=8).
// Its row state is about twice collate_kernel's: 8 units take ~147 VGPRs (occupancy 3 waves per SIMD), 4 units ~81
// (5..6).  Measured on 1M pairs: 4 units 6 % under 8, 6 units between, 2 units 21 % over 4.
#ifndef DPT_COLLATE_PAIR_UNITS
#define DPT_COLLATE_PAIR_UNITS 4
#endif
constexpr unsigned UNITS = DPT_COLLATE_UNITS;  // units per thread and round
constexpr unsigned CHUNK = THREADS * UNITS;    // units per block and round
constexpr unsigned PAIR_UNITS = DPT_COLLATE_PAIR_UNITS;
constexpr unsigned PAIR_CHUNK = THREADS * PAIR_UNITS;
constexpr unsigned MAX_BLOCKS_LIMIT = 4096;    // (blockIdx.x * CHUNK stays under 2^32 by far)
constexpr unsigned MAX_DEVICES = 64;
static_assert(2ull * CHUNK * CHUNK < (1ull << 32) && (uint64_t)MAX_BLOCKS_LIMIT * CHUNK < (1ull << 31), "32-bit unit arithmetic");
static_assert(2ull * PAIR_CHUNK * PAIR_CHUNK < (1ull << 32) && (uint64_t)MAX_BLOCKS_LIMIT * PAIR_CHUNK < (1ull << 31),
              "32-bit unit arithmetic");

// how the flattened units map to rows (made on the host, launch_collate)
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

template <typename T, int V>
__global__ void __launch_bounds__(THREADS) collate_kernel(CollateLaunch a, Geometry g) {
    const uint32_t L = a.row_len, LU = g.lu;
    const bool bos = (a.flags & DPT_COLLATE_BOS) != 0, eos = (a.flags & DPT_COLLATE_EOS) != 0;
    const bool pad_left = (a.flags & DPT_COLLATE_PAD_LEFT) != 0, trunc_left = (a.flags & DPT_COLLATE_TRUNC_LEFT) != 0;
    const uint32_t n_special = (bos ? 1u : 0u) + (eos ? 1u : 0u);
    const uint32_t room = L - n_special;   // (the host checked L >= n_special)
    const uint64_t off0 = a.off[0];
    T *const out_ids = static_cast<T *>(a.input_ids);
    T *const out_mask = static_cast<T *>(a.mask);
    T *const out_lab = static_cast<T *>(a.labels);

    // the first unit of this block's chunk: row row0, unit r0 of it (blockIdx.x * CHUNK < 2^23)
    const uint32_t f0 = blockIdx.x * CHUNK;
    uint64_t row0 = f0 / LU;
    uint32_t r0 = f0 - (uint32_t)row0 * LU;
    for (uint64_t c = blockIdx.x; c < g.chunks; c += gridDim.x) {
        uint64_t row[UNITS], src[UNITS];
        uint32_t col[UNITS], len[UNITS], start[UNITS];
        bool live[UNITS];
        // the rows' offsets, counts and statuses
#pragma unroll
        for (unsigned u = 0; u < UNITS; ++u) {
            const uint32_t x = r0 + threadIdx.x + u * THREADS;   // (< lu + CHUNK <= 2^31 + CHUNK)
            const uint32_t q = g.magic ? (uint32_t)(((uint64_t)x * g.magic) >> 32) : (x >= LU ? 1u : 0u);
            row[u] = row0 + q;
            col[u] = (x - q * LU) * (uint32_t)V;
            live[u] = row[u] < a.n_str;
            uint64_t o = 0, n = 0;
            int32_t st = 0;
            if (live[u]) {
                o = a.off[row[u]];
                n = a.counts ? a.counts[row[u]] : a.off[row[u] + 1] - o;
                if (a.status) st = a.status[row[u]];
            }
            const uint32_t keep = n < room ? (uint32_t)n : room;
            len[u] = st != 0 ? 0u : keep + n_special;
            start[u] = pad_left ? L - len[u] : 0u;
            // ids index of sequence position 0 (the BOS's place when there is one)
            src[u] = o - off0 + (trunc_left ? n - keep : 0) - (bos ? 1u : 0u);
        }
        // the ids
        int32_t tok[UNITS][V];
#pragma unroll
        for (unsigned u = 0; u < UNITS; ++u) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t p = col[u] + (uint32_t)e - start[u];   // position in the sequence (wraps: pad)
                int32_t v = a.pad_id;
                if (live[u] && p < len[u]) {
                    if (bos && p == 0u) v = a.bos_id;
                    else if (eos && p == len[u] - 1u) v = a.eos_id;
                    else v = a.ids[src[u] + p];
                }
                tok[u][e] = v;
            }
        }
        // the stores
#pragma unroll
        for (unsigned u = 0; u < UNITS; ++u) {
            if (!live[u]) continue;
            Vec<T, V> vi, vm, vl;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const bool in_seq = col[u] + (uint32_t)e - start[u] < len[u];
                vi[e] = (T)tok[u][e];
                vm[e] = in_seq ? (T)1 : (T)0;
                vl[e] = in_seq ? (T)tok[u][e] : (T)a.ignore_id;
            }
            const uint64_t at = row[u] * a.row_stride + col[u];
            store_unit<T, V>(out_ids + at, vi);
            if (out_mask) store_unit<T, V>(out_mask + at, vm);
            if (out_lab) store_unit<T, V>(out_lab + at, vl);
            if (a.lengths && col[u] == 0u) a.lengths[row[u]] = len[u];
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

// string ``row``'s offset, token count and status on one side (zeros for a unit past the last row)
__device__ __forceinline__ void load_side(const CollateSide &s, uint64_t row, bool live, uint64_t &o, uint64_t &n, int32_t &st) {
    o = 0, n = 0, st = 0;
    if (live) {
        o = s.off[row];
        n = s.counts ? s.counts[row] : s.off[row + 1] - o;
        if (s.status) st = s.status[row];
    }
}

// The pair rule (include/dpt.h dpt_collate_pair): seq = [bos] A_kept [sep] B_kept [eos].  The kept counts in closed
// form: the side that gives first keeps what the other leaves of the room, kA = min(cA, room) and kB = min(cB, room -
// kA) when B gives first (the sides swapped under TRIM_A_FIRST) -- the header's over / dA / dB arithmetic, which
// tests/test_collate_pair_ref.py checks exhaustively.  A unit's row state: bseq, the sequence position of B's first
// place (bos + kA + sep), splits the row into the A zone [0, bseq) and the B zone [bseq, len); FAILED (with len 0) marks
// a row one of whose statuses is non-zero.
constexpr uint32_t FAILED = 0xFFFFFFFFu;   // (bseq <= row_len <= 2^31)

template <typename T, int V>
__global__ void __launch_bounds__(THREADS) collate_pair_kernel(CollatePairLaunch a, Geometry g) {
    const uint32_t L = a.row_len, LU = g.lu;
    const bool bos = (a.flags & DPT_COLLATE_BOS) != 0, eos = (a.flags & DPT_COLLATE_EOS) != 0, sep = (a.flags & DPT_COLLATE_SEP) != 0;
    const bool pad_left = (a.flags & DPT_COLLATE_PAD_LEFT) != 0, trunc_left = (a.flags & DPT_COLLATE_TRUNC_LEFT) != 0;
    const bool mask_a = (a.flags & DPT_COLLATE_MASK_A) != 0, a_first = (a.flags & DPT_COLLATE_TRIM_A_FIRST) != 0;
    const uint32_t n_bos = bos ? 1u : 0u, n_sep = sep ? 1u : 0u;
    const uint32_t n_special = n_bos + n_sep + (eos ? 1u : 0u);
    const uint32_t room = L - n_special;   // (the host checked L >= n_special)
    const uint64_t a_off0 = a.a.off[0], b_off0 = a.b.off[0];
    T *const out_ids = static_cast<T *>(a.input_ids);
    T *const out_mask = static_cast<T *>(a.mask);
    T *const out_lab = static_cast<T *>(a.labels);
    T *const out_type = static_cast<T *>(a.token_type);

    const uint32_t f0 = blockIdx.x * PAIR_CHUNK;
    uint64_t row0 = f0 / LU;
    uint32_t r0 = f0 - (uint32_t)row0 * LU;
    for (uint64_t c = blockIdx.x; c < g.chunks; c += gridDim.x) {
        uint64_t row[PAIR_UNITS], src_a[PAIR_UNITS], src_b[PAIR_UNITS];
        uint32_t col[PAIR_UNITS], len[PAIR_UNITS], start[PAIR_UNITS], bseq[PAIR_UNITS];
        bool live[PAIR_UNITS];
        // both sides' offsets, counts and statuses
#pragma unroll
        for (unsigned u = 0; u < PAIR_UNITS; ++u) {
            const uint32_t x = r0 + threadIdx.x + u * THREADS;
            const uint32_t q = g.magic ? (uint32_t)(((uint64_t)x * g.magic) >> 32) : (x >= LU ? 1u : 0u);
            row[u] = row0 + q;
            col[u] = (x - q * LU) * (uint32_t)V;
            live[u] = row[u] < a.n_str;
            uint64_t oa, na, ob, nb;
            int32_t sta, stb;
            load_side(a.a, row[u], live[u], oa, na, sta);
            load_side(a.b, row[u], live[u], ob, nb, stb);
            const uint64_t ca = a.max_a && na > a.max_a ? a.max_a : na, cb = a.max_b && nb > a.max_b ? a.max_b : nb;
            uint32_t ka, kb;
            if (a_first) {
                kb = cb < room ? (uint32_t)cb : room;
                ka = ca < room - kb ? (uint32_t)ca : room - kb;
            } else {
                ka = ca < room ? (uint32_t)ca : room;
                kb = cb < room - ka ? (uint32_t)cb : room - ka;
            }
            const bool failed = (sta | stb) != 0;
            bseq[u] = failed ? FAILED : n_bos + ka + n_sep;
            len[u] = failed ? 0u : ka + kb + n_special;
            start[u] = pad_left ? L - len[u] : 0u;
            // ids index of sequence position 0, per side
            src_a[u] = oa - a_off0 + (trunc_left ? na - ka : 0) - n_bos;
            src_b[u] = ob - b_off0 + (trunc_left ? nb - kb : 0) - bseq[u];
        }
        // the ids
        int32_t tok[PAIR_UNITS][V];
#pragma unroll
        for (unsigned u = 0; u < PAIR_UNITS; ++u) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t p = col[u] + (uint32_t)e - start[u];   // position in the sequence (wraps: pad)
                int32_t v = a.pad_id;
                if (live[u] && p < len[u]) {
                    const bool in_a = p < bseq[u];
                    if (bos && p == 0u) v = a.bos_id;
                    else if (sep && p + 1u == bseq[u]) v = a.sep_id;
                    else if (eos && p == len[u] - 1u) v = a.eos_id;
                    else v = (in_a ? a.a.ids : a.b.ids)[(in_a ? src_a[u] : src_b[u]) + p];
                }
                tok[u][e] = v;
            }
        }
        // the stores
#pragma unroll
        for (unsigned u = 0; u < PAIR_UNITS; ++u) {
            if (!live[u]) continue;
            Vec<T, V> vi, vm, vl, vt;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t p = col[u] + (uint32_t)e - start[u];
                const bool in_seq = p < len[u], in_b = in_seq && p >= bseq[u];
                vi[e] = (T)tok[u][e];
                vm[e] = in_seq ? (T)1 : (T)0;
                vl[e] = (mask_a ? in_b : in_seq) ? (T)tok[u][e] : (T)a.ignore_id;
                vt[e] = in_b ? (T)1 : (T)0;
            }
            const uint64_t at = row[u] * a.row_stride + col[u];
            store_unit<T, V>(out_ids + at, vi);
            if (out_mask) store_unit<T, V>(out_mask + at, vm);
            if (out_lab) store_unit<T, V>(out_lab + at, vl);
            if (out_type) store_unit<T, V>(out_type + at, vt);
            if (col[u] == 0u) {
                if (a.lengths) a.lengths[row[u]] = len[u];
                if (a.b_start) a.b_start[row[u]] = bseq[u] != FAILED ? start[u] + bseq[u] : 0u;
            }
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
unsigned grid_cap_of(K kernel, unsigned *cache) {
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

template <typename T, int V>
unsigned grid_cap() {
    static unsigned cache[MAX_DEVICES];   // (0: not asked yet; a race stores the same value twice)
    return grid_cap_of(collate_kernel<T, V>, cache);
}

template <typename T, int V>
hipError_t launch(const CollateLaunch &p, hipStream_t stream) {
    Geometry g;
    const unsigned blocks = make_geometry(g, p.n_str, p.row_len / (uint32_t)V, CHUNK, grid_cap<T, V>());
    hipLaunchKernelGGL((collate_kernel<T, V>), dim3(blocks), dim3(THREADS), 0, stream, p, g);
    return hipGetLastError();
}

template <typename T, int V>
hipError_t launch_pair(const CollatePairLaunch &p, hipStream_t stream) {
    static unsigned cache[MAX_DEVICES];
    Geometry g;
    const unsigned blocks = make_geometry(g, p.n_str, p.row_len / (uint32_t)V, PAIR_CHUNK, grid_cap_of(collate_pair_kernel<T, V>, cache));
    hipLaunchKernelGGL((collate_pair_kernel<T, V>), dim3(blocks), dim3(THREADS), 0, stream, p, g);
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

}  // namespace col

hipError_t launch_collate(const CollateLaunch &p, hipStream_t stream) {
    if (p.n_str == 0) return hipSuccess;
    const bool i64 = (p.flags & DPT_COLLATE_I64) != 0;
    const unsigned width = i64 ? 8 : 4, v = 16 / width;
    // the 16-byte path: a unit of v elements never leaves its row and every store is 16-byte aligned
    const uintptr_t bases = (uintptr_t)p.input_ids | (uintptr_t)p.mask | (uintptr_t)p.labels;
    const bool wide = !col::no_wide() && bases % 16 == 0 && p.row_len % v == 0 && p.row_stride % v == 0;
    if (i64) return wide ? col::launch<int64_t, 2>(p, stream) : col::launch<int64_t, 1>(p, stream);
    return wide ? col::launch<int32_t, 4>(p, stream) : col::launch<int32_t, 1>(p, stream);
}

hipError_t launch_collate_pair(const CollatePairLaunch &p, hipStream_t stream) {
    if (p.n_str == 0) return hipSuccess;
    const bool i64 = (p.flags & DPT_COLLATE_I64) != 0;
    const unsigned width = i64 ? 8 : 4, v = 16 / width;
    const uintptr_t bases = (uintptr_t)p.input_ids | (uintptr_t)p.mask | (uintptr_t)p.labels | (uintptr_t)p.token_type;
    const bool wide = !col::no_wide() && bases % 16 == 0 && p.row_len % v == 0 && p.row_stride % v == 0;
    if (i64) return wide ? col::launch_pair<int64_t, 2>(p, stream) : col::launch_pair<int64_t, 1>(p, stream);
    return wide ? col::launch_pair<int32_t, 4>(p, stream) : col::launch_pair<int32_t, 1>(p, stream);
}

}  // namespace dpt
