// dpt_packing.hip -- in-order greedy sequence packing of an encoded batch into rows of L tokens (include/dpt.h
// dpt_pack_sizes, dpt_pack_plan, dpt_pack_write).
//
// sizes_kernel: one thread per string, the string's packed length (dpt_collate's ``lengths``).
//
// The plan.  With P = tok_off (the caller's prefix sum of the lengths), the row that starts at string s ends before
// nxt(s) = the smallest t > s with P[t+1] - P[s] > L (n_str when there is none): one binary search per string.  The
// row starts are the orbit of the first string with tokens under nxt -- a pointer chain, resolved in three launches
// that talk through the workspace only (no block waits for another one inside a launch):
//   P1 plan_jump_kernel   a block per B consecutive strings: nxt for each (clamped to (s, n_str]), then log2(B)
//                         rounds of pointer jumping in LDS give, for an orbit that enters the block at s, the first
//                         element past the block (exit), the rows begun inside it (cnt) and the last in-block start
//                         (last).  nxt, exit and cnt | last << 16 go to the workspace.
//   P2 plan_walk_kernel   one wave: e = exit[e] from block to block, at most ceil(n_str / B) steps of one dependent
//                         load pair.  Per block: its entry (NONE for a block no row starts in), the rows begun before
//                         it and the start of the row that is open where it begins.  Writes n_rows.
//   P3 plan_place_kernel  a block per B strings: the jump tables of all log2(B) levels in LDS mark the orbit from the
//                         block's entry (top level down: after level k every 2^k-th element is marked); a start's row
//                         is base + cnt[entry] - cnt[start]; a max-scan hands every string its row's start.  Starts
//                         write row_first / row_fill; then the rows past n_rows get their empty values.
// Every loop has a trip count fixed before it starts and every index is clamped before use, so a tok_off that is no
// prefix sum gives meaningless rows, never a fault or a hang.
//
// write_kernel: threads over the OUTPUT, [row_cap, row_len] flattened in units of V elements as in dpt_collate.hip
// (V = 1, or 16 bytes' worth under the same alignment conditions), so every store instruction of a wave is a
// contiguous row segment.  A unit finds its string among [row_first[r], row_first[r+1]) by a binary search over
// tok_off (neighbouring lanes walk the same few cache lines) and keeps it while its elements stay inside; an id is
// loaded only when its index is inside the string's own token range and the string's status is 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_internal.h"
#include "dpt_wave.h"

namespace dpt {
namespace pk {

constexpr unsigned B = PACK_BLOCK_STRINGS;   // strings per plan block = its threads
constexpr unsigned LOG_B = 10;
static_assert(B == 1u << LOG_B && B <= 1024, "one thread per string, B a power of two");
constexpr unsigned NONE = 0xFFFFFFFFu;
constexpr unsigned SEARCH_STEPS = 32;        // halvings that empty any range of under 2^32 entries

// the first j in [lo, hi) with P[j] - base > key, hi when there is none (P non-decreasing from base on)
__device__ __forceinline__ uint32_t upper_bound(const uint64_t *__restrict__ P, uint64_t base, uint64_t key, uint32_t lo, uint32_t hi) {
    for (unsigned it = 0; it < SEARCH_STEPS && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P[mid] - base <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) sizes_kernel(CollateSide src, const uint32_t n_str, const uint32_t room, const uint32_t n_special,
                                                    uint32_t *__restrict__ lengths) {
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n_str; s += gridDim.x * 256u) {
        const uint64_t n = src.counts ? src.counts[s] : src.off[s + 1] - src.off[s];
        const bool failed = src.status && src.status[s] != 0;
        lengths[s] = failed ? 0u : (n < room ? (uint32_t)n : room) + n_special;
    }
}

// ---- the plan

// the workspace: three uint32 per string, three per block
struct Ws {
    uint32_t *nxt, *exit, *cl;                     // per string (P1)
    uint32_t *blk_entry, *blk_base, *blk_open;     // per block (P2)
    __host__ __device__ Ws(void *ws, uint32_t n_str, uint32_t n_blk) {
        nxt = static_cast<uint32_t *>(ws);
        exit = nxt + n_str;
        cl = exit + n_str;
        blk_entry = cl + n_str;
        blk_base = blk_entry + n_blk;
        blk_open = blk_base + n_blk;
    }
};

__global__ void __launch_bounds__(B) plan_jump_kernel(const uint64_t *__restrict__ P, const uint32_t n_str, const uint32_t L, const uint32_t n_blk,
                                                      void *ws_) {
    __shared__ uint32_t ptr[B], cnt[B], last[B];
    const Ws ws(ws_, n_str, n_blk);
    const uint32_t t = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const uint32_t b0 = b * B, bend = n_str - b0 < B ? n_str : b0 + B, s = b0 + t;
        const bool live = s < n_str;
        uint32_t nx = n_str;
        if (live) {
            // (the found j is in [s + 1, n_str + 1]: nxt = j - 1, and at least s + 1 whatever P holds)
            const uint32_t j = upper_bound(P, P[s], L, s + 1u, n_str + 1u);
            nx = j - 1u > s ? j - 1u : s + 1u;
        }
        ptr[t] = nx, cnt[t] = 1u, last[t] = t;
        __syncthreads();
        // after round k ptr is the 2^k-th successor, or the first one past the block
#pragma unroll 1
        for (unsigned k = 0; k < LOG_B; ++k) {
            uint32_t p = ptr[t], c = cnt[t], l = last[t];
            if (p < bend) {
                const uint32_t j = p - b0;   // (p > s: j > t)
                c += cnt[j], l = last[j], p = ptr[j];
            }
            __syncthreads();
            ptr[t] = p, cnt[t] = c, last[t] = l;
            __syncthreads();
        }
        if (live) {
            ws.nxt[s] = nx;
            ws.exit[s] = ptr[t];
            ws.cl[s] = cnt[t] | (last[t] << 16);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) plan_walk_kernel(const uint64_t *__restrict__ P, const uint32_t n_str, const uint32_t n_blk, void *ws_,
                                                       uint64_t *__restrict__ n_rows) {
    const Ws ws(ws_, n_str, n_blk);
    const uint32_t lane = threadIdx.x;
    // every lane walks (the values are wave-uniform); the lanes share the stores of the blocks that are skipped
    uint32_t e = upper_bound(P, P[0], 0, 1u, n_str + 1u) - 1u;   // the first string with tokens, n_str: none
    uint32_t rows = 0, open = NONE, fill_from = 0;
    for (uint32_t step = 0; step < n_blk && e < n_str; ++step) {
        const uint32_t b = e / B;
        for (uint32_t k = fill_from + lane; k < b; k += 64u) ws.blk_entry[k] = NONE, ws.blk_base[k] = rows, ws.blk_open[k] = open;
        if (lane == 0) ws.blk_entry[b] = e, ws.blk_base[b] = rows, ws.blk_open[b] = open;
        const uint32_t x = ws.exit[e], cl = ws.cl[e];
        rows += cl & 0xFFFFu;
        open = b * B + (cl >> 16);
        fill_from = b + 1u;
        const uint32_t bend = n_str - b * B < B ? n_str : (b + 1u) * B;
        e = x < bend ? bend : x;   // (exit is past the block by construction)
    }
    for (uint32_t k = fill_from + lane; k < n_blk; k += 64u) ws.blk_entry[k] = NONE, ws.blk_base[k] = rows, ws.blk_open[k] = open;
    if (lane == 0) *n_rows = rows;
}

// inclusive max-scan over the block's B threads (scratch: one entry per wave)
__device__ __forceinline__ uint32_t block_incl_scan_max(uint32_t v, uint32_t *scratch) {
    const uint32_t w = threadIdx.x >> 6;
    v = wave_incl_scan_max(v);
    if ((threadIdx.x & 63u) == 63u) scratch[w] = v;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < w; ++k) before = max(before, scratch[k]);
    __syncthreads();
    return max(v, before);
}

__global__ void __launch_bounds__(B) plan_place_kernel(PackPlanLaunch a, const uint32_t n_blk) {
    __shared__ uint16_t lvl[LOG_B][B + 2];   // jump tables; slot B: past the block (jumps to itself)
    __shared__ uint16_t cnt_of[B];
    __shared__ uint8_t mark[B + 4];
    __shared__ uint32_t scratch[B / 64];
    const uint64_t *__restrict__ P = a.tok_off;
    const uint32_t n_str = a.n_str, t = threadIdx.x;
    const Ws ws(a.ws, n_str, n_blk);
    for (uint32_t b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const uint32_t b0 = b * B, bend = n_str - b0 < B ? n_str : b0 + B, s = b0 + t;
        const bool live = s < n_str;
        uint32_t entry = ws.blk_entry[b];
        const uint32_t base = ws.blk_base[b], open = ws.blk_open[b];
        if (entry < b0 || entry >= bend) entry = NONE;
        uint32_t nx = n_str, c_s = 0;
        bool is_start = false;
        if (entry != NONE) {   // (block-uniform)
            if (live) {
                nx = ws.nxt[s];
                c_s = ws.cl[s] & 0xFFFFu;
            }
            const uint32_t j = live && nx > s && nx < bend ? nx - b0 : B;
            lvl[0][t] = (uint16_t)j;
            cnt_of[t] = (uint16_t)c_s;
            mark[t] = 0;
            if (t < LOG_B) lvl[t][B] = (uint16_t)B;
            if (t == 0) mark[B] = 0;
            __syncthreads();
#pragma unroll 1
            for (unsigned k = 1; k < LOG_B; ++k) {
                lvl[k][t] = lvl[k - 1][lvl[k - 1][t]];
                __syncthreads();
            }
            if (t == 0) mark[entry - b0] = 1;
            __syncthreads();
#pragma unroll 1
            for (int k = (int)LOG_B - 1; k >= 0; --k) {
                if (mark[t]) mark[lvl[k][t]] = 1;
                __syncthreads();
            }
            is_start = live && mark[t] != 0;
        }
        // the start of each string's row: the nearest start at or before it, else the row open at the block's beginning
        const uint32_t sp = block_incl_scan_max(is_start ? t + 1u : 0u, scratch);
        uint32_t start = open, row = base - 1u;
        if (sp) {
            start = b0 + sp - 1u;
            row = base + (uint32_t)cnt_of[entry - b0] - (uint32_t)cnt_of[sp - 1u];
        }
        if (live) {
            const uint64_t p_s = P[s];
            const bool placed = P[s + 1] != p_s && start <= s;
            if (a.str_row) a.str_row[s] = placed ? row : NONE;
            if (a.str_col) {
                uint32_t c = 0;
                if (placed) c = (uint32_t)(p_s - P[start]);   // (start <= s)
                a.str_col[s] = c;
            }
            if (is_start) {
                if (a.row_first && row <= a.row_cap) a.row_first[row] = s;
                if (a.row_fill && row < a.row_cap) a.row_fill[row] = (uint32_t)(P[nx < n_str ? nx : n_str] - p_s);
            }
        }
        __syncthreads();
    }
    // the rows past the need
    const uint64_t n_rows = *a.n_rows;
    for (uint64_t r = n_rows + (uint64_t)blockIdx.x * B + t; r <= a.row_cap; r += (uint64_t)gridDim.x * B) {
        if (a.row_first) a.row_first[r] = n_str;
        if (a.row_fill && r < a.row_cap) a.row_fill[r] = 0u;
    }
}

// ---- the rows

constexpr unsigned THREADS = 256, UNITS = 4, CHUNK = THREADS * UNITS;
constexpr unsigned MAX_BLOCKS_LIMIT = 4096, MAX_DEVICES = 64;

template <typename T, int V>
using Vec = T __attribute__((ext_vector_type(V)));

template <typename T, int V>
__device__ __forceinline__ void store_unit(T *p, Vec<T, V> v) {
    __builtin_nontemporal_store(v, reinterpret_cast<Vec<T, V> *>(p));
}

// the string that holds a row position
struct Seq {
    uint32_t s;          // the string
    uint32_t begin;      // the row column of its sequence position 0
    uint32_t len;        // its sequence's length
    uint32_t n;          // its source token count, 0 when its status is not 0 (no id of it is read)
    uint64_t first;      // ids index of its first token
    uint64_t src;        // ids index of its first kept token
};

template <typename T, int V>
__global__ void __launch_bounds__(THREADS) write_kernel(PackWriteLaunch a, const uint32_t lu, const uint64_t magic, const uint64_t chunks) {
    static_assert(2ull * CHUNK * CHUNK < (1ull << 32), "32-bit unit arithmetic");
    const uint64_t *__restrict__ P = a.tok_off;
    const uint32_t L = a.r.row_len, n_str = (uint32_t)a.r.n_str, flags = a.r.flags;
    const uint32_t n_bos = flags & DPT_COLLATE_BOS ? 1u : 0u, n_eos = flags & DPT_COLLATE_EOS ? 1u : 0u;
    const uint64_t off0 = a.src.off[0];
    const uint64_t n_rows = *a.n_rows;
    T *const out_ids = static_cast<T *>(a.r.input_ids);
    T *const out_pos = static_cast<T *>(a.position_ids);
    T *const out_seg = static_cast<T *>(a.segment_ids);
    T *const out_lab = static_cast<T *>(a.r.labels);

    for (uint64_t k = blockIdx.x; k < chunks; k += gridDim.x) {
        const uint64_t f = k * CHUNK;
        const uint64_t row0 = f / lu;
        const uint32_t r0 = (uint32_t)(f - row0 * lu);
#pragma unroll
        for (unsigned u = 0; u < UNITS; ++u) {
            const uint32_t x = r0 + threadIdx.x + u * THREADS;   // (< lu + CHUNK)
            const uint32_t q = magic ? (uint32_t)(((uint64_t)x * magic) >> 32) : (x >= lu ? 1u : 0u);
            const uint64_t row = row0 + q;
            const uint32_t col = (x - q * lu) * (uint32_t)V;
            if (row >= a.row_cap) continue;
            // the row's strings [f0, f1), clamped: row_first is the caller's
            uint32_t f0 = 0, f1 = 0;
            if (row < n_rows) {
                f0 = a.row_first[row], f1 = a.row_first[row + 1];
                f1 = f1 < n_str ? f1 : n_str;
                f0 = f0 < f1 ? f0 : f1;
            }
            const uint64_t p0 = P[f0];   // (f0 <= n_str)
            Seq q_ = {0, 0, 0, 0, 0, 0};
            uint32_t seq_end = 0;        // the columns below it are behind the current string
            bool done = f0 == f1;        // nothing (more) in the row: pad
            Vec<T, V> vi, vp, vs, vl;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t c = col + (uint32_t)e;
                if (!done && c >= seq_end) {
                    // the string with begin <= c < begin + len: the last j in (f0, f1] with P[j] - p0 <= c is its end
                    const uint32_t j = upper_bound(P, p0, c, f0 + 1u, f1 + 1u);
                    if (j > f1) done = true;   // c is past the row's tokens
                    else {
                        const uint32_t s = j - 1u;
                        const uint64_t b_ = P[s] - p0, e_ = P[j] - p0;
                        q_.s = s;
                        q_.begin = (uint32_t)b_;
                        q_.len = (uint32_t)(e_ - b_);
                        seq_end = (uint32_t)e_;
                        const uint64_t o = a.src.off[s];
                        const uint64_t n = a.src.counts ? a.src.counts[s] : a.src.off[s + 1] - o;
                        const bool failed = a.src.status && a.src.status[s] != 0;
                        const uint32_t kept = q_.len - n_bos - n_eos;   // (wraps on a malformed tok_off: the index check below holds)
                        q_.n = failed ? 0u : (n < (1ull << 32) ? (uint32_t)n : 0xFFFFFFFFu);
                        q_.first = o - off0;
                        q_.src = q_.first + ((flags & DPT_COLLATE_TRUNC_LEFT) && n > kept ? n - kept : 0);
                        if (b_ > c || e_ > L || e_ <= c) done = true;   // (a malformed tok_off)
                    }
                }
                const uint32_t p = c - q_.begin;
                const bool in_seq = !done && p < q_.len;
                int32_t tok = a.r.pad_id;
                if (in_seq) {
                    if (n_bos && p == 0u) tok = a.r.bos_id;
                    else if (n_eos && p == q_.len - 1u) tok = a.r.eos_id;
                    else {
                        // the id's index inside its own string: TRUNC_LEFT's skip + the position less the bos
                        const uint64_t at = q_.src + (p - n_bos);
                        if (at >= q_.first && at - q_.first < q_.n) tok = a.src.ids[at];
                    }
                }
                vi[e] = (T)tok;
                vp[e] = in_seq ? (T)p : (T)0;
                vs[e] = in_seq ? (T)(q_.s - f0 + 1u) : (T)0;
                vl[e] = in_seq && !((flags & DPT_PACK_MASK_FIRST) && p == 0u) ? (T)tok : (T)a.r.ignore_id;
            }
            const uint64_t at = row * a.r.row_stride + col;
            store_unit<T, V>(out_ids + at, vi);
            if (out_pos) store_unit<T, V>(out_pos + at, vp);
            if (out_seg) store_unit<T, V>(out_seg + at, vs);
            if (out_lab) store_unit<T, V>(out_lab + at, vl);
        }
    }
}

template <typename K>
unsigned grid_cap(K kernel, unsigned *cache) {
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
hipError_t launch_write(const PackWriteLaunch &p, hipStream_t stream) {
    static unsigned cache[MAX_DEVICES];   // (0: not asked yet; a race stores the same value twice)
    const uint32_t lu = p.r.row_len / (uint32_t)V;
    const uint64_t units = p.row_cap * lu, chunks = (units + CHUNK - 1) / CHUNK;
    const unsigned cap = grid_cap(write_kernel<T, V>, cache);
    const unsigned blocks = (unsigned)(chunks < cap ? chunks : cap);
    const uint64_t magic = lu < CHUNK ? ((1ull << 32) + lu - 1) / lu : 0;   // (exact: the dividend stays under 2 x CHUNK)
    hipLaunchKernelGGL((write_kernel<T, V>), dim3(blocks), dim3(THREADS), 0, stream, p, lu, magic, chunks);
    return hipGetLastError();
}

}  // namespace pk

uint64_t pack_plan_workspace_bytes(uint64_t n_str) {
    const uint64_t n_blk = (n_str + pk::B - 1) / pk::B;
    return 12 * (n_str + n_blk);
}

hipError_t launch_pack_sizes(const CollateSide &src, uint32_t n_str, uint32_t room, uint32_t n_special, uint32_t *lengths, hipStream_t stream) {
    if (n_str == 0) return hipSuccess;
    const uint64_t want = ((uint64_t)n_str + 255) / 256;
    const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(pk::sizes_kernel, dim3(blocks), dim3(256), 0, stream, src, n_str, room, n_special, lengths);
    return hipGetLastError();
}

hipError_t launch_pack_plan(const PackPlanLaunch &p, hipStream_t stream) {
    if (p.n_str == 0) {
        // no string: no row.  row_first[r] = n_str = 0 and row_fill[r] = 0 are all zero bytes
        hipError_t e = hipMemsetAsync(p.n_rows, 0, sizeof(uint64_t), stream);
        if (e == hipSuccess && p.row_first) e = hipMemsetAsync(p.row_first, 0, ((uint64_t)p.row_cap + 1) * sizeof(uint32_t), stream);
        if (e == hipSuccess && p.row_fill && p.row_cap) e = hipMemsetAsync(p.row_fill, 0, (uint64_t)p.row_cap * sizeof(uint32_t), stream);
        return e;
    }
    const uint32_t n_blk = (p.n_str + pk::B - 1) / pk::B;
    const unsigned blocks = n_blk < PACK_GRID_CAP ? n_blk : PACK_GRID_CAP;
    hipLaunchKernelGGL(pk::plan_jump_kernel, dim3(blocks), dim3(pk::B), 0, stream, p.tok_off, p.n_str, p.row_len, n_blk, p.ws);
    hipLaunchKernelGGL(pk::plan_walk_kernel, dim3(1), dim3(64), 0, stream, p.tok_off, p.n_str, n_blk, p.ws, p.n_rows);
    hipLaunchKernelGGL(pk::plan_place_kernel, dim3(blocks), dim3(pk::B), 0, stream, p, n_blk);
    return hipGetLastError();
}

hipError_t launch_pack_write(const PackWriteLaunch &p, hipStream_t stream) {
    if (p.r.n_str == 0 || p.row_cap == 0) return hipSuccess;
    const bool i64 = (p.r.flags & DPT_COLLATE_I64) != 0;
    const unsigned width = i64 ? 8 : 4, v = 16 / width;
    // the 16-byte path: a unit of v elements never leaves its row and every store is 16-byte aligned
    const uintptr_t bases = (uintptr_t)p.r.input_ids | (uintptr_t)p.position_ids | (uintptr_t)p.segment_ids | (uintptr_t)p.r.labels;
    const bool wide = bases % 16 == 0 && p.r.row_len % v == 0 && p.r.row_stride % v == 0;
    if (i64) return wide ? pk::launch_write<int64_t, 2>(p, stream) : pk::launch_write<int64_t, 1>(p, stream);
    return wide ? pk::launch_write<int32_t, 4>(p, stream) : pk::launch_write<int32_t, 1>(p, stream);
}

}  // namespace dpt
