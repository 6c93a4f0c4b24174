// Epoch rank metrics (dmpnn.h "Epoch rank metrics"): ROC-AUC and PRC-AUC of a binary head from the epoch's (key, label) buffer, by an
// all-pairs count — n-body style, no sort, no atomics, every floating-point addition in a fixed order.
//
//   k_rank_append   one thread per (molecule, task): the order-preserving uint32 key of the score and the label, into rows
//                   [row0, row0 + n_mols) of the buffer.  Integer tests on the score's bits: no denormal mode can change a key.
//   k_rank_pairs    workgroup (ib, c): the kRankThreads rows i of block ib of column c, one per thread, its key in a register.  The
//                   column's j elements pass through LDS in tiles of kRankTile {key, key if positive else 0} pairs; every lane reads
//                   the SAME j (a broadcast read, ds_read_b128 = two pairs), and a pair costs four compares and four conditional adds
//                   into uint32 counters: all greater, positive greater, all equal, positive equal.  An unranked j has key 0 and meets
//                   no counter of a ranked i (whose key is never 0).  "Equal in a row before i" (first_i) is counted only while the
//                   loop is inside the workgroup's own kRankThreads rows: the equal count on entering them is the count of the rows
//                   before the block.  Then each thread's 2 gp + ep (uint64) and PRC term (double), xor shuffles, the waves through LDS
//                   in wave order, one partial {n_pos, n_neg, n_skipped, n_thresholds, U2, A} per workgroup.
//   k_rank_finish   one thread per column: the partials in block order, roc = U2 / (2 P N), prc = A / P, the 8 doubles of `out`.
// The loop is VALU-bound (as compiled, 8 VALU operations — four compares, two selects, two add-with-carry — and half an LDS
// instruction per pair); the cost is quadratic in the column, bounded by DMPNN_RANK_MAX_ROWS.
#include "dmpnn_common.hpp"

namespace dmpnn {
namespace {

constexpr int kRankThreads = 256;            // rows i per workgroup
constexpr int kRankTile = DMPNN_RANK_TILE;   // pairs j per LDS tile (16 KB)
constexpr int kRankPart = 6;                 // 8-byte words per partial
constexpr int kRankMaxTasks = 65535;         // columns of one launch (the grid's second dimension)
constexpr int kRankUnroll = 8;               // pairs per trip of the inner loop (four ds_read_b128)
static_assert(kRankTile % kRankThreads == 0 && kRankThreads % kRankUnroll == 0, "a workgroup's own rows lie inside one tile, on a trip boundary");

struct RankAppendK {
    const float* P; int64_t ldp; const float* T; int64_t ldt;
    uint32_t* keys; unsigned char* labels;
    int64_t total, row0; int t, group;
};

__global__ __launch_bounds__(kRankThreads) void k_rank_append(RankAppendK a) {
    const int64_t idx = (int64_t)blockIdx.x * kRankThreads + threadIdx.x;
    if (idx >= a.total) return;
    const int64_t r = idx / a.t;
    const int j = (int)(idx - r * a.t);
    const uint32_t yb = __float_as_uint(a.T[r * a.ldt + j]);
    uint32_t pb = __float_as_uint(a.P[r * a.ldp + (int64_t)j * a.group]);
    uint32_t key = 0;
    unsigned char lab;
    if ((yb & 0x7F800000u) == 0x7F800000u) lab = 2;        // the target is NaN / infinite: missing
    else if ((pb & 0x7F800000u) == 0x7F800000u) lab = 3;   // a prediction that is not finite: skipped, and counted
    else {
        if ((pb << 1) == 0) pb = 0;                         // -0.0 ties with +0.0
        key = (pb & 0x80000000u) ? ~pb : (pb | 0x80000000u);
        lab = __uint_as_float(yb) > 0.5f ? 1 : 0;
    }
    const int64_t o = (a.row0 + r) * a.t + j;
    a.keys[o] = key;
    a.labels[o] = lab;
}

struct RankK {
    const uint32_t* keys; const unsigned char* labels;
    int64_t ld;          // elements between two rows of a column (n_tasks; the pooled column: 1)
    int n, n_blocks;     // rows of a column, workgroups per column
    unsigned long long* part;   // [columns][n_blocks][kRankPart]
    double* out; int n_cols;    // (k_rank_finish) row c of out: column c
};

struct RankCounts { uint32_t g_all, g_pos, e_all, e_pos, e_before; };

// pairs [lo, hi) of the tile (both multiples of kRankUnroll) against this thread's key; OWN: the pairs are the workgroup's own rows,
// pair lo is row 0 of the block, and an equal key in a row before this thread's counts into e_before
template <bool OWN>
__device__ __forceinline__ void rank_count(const uint4* tile2, int lo, int hi, uint32_t ki, RankCounts& c) {
    for (int q = lo; q < hi; q += kRankUnroll) {
#pragma unroll
        for (int u = 0; u < kRankUnroll / 2; ++u) {
            const uint4 w = tile2[(q >> 1) + u];   // {key, poskey} of pairs q + 2u and q + 2u + 1: the same address in every lane
            c.g_all += w.x > ki ? 1u : 0u; c.g_pos += w.y > ki ? 1u : 0u; c.e_all += w.x == ki ? 1u : 0u; c.e_pos += w.y == ki ? 1u : 0u;
            c.g_all += w.z > ki ? 1u : 0u; c.g_pos += w.w > ki ? 1u : 0u; c.e_all += w.z == ki ? 1u : 0u; c.e_pos += w.w == ki ? 1u : 0u;
            if constexpr (OWN) {
                const int jl = q - lo + 2 * u;
                c.e_before += (w.x == ki && jl < (int)threadIdx.x) ? 1u : 0u;
                c.e_before += (w.z == ki && jl + 1 < (int)threadIdx.x) ? 1u : 0u;
            }
        }
    }
}

__global__ __launch_bounds__(kRankThreads) void k_rank_pairs(RankK a) {
    __shared__ uint4 tile2[kRankTile / 2];
    __shared__ unsigned long long red_c[kRankThreads / 64], red_u[kRankThreads / 64];
    __shared__ double red_a[kRankThreads / 64];
    const int tid = threadIdx.x, n = a.n, col = blockIdx.y;
    const int i0 = blockIdx.x * kRankThreads, i = i0 + tid;
    const uint32_t* K = a.keys + col;
    const unsigned char* L = a.labels + col;
    unsigned lab = 2;
    uint32_t ki = 0;
    if (i < n) {
        lab = L[(int64_t)i * a.ld];
        ki = lab < 2 ? K[(int64_t)i * a.ld] : 0u;
    }
    RankCounts c{0, 0, 0, 0, 0};
    uint2* tile = reinterpret_cast<uint2*>(tile2);
    for (int t0 = 0; t0 < n; t0 += kRankTile) {
        __syncthreads();   // (the previous tile has been read)
        for (int q = tid; q < kRankTile; q += kRankThreads) {
            const int j = t0 + q;
            uint2 e = make_uint2(0u, 0u);   // (beyond the column, or not ranked: key 0)
            if (j < n) {
                const unsigned lj = L[(int64_t)j * a.ld];
                if (lj < 2) {
                    e.x = K[(int64_t)j * a.ld];
                    e.y = lj == 1 ? e.x : 0u;
                }
            }
            tile[q] = e;
        }
        __syncthreads();
        const int left = n - t0;
        const int cnt = left >= kRankTile ? kRankTile : (left + kRankUnroll - 1) / kRankUnroll * kRankUnroll;   // (the pad pairs hold key 0)
        const int own = i0 - t0;   // the block's own rows start at this pair of the tile, when it lies in [0, kRankTile)
        if (own >= 0 && own < kRankTile) {
            const int own_hi = own + kRankThreads < cnt ? own + kRankThreads : cnt;
            rank_count<false>(tile2, 0, own, ki, c);
            c.e_before = c.e_all;   // the equal keys in the rows before the block
            rank_count<true>(tile2, own, own_hi, ki, c);
            rank_count<false>(tile2, own_hi, cnt, ki, c);
        } else {
            rank_count<false>(tile2, 0, cnt, ki, c);
        }
    }
    // this row's share: the class counts, 2 gp + ep of a negative, the PRC term of the first row of its threshold
    const bool ranked = lab < 2, first = ranked && c.e_before == 0;
    const uint32_t gp = c.g_pos, gn = c.g_all - c.g_pos, ep = c.e_pos, en = c.e_all - c.e_pos;
    unsigned long long cnts = (lab == 1 ? 1ull : 0ull) | (lab == 0 ? 1ull << 16 : 0ull) | (lab == 3 ? 1ull << 32 : 0ull) | (first ? 1ull << 48 : 0ull);
    unsigned long long u2 = lab == 0 ? 2ull * gp + ep : 0ull;
    double term = 0.0;
    if (first) {
        const double above = (double)gp + (double)gn;
        const double p_i = ((double)gp + (double)ep) / (above + (double)ep + (double)en);
        const double p_prev = above > 0.0 ? (double)gp / above : 1.0;
        term = (double)ep * (p_i + p_prev) * 0.5;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        cnts += __shfl_xor(cnts, off);
        u2 += __shfl_xor(u2, off);
        term += __shfl_xor(term, off);
    }
    if ((tid & 63) == 0) { red_c[tid >> 6] = cnts; red_u[tid >> 6] = u2; red_a[tid >> 6] = term; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long sc = 0, su = 0;
        double sa = 0.0;
        for (int w = 0; w < kRankThreads / 64; ++w) { sc += red_c[w]; su += red_u[w]; sa += red_a[w]; }   // (wave order)
        unsigned long long* o = a.part + ((int64_t)col * a.n_blocks + blockIdx.x) * kRankPart;
        o[0] = sc & 0xFFFFull; o[1] = (sc >> 16) & 0xFFFFull; o[2] = (sc >> 32) & 0xFFFFull; o[3] = sc >> 48;
        o[4] = su;
        o[5] = (unsigned long long)__double_as_longlong(sa);
    }
}

__global__ __launch_bounds__(kRankThreads) void k_rank_finish(RankK a) {
    const int c = blockIdx.x * kRankThreads + threadIdx.x;
    if (c >= a.n_cols) return;
    unsigned long long s[5] = {0, 0, 0, 0, 0};
    double A = 0.0;
    const unsigned long long* p = a.part + (int64_t)c * a.n_blocks * kRankPart;
    for (int b = 0; b < a.n_blocks; ++b, p += kRankPart) {   // (block order)
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += p[k];
        A += __longlong_as_double((long long)p[5]);
    }
    double* o = a.out + (int64_t)c * DMPNN_RANK_OUT;
    const double P = (double)s[0], N = (double)s[1];
    const bool both = s[0] > 0 && s[1] > 0;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
    for (int k = 0; k < 5; ++k) o[k] = (double)s[k];
    o[5] = both ? (double)s[4] / (2.0 * P * N) : nan;
    o[6] = both ? A / P : nan;
    o[7] = 0.0;
}

inline int64_t rank_blocks(int64_t n) { return (n + kRankThreads - 1) / kRankThreads; }
inline size_t rank_part_bytes(int64_t n, int64_t cols) { return (size_t)rank_blocks(n) * (size_t)cols * kRankPart * sizeof(unsigned long long); }

int launch_rank_column_set(const dmpnn_rank_args& a, int64_t n, int64_t cols, unsigned long long* part, double* out, hipStream_t s) {
    RankK q{};
    q.keys = a.keys; q.labels = a.labels; q.ld = cols; q.n = (int)n; q.n_blocks = (int)rank_blocks(n);
    q.part = part; q.out = out; q.n_cols = (int)cols;
    hipLaunchKernelGGL(k_rank_pairs, dim3((unsigned)q.n_blocks, (unsigned)cols), dim3(kRankThreads), 0, s, q);
    DMPNN_CHECK_LAUNCH("k_rank_pairs");
    hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)((cols + kRankThreads - 1) / kRankThreads)), dim3(kRankThreads), 0, s, q);
    DMPNN_CHECK_LAUNCH("k_rank_finish");
    return DMPNN_OK;
}

}  // namespace

int rank_append_check(const dmpnn_rank_append_args& a) {
    DMPNN_CHECK_ARG(a.n_mols >= 0 && a.n_tasks >= 0 && a.capacity >= 0 && a.row0 >= 0,
                    "rank_append: negative size (n_mols %lld, n_tasks %lld, capacity %lld, row0 %lld)", (long long)a.n_mols, (long long)a.n_tasks,
                    (long long)a.capacity, (long long)a.row0);
    DMPNN_CHECK_ARG(a.n_mols < (int64_t(1) << 31) && a.n_tasks < (int64_t(1) << 24) && a.n_mols * a.n_tasks < (int64_t(1) << 31),
                    "rank_append: n_mols x n_tasks too large for one launch (%lld x %lld)", (long long)a.n_mols, (long long)a.n_tasks);
    DMPNN_CHECK_ARG(a.group == 1 || a.group == 2, "rank_append: group (%d) must be 1 or 2", (int)a.group);
    DMPNN_CHECK_ARG(a.preds && a.targets && a.keys && a.labels, "rank_append: null preds / targets / keys / labels");
    DMPNN_CHECK_ARG(a.ld_p >= a.n_tasks * a.group && a.ld_t >= a.n_tasks, "rank_append: ld_p (%lld) below the row's %lld values or ld_t (%lld) below n_tasks (%lld)",
                    (long long)a.ld_p, (long long)(a.n_tasks * a.group), (long long)a.ld_t, (long long)a.n_tasks);
    DMPNN_CHECK_ARG((reinterpret_cast<uintptr_t>(a.keys) & 3u) == 0, "rank_append: keys must be 4-byte aligned");
    if (a.row0 > a.capacity || a.n_mols > a.capacity - a.row0) {
        set_error("rank_append: rows [%lld, %lld) do not fit a buffer of %lld rows", (long long)a.row0, (long long)(a.row0 + a.n_mols), (long long)a.capacity);
        return DMPNN_ENOSPC;
    }
    return DMPNN_OK;
}

int launch_rank_append(const dmpnn_rank_append_args& a, hipStream_t s) {
    const int64_t total = a.n_mols * a.n_tasks;
    if (total <= 0) return DMPNN_OK;
    RankAppendK q{a.preds, a.ld_p, a.targets, a.ld_t, a.keys, a.labels, total, a.row0, (int)a.n_tasks, (int)a.group};
    hipLaunchKernelGGL(k_rank_append, dim3((unsigned)((total + kRankThreads - 1) / kRankThreads)), dim3(kRankThreads), 0, s, q);
    DMPNN_CHECK_LAUNCH("k_rank_append");
    return DMPNN_OK;
}

// the per-task partials [n_tasks][blocks(rows)], then the pooled column's [blocks(rows n_tasks)]
size_t rank_ws_bytes(const dmpnn_rank_args& a) {
    if (a.rows <= 0 || a.n_tasks <= 0 || a.rows > DMPNN_RANK_MAX_ROWS || a.n_tasks > kRankMaxTasks) return 0;
    size_t b = rank_part_bytes(a.rows, a.n_tasks);
    if (a.pooled == 1 && a.rows * a.n_tasks <= DMPNN_RANK_MAX_ROWS) b += rank_part_bytes(a.rows * a.n_tasks, 1);
    return (b + 255) & ~size_t(255);
}

int rank_check(const dmpnn_rank_args& a) {
    DMPNN_CHECK_ARG(a.rows >= 0 && a.n_tasks >= 1 && a.n_tasks <= kRankMaxTasks, "rank_metrics: bad sizes (rows %lld, n_tasks %lld)", (long long)a.rows,
                    (long long)a.n_tasks);
    DMPNN_CHECK_ARG(a.pooled == 0 || a.pooled == 1, "rank_metrics: pooled (%d) must be 0 or 1", (int)a.pooled);
    DMPNN_CHECK_ARG(a.rows <= DMPNN_RANK_MAX_ROWS && (!a.pooled || a.rows * a.n_tasks <= DMPNN_RANK_MAX_ROWS),
                    "rank_metrics: %lld keys ranked together, the cap is DMPNN_RANK_MAX_ROWS = %d (beyond it for the pooled column alone: pooled = 0)",
                    (long long)(a.pooled ? a.rows * a.n_tasks : a.rows), DMPNN_RANK_MAX_ROWS);
    DMPNN_CHECK_ARG(a.keys && a.labels && a.out, "rank_metrics: null keys / labels / out");
    DMPNN_CHECK_ARG((reinterpret_cast<uintptr_t>(a.out) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a.keys) & 3u) == 0, "rank_metrics: out must be 8-byte, keys 4-byte aligned");
    const size_t need = rank_ws_bytes(a);
    if (need && (!a.ws || a.ws_bytes < need)) {
        set_error("rank_metrics: workspace missing or too small (%zu < %zu bytes)", a.ws_bytes, need);
        return DMPNN_ENOSPC;
    }
    DMPNN_CHECK_ARG(!need || (reinterpret_cast<uintptr_t>(a.ws) & 7u) == 0, "rank_metrics: workspace must be 8-byte aligned");
    return DMPNN_OK;
}

int launch_rank_metrics(const dmpnn_rank_args& a, hipStream_t s) {
    const int64_t cols = a.n_tasks + a.pooled;
    if (a.rows == 0) {   // no launch: zeros for the counts, and all-ones bytes — a NaN — over roc and prc
        if (hipMemsetAsync(a.out, 0, (size_t)cols * DMPNN_RANK_OUT * sizeof(double), s) != hipSuccess ||
            hipMemset2DAsync(a.out + 5, DMPNN_RANK_OUT * sizeof(double), 0xFF, 2 * sizeof(double), (size_t)cols, s) != hipSuccess) {
            set_error("rank_metrics: clearing out failed: %s", hipGetErrorString(hipGetLastError()));
            return DMPNN_EHIP;
        }
        return DMPNN_OK;
    }
    unsigned long long* part = static_cast<unsigned long long*>(a.ws);
    DMPNN_TRY(launch_rank_column_set(a, a.rows, a.n_tasks, part, a.out, s));
    if (a.pooled)
        DMPNN_TRY(launch_rank_column_set(a, a.rows * a.n_tasks, 1, part + rank_part_bytes(a.rows, a.n_tasks) / sizeof(unsigned long long),
                                         a.out + a.n_tasks * DMPNN_RANK_OUT, s));
    return DMPNN_OK;
}

}  // namespace dmpnn
