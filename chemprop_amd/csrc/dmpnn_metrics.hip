// The metric stage behind the inference head (dmpnn.h "Epoch metric statistics": dmpnn_metric_stats on any preds, dmpnn_validate_head
// behind predict_core): one batch's per-task sums, added into the caller's persistent buffer of doubles.  Every epoch metric of a
// validation run is a function of these sums and sums add across batches, so the epoch ends with one copy of a few hundred bytes.
//
//   k_metric_cols<kind>  regression / binary — k_mcc_cols' layout: workgroup rb n_cb + cb takes the kMetRows molecule rows of row block
//                        rb and the kMetThreads task columns of column block cb; thread i is on column i % C and on the rows i / C,
//                        i / C + kMetThreads / C, ... (C = the smallest power of two >= min(t, kMetThreads)), every p and t converted
//                        to double before the subtraction.  Threads on one column: the lanes C apart of a wave (xor shuffles down to
//                        C), then the waves through LDS in wave order.  Leaves part[rb][j][0 .. per).
//   k_metric_confusion   multiclass: workgroup rb t + j, one thread per molecule row, the row's cell [target class][argmax] counted
//                        into an LDS histogram by INTEGER atomics (exact, so the order does not matter); leaves part[rb][j][nc nc].
//   k_metric_finish      one thread per slot: the row blocks' partials in block order, then the ONE stats[k] += batch_sum of that slot;
//                        thread 0 also the header (loss_out of the same call, read on the same stream).
// No floating-point atomics and a fixed order everywhere: the buffer after a call is a function of its inputs and starting contents
// alone.  fp64 adds run at a fraction of the fp32 rate, which does not matter here — at 512 molecules x 12 tasks the stage adds
// 43 008 doubles in all; it is two launch latencies, not arithmetic.
#include <cmath>

#include "dmpnn_common.hpp"

namespace dmpnn {
namespace {

constexpr int kMetRows = 128;       // molecule rows per row block
constexpr int kMetThreads = 256;    // threads of k_metric_cols / k_metric_finish = task columns per column block
constexpr int kMetRegSums = 7;      // n, sum e^2, sum |e|, sum t, sum t^2, sum e_b^2, sum |e_b|  (slot 7 reserved)
constexpr int kMetBinSums = 5;      // n, TP, FP, TN, FN                                           (slots 5..7 reserved)

struct MetricK {
    const float* P; int64_t ldp; const float* T; int64_t ldt; const unsigned char* lt; const unsigned char* gt;
    const float* loss; double* stats; double* part;
    int64_t B; int t, per, nv, nc, group, lgC, n_blocks, n_cb, kind; float thr;
};

// v[k] of the threads on one column (tid % C) summed into thread `column` (tid < C): k_mcc_cols' reduction, in double
template <int NV>
__device__ __forceinline__ void metric_col_reduce(double (&v)[NV], int C, double* red) {
    const int tid = threadIdx.x;
    for (int off = 32; off >= C; off >>= 1) {   // (uniform; C < 64: the lanes of a wave on the same column)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += __shfl_xor(v[k], off);
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k * kMetThreads + tid] = v[k];
    __syncthreads();
    if (tid < C) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = 0.0;
            for (int wv = 0; wv < kMetThreads / 64; ++wv) {   // (the waves that hold this column, in wave order)
                const int idx = wv * 64 + (tid & 63);
                if ((idx & (C - 1)) == tid) s += red[k * kMetThreads + idx];
            }
            v[k] = s;
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(kMetThreads) void k_metric_cols(MetricK a) {
    constexpr int NV = KIND == DMPNN_METRIC_REGRESSION ? kMetRegSums : kMetBinSums;
    __shared__ double red[NV * kMetThreads];
    const int tid = threadIdx.x, t = a.t, C = 1 << a.lgC, c = tid & (C - 1), rl = tid >> a.lgC, RL = kMetThreads >> a.lgC;
    const int64_t rb = blockIdx.x / a.n_cb;   // (workgroup rb n_cb + cb)
    const int cb = (int)(blockIdx.x - rb * a.n_cb), j = cb * kMetThreads + c;
    const int64_t r0 = rb * kMetRows, r1 = r0 + kMetRows < a.B ? r0 + kMetRows : a.B;
    const bool valid = j < t;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    if (valid)
        for (int64_t r = r0 + rl; r < r1; r += RL) {
            const float yf = a.T[r * a.ldt + j];
            if (!isfinite(yf)) continue;
            const float pf = a.P[r * a.ldp + (int64_t)j * a.group];
            if constexpr (KIND == DMPNN_METRIC_REGRESSION) {
                const double y = (double)yf, e = (double)pf - y;
                const int64_t mi = r * t + j;
                const bool clip = (a.lt && a.lt[mi] && pf < yf) || (a.gt && a.gt[mi] && pf > yf);   // BoundedMixin: p becomes t there
                const double eb = clip ? 0.0 : e;
                v[0] += 1.0; v[1] += e * e; v[2] += fabs(e); v[3] += y; v[4] += y * y; v[5] += eb * eb; v[6] += fabs(eb);
            } else {
                const bool pp = pf > a.thr, tp = yf > 0.5f;
                v[0] += 1.0; v[1] += (pp && tp) ? 1.0 : 0.0; v[2] += (pp && !tp) ? 1.0 : 0.0; v[3] += (!pp && !tp) ? 1.0 : 0.0;
                v[4] += (!pp && tp) ? 1.0 : 0.0;
            }
        }
    metric_col_reduce<NV>(v, C, red);
    if (tid < C && valid) {
        double* o = a.part + ((int64_t)rb * t + j) * a.per;
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k] = v[k];
        for (int k = NV; k < a.per; ++k) o[k] = 0.0;
    }
}

__global__ __launch_bounds__(kMetRows) void k_metric_confusion(MetricK a) {
    __shared__ int hist[DMPNN_METRIC_MAX_CLASSES * DMPNN_METRIC_MAX_CLASSES];
    const int tid = threadIdx.x, nc = a.nc, cells = nc * nc;
    const int64_t rb = blockIdx.x / a.t;   // (workgroup rb t + j)
    const int j = (int)(blockIdx.x - rb * a.t);
    for (int k = tid; k < cells; k += kMetRows) hist[k] = 0;
    __syncthreads();
    const int64_t r = rb * kMetRows + tid;
    if (r < a.B) {
        const float y = a.T[r * a.ldt + j];
        if (y > -1.f && y < (float)nc) {   // finite, and (int)y — truncation towards 0 — lies in [0, nc); a NaN fails both
            const float* p = a.P + r * a.ldp + (int64_t)j * nc;
            int best = 0;
            float bv = p[0];
            for (int k = 1; k < nc; ++k) {   // (strictly greater: the lowest index among equal maxima)
                const float x = p[k];
                if (x > bv) { bv = x; best = k; }
            }
            atomicAdd(&hist[(int)y * nc + best], 1);
        }
    }
    __syncthreads();
    double* o = a.part + ((int64_t)rb * a.t + j) * a.per;
    for (int k = tid; k < cells; k += kMetRows) o[k] = (double)hist[k];
}

__global__ __launch_bounds__(kMetThreads) void k_metric_finish(MetricK a) {
    const int64_t S = (int64_t)a.t * a.per, k = (int64_t)blockIdx.x * kMetThreads + threadIdx.x;
    if (k < S) {
        double s = 0.0;
        for (int blk = 0; blk < a.n_blocks; ++blk) s += a.part[(int64_t)blk * S + k];
        double* o = a.stats + DMPNN_METRIC_HEADER + k;
        if ((int)(k % a.per) >= a.nv) *o = 0.0;   // (a reserved slot)
        else *o += s;
    }
    if (k != 0) return;
    if (a.loss) {   // [loss, n_finite] of the same call: the epoch's val_loss is the count-weighted mean
        const float n = a.loss[1];
        if (n > 0.f) { a.stats[0] += (double)a.loss[0] * (double)n; a.stats[1] += (double)n; }
    }
    a.stats[2] += 1.0;
    a.stats[3] += (double)a.B;
}

inline int64_t metric_row_blocks(int64_t B) { return (B + kMetRows - 1) / kMetRows; }
inline int64_t metric_tasks(const dmpnn_metric_args& a) { return a.kind == DMPNN_METRIC_NONE ? 0 : a.n_tasks; }

}  // namespace

int metric_per_task(int kind, int n_classes) {
    if (kind == DMPNN_METRIC_NONE) return 0;
    if (kind == DMPNN_METRIC_REGRESSION || kind == DMPNN_METRIC_BINARY) return 8;
    if (kind == DMPNN_METRIC_MULTICLASS && n_classes >= 2 && n_classes <= DMPNN_METRIC_MAX_CLASSES) return n_classes * n_classes;
    return -1;
}

size_t metric_ws_bytes(const dmpnn_metric_args& a) {
    const int per = metric_per_task(a.kind, a.n_classes);
    if (per <= 0 || a.n_mols <= 0 || a.n_tasks <= 0) return 0;
    return (((size_t)metric_row_blocks(a.n_mols) * (size_t)a.n_tasks * (size_t)per * sizeof(double)) + 255) & ~size_t(255);
}

int metric_check(const dmpnn_metric_args& a) {
    const int per = metric_per_task(a.kind, a.n_classes);
    DMPNN_CHECK_ARG(a.kind >= DMPNN_METRIC_NONE && a.kind <= DMPNN_METRIC_MULTICLASS, "metric_stats: unknown kind %d", (int)a.kind);
    DMPNN_CHECK_ARG(per >= 0, "metric_stats: n_classes (%d) outside 2..%d", (int)a.n_classes, DMPNN_METRIC_MAX_CLASSES);
    DMPNN_CHECK_ARG(a.n_mols >= 0 && a.n_mols < (int64_t(1) << 31) && a.n_tasks >= 0 && a.n_tasks < (int64_t(1) << 24),
                    "metric_stats: bad sizes (n_mols %lld, n_tasks %lld)", (long long)a.n_mols, (long long)a.n_tasks);
    const int64_t t = metric_tasks(a);
    if (a.kind != DMPNN_METRIC_NONE) {
        const bool grouped = a.kind != DMPNN_METRIC_MULTICLASS;
        DMPNN_CHECK_ARG(!grouped || a.group == 1 || a.group == 2 || a.group == 4, "metric_stats: group (%d) must be 1, 2 or 4", (int)a.group);
        DMPNN_CHECK_ARG(a.kind != DMPNN_METRIC_BINARY || std::isfinite(a.threshold), "metric_stats: the threshold must be finite");
        DMPNN_CHECK_ARG(a.preds && a.targets, "metric_stats: null preds / targets");
        const int64_t width = t * (grouped ? a.group : a.n_classes);
        DMPNN_CHECK_ARG(a.ld_p >= width && a.ld_t >= t, "metric_stats: ld_p (%lld) below the row's %lld values or ld_t (%lld) below n_tasks (%lld)",
                        (long long)a.ld_p, (long long)width, (long long)a.ld_t, (long long)t);
        // (the launches' grids: row blocks x column blocks | tasks)
        DMPNN_CHECK_ARG(metric_row_blocks(a.n_mols) * (t > 0 ? t : 1) < (int64_t(1) << 31), "metric_stats: n_mols x n_tasks too large for one launch");
    }
    DMPNN_CHECK_ARG(a.stats && (reinterpret_cast<uintptr_t>(a.stats) & 7u) == 0, "metric_stats: stats missing or not 8-byte aligned");
    const size_t need_stats = (DMPNN_METRIC_HEADER + (size_t)t * (size_t)per) * sizeof(double);
    DMPNN_CHECK_ARG(a.stats_bytes >= need_stats, "metric_stats: stats_bytes too small (%zu < %zu)", a.stats_bytes, need_stats);
    const size_t need = metric_ws_bytes(a);
    if (need && (!a.ws || a.ws_bytes < need)) {
        set_error("metric_stats: workspace missing or too small (%zu < %zu bytes)", a.ws_bytes, need);
        return DMPNN_ENOSPC;
    }
    DMPNN_CHECK_ARG(!need || (reinterpret_cast<uintptr_t>(a.ws) & 7u) == 0, "metric_stats: workspace must be 8-byte aligned");
    return DMPNN_OK;
}

int launch_metric_stats(const dmpnn_metric_args& a, hipStream_t s) {
    if (a.n_mols <= 0) return DMPNN_OK;
    const int64_t t = metric_tasks(a);
    const int per = metric_per_task(a.kind, a.n_classes);
    MetricK q{};
    q.P = a.preds; q.ldp = a.ld_p; q.T = a.targets; q.ldt = a.ld_t; q.lt = a.lt_mask; q.gt = a.gt_mask;
    q.loss = a.loss; q.stats = a.stats; q.part = static_cast<double*>(a.ws);
    q.B = a.n_mols; q.t = (int)t; q.per = per; q.nc = a.n_classes; q.group = a.group; q.kind = a.kind; q.thr = a.threshold;
    q.nv = a.kind == DMPNN_METRIC_REGRESSION ? kMetRegSums : (a.kind == DMPNN_METRIC_BINARY ? kMetBinSums : per);
    q.n_blocks = (int)metric_row_blocks(a.n_mols);
    q.n_cb = (int)((t + kMetThreads - 1) / kMetThreads);
    while ((1 << q.lgC) < kMetThreads && (1 << q.lgC) < t) ++q.lgC;   // (C: the smallest power of two >= min(t, kMetThreads))
    if (t > 0 && a.kind == DMPNN_METRIC_MULTICLASS) {
        hipLaunchKernelGGL(k_metric_confusion, dim3((unsigned)((int64_t)q.n_blocks * t)), dim3(kMetRows), 0, s, q);
        DMPNN_CHECK_LAUNCH("k_metric_confusion");
    } else if (t > 0) {
        const dim3 grid((unsigned)((int64_t)q.n_blocks * q.n_cb));
        if (a.kind == DMPNN_METRIC_REGRESSION) hipLaunchKernelGGL(k_metric_cols<DMPNN_METRIC_REGRESSION>, grid, dim3(kMetThreads), 0, s, q);
        else hipLaunchKernelGGL(k_metric_cols<DMPNN_METRIC_BINARY>, grid, dim3(kMetThreads), 0, s, q);
        DMPNN_CHECK_LAUNCH("k_metric_cols");
    }
    const int64_t S = t * per;
    hipLaunchKernelGGL(k_metric_finish, dim3((unsigned)(S > 0 ? (S + kMetThreads - 1) / kMetThreads : 1)), dim3(kMetThreads), 0, s, q);
    DMPNN_CHECK_LAUNCH("k_metric_finish");
    return DMPNN_OK;
}

}  // namespace dmpnn
