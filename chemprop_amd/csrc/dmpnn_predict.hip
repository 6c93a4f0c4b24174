// The last launch of the inference head (dmpnn_predict_head: predict_core in the head's host driver dmpnn_head.hip; the kernels in front of
// this one — k_agg_bn_fwd_own_bounds, k_head_rows<., 1>, k_loss behind it — are dmpnn_head_kernels.hpp's): per molecule row the
// predictor's OUTPUT layer, its output transform (nn/predictors.py: the eval-mode forward of the six predictor classes with
// UnscaleTransform / transform_variance) and every store of the call — the raw outputs, the transformed predictions, the row of the
// fingerprint — where the module path runs a contraction, two to six elementwise launches and a copy.
//
// Layout: a workgroup of kTailRows waves, ONE wave per molecule row, lanes over the reduction index K (the output layer of a
// property model is a handful of dot products: a 16 x 16 MFMA tile would be 1/16 full, k_out_fwd's reasoning).  The rows of A and
// of W are read through buffer loads — an index out of range reads 0, so the loop body has no branch — in groups of eight outputs
// per pass over K (eight accumulators: the kernel stays far from the register budget whatever n_out is), reduced by lane
// shuffles.  A row's n_out raw values then go through LDS: the transform's groups — softmax over the nc classes of a task, the
// chunked columns k t + j of the mean-variance / evidential / quantile predictors — gather values that other lanes reduced.
// n_out > DMPNN_PREDICT_MAX_OUT: the contraction kernels ran the layer; the <false> build reads the raw rows from memory instead.
// DMPNN_PT_SPECTRAL couples an element to its whole row (p = a / sum_row a): the row's sum, and its maximum for exp, are wave
// reductions once per row in front of the element loop, in both builds.
// DMPNN_PT_DIRICHLET_BINARY / _MULTICLASS (BinaryDirichletFFN / MulticlassDirichletFFN.forward): alpha = softplus(x) + 1 over a task's
// classes, gathered like the softmax's — (alpha_1 / S, 2 / S) per task with S = alpha_0 + alpha_1, and alpha_k / sum_k alpha_k.
#include "dmpnn_gemm_impl.hpp"   // (gemm::make_rsrc / clamp_bytes / kOOB: the buffer descriptors of every kernel here)

namespace dmpnn {
namespace {

constexpr int kTailRows = 4;     // molecule rows (waves) per workgroup
constexpr int kTailGroup = 8;    // outputs per pass over K

__device__ __forceinline__ float tail_ldf(gemm::rsrc_t r, bool ok, unsigned idx) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, ok ? idx * 4u : gemm::kOOB, 0, 0));
}

// element e of the transformed row (the layouts of dmpnn.h: [t] | [t, nc] | [t, 2 or 4]); x(c): raw column c of this row
template <class X>
__device__ __forceinline__ float tail_transform(const PredictTail& q, int e, X x) {
    auto sc = [&](int j) { return q.scale ? q.scale[j] : 1.f; };
    auto mn = [&](int j) { return q.mean ? q.mean[j] : 0.f; };
    const int t = q.t;
    switch (q.transform) {
        case DMPNN_PT_UNSCALE: return x(e) * sc(e) + mn(e);
        case DMPNN_PT_SIGMOID: return 1.f / (1.f + expf(-x(e)));
        case DMPNN_PT_SOFTMAX: {
            const int c0 = (e / q.nc) * q.nc;
            float mx = x(c0);
            for (int k = 1; k < q.nc; ++k) mx = fmaxf(mx, x(c0 + k));
            float se = 0.f;
            for (int k = 0; k < q.nc; ++k) se += expf(x(c0 + k) - mx);
            return expf(x(e) - mx) / se;
        }
        case DMPNN_PT_MVE: {
            const int j = e >> 1;
            const float s = sc(j);
            return (e & 1) ? softplus_f(x(t + j)) * (s * s) : x(j) * s + mn(j);
        }
        case DMPNN_PT_EVIDENTIAL: {
            const int j = e >> 2, k = e & 3;
            const float s = sc(j);
            if (k == 0) return x(j) * s + mn(j);
            const float v = softplus_f(x(k * t + j));
            return k == 1 ? v : (k == 2 ? v + 1.f : v * (s * s));
        }
        case DMPNN_PT_QUANTILE: {
            const int j = e >> 1;
            const float s = sc(j), m = mn(j), lo = x(j) * s + m, up = x(t + j) * s + m;
            return (e & 1) ? up - lo : (lo + up) / 2.f;
        }
        // the Dirichlet heads, alpha(c) = softplus(x(c)) + 1 — dirichlet_loss's alphas (predict_check keeps 2 j + 1 and c0 + k inside the row)
        case DMPNN_PT_DIRICHLET_BINARY: {   // BinaryDirichletFFN.forward: (p_1, 2 / S) per task, column 2 j + k the evidence of class k
            const int j = e >> 1;
            const float a1 = softplus_f(x(2 * j + 1)) + 1.f, S = (softplus_f(x(2 * j)) + 1.f) + a1;
            return (e & 1) ? 2.f / S : a1 / S;
        }
        case DMPNN_PT_DIRICHLET_MULTICLASS: {   // MulticlassDirichletFFN.forward: alpha / sum over the task's classes
            const int c0 = (e / q.nc) * q.nc;
            float S = 0.f;
            for (int k = 0; k < q.nc; ++k) S += softplus_f(x(c0 + k)) + 1.f;
            return (softplus_f(x(e)) + 1.f) / S;
        }
        default: return x(e);
    }
}

template <bool MATVEC>
__global__ __launch_bounds__(64 * kTailRows) void k_predict_tail(PredictTail q) {
    __shared__ float xs[kTailRows][MATVEC ? DMPNN_PREDICT_MAX_OUT : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * kTailRows, r = row0 + wave;
    const int nrows = (int)(q.B - row0 < kTailRows ? q.B - row0 : kTailRows);
    const bool live = wave < nrows;
    if constexpr (MATVEC) {
        // (descriptors from the workgroup's values only: one built from the wave's row would be divergent to the compiler, and every
        //  load would sit in a loop over the lanes' descriptors)
        const gemm::rsrc_t rA = gemm::make_rsrc(q.A + row0 * q.lda, gemm::clamp_bytes(((int64_t)(nrows - 1) * q.lda + q.K) * 4));
        const gemm::rsrc_t rW = gemm::make_rsrc(q.W, gemm::clamp_bytes((int64_t)q.n_out * q.K * 4));
        const gemm::rsrc_t rb = gemm::make_rsrc(q.b ? q.b : q.W, q.b ? (unsigned)q.n_out * 4u : 0u);   // (no bias: a zero-length buffer reads 0)
        const unsigned a0 = (unsigned)wave * (unsigned)q.lda;
        for (int j0 = 0; j0 < q.n_out; j0 += kTailGroup) {
            float acc[kTailGroup], bv[kTailGroup];
#pragma unroll
            for (int u = 0; u < kTailGroup; ++u) { acc[u] = 0.f; bv[u] = tail_ldf(rb, j0 + u < q.n_out, (unsigned)(j0 + u)); }
            for (int k = lane; k < q.K; k += 64) {
                const float x = tail_ldf(rA, live, a0 + (unsigned)k);
#pragma unroll
                for (int u = 0; u < kTailGroup; ++u) acc[u] += x * tail_ldf(rW, j0 + u < q.n_out, (unsigned)(j0 + u) * (unsigned)q.K + (unsigned)k);
            }
#pragma unroll
            for (int u = 0; u < kTailGroup; ++u) {
                float v = acc[u];
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                if (lane == u && j0 + u < q.n_out) xs[wave][j0 + u] = v + bv[u];
            }
        }
        __syncthreads();   // (the row's raw values: written by eight lanes per group, read by every lane below)
    }
    if (!live) return;
    auto x = [&](int c) -> float {
        if constexpr (MATVEC) return xs[wave][c];
        else return q.raw[r * q.n_out + c];
    };
    // (uniform) DMPNN_PT_SPECTRAL, p = a / sum_row a with a = softplus(x) | exp(x - max_row x): the row's maximum and sum once per row, as
    // wave reductions in front of the element loop — a spectrum is hundreds of columns wide, not a softmax's handful of classes
    const bool spectral = q.transform == DMPNN_PT_SPECTRAL && q.preds;
    float sp_mx = 0.f, sp_sum = 1.f;
    auto sp_act = [&](float v) { return q.spectral_act == 1 ? expf(v - sp_mx) : softplus_f(v); };
    if (spectral) {
        if (q.spectral_act == 1) {
            float m = -INFINITY;
            for (int e = lane; e < q.n_out; e += 64) m = fmaxf(m, x(e));
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            sp_mx = m;
        }
        float s = 0.f;
        for (int e = lane; e < q.n_out; e += 64) s += sp_act(x(e));
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        sp_sum = s;
    }
    for (int e = lane; e < q.n_out; e += 64) {
        if constexpr (MATVEC) q.raw[r * q.n_out + e] = x(e);
        if (q.preds) q.preds[r * q.n_out + e] = spectral ? sp_act(x(e)) / sp_sum : tail_transform(q, e, x);
    }
    if (q.fp)
        for (int c = lane; c < q.fp_w; c += 64) q.fp[r * q.ld_fp + c] = q.Z[r * q.ldz + c];
}

}  // namespace

int launch_predict_tail(const PredictTail& q, hipStream_t s) {
    if (q.B <= 0) return DMPNN_OK;
    const dim3 grid((unsigned)((q.B + kTailRows - 1) / kTailRows)), block(64 * kTailRows);
    if (q.W) {
        DMPNN_CHECK_ARG(q.n_out >= 1 && q.n_out <= DMPNN_PREDICT_MAX_OUT, "predict tail: the output layer rides for 1..%d outputs (got %d)", DMPNN_PREDICT_MAX_OUT, q.n_out);
        hipLaunchKernelGGL(k_predict_tail<true>, grid, block, 0, s, q);
    } else {
        hipLaunchKernelGGL(k_predict_tail<false>, grid, block, 0, s, q);
    }
    DMPNN_CHECK_LAUNCH("k_predict_tail");
    return DMPNN_OK;
}

}  // namespace dmpnn
