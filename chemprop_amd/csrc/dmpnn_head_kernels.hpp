// The kernels of the head (dmpnn_head.hip, its only includer: one translation unit): the predictor's dropout mask, batch norm, the
// criteria, the output layer as dot products, the column kernels (aggregation + batch norm, forward and backward) and the row kernels
// (predictor + criterion + their backward), with their argument structs and size constants.  The host driver is dmpnn_head.hip.
#pragma once
#include "dmpnn_common.hpp"
#include "dmpnn_mega16_impl.hpp"   // (mega16::SplitArgs / split_weights_wave / SplitW / scale_for / split4: the predictor's first layer on the f16 pipe)

namespace dmpnn {
extern thread_local long long* g_debug_stamps;   // (dmpnn_debug_timestamps: cycle stamps of one workgroup, scripts/probe_head_rows.py)
namespace {

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// ---- the predictor's dropout (dmpnn_head_args.ffn_dropout_p): the mask of layer l's input, regenerated wherever it is needed ----------
// Element (r, c) of an input N columns wide is kept when drop_hash(seed, DMPNN_DROP_SITE_FFN + l, r nblk + c / 1024, c % 1024) >= thr,
// nblk = ceil(N / 1024): the hash keys on row * 1024 + col, so a row wider than 1024 takes nblk consecutive hash rows.  on == 0: no mask.
struct FfnDrop {
    unsigned lo, hi, site, thr, nblk;
    float scale, unscale;                  // 1 / (1 - p), 1 - p
    int on;
    __device__ __forceinline__ bool keep(int64_t r, int c) const {
        return drop_hash(lo, hi, site, (unsigned)r * nblk + ((unsigned)c >> 10), (unsigned)c & 1023u) >= thr;
    }
    // d(layer input) / d(pre-activation) at an element whose masked value is x = mask tau(pre) scale: scale tau'(pre) where kept, 0 where
    // dropped.  ReLU class: tau' from the sign of x; tanh / ELU: from tau(pre) = x (1 - p)
    __device__ __forceinline__ float act_grad(int64_t r, int c, float x, int act, float slope) const {
        const bool smooth = act_is_smooth(act);
        return keep(r, c) ? scale * act_grad_from_out(smooth ? x * unscale : x, act, slope) : 0.f;
    }
};
FfnDrop ffn_drop(const dmpnn_head_args& h, int l) {
    FfnDrop d;
    memset(&d, 0, sizeof(d));
    if (!(h.ffn_dropout_p > 0.f) || l < 1 || l >= h.n_layers) return d;
    d.lo = (unsigned)(h.ffn_dropout_seed & 0xFFFFFFFFull); d.hi = (unsigned)(h.ffn_dropout_seed >> 32);
    d.site = (unsigned)(DMPNN_DROP_SITE_FFN + l); d.thr = drop_threshold(h.ffn_dropout_p);
    d.nblk = (unsigned)((h.dims[l] + 1023) / 1024);
    d.scale = 1.f / (1.f - h.ffn_dropout_p); d.unscale = 1.f - h.ffn_dropout_p;
    d.on = 1;
    return d;
}
// the chain form's mask: X [rows, cols] (row stride ldx) *= mask scale in place, behind the contraction whose epilogue applied tau
// (a product, not a select: a NaN stays NaN where dropped, as under nn.Dropout)
__global__ void k_ffn_drop(float* __restrict__ X, int64_t ldx, int64_t rows, int cols, FfnDrop d) {
    const int64_t n = rows * cols;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols; const int c = (int)(i - r * cols);
        X[r * ldx + c] *= d.keep(r, c) ? d.scale : 0.f;
    }
}

// ---- BatchNorm1d over the rows of X [B, d] -------------------------------------------------------------------------
// One workgroup of 1024 threads per 16 columns: 64 row lanes per column, so a thread walks B / 64 rows (8 at 512 molecules;
// the first version — 4 row lanes, 128 dependent iterations per pass — took 65 us for 0.6 MB).  Two passes over the rows for
// the statistics (mean, then the mean squared deviation: the arithmetic of torch's batch_norm on a [B, d] input to fp32
// rounding), a third for y.  B x d is ~0.6 MB: it lives in L2.
constexpr int kBnCols = 16, kBnLanes = 64;
struct BnArgs {
    const float* X; int64_t ldx; float* Y; int64_t ldy;
    __device__ float* X_out() const { return const_cast<float*>(X); }   // (k_agg_bn_fwd writes the aggregate it then normalises)
    const float* gamma; const float* beta; float* run_mean; float* run_var;
    float* save_mean; float* save_invstd;      // [d] each (training: for the backward pass)
    int64_t B; int d; float eps, momentum; int training;
    int64_t* n_tracked;                        // nn.BatchNorm1d.num_batches_tracked (training: += 1) or NULL
};
// column sums over the 64 row lanes: the four row lanes of a wave by lane shuffles, the sixteen waves through LDS
__device__ __forceinline__ float bn_col_sum(float (*red)[kBnCols], int tx, int ty, float v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    __syncthreads();            // (the previous use of `red` is over)
    if ((ty & 3) == 0) red[ty >> 2][tx] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kBnLanes / 4; ++i) s += red[i][tx];
    return s;
}
// REG: B <= 8 x 64 rows — a thread's rows stay in registers (X is read once instead of three times)
constexpr int kBnRegRows = 8;
template <bool REG>
__global__ __launch_bounds__(1024) void k_bn_fwd(BnArgs a) {
    __shared__ float red[kBnLanes / 4][kBnCols];
    const int tx = threadIdx.x & (kBnCols - 1), ty = threadIdx.x / kBnCols;
    const int c = blockIdx.x * kBnCols + tx;
    const bool ok = c < a.d;
    float mean, invstd;
    float xs[kBnRegRows];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < kBnRegRows; ++i) {
            const int64_t r = ty + (int64_t)kBnLanes * i;
            xs[i] = (ok && r < a.B) ? a.X[r * a.ldx + c] : 0.f;
        }
    }
    if (a.training) {
        if (a.n_tracked && blockIdx.x == 0 && threadIdx.x == 0) *a.n_tracked += 1;
        float s = 0.f;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < kBnRegRows; ++i) s += xs[i];
        } else if (ok) {
            for (int64_t r = ty; r < a.B; r += kBnLanes) s += a.X[r * a.ldx + c];
        }
        mean = bn_col_sum(red, tx, ty, s) / (float)a.B;
        float q = 0.f;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < kBnRegRows; ++i) { const float dlt = xs[i] - mean; q += (ty + (int64_t)kBnLanes * i < a.B) ? dlt * dlt : 0.f; }
        } else if (ok) {
            for (int64_t r = ty; r < a.B; r += kBnLanes) { const float dlt = a.X[r * a.ldx + c] - mean; q += dlt * dlt; }
        }
        const float ss = bn_col_sum(red, tx, ty, q);
        const float var = ss / (float)a.B;                       // biased: what normalises (nn.BatchNorm1d)
        invstd = 1.f / sqrtf(var + a.eps);
        if (ok && ty == 0) {
            a.save_mean[c] = mean; a.save_invstd[c] = invstd;
            if (a.run_mean) a.run_mean[c] = (1.f - a.momentum) * a.run_mean[c] + a.momentum * mean;
            // running_var takes the UNBIASED estimate (torch: var * B / (B - 1))
            if (a.run_var) a.run_var[c] = (1.f - a.momentum) * a.run_var[c] + a.momentum * (a.B > 1 ? ss / (float)(a.B - 1) : var);
        }
    } else {
        mean = ok ? a.run_mean[c] : 0.f;
        invstd = ok ? 1.f / sqrtf(a.run_var[c] + a.eps) : 0.f;
    }
    if (ok) {
        const float g = a.gamma ? a.gamma[c] : 1.f, b = a.beta ? a.beta[c] : 0.f;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < kBnRegRows; ++i) {
                const int64_t r = ty + (int64_t)kBnLanes * i;
                if (r < a.B) a.Y[r * a.ldy + c] = (xs[i] - mean) * invstd * g + b;
            }
        } else {
            for (int64_t r = ty; r < a.B; r += kBnLanes) a.Y[r * a.ldy + c] = (a.X[r * a.ldx + c] - mean) * invstd * g + b;
        }
    }
}

// gX = gamma invstd / B (B gY - sum gY - xhat sum(gY xhat));  g_gamma = sum gY xhat;  g_beta = sum gY      (training)
// gX = gY gamma invstd                                                                                     (eval statistics)
struct BnBwdArgs {
    const float* gY; int64_t ldgy; const float* X; int64_t ldx; float* gX; int64_t ldgx;
    const float* gamma; const float* save_mean; const float* save_invstd; const float* run_mean; const float* run_var;
    float* g_gamma; float* g_beta;
    int64_t B; int d; float eps; int training;
};
template <bool REG>
__global__ __launch_bounds__(1024) void k_bn_bwd(BnBwdArgs a) {
    __shared__ float red[kBnLanes / 4][kBnCols];
    const int tx = threadIdx.x & (kBnCols - 1), ty = threadIdx.x / kBnCols;
    const int c = blockIdx.x * kBnCols + tx;
    const bool ok = c < a.d;
    const float mean = ok ? (a.training ? a.save_mean[c] : a.run_mean[c]) : 0.f;
    const float invstd = ok ? (a.training ? a.save_invstd[c] : 1.f / sqrtf(a.run_var[c] + a.eps)) : 0.f;
    float s1 = 0.f, s2 = 0.f;
    float gs[kBnRegRows], xh[kBnRegRows];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < kBnRegRows; ++i) {
            const int64_t r = ty + (int64_t)kBnLanes * i;
            const bool in = ok && r < a.B;
            gs[i] = in ? a.gY[r * a.ldgy + c] : 0.f;
            xh[i] = in ? (a.X[r * a.ldx + c] - mean) * invstd : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kBnRegRows; ++i) { s1 += gs[i]; s2 += gs[i] * xh[i]; }
    } else if (ok) {
        for (int64_t r = ty; r < a.B; r += kBnLanes) {
            const float g = a.gY[r * a.ldgy + c];
            s1 += g;
            s2 += g * ((a.X[r * a.ldx + c] - mean) * invstd);
        }
    }
    s1 = bn_col_sum(red, tx, ty, s1);
    s2 = bn_col_sum(red, tx, ty, s2);
    if (!ok) return;
    if (ty == 0) {
        if (a.g_gamma) a.g_gamma[c] = s2;
        if (a.g_beta) a.g_beta[c] = s1;
    }
    const float gam = a.gamma ? a.gamma[c] : 1.f;
    const float k = gam * invstd, invB = 1.f / (float)a.B;
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < kBnRegRows; ++i) {
            const int64_t r = ty + (int64_t)kBnLanes * i;
            if (r < a.B) a.gX[r * a.ldgx + c] = a.training ? k * (gs[i] - invB * s1 - xh[i] * invB * s2) : k * gs[i];
        }
    } else {
        for (int64_t r = ty; r < a.B; r += kBnLanes) {
            const float g = a.gY[r * a.ldgy + c];
            if (a.training) {
                const float xhat = (a.X[r * a.ldx + c] - mean) * invstd;
                a.gX[r * a.ldgx + c] = k * (g - invB * s1 - xhat * invB * s2);
            } else {
                a.gX[r * a.ldgx + c] = k * g;
            }
        }
    }
}

// ---- criterion (nn/metrics.py:78-127): ONE workgroup ----------------------------------------------------------------
//   mask = isfinite(target) (models/model.py:152-153), target = nan_to_num(target)
//   bounded: P' = T where (P < T and lt) or (P > T and gt)   (metrics.py:157-161)
//   L = (P' - T)^2 | |P' - T|;   loss = sum(L w_i t_j mask) / sum(mask);   gP = dL/dP w_i t_j mask / sum(mask)
// the unreduced loss of one (prediction, target) pair and its derivative in the prediction:
//   MSE (metrics.py:137-141), MAE (:146-148), BCE with logits (:292-295: F.binary_cross_entropy_with_logits — the classification
//   predictor's train_step hands over raw logits, predictors.py:246-247):  L = (1 - y) x - log_sigmoid(x),  dL/dx = sigmoid(x) - y
__device__ __forceinline__ float loss_value(int kind, float p, float y) {
    if (kind == DMPNN_LOSS_BCE) return (1.f - y) * p - (fminf(p, 0.f) - log1pf(expf(-fabsf(p))));
    const float d = p - y;
    return kind == DMPNN_LOSS_MAE ? fabsf(d) : d * d;
}
__device__ __forceinline__ float loss_deriv(int kind, float p, float y) {
    if (kind == DMPNN_LOSS_BCE) return 1.f / (1.f + expf(-p)) - y;
    const float d = p - y;
    return kind == DMPNN_LOSS_MAE ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 2.f * d;
}

struct LossArgs {
    const float* P; int64_t ldp; const float* T; int64_t ldt; const float* w; const float* tw;
    const unsigned char* lt; const unsigned char* gt;
    float* gP; int64_t ldg; float* out;   // out[0] = loss, out[1] = number of finite targets
    int64_t B; int t; int kind;
    int nc;                               // DMPNN_LOSS_CE / _DIRICHLET: classes per task — P / gP rows hold t * nc logits / raw evidences, T the class index of every task
                                          // DMPNN_LOSS_MVE / _EVIDENTIAL: 2 / 4 — P / gP rows hold nc chunks of t columns (torch.chunk(Y, n_targets, 1))
    float v_kl, eps;                      // DMPNN_LOSS_EVIDENTIAL; v_kl also DMPNN_LOSS_DIRICHLET
    float q_alpha;                        // DMPNN_LOSS_QUANTILE
    float lg_nc;                          // DMPNN_LOSS_DIRICHLET: lgamma(nc), formed on the host (the same number for every pair)
};
// QuantileLoss (nn/metrics.py:589-610) on the raw outputs of QuantileFFN (predictors.py:215-232): mean -+ interval / 2 ARE the lower and
// upper bounds the MLP put out; per bound amax(tau e, (tau - 1) e) with e = y - bound, tau = alpha / 2 | 1 - alpha / 2
// (its derivative in the bound: -tau for e > 0, 1 - tau for e < 0, their mean at e = 0: torch.amax shares the gradient among ties)
__device__ __forceinline__ float pinball(float e, float tau, float* g) {
    if (g) *g = e > 0.f ? -tau : (e < 0.f ? 1.f - tau : 0.5f - tau);
    return fmaxf(tau * e, (tau - 1.f) * e);
}
// the derivative of F.softplus (softplus_f, dmpnn_common.hpp: beta 1, threshold 20)
__device__ __forceinline__ float softplus_d(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }
// digamma for x >= 1 (alpha = softplus + 1): the recurrence up to x >= 6, then the asymptotic series (error < 1e-7 there)
__device__ __forceinline__ float digamma_f(float x) {
    float r = 0.f;
    while (x < 6.f) { r -= 1.f / x; x += 1.f; }
    const float i = 1.f / x, i2 = i * i;
    return r + logf(x) - 0.5f * i - i2 * (1.f / 12.f - i2 * (1.f / 120.f - i2 * (1.f / 252.f)));
}
// trigamma for x >= 1: the recurrence up to x >= 6, then the asymptotic series (its next term, 1 / (30 x^9), is < 4e-9 there)
__device__ __forceinline__ float trigamma_f(float x) {
    float r = 0.f;
    while (x < 6.f) { r += 1.f / (x * x); x += 1.f; }
    const float i = 1.f / x, i2 = i * i;
    return r + i * (1.f + 0.5f * i + i2 * (1.f / 6.f - i2 * (1.f / 30.f - i2 * (1.f / 42.f))));
}
// DirichletLoss (nn/metrics.py) on the raw outputs x[0 .. K) of one task of BinaryDirichletFFN / MulticlassDirichletFFN (predictors.py):
// alpha = softplus(x) + 1, S = sum alpha, p = alpha / S, y = one_hot(cls);  L = sum (y - p)^2 + sum p (1 - p) / (S + 1) + v_kl KL(Dir(alpha~) || Dir(1))
// with alpha~ = y + (1 - y) alpha; lgK = lgamma(K).  x is read from memory in every pass (an array indexed by a runtime K would live in scratch).
// g != NULL: g[m] = f dL/dx_m —  dL_mse/dalpha_m = -2 ([m == cls] - p_cls) / S + 2 (p_m - Q) / (S + 1) - (1 - Q) / (S + 1)^2, Q = sum p^2;
// dL_kl/dalpha_m = (alpha_m - 1) psi'(alpha_m) - (S~ - K) psi'(S~) for m != cls (the digammas cancel), 0 for m == cls
__device__ __forceinline__ float dirichlet_loss(const float* __restrict__ x, int K, float lgK, int cls, float v_kl, float* __restrict__ g, float f) {
    float S = 0.f, St = 0.f, A2 = 0.f, ac = 0.f;
    for (int k = 0; k < K; ++k) {
        const float al = softplus_f(x[k]) + 1.f;
        S += al; A2 += al * al;
        St += k == cls ? 1.f : al;
        if (k == cls) ac = al;
    }
    const float iS = 1.f / S, iS1 = 1.f / (S + 1.f);
    const float dgS = digamma_f(St);
    float mse = 0.f, var = 0.f, kl = lgammaf(St) - lgK;
    for (int k = 0; k < K; ++k) {
        const float al = softplus_f(x[k]) + 1.f, p = al * iS, e = (k == cls ? 1.f : 0.f) - p;
        mse += e * e; var += p * (1.f - p);
        if (k != cls) kl += (al - 1.f) * (digamma_f(al) - dgS) - lgammaf(al);
    }
    if (g) {
        const float Q = A2 * iS * iS, pc = ac * iS, tgS = ((float)K - St) * trigamma_f(St), c0 = (1.f - Q) * iS1 * iS1;
        for (int m = 0; m < K; ++m) {
            const float al = softplus_f(x[m]) + 1.f;
            const float dmse = -2.f * ((m == cls ? 1.f : 0.f) - pc) * iS + 2.f * (al * iS - Q) * iS1 - c0;
            const float dkl = m == cls ? 0.f : (al - 1.f) * trigamma_f(al) + tgS;
            g[m] = (dmse + v_kl * dkl) * softplus_d(x[m]) * f;
        }
    }
    return mse + var * iS1 + v_kl * kl;
}
// MVELoss (nn/metrics.py:203-219) on the raw outputs of MveFFN (predictors.py:173-190): unreduced loss, d / d mean, d / d raw variance
__device__ __forceinline__ float mve_loss(float mean, float raw, float y, float* g_mean, float* g_raw) {
    const float var = softplus_f(raw), d = mean - y;
    if (g_mean) {
        *g_mean = d / var;
        *g_raw = (0.5f / var - d * d / (2.f * var * var)) * softplus_d(raw);
    }
    return d * d / (2.f * var) + 0.5f * logf(6.283185307179586f * var);
}
// EvidentialLoss (nn/metrics.py:222-262) on the raw outputs of EvidentialFFN (predictors.py:193-212); g[4]: d / d (mean, raw v, raw alpha, raw beta)
__device__ __forceinline__ float evidential_loss(const float (&x)[4], float y, float v_kl, float eps, float* g) {
    const float v = softplus_f(x[1]), al = softplus_f(x[2]) + 1.f, be = softplus_f(x[3]);
    const float res = y - x[0], tbl = 2.f * be * (1.f + v), D = v * res * res + tbl, ares = fabsf(res);
    const float nll = 0.5f * logf(3.141592653589793f / v) - al * logf(tbl) + (al + 0.5f) * logf(D) + lgammaf(al) - lgammaf(al + 0.5f);
    const float reg = (2.f * v + al) * ares;
    if (g) {
        const float sg = res > 0.f ? 1.f : (res < 0.f ? -1.f : 0.f);
        g[0] = -((al + 0.5f) * 2.f * v * res / D + v_kl * (2.f * v + al) * sg);
        g[1] = (-0.5f / v - al / (1.f + v) + (al + 0.5f) * (res * res + 2.f * be) / D + v_kl * 2.f * ares) * softplus_d(x[1]);
        g[2] = (logf(D) - logf(tbl) + digamma_f(al) - digamma_f(al + 0.5f) + v_kl * ares) * softplus_d(x[2]);
        g[3] = (-al / be + (al + 0.5f) * 2.f * (1.f + v) / D) * softplus_d(x[3]);
    }
    return nll + v_kl * (reg - eps);
}
__global__ __launch_bounds__(1024) void k_loss(LossArgs a) {
    __shared__ float red[2][16];
    __shared__ float tot[2];
    const int64_t n = a.B * a.t;
    float sl = 0.f, sm = 0.f;
    // (uniform) the Dirichlet criterion — the task's nc evidence outputs, laid out like the logits of cross entropy — in a loop of its
    // own, in front of the tests that mean "chunked outputs": its registers stay out of the other criteria's loop
    if (a.kind == DMPNN_LOSS_DIRICHLET) {
        for (int64_t i = threadIdx.x; i < n; i += 1024) {
            const int64_t r = i / a.t; const int j = (int)(i - r * a.t);
            const float y = a.T[r * a.ldt + j];
            if (!isfinite(y)) continue;
            const int cls = (int)y;
            const float L = dirichlet_loss(a.P + r * a.ldp + (int64_t)j * a.nc, a.nc, a.lg_nc, cls, a.v_kl, nullptr, 0.f);
            sl += ((cls >= 0 && cls < a.nc) ? L : __int_as_float(0x7fc00000)) * (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f);
            sm += 1.f;
        }
    } else
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int64_t r = i / a.t; const int j = (int)(i - r * a.t);
        const float y = a.T[r * a.ldt + j];
        const bool m = isfinite(y);
        if (!m) continue;
        if (a.kind == DMPNN_LOSS_CE) {   // (uniform) F.cross_entropy over the task's nc logits: logsumexp - x[class]   (metrics.py:298-304)
            const float* x = a.P + r * a.ldp + (int64_t)j * a.nc;
            float mx = x[0];
            for (int k = 1; k < a.nc; ++k) mx = fmaxf(mx, x[k]);
            float se = 0.f;
            for (int k = 0; k < a.nc; ++k) se += expf(x[k] - mx);
            const int cls = (int)y;
            const float L = (mx + logf(se)) - x[(cls >= 0 && cls < a.nc) ? cls : 0];
            sl += ((cls >= 0 && cls < a.nc) ? L : __int_as_float(0x7fc00000)) * (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f);
            sm += 1.f;
            continue;
        }
        if (a.kind >= DMPNN_LOSS_MVE) {   // (uniform) chunked outputs: column k t + j is target k of task j
            const float* x = a.P + r * a.ldp + j;
            float L;
            if (a.kind == DMPNN_LOSS_MVE) L = mve_loss(x[0], x[a.t], y, nullptr, nullptr);
            else if (a.kind == DMPNN_LOSS_QUANTILE) L = pinball(y - x[0], 0.5f * a.q_alpha, nullptr) + pinball(y - x[a.t], 1.f - 0.5f * a.q_alpha, nullptr);
            else { const float xs[4] = {x[0], x[a.t], x[2 * a.t], x[3 * a.t]}; L = evidential_loss(xs, y, a.v_kl, a.eps, nullptr); }
            sl += L * (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f);
            sm += 1.f;
            continue;
        }
        float p = a.P[r * a.ldp + j];
        if ((a.lt && a.lt[r * a.t + j] && p < y) || (a.gt && a.gt[r * a.t + j] && p > y)) p = y;
        const float L = loss_value(a.kind, p, y);
        sl += L * (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f);
        sm += 1.f;
    }
    for (int off = 32; off > 0; off >>= 1) { sl += __shfl_xor(sl, off); sm += __shfl_xor(sm, off); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sl; red[1][threadIdx.x >> 6] = sm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a0 = 0.f, a1 = 0.f;
        for (int i = 0; i < 16; ++i) { a0 += red[0][i]; a1 += red[1][i]; }
        tot[0] = a0; tot[1] = a1;
        a.out[0] = a0 / a1;   // (no finite target: 0 / 0 = NaN, like the reference)
        a.out[1] = a1;
    }
    __syncthreads();
    if (!a.gP) return;
    const float inv = 1.f / tot[1];
    if (a.kind == DMPNN_LOSS_DIRICHLET) {   // (uniform; a loop of its own, as above)
        for (int64_t i = threadIdx.x; i < n; i += 1024) {
            const int64_t r = i / a.t; const int j = (int)(i - r * a.t);
            const float y = a.T[r * a.ldt + j];
            float* gx = a.gP + r * a.ldg + (int64_t)j * a.nc;
            if (!isfinite(y)) {
                for (int k = 0; k < a.nc; ++k) gx[k] = 0.f;
                continue;
            }
            dirichlet_loss(a.P + r * a.ldp + (int64_t)j * a.nc, a.nc, a.lg_nc, (int)y, a.v_kl, gx, (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f) * inv);
        }
        return;
    }
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int64_t r = i / a.t; const int j = (int)(i - r * a.t);
        const float y = a.T[r * a.ldt + j];
        if (a.kind == DMPNN_LOSS_CE) {   // (uniform) dL/dx_k = softmax_k - [k == class]
            const float* x = a.P + r * a.ldp + (int64_t)j * a.nc;
            float* gx = a.gP + r * a.ldg + (int64_t)j * a.nc;
            if (!isfinite(y)) {
                for (int k = 0; k < a.nc; ++k) gx[k] = 0.f;
                continue;
            }
            float mx = x[0];
            for (int k = 1; k < a.nc; ++k) mx = fmaxf(mx, x[k]);
            float se = 0.f;
            for (int k = 0; k < a.nc; ++k) se += expf(x[k] - mx);
            const float f = (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f) * inv, ise = 1.f / se;
            const int cls = (int)y;
            for (int k = 0; k < a.nc; ++k) gx[k] = (expf(x[k] - mx) * ise - (k == cls ? 1.f : 0.f)) * f;
            continue;
        }
        if (a.kind >= DMPNN_LOSS_MVE) {   // (uniform)
            const float* x = a.P + r * a.ldp + j;
            float* gx = a.gP + r * a.ldg + j;
            float g4[4] = {0.f, 0.f, 0.f, 0.f};
            if (isfinite(y)) {
                if (a.kind == DMPNN_LOSS_MVE) mve_loss(x[0], x[a.t], y, &g4[0], &g4[1]);
                else if (a.kind == DMPNN_LOSS_QUANTILE) { pinball(y - x[0], 0.5f * a.q_alpha, &g4[0]); pinball(y - x[a.t], 1.f - 0.5f * a.q_alpha, &g4[1]); }
                else { const float xs[4] = {x[0], x[a.t], x[2 * a.t], x[3 * a.t]}; evidential_loss(xs, y, a.v_kl, a.eps, g4); }
            }
            const float f = (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f) * inv;
            for (int k = 0; k < a.nc; ++k) gx[(int64_t)k * a.t] = g4[k] * f;
            continue;
        }
        float g = 0.f;
        if (isfinite(y)) {
            float p = a.P[r * a.ldp + j];
            if ((a.lt && a.lt[r * a.t + j] && p < y) || (a.gt && a.gt[r * a.t + j] && p > y)) p = y;
            const float dl = loss_deriv(a.kind, p, y);
            g = dl * (a.w ? a.w[r] : 1.f) * (a.tw ? a.tw[j] : 1.f) * inv;
        }
        a.gP[r * a.ldg + j] = g;
    }
}

// ---- the spectral criteria (DMPNN_LOSS_SID / _WASSERSTEIN, dmpnn.h): a grid over molecule rows ---------------------------------
// A spectrum has hundreds to thousands of tasks and every (molecule, task) pair is coupled to its whole row, so k_loss's one
// workgroup over all pairs does not fit.  k_spectral_rows: ONE workgroup of kSpecCols threads per molecule row, thread i on column
// pass * kSpecCols + i (coalesced), the row re-read from memory in every sweep (it is in the CU's cache after the first):
//     a = softplus(x) | exp(x - max x),  A = sum a,  p = a / A,  c = max(p, thr),  Z = sum m c,  q = c / Z
//     SID:         L_j = m (q - y) log(q / y);                 G_j = dL/dq_j = tw_j m_j (log(q_j / y_j) + 1 - y_j / q_j)
//     Wasserstein: D_j = sum_{k <= j} (y_k - q_k), L_j = |D_j|;  G_j = -sum_{k >= j} tw_k m_k sign(D_k)   (masked columns included)
//     S = sum G q;  dl/dc_j = (G_j - m_j S) / Z;  dl/dp_j = [p_j >= thr] dl/dc_j;  R = sum_k dl/dp_k p_k = (V - S U) / Z with
//     V = sum_{p >= thr} G p, U = sum_{p >= thr} m p (without a threshold R is analytically 0 and is not formed);
//     dl/da_j = (dl/dp_j - R) / A;  dl/dx_j = dl/da_j a'(x_j) w_i            (a' = sigmoid(x) | a)
// Sums: lane shuffles inside a wave, the four waves' totals through LDS in wave order, thread partials in pass order — a fixed order.
// The running sums of the Wasserstein distance are scans inside a wave (shuffles), a carry across the waves and the passes; the
// gradient's suffix sums run the same way from the last pass to the first.  The row's loss w_i sum_j tw_j m_j L_j (NaN for a row
// without a finite target), its count of finite targets and the gradient WITHOUT the grid-wide factor 1 / sum m leave the kernel;
// k_spectral_finish sums the counts (integers) in every workgroup, the rows' losses in workgroup 0 in a fixed order, and scales the
// gradient: two launches, no atomics, no host read, bit-identical from call to call.
constexpr int kSpecCols = 256;                 // columns per pass = threads per workgroup (one molecule row per workgroup)
constexpr int kSpecWaves = kSpecCols / 64;
struct SpectralArgs {
    const float* X; int64_t ldx; const float* T; int64_t ldt; const float* w; const float* tw;
    float* gP; int64_t ldg; float* out;   // gP (or NULL: the loss alone) rows of ldg; out[0] = loss, out[1] = number of finite targets
    int64_t B; int t; int kind; int act; float thr;   // act: 0 softplus, 1 exp;  thr: 0 = none
    float* rowloss; int* cnt;                          // [B] each (workspace): what k_spectral_rows leaves for k_spectral_finish
};
// the same sum in every thread of the workgroup; red: kSpecWaves floats of LDS, shared by every call (hence the leading barrier)
__device__ __forceinline__ float spec_block_sum(float v, float* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float spec_block_max(float v, float* red) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
// one pass of kSpecCols columns: the inclusive prefix sum (REV: suffix sum) of v over the workgroup's threads on top of `carry`, the
// sum of every pass before (REV: behind) this one, which takes this pass's total
template <bool REV>
__device__ __forceinline__ float spec_block_scan(float v, float& carry, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const float u = REV ? __shfl_down(v, off) : __shfl_up(v, off);
        if (REV ? lane + off < 64 : lane >= off) v += u;
    }
    __syncthreads();
    if (lane == (REV ? 0 : 63)) red[wave] = v;
    __syncthreads();
    float pre = carry, all = carry;
    for (int k = 0; k < kSpecWaves; ++k) {
        const int wk = REV ? kSpecWaves - 1 - k : k;   // (the waves in the scan's direction)
        if (REV ? wk > wave : wk < wave) pre += red[wk];
        all += red[wk];
    }
    carry = all;
    return v + pre;
}
__global__ __launch_bounds__(kSpecCols) void k_spectral_rows(SpectralArgs a) {
    __shared__ float red[kSpecWaves];
    __shared__ int redi[kSpecWaves];
    const int tid = threadIdx.x, t = a.t;
    const int64_t r = blockIdx.x;
    const float* __restrict__ x = a.X + r * a.ldx;
    const float* __restrict__ T = a.T + r * a.ldt;
    float* g = a.gP ? a.gP + r * a.ldg : nullptr;
    const bool ex = a.act == 1, sid = a.kind == DMPNN_LOSS_SID;
    const float thr = a.thr;
    // exp: the row maximum is subtracted first (the same p in exact arithmetic; finite where exp(x) alone overflows)
    float mx = 0.f;
    if (ex) {
        float m = -INFINITY;
        for (int j = tid; j < t; j += kSpecCols) m = fmaxf(m, x[j]);
        mx = spec_block_max(m, red);
    }
    auto act = [&](float v) { return ex ? expf(v - mx) : softplus_f(v); };
    float s0 = 0.f;
    for (int j = tid; j < t; j += kSpecCols) s0 += act(x[j]);
    const float A = spec_block_sum(s0, red);
    float sz = 0.f, su = 0.f;
    int c = 0;
    for (int j = tid; j < t; j += kSpecCols) {
        if (!isfinite(T[j])) continue;
        const float p = act(x[j]) / A;
        ++c; sz += fmaxf(p, thr);
        if (p >= thr) su += p;
    }
    const float Z = spec_block_sum(sz, red), U = spec_block_sum(su, red);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((tid & 63) == 0) redi[tid >> 6] = c;   // (read behind the barriers of the sums below)
    // the row's loss; into g the derivative G_j of sum_j tw_j m_j L_j in q_j (SID) or the weighted signs tw_j m_j sign(D_j) (Wasserstein)
    float sl = 0.f, sS = 0.f, sV = 0.f;
    if (sid) {
        for (int j = tid; j < t; j += kSpecCols) {
            const float y = T[j];
            float G = 0.f;
            if (isfinite(y)) {
                const float p = act(x[j]) / A, q = fmaxf(p, thr) / Z, lr = logf(q / y), twj = a.tw ? a.tw[j] : 1.f;
                sl += twj * (q * lr + y * logf(y / q));
                G = twj * (lr + 1.f - y / q);
                sS += G * q;
                if (p >= thr) sV += G * p;
            }
            if (g) g[j] = G;
        }
    } else {
        const int last = ((t - 1) / kSpecCols) * kSpecCols;
        float carry = 0.f;
        for (int j0 = 0; j0 <= last; j0 += kSpecCols) {   // (every thread takes part in every pass's scan)
            const int j = j0 + tid;
            const bool in = j < t;
            const float y = in ? T[j] : 0.f;
            const bool m = in && isfinite(y);
            const float q = in ? fmaxf(act(x[j]) / A, thr) / Z : 0.f;
            const float D = spec_block_scan<false>((m ? y : 0.f) - q, carry, red);
            if (m) {
                const float twj = a.tw ? a.tw[j] : 1.f;
                sl += twj * fabsf(D);
                if (g) g[j] = twj * (D > 0.f ? 1.f : (D < 0.f ? -1.f : 0.f));
            } else if (in && g) g[j] = 0.f;
        }
        if (g) {   // (uniform) G_j = -sum_{k >= j} of the signs: each thread re-reads what it wrote itself
            carry = 0.f;
            for (int j0 = last; j0 >= 0; j0 -= kSpecCols) {
                const int j = j0 + tid;
                const bool in = j < t;
                const float G = -spec_block_scan<true>(in ? g[j] : 0.f, carry, red);
                if (in) {
                    const float p = act(x[j]) / A;
                    sS += G * (fmaxf(p, thr) / Z);
                    if (p >= thr) sV += G * p;
                    g[j] = G;
                }
            }
        }
    }
    const float SL = spec_block_sum(sl, red);
    if (tid == 0) {
        const int n = (redi[0] + redi[1]) + (redi[2] + redi[3]);
        a.cnt[r] = n;
        a.rowloss[r] = n > 0 ? (a.w ? a.w[r] : 1.f) * SL : __int_as_float(0x7fc00000);   // (a row without a finite target: NaN, dmpnn.h)
    }
    if (!g) return;   // (uniform)
    const float S = spec_block_sum(sS, red), V = spec_block_sum(sV, red);
    const float R = thr > 0.f ? (V - S * U) / Z : 0.f, wr = a.w ? a.w[r] : 1.f;
    for (int j = tid; j < t; j += kSpecCols) {
        const float xv = x[j], av = act(xv), p = av / A;
        const float gp = p >= thr ? (g[j] - (isfinite(T[j]) ? S : 0.f)) / Z : 0.f;
        g[j] = (gp - R) / A * (ex ? av : softplus_d(xv)) * wr;
    }
}
__global__ __launch_bounds__(kSpecCols) void k_spectral_finish(SpectralArgs a) {
    __shared__ float red[kSpecWaves];
    __shared__ int redi[kSpecWaves];
    const int tid = threadIdx.x;
    int c = 0;
    for (int64_t i = tid; i < a.B; i += kSpecCols) c += a.cnt[i];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((tid & 63) == 0) redi[tid >> 6] = c;
    __syncthreads();
    const float M = (float)((redi[0] + redi[1]) + (redi[2] + redi[3]));
    if (blockIdx.x == 0) {
        float s = 0.f;
        for (int64_t i = tid; i < a.B; i += kSpecCols) s += a.rowloss[i];
        s = spec_block_sum(s, red);
        if (tid == 0) { a.out[0] = s / M; a.out[1] = M; }   // (no finite target: NaN, like every criterion)
    }
    if (!a.gP) return;
    const float inv = 1.f / M;
    const int64_t n = a.B * a.t;
    for (int64_t i = (int64_t)blockIdx.x * kSpecCols + tid; i < n; i += (int64_t)gridDim.x * kSpecCols) {
        const int64_t r = i / a.t;
        a.gP[r * a.ldg + (i - r * a.t)] *= inv;
    }
}

// ---- the binary MCC criterion (DMPNN_LOSS_MCC, dmpnn.h): a column reduction over blocks of molecule rows -------------------------
// The loss of one (molecule, task) pair depends on four batch-wide sums of its task's column, so no gradient can be written before
// a grid-wide reduction down the columns: two launches.
//   k_mcc_cols:   workgroup rb n_cb + cb takes the kMccRows molecule rows of row block rb and the kMccThreads task columns of column
//                 block cb and leaves TP, FP, TN, FN of its rows per task in part[rb][.][j], its count of finite targets in
//                 cnt[rb n_cb + cb].
//   k_mcc_finish: per column block the blocks' partials per task in block order (double), MCC_j and the two gradient coefficients
//                 per task (double: N = TP TN - FP FN cancels), then dl/dx for the row blocks the workgroup owns (gP == NULL: one
//                 workgroup, the loss alone); workgroup 0 writes out[0] = 1 - sum_j tw_j MCC_j / t and out[1] = sum m.
// Threads to (row, task): C = 2^lgC = the smallest power of two >= min(t, kMccThreads); thread i is on column i % C of the column
// block and on the rows i / C, i / C + kMccThreads / C, ... of the row block.  X and T are row-major with t columns: for t <= 64 a wave
// reads 64 / C whole rows, which lie one behind the other in memory (t = 12: 48 consecutive floats, 16 lanes idle), for t in the
// hundreds 64 consecutive columns of one row.  Threads on the same column: the lanes C apart of a wave (xor shuffles down to C), then
// the waves through LDS in wave order — a fixed order; no atomics; bit-identical from call to call.
constexpr int kMccRows = 128;                  // molecule rows one k_mcc_cols workgroup takes
constexpr int kMccThreads = 256;               // threads per workgroup = task columns per column block
constexpr int kMccFinishMaxBlocks = 128;       // workgroups of k_mcc_finish (each one adds up every row block's partials)
struct MccArgs {
    const float* X; int64_t ldx; const float* T; int64_t ldt; const float* w; const float* tw;
    float* gP; int64_t ldg; float* out;   // gP (or NULL: the loss alone) rows of ldg; out[0] = loss, out[1] = number of finite targets
    int64_t B; int t; int lgC;            // C = 1 << lgC
    int n_blocks, n_cb;                   // row blocks of kMccRows rows, column blocks of kMccThreads columns
    float* part; int* cnt;                // [n_blocks][4][t] (TP, FP, TN, FN), [n_blocks n_cb] (workspace)
};
// p = sigmoid(x) and q = 1 - p = sigmoid(-x), neither by a subtraction from 1
__device__ __forceinline__ void sigmoid_pair(float x, float& p, float& q) {
    const float e = expf(-fabsf(x)), r = 1.f / (1.f + e), s = e * r;
    p = x >= 0.f ? r : s;
    q = x >= 0.f ? s : r;
}
// v[k] of the threads on one column (tid % C) summed: into thread `column` (tid < C); red: NV * kMccThreads values of LDS
template <class V, int NV>
__device__ __forceinline__ void mcc_col_reduce(V (&v)[NV], int C, V* red) {
    const int tid = threadIdx.x;
    for (int off = 32; off >= C; off >>= 1) {   // (uniform; C < 64: the lanes of a wave on the same column)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += __shfl_xor(v[k], off);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k * kMccThreads + tid] = v[k];
    __syncthreads();
    if (tid < C) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            V s = 0;
            for (int wv = 0; wv < kMccThreads / 64; ++wv) {   // (the waves that hold this column, in wave order)
                const int idx = wv * 64 + (tid & 63);
                if ((idx & (C - 1)) == tid) s += red[k * kMccThreads + idx];
            }
            v[k] = s;
        }
    }
}
__global__ __launch_bounds__(kMccThreads) void k_mcc_cols(MccArgs a) {
    __shared__ float red[4 * kMccThreads];
    __shared__ int redi[kMccThreads / 64];
    const int tid = threadIdx.x, t = a.t, C = 1 << a.lgC, c = tid & (C - 1), rl = tid >> a.lgC, RL = kMccThreads >> a.lgC;
    const int64_t rb = blockIdx.x / a.n_cb;   // (workgroup rb n_cb + cb)
    const int cb = (int)(blockIdx.x - rb * a.n_cb), j = cb * kMccThreads + c;
    const int64_t r0 = rb * kMccRows, r1 = r0 + kMccRows < a.B ? r0 + kMccRows : a.B;
    const bool valid = j < t;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 0;
    if (valid)
        for (int64_t r = r0 + rl; r < r1; r += RL) {
            const float y = a.T[r * a.ldt + j];
            if (!isfinite(y)) continue;
            ++n;
            float p, q;
            sigmoid_pair(a.X[r * a.ldx + j], p, q);
            const float wy = (a.w ? a.w[r] : 1.f) * y, wn = (a.w ? a.w[r] : 1.f) * (1.f - y);
            v[0] += wy * p; v[1] += wn * p; v[2] += wn * q; v[3] += wy * q;
        }
    mcc_col_reduce<float, 4>(v, C, red);
    if (tid < C && valid) {
        float* o = a.part + rb * 4 * t + j;
        o[0] = v[0]; o[t] = v[1]; o[2 * (int64_t)t] = v[2]; o[3 * (int64_t)t] = v[3];
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((tid & 63) == 0) redi[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) a.cnt[blockIdx.x] = (redi[0] + redi[1]) + (redi[2] + redi[3]);
}
__global__ __launch_bounds__(kMccThreads) void k_mcc_finish(MccArgs a) {
    __shared__ double red[4 * kMccThreads];
    __shared__ float coef[2 * kMccThreads];
    __shared__ int redi[kMccThreads / 64];
    const int tid = threadIdx.x, t = a.t, C = 1 << a.lgC, c = tid & (C - 1), rl = tid >> a.lgC, RL = kMccThreads >> a.lgC;
    double lsum = 0.0;   // (workgroup 0, threads < C: sum over this thread's columns of tw_j MCC_j)
    for (int cb = 0; cb < a.n_cb; ++cb) {
        const int j = cb * kMccThreads + c;
        const bool valid = j < t;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (valid)
            for (int blk = rl; blk < a.n_blocks; blk += RL) {
                const float* p = a.part + (int64_t)blk * 4 * t + j;
                v[0] += p[0]; v[1] += p[t]; v[2] += p[2 * (int64_t)t]; v[3] += p[3 * (int64_t)t];
            }
        mcc_col_reduce<double, 4>(v, C, red);
        if (tid < C) {   // (tid == c)
            float al = 0.f, be = 0.f;
            if (valid) {
                const double TP = v[0], FP = v[1], TN = v[2], FN = v[3];
                const double A = TP + FP, Bq = TP + FN, Cq = TN + FP, E = TN + FN, N = TP * TN - FP * FN;
                const double iS = 1.0 / sqrt(A * Bq * Cq * E + 1e-8), mcc = N * iS, hN = 0.5 * mcc * iS * iS;   // hN = N / (2 S^3)
                // g(dN, dD) = dN / S - N dD / (2 S^3); one class absent: N and the present class's dN, dD are exactly 0
                const double alpha = (TN * iS - hN * (Bq * Cq * E + A * Cq * E)) - (-FP * iS - hN * (A * Cq * E + A * Bq * Cq));
                const double beta = (-FN * iS - hN * (Bq * Cq * E + A * Bq * E)) - (TP * iS - hN * (A * Bq * E + A * Bq * Cq));
                const double twj = a.tw ? (double)a.tw[j] : 1.0, sc = -twj / (double)t;
                al = (float)(sc * alpha); be = (float)(sc * beta);
                if (blockIdx.x == 0) lsum += twj * mcc;
            }
            coef[tid] = al; coef[kMccThreads + tid] = be;
        }
        __syncthreads();
        if (a.gP && valid) {
            const float al = coef[c], be = coef[kMccThreads + c];
            for (int64_t rb = blockIdx.x; rb < a.n_blocks; rb += gridDim.x) {
                const int64_t r0 = rb * kMccRows, r1 = r0 + kMccRows < a.B ? r0 + kMccRows : a.B;
                for (int64_t r = r0 + rl; r < r1; r += RL) {
                    const float y = a.T[r * a.ldt + j];
                    float g = 0.f;   // (no finite target: exactly 0)
                    if (isfinite(y)) {
                        float p, q;
                        sigmoid_pair(a.X[r * a.ldx + j], p, q);
                        g = (a.w ? a.w[r] : 1.f) * (y * al + (1.f - y) * be) * (p * q);
                    }
                    a.gP[r * a.ldg + j] = g;
                }
            }
        }
        // (coef is written again behind the two barriers of the next pass's mcc_col_reduce)
    }
    if (blockIdx.x != 0) return;
    for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off);
    int n = 0;
    for (int64_t i = tid; i < (int64_t)a.n_blocks * a.n_cb; i += kMccThreads) n += a.cnt[i];
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = lsum; redi[tid >> 6] = n; }
    __syncthreads();
    if (tid == 0) {
        a.out[0] = (float)(1.0 - ((red[0] + red[1]) + (red[2] + red[3])) / (double)t);   // (no finite target: 1, dmpnn.h)
        a.out[1] = (float)((redi[0] + redi[1]) + (redi[2] + redi[3]));
    }
}

// ---- the predictor's OUTPUT layer for a handful of tasks (n_tasks <= kOutMaxTasks: the usual regression head) ----------------
// P = A W^T + b with W [t, K]: t dot products per row — one wave per row, lanes over K (a 16 x 16 MFMA tile would be 1/16 full
// and the generic contraction kernel spends 17 us on its pipeline for 0.3 MFLOP).
constexpr int kOutMaxTasks = 4;
struct OutFwdArgs { const float* A; int64_t lda; const float* W; const float* b; float* P; int64_t B; int K, t; };
__global__ __launch_bounds__(256) void k_out_fwd(OutFwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.B) return;
    float acc[kOutMaxTasks] = {0.f, 0.f, 0.f, 0.f};
    for (int k = lane; k < a.K; k += 64) {
        const float x = a.A[r * a.lda + k];
#pragma unroll
        for (int j = 0; j < kOutMaxTasks; ++j)
            if (j < a.t) acc[j] += x * a.W[(int64_t)j * a.K + k];
    }
#pragma unroll
    for (int j = 0; j < kOutMaxTasks; ++j) {
        float v = acc[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0 && j < a.t) a.P[r * a.t + j] = v + (a.b ? a.b[j] : 0.f);
    }
}
// Its whole backward in one launch (16 columns x 64 row lanes per workgroup, like the batch-norm kernels):
//   gA[r][k] = (sum_j gP[r][j] W[j][k]) tau'(A[r][k])      (A = tau(previous layer): the derivative from the output)
//   gW[j][k] = sum_r gP[r][j] A[r][k],   gb[j] = sum_r gP[r][j]
struct OutBwdArgs {
    const float* gP; const float* A; int64_t lda; const float* W; float* gA; int64_t ldga; float* gW; float* gb;
    int64_t B; int K, t, act; float slope;
    FfnDrop drop;                          // the mask of A (the layer's input; off for the first layer)
};
__global__ __launch_bounds__(1024) void k_out_bwd(OutBwdArgs a) {
    __shared__ float red[kBnLanes][kBnCols];
    const int tx = threadIdx.x & (kBnCols - 1), ty = threadIdx.x / kBnCols;
    const int k = blockIdx.x * kBnCols + tx;
    const bool ok = k < a.K;
    float w[kOutMaxTasks], gw[kOutMaxTasks], gbs[kOutMaxTasks];
#pragma unroll
    for (int j = 0; j < kOutMaxTasks; ++j) { w[j] = (ok && j < a.t) ? a.W[(int64_t)j * a.K + k] : 0.f; gw[j] = 0.f; gbs[j] = 0.f; }
    for (int64_t r = ty; r < a.B; r += kBnLanes) {
        const float x = ok ? a.A[r * a.lda + k] : 0.f;
        float g = 0.f;
#pragma unroll
        for (int j = 0; j < kOutMaxTasks; ++j)
            if (j < a.t) { const float gp = a.gP[r * a.t + j]; g += gp * w[j]; gw[j] += gp * x; gbs[j] += gp; }
        if (ok && a.gA) a.gA[r * a.ldga + k] = g * (a.drop.on ? a.drop.act_grad(r, k, x, a.act, a.slope) : act_grad_from_out(x, a.act, a.slope));
    }
    for (int j = 0; j < a.t; ++j) {
        const float sw = bn_col_sum(red, tx, ty, gw[j]);
        if (ok && ty == 0 && a.gW) a.gW[(int64_t)j * a.K + k] = sw;
        if (a.gb && blockIdx.x == 0) {     // (uniform per workgroup: every thread of workgroup 0 takes part in the reduction)
            const float sb = bn_col_sum(red, tx, ty, gbs[j]);
            if (tx == 0 && ty == 0) a.gb[j] = sb;
        }
    }
}

// Criterion + the output layer's backward in ONE launch (training, <= kOutAllMaxRows molecules).  Every workgroup (16 columns of
// the layer's input, like k_out_bwd) first forms dl/dP for ALL molecules in its own LDS from the predictions k_out_fwd wrote —
// B t values, cheaper to redo per workgroup than a launch of its own — then runs its slice of the backward on them.  Workgroup
// 0 writes the loss and the count.  Same arithmetic as the two kernels it replaces (k_loss's lane / wave order, k_out_bwd's
// column sums).  (Recomputing the predictions per workgroup as well was tried: 89 us — 16 waves walking 512 rows each is a
// latency chain, where k_out_fwd's one wave per row is 5 us.)
constexpr int64_t kOutAllMaxRows = 1024;
struct OutAllArgs {
    OutBwdArgs o;                   // (o.gP unused: dl/dP lives in LDS)
    LossArgs l;                     // (l.gP / l.ldg unused)
};
__global__ __launch_bounds__(1024) void k_out_all(OutAllArgs q) {
    __shared__ float Ps[kOutAllMaxRows * kOutMaxTasks];
    __shared__ float gPs[kOutAllMaxRows * kOutMaxTasks];
    __shared__ float red[kBnLanes][kBnCols];
    __shared__ float red2[2][16];
    __shared__ float tot[2];
    const OutBwdArgs& a = q.o;
    const LossArgs& L = q.l;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = a.t;
    for (int64_t i = threadIdx.x; i < a.B * t; i += 1024) Ps[i] = L.P[(i / t) * L.ldp + (i % t)];
    __syncthreads();
    // ---- criterion (k_loss's arithmetic) ----
    const int64_t n = a.B * t;
    float sl = 0.f, sm = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int64_t r = i / t; const int j = (int)(i - r * t);
        const float y = L.T[r * L.ldt + j];
        if (!isfinite(y)) continue;
        float p = Ps[i];
        if ((L.lt && L.lt[i] && p < y) || (L.gt && L.gt[i] && p > y)) p = y;
        const float Lv = loss_value(L.kind, p, y);
        sl += Lv * (L.w ? L.w[r] : 1.f) * (L.tw ? L.tw[j] : 1.f);
        sm += 1.f;
    }
    for (int off = 32; off > 0; off >>= 1) { sl += __shfl_xor(sl, off); sm += __shfl_xor(sm, off); }
    if (lane == 0) { red2[0][wave] = sl; red2[1][wave] = sm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a0 = 0.f, a1 = 0.f;
        for (int i = 0; i < 16; ++i) { a0 += red2[0][i]; a1 += red2[1][i]; }
        tot[0] = a0; tot[1] = a1;
        if (blockIdx.x == 0) { L.out[0] = a0 / a1; L.out[1] = a1; }
    }
    __syncthreads();
    const float inv = 1.f / tot[1];
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int64_t r = i / t; const int j = (int)(i - r * t);
        const float y = L.T[r * L.ldt + j];
        float g = 0.f;
        if (isfinite(y)) {
            float p = Ps[i];
            if ((L.lt && L.lt[i] && p < y) || (L.gt && L.gt[i] && p > y)) p = y;
            const float dl = loss_deriv(L.kind, p, y);
            g = dl * (L.w ? L.w[r] : 1.f) * (L.tw ? L.tw[j] : 1.f) * inv;
        }
        gPs[i] = g;
    }
    __syncthreads();
    // ---- the layer's backward on this workgroup's 16 columns (k_out_bwd's arithmetic) ----
    const int tx = threadIdx.x & (kBnCols - 1), ty = threadIdx.x / kBnCols;
    const int k = blockIdx.x * kBnCols + tx;
    const bool ok = k < a.K;
    float w[kOutMaxTasks], gw[kOutMaxTasks], gbs[kOutMaxTasks];
#pragma unroll
    for (int j = 0; j < kOutMaxTasks; ++j) { w[j] = (ok && j < t) ? a.W[(int64_t)j * a.K + k] : 0.f; gw[j] = 0.f; gbs[j] = 0.f; }
    for (int64_t r = ty; r < a.B; r += kBnLanes) {
        const float x = ok ? a.A[r * a.lda + k] : 0.f;
        float g = 0.f;
#pragma unroll
        for (int j = 0; j < kOutMaxTasks; ++j)
            if (j < t) { const float gp = gPs[r * t + j]; g += gp * w[j]; gw[j] += gp * x; gbs[j] += gp; }
        if (ok && a.gA) a.gA[r * a.ldga + k] = g * (a.drop.on ? a.drop.act_grad(r, k, x, a.act, a.slope) : act_grad_from_out(x, a.act, a.slope));
    }
    for (int j = 0; j < t; ++j) {
        const float sw = bn_col_sum(red, tx, ty, gw[j]);
        if (ok && ty == 0 && a.gW) a.gW[(int64_t)j * a.K + k] = sw;
        if (a.gb && blockIdx.x == 0) {
            const float sb = bn_col_sum(red, tx, ty, gbs[j]);
            if (tx == 0 && ty == 0) a.gb[j] = sb;
        }
    }
}

// =====================================================================================================================
// Round 5: the head of a training step in FOUR launches (was nine) for the usual predictor — one hidden layer, <= kOutMaxTasks
// outputs, <= kRowsMaxB molecules, widths <= kRowsMaxWidth (five launches beyond kFuseAggMols molecules: the aggregation in front):
//   k_agg_bn_fwd        per 8 | 16 columns: H = agg(H_v) (the rows added in increasing atom order, like k_mol_reduce) and Z = bn(H)
//                       on the values still in registers; the workgroups behind those SPLIT the hidden layer's weight (fragment-major
//                       hi | lo, both orientations) — the split rides in this launch like the block's rides in K0: nothing about
//                       weights is cached;
//   k_head_rows<., 1>   per (16 molecules, 64 columns): A1 = tau(Z W0^T + b0) on the f16 pipe (3-product split, fp32 accumulation:
//                       the block's arithmetic);
//   k_head_rows<., 2>   per (16 molecules, 64 columns), everything that is local to a row from the whole rows of A1: P = A1 W1^T + b1,
//                       the criterion (every workgroup counts the finite targets of the WHOLE batch itself: B t values), dl/dP,
//                       dl/dA1, then its slice of dl/dZ = dl/dA1 . W0 on the f16 pipe; what sums over rows (gW1, gb1, the loss)
//                       leaves as one partial per row block;
//   k_bn_agg_bwd        per 8 | 16 columns: batch norm backward and the broadcast of dl/dH to the atoms' rows (k_mol_bwd's
//                       arithmetic); one more workgroup sums the partials in a fixed order (deterministic).
// The hidden layer's weight gradient rides in the block's backward launches as before (ExtraWgrad) or runs as its own product.
// What set the shapes (profiles/r05_head_*): a CU pulls ~55 GB/s — whole rows per workgroup (32 workgroups, 820 KB of weight
// fragments each) took 27-33 us, 16 columns x all atoms per workgroup (19 workgroups) 11 us for the aggregation alone; and a
// conditional load `ok ? p[i] : 0` compiles to a branch with a full wait behind it — every scalar below is a buffer load instead.
// DMPNN_HEAD=chain (environment, read per call): the nine-launch chain of rounds 3-4, kept for every other shape; =rows: a training
// call that would take the chain is an error (tests).
constexpr int64_t kRowsMaxB = 1024;      // (4 molecules per thread of the column kernels)
constexpr int64_t kFuseAggMols = 512;    // batches up to this size are aggregated inside k_agg_bn_fwd
constexpr int kRowsMaxWidth = 320;       // WN <= 5 column tiles per wave
constexpr int kRowsMaxK = 512;           // with molecule descriptors: the first layer's reduction width d_h + d_xd (k_head_rows<8, 1>)
typedef float f32x4 __attribute__((ext_vector_type(4)));
using mega16::h4;
using mega16::h8;
using mega16::SplitW;

// Buffer loads for the column kernels' scalars: an offset out of range (or a NULL array: a zero-length buffer) reads 0 — no branch,
// no select on the loaded value, so a batch of requests goes out before the first wait (a conditional `ok ? p[i] : 0` compiles to a
// branch with a full wait behind EVERY load: 16 serialised round trips for a thread's molecule bounds, 11 us).
__device__ __forceinline__ gemm::rsrc_t col_buf(const void* p, int64_t bytes, const void* dummy) {
    return gemm::make_rsrc(p ? p : dummy, p ? gemm::clamp_bytes(bytes) : 0u);
}
__device__ __forceinline__ float col_ldf(gemm::rsrc_t r, bool ok, int64_t idx) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, ok ? (unsigned)idx * 4u : gemm::kOOB, 0, 0));
}
__device__ __forceinline__ int col_ldi(gemm::rsrc_t r, bool ok, int64_t idx) {
    return (int)__builtin_amdgcn_raw_buffer_load_b32(r, ok ? (unsigned)idx * 4u : gemm::kOOB, 0, 0);
}
// W0 [N, K] (nn.Linear layout) -> the two operands of the row kernel, both in the tile kernels' fragment-major order
// [column tile][chunk][hi | lo][lg][li][8 halfs] (mega16::split_weights_wave) and both from ONE power-of-two scale per row n:
//   fwd: column index n, reduction index k — the operand of Z . W0^T;       inv_scale[n] = 1 / s_n
//   bwd: column index k, reduction index n — the operand of dl/dA1 . W0, holding the SAME halves W0[n][k] s_n: the scale belongs to
//        the reduction index there, so the row kernel folds 1 / s_n into the columns of dl/dA1 before it splits them (exact).
// One workgroup per 32 rows n (= one reduction chunk of `bwd`, two column tiles of `fwd`): row maxima by the waves (coalesced),
// then every thread converts 8 consecutive k of a row (fwd) / 8 consecutive n of a column (bwd: lanes along k, coalesced) into one
// 16-byte store each.  (split_weights_wave with tr = 1 reads a column per wave — 64 cache lines per load instruction: 20 us here.)
// With molecule descriptors W0 is [N, d_h + d_xd]: `fwd` covers every column, `bwd` only the first Kb = d_h (no gradient toward X_d);
// the row scale s_n is the maximum over the whole row in both.
struct HeadSplit { const float* W; int N, K; unsigned char* fwd; unsigned char* bwd; float* inv_scale; int ncf, ncb, Kb; };
__device__ __forceinline__ void head_split_block(const HeadSplit& a, int blk) {
    __shared__ float sc[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;   // 1024 threads
    const int n0 = blk * 32;
    const gemm::rsrc_t rW = gemm::make_rsrc(a.W, (unsigned)(a.N * a.K * 4));
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int n = n0 + 2 * wave + rr;
        float mx = 0.f;
#pragma unroll
        for (int u = 0; u < kRowsMaxK / 64; ++u) {   // (buffer loads: out of range reads 0 — no branch, all in flight together)
            const int k = lane + 64 * u;
            mx = fmaxf(mx, fabsf(col_ldf(rW, n < a.N && k < a.K, (int64_t)n * a.K + k)));
        }
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        const float sn = n < a.N ? mega16::scale_for(mx) : 0.f;
        if (lane == 0) {
            sc[2 * wave + rr] = sn;
            if (n < a.N) a.inv_scale[n] = 1.f / sn;
        }
    }
    __syncthreads();
    auto put = [&](unsigned char* base, int T, int nc, int c, int lg, int li, const float (&x)[8]) {
        h8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) { hi[j] = (_Float16)x[j]; lo[j] = (_Float16)(x[j] - (float)hi[j]); }
        _Float16* o = reinterpret_cast<_Float16*>(base) + (((int64_t)T * nc + c) * 2) * 512 + (lg * 16 + li) * 8;
        *reinterpret_cast<h8*>(o) = hi;
        *reinterpret_cast<h8*>(o + 512) = lo;
    };
    const int nk8 = a.ncf * 4, last_tile = (a.N - 1) >> 4;
    for (int it = tid; it < 32 * nk8; it += 1024) {
        const int nl = it / nk8, k8 = it - nl * nk8, n = n0 + nl, k = 8 * k8;
        if ((n >> 4) > last_tile) continue;   // (rows past N inside the last 16-row tile are written as zeros; tiles past it do not exist)
        const float sn = sc[nl];
        const bool l0 = n < a.N && k < a.K, l1 = n < a.N && k + 4 < a.K;   // (K % 4 == 0)
        const float4 v0 = gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(rW, l0 ? (unsigned)(n * a.K + k) * 4u : gemm::kOOB, 0, 0));
        const float4 v1 = gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(rW, l1 ? (unsigned)(n * a.K + k + 4) * 4u : gemm::kOOB, 0, 0));
        const float x[8] = {v0.x * sn, v0.y * sn, v0.z * sn, v0.w * sn, v1.x * sn, v1.y * sn, v1.z * sn, v1.w * sn};
        put(a.fwd, n >> 4, a.ncf, k8 >> 2, k8 & 3, n & 15, x);
    }
    const int Kp = (a.Kb + 15) & ~15;
    for (int it = tid; it < Kp * 4; it += 1024) {
        const int lg = it / Kp, k = it - lg * Kp;
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = n0 + 8 * lg + j;
            x[j] = col_ldf(rW, n < a.N && k < a.Kb, (int64_t)n * a.K + k) * sc[8 * lg + j];
        }
        put(a.bwd, k >> 4, a.ncb, blk, lg, k & 15, x);
    }
}

// The descriptor columns of the fingerprint Z [B, ldz] = cat(bn(H), X_d, zeros): columns [c0, c0 + w) of every row, X_d [B, nx]
// (row stride ldx, any alignment) and zeros up to the padded width.  A workgroup takes `per` consecutive elements of the B x w block.
struct XdFill { const float* X; int64_t ldx; float* Z; int64_t ldz; int64_t B; int c0, w, nx; int64_t per; };
__device__ __forceinline__ void xd_fill_block(const XdFill& a, int blk) {
    const int64_t e0 = (int64_t)blk * a.per, n = a.B * a.w;
    const int64_t e1 = e0 + a.per < n ? e0 + a.per : n;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int64_t r = e / a.w; const int c = (int)(e - r * a.w);
        a.Z[r * a.ldz + a.c0 + c] = c < a.nx ? a.X[r * a.ldx + c] : 0.f;
    }
}
// the chain form's copy (the four-launch form's rides in k_agg_bn_fwd)
__global__ __launch_bounds__(1024) void k_xd_fill(XdFill a) { xd_fill_block(a, (int)blockIdx.x); }
inline int xd_fill_blocks(const XdFill& a) { return (int)((a.B * a.w + a.per - 1) / a.per); }

struct AggBnArgs {
    BnArgs b;                              // X = H [B, d] (written here), Y = Z (BN only)
    const float* Hv; int64_t ldhv; int64_t nV; const int* bounds; int agg_mode; float agg_norm;
    int use_done;                          // 1: bounds[2 B + 4 + m] != 0 — X already holds molecule m's aggregate (the forward tile kernel wrote it)
    int n_col_blocks;                      // workgroups [0, n_col_blocks): columns; then n_split_blocks: the weight split (32 rows of W0
    int n_split_blocks;                    // each); the rest: the descriptor columns of Z (xd)
    HeadSplit split;
    XdFill xd;
    long long* dbg;                        // optional cycle stamps: [0..5] column workgroup 1, [6..9] the first split workgroup
    int dh_c; int64_t nBt;                 // a multicomponent fingerprint: column c of X / Y is column c % dh_c of component c / dh_c, whose
                                           // molecule r is c / dh_c B + r of the bounds table (nBt molecules); one block: dh_c = d, nBt = B
    const int64_t* batch;                  // k_agg_bn_fwd_own_bounds: the batch vector [nV] the workgroups take the molecules' bounds from
};
// Geometry of the two column kernels: a workgroup = QPW column QUADS (16-byte loads and stores: a quarter of the memory instructions
// of a thread-per-column layout, whose 1 500 four-segment wave loads per CU cost the aggregation 11 us) x 1024 / QPW row lanes; thread
// (tq = tid % QPW, ty = tid / QPW) holds RR molecules (B <= RR 1024 / QPW) of its quad in registers.  QPW shrinks as the batch grows:
// a CU moves ~55 GB/s, and what these kernels move is H_v (aggregation) / dl/dH_v (broadcast) — 5.5 MB at 512 molecules, so the
// columns are spread over 38 workgroups there (2 quads each) where 64 molecules do with 19 (4 quads).
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// sums over the row lanes of every column: the row lanes of a wave by shuffles, the 16 waves through LDS
template <int QPW>
__device__ __forceinline__ float4 quad_col_sum(float4 (*red)[4], int tq, float4 v) {
#pragma unroll
    for (int off = QPW; off < 64; off <<= 1) {
        v.x += __shfl_xor(v.x, off); v.y += __shfl_xor(v.y, off); v.z += __shfl_xor(v.z, off); v.w += __shfl_xor(v.w, off);
    }
    __syncthreads();   // (the previous use of `red` is over)
    if ((threadIdx.x & 63) < QPW) red[threadIdx.x >> 6][tq] = v;
    __syncthreads();
    float4 s = red[0][tq];
#pragma unroll 4
    for (int w = 1; w < 16; ++w) s = f4_add(s, red[w][tq]);
    return s;
}
// two sums at once (batch norm backward: sum gY and sum gY xhat): one pair of barriers
template <int QPW>
__device__ __forceinline__ void quad_col_sum2(float4 (*red)[2][4], int tq, float4& u, float4& v) {
#pragma unroll
    for (int off = QPW; off < 64; off <<= 1) {
        u.x += __shfl_xor(u.x, off); u.y += __shfl_xor(u.y, off); u.z += __shfl_xor(u.z, off); u.w += __shfl_xor(u.w, off);
        v.x += __shfl_xor(v.x, off); v.y += __shfl_xor(v.y, off); v.z += __shfl_xor(v.z, off); v.w += __shfl_xor(v.w, off);
    }
    if ((threadIdx.x & 63) < QPW) { red[threadIdx.x >> 6][0][tq] = u; red[threadIdx.x >> 6][1][tq] = v; }
    __syncthreads();
    u = red[0][0][tq]; v = red[0][1][tq];
#pragma unroll 4
    for (int w = 1; w < 16; ++w) { u = f4_add(u, red[w][0][tq]); v = f4_add(v, red[w][1][tq]); }
}
// OWN (k_agg_bn_fwd_own_bounds, the inference head): no bounds table in memory — every column workgroup takes the molecules' atom
// ranges and the validity flag from the batch vector itself, into LDS (k_mol_bounds_one's pass: nV x 8 bytes per workgroup, beside
// the nV x 16 bytes per quad of H_v it is about to read; cheaper than the launch it replaces); nBt <= kOwnBoundsMols.
constexpr int64_t kOwnBoundsMols = 2048;
template <int QPW, int RR, bool BN, bool OWN>
__device__ __forceinline__ void agg_bn_fwd_body(const AggBnArgs& q) {
    constexpr int kQLanes = 1024 / QPW;
    if ((int)blockIdx.x >= q.n_col_blocks) {   // (uniform per workgroup)
        if ((int)blockIdx.x >= q.n_col_blocks + q.n_split_blocks) {
            xd_fill_block(q.xd, (int)blockIdx.x - q.n_col_blocks - q.n_split_blocks);
            return;
        }
        const bool st = q.dbg && (int)blockIdx.x == q.n_col_blocks && threadIdx.x == 0;
        if (st) q.dbg[6] = (long long)__builtin_readcyclecounter();
        head_split_block(q.split, (int)blockIdx.x - q.n_col_blocks);
        if (st) q.dbg[7] = (long long)__builtin_readcyclecounter();
        return;
    }
    int n_stamp = 0;
    auto stamp = [&]() {
        if (q.dbg && blockIdx.x == 1 && threadIdx.x == 0 && n_stamp < 6) q.dbg[n_stamp] = (long long)__builtin_readcyclecounter();
        ++n_stamp;
    };
    stamp();  // 0 entry
    __shared__ float4 red[16][4];
    const BnArgs& a = q.b;
    const int tq = threadIdx.x % QPW, ty = threadIdx.x / QPW;
    const int c = (blockIdx.x * QPW + tq) * 4;
    const bool ok = c < a.d;   // (d % 4 == 0: a quad is inside or outside)
    // (the component of this quad — dh_c % 4 == 0: a quad never straddles two — its column in H_v and its first molecule in the table)
    const int comp = ok ? c / q.dh_c : 0;
    const int cv = c - comp * q.dh_c;
    const int64_t mo = (int64_t)comp * a.B, nBt = q.nBt;
    __shared__ int own_tb[OWN ? 2 * kOwnBoundsMols + 1 : 1];   // first[nBt] | end[nBt] | flag
    int flag;
    int v0[RR], nv[RR], dn[RR];
    if constexpr (OWN) {
        for (int i = threadIdx.x; i < 2 * (int)nBt + 1; i += 1024) own_tb[i] = 0;
        __syncthreads();
        int bad = 0;
        for (int64_t v = threadIdx.x; v < q.nV; v += 1024) {   // (k_mol_bounds_one's pass and rules)
            const int64_t b = q.batch[v];
            const int64_t prev = v > 0 ? q.batch[v - 1] : -1;
            const int64_t next = v + 1 < q.nV ? q.batch[v + 1] : nBt;
            if (b < 0 || b >= nBt) { bad |= 1; continue; }
            if (b < prev) bad |= 2;
            if (b != prev) own_tb[b] = (int)v;
            if (b != next) own_tb[nBt + b] = (int)(v + 1);
        }
        if (bad) atomicOr(&own_tb[2 * nBt], bad);
        __syncthreads();
        flag = own_tb[2 * nBt];
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const int64_t r = ty + (int64_t)kQLanes * i;
            v0[i] = r < a.B ? own_tb[mo + r] : 0;
            nv[i] = r < a.B ? own_tb[nBt + mo + r] : 0;
            dn[i] = 0;
        }
    } else {
        const gemm::rsrc_t rBd = gemm::make_rsrc(q.bounds, (unsigned)((3 * nBt + 4) * 4));
        flag = col_ldi(rBd, true, 2 * nBt);
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const int64_t r = ty + (int64_t)kQLanes * i;
            v0[i] = col_ldi(rBd, r < a.B, mo + r);
            nv[i] = col_ldi(rBd, r < a.B, nBt + mo + r);
            dn[i] = col_ldi(rBd, q.use_done && r < a.B, 2 * nBt + 4 + mo + r);
        }
    }
    // (batch norm's per-column constants: requested now, used behind the statistics)
    auto ldq = [&](const float* p) {
        return gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(col_buf(p, (int64_t)a.d * 4, q.bounds), ok ? (unsigned)c * 4u : gemm::kOOB, 0, 0));
    };
    const float4 gam0 = ldq(a.gamma), bet0 = ldq(a.beta), rm0 = ldq(a.run_mean), rv0 = ldq(a.run_var);
    stamp();  // 1 requests out
    int nmax = 0;
#pragma unroll
    for (int i = 0; i < RR; ++i) {
        nv[i] -= v0[i];
        if (nv[i] < 0 || !ok || dn[i]) nv[i] = 0;
        nmax = nv[i] > nmax ? nv[i] : nmax;
    }
    stamp();  // 2 bounds here
    // segment sums: AT atoms of every one of the thread's molecules per round — AT RR independent 16-byte loads in flight (a molecule's
    // rows are still added in increasing atom order: the reference's scatter order)
    constexpr int AT = 16 / RR;
    const gemm::rsrc_t rH = gemm::make_rsrc(q.Hv, gemm::clamp_bytes(((int64_t)q.nV * q.ldhv) * 4));
    float4 xs[RR];
#pragma unroll
    for (int i = 0; i < RR; ++i) xs[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const gemm::rsrc_t rX = gemm::make_rsrc(a.X, gemm::clamp_bytes(a.B * a.ldx * 4));
    if (!q.Hv) {   // (uniform) the aggregate is given (dmpnn_molagg_fwd ran in front: batches whose H_v 19 CUs cannot pull fast enough)
        if constexpr (!BN) return;
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const int64_t r = ty + (int64_t)kQLanes * i;
            xs[i] = gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(rX, (ok && r < a.B) ? (unsigned)(r * a.ldx + c) * 4u : gemm::kOOB, 0, 0));
        }
        nmax = 0;
    } else if (q.use_done) {   // (uniform) ... or given for the molecules the forward tile kernel carried (done): the others are summed below
        float4 hx[RR];
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const int64_t r = ty + (int64_t)kQLanes * i;
            hx[i] = gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(rX, (ok && r < a.B && dn[i]) ? (unsigned)(r * a.ldx + c) * 4u : gemm::kOOB, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < RR; ++i) xs[i] = hx[i];
    }
    for (int s0 = 0; s0 < nmax; s0 += AT) {
        float4 tv[AT][RR];
#pragma unroll
        for (int u = 0; u < AT; ++u)
#pragma unroll
            for (int i = 0; i < RR; ++i)
                tv[u][i] = gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(
                    rH, s0 + u < nv[i] ? (unsigned)((int64_t)(v0[i] + s0 + u) * q.ldhv + cv) * 4u : gemm::kOOB, 0, 0));
#pragma unroll
        for (int u = 0; u < AT; ++u)
#pragma unroll
            for (int i = 0; i < RR; ++i)
                if (s0 + u < nv[i]) xs[i] = (s0 + u == 0) ? tv[u][i] : f4_add(xs[i], tv[u][i]);   // include_self=False: the first addend is copied
    }
    const float nanv = __int_as_float(0x7fc00000);
#pragma unroll
    for (int i = 0; i < RR; ++i) {
        const int64_t r = ty + (int64_t)kQLanes * i;
        float4 y = xs[i];
        if (!q.Hv) break;
        if (!dn[i]) {   // (a molecule the tile kernel wrote arrives divided)
            if (q.agg_mode == DMPNN_MOLAGG_MEAN && nv[i] > 0) { const float n = (float)nv[i]; y = make_float4(y.x / n, y.y / n, y.z / n, y.w / n); }
            if (q.agg_mode == DMPNN_MOLAGG_NORM) y = make_float4(y.x / q.agg_norm, y.y / q.agg_norm, y.z / q.agg_norm, y.w / q.agg_norm);
        }
        if (flag) y = make_float4(nanv, nanv, nanv, nanv);
        xs[i] = (ok && r < a.B) ? y : make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && r < a.B && (!dn[i] || flag)) *reinterpret_cast<float4*>(a.X_out() + r * a.ldx + c) = y;
    }
    stamp();  // 3 aggregated
    if constexpr (!BN) return;
    float4 mean, invstd;
    if (a.training) {
        if (a.n_tracked && blockIdx.x == 0 && threadIdx.x == 0) *a.n_tracked += 1;
        float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < RR; ++i) sm = f4_add(sm, xs[i]);
        sm = quad_col_sum<QPW>(red, tq, sm);
        const float fB = (float)a.B;
        mean = make_float4(sm.x / fB, sm.y / fB, sm.z / fB, sm.w / fB);
        float4 qq = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < RR; ++i)
            if (ty + (int64_t)kQLanes * i < a.B) {
                const float4 dl = make_float4(xs[i].x - mean.x, xs[i].y - mean.y, xs[i].z - mean.z, xs[i].w - mean.w);
                qq = f4_add(qq, make_float4(dl.x * dl.x, dl.y * dl.y, dl.z * dl.z, dl.w * dl.w));
            }
        const float4 ss = quad_col_sum<QPW>(red, tq, qq);
        const float4 var = make_float4(ss.x / fB, ss.y / fB, ss.z / fB, ss.w / fB);   // biased: what normalises (nn.BatchNorm1d)
        invstd = make_float4(1.f / sqrtf(var.x + a.eps), 1.f / sqrtf(var.y + a.eps), 1.f / sqrtf(var.z + a.eps), 1.f / sqrtf(var.w + a.eps));
        if (ok && ty == 0) {
            *reinterpret_cast<float4*>(a.save_mean + c) = mean;
            *reinterpret_cast<float4*>(a.save_invstd + c) = invstd;
            const float m = a.momentum, om = 1.f - a.momentum, fB1 = (float)(a.B - 1);
            if (a.run_mean) *reinterpret_cast<float4*>(a.run_mean + c) = make_float4(om * rm0.x + m * mean.x, om * rm0.y + m * mean.y, om * rm0.z + m * mean.z, om * rm0.w + m * mean.w);
            // running_var takes the UNBIASED estimate (torch: var * B / (B - 1))
            const float4 ub = a.B > 1 ? make_float4(ss.x / fB1, ss.y / fB1, ss.z / fB1, ss.w / fB1) : var;
            if (a.run_var) *reinterpret_cast<float4*>(a.run_var + c) = make_float4(om * rv0.x + m * ub.x, om * rv0.y + m * ub.y, om * rv0.z + m * ub.z, om * rv0.w + m * ub.w);
        }
    } else {
        mean = rm0;
        invstd = make_float4(1.f / sqrtf(rv0.x + a.eps), 1.f / sqrtf(rv0.y + a.eps), 1.f / sqrtf(rv0.z + a.eps), 1.f / sqrtf(rv0.w + a.eps));
    }
    stamp();  // 4 statistics
    if (ok) {
        const float4 g = a.gamma ? gam0 : make_float4(1.f, 1.f, 1.f, 1.f), bb = a.beta ? bet0 : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const int64_t r = ty + (int64_t)kQLanes * i;
            if (r < a.B)
                *reinterpret_cast<float4*>(a.Y + r * a.ldy + c) = make_float4((xs[i].x - mean.x) * invstd.x * g.x + bb.x, (xs[i].y - mean.y) * invstd.y * g.y + bb.y,
                                                                              (xs[i].z - mean.z) * invstd.z * g.z + bb.z, (xs[i].w - mean.w) * invstd.w * g.w + bb.w);
        }
    }
    stamp();  // 5 end
}
template <int QPW, int RR, bool BN>
__global__ __launch_bounds__(1024) void k_agg_bn_fwd(AggBnArgs q) { agg_bn_fwd_body<QPW, RR, BN, false>(q); }
template <int QPW, int RR, bool BN>
__global__ __launch_bounds__(1024) void k_agg_bn_fwd_own_bounds(AggBnArgs q) { agg_bn_fwd_body<QPW, RR, BN, true>(q); }

struct BnAggBwdArgs {
    BnBwdArgs b;                           // gY = dl/dZ [B, d], X = H; gX unused (the rows go to the atoms)
    float* gHv; int64_t ldg; const int* bounds; int64_t nV; int agg_mode; float agg_norm;
    // the row kernel's partials (or part == NULL): out[i] = sum over workgroups of part[w * part_stride + i]
    const float* part; int n_part, part_stride, tN, t;
    float* gW1; float* gb1; float* loss_out;
    long long* dbg;                        // optional cycle stamps of column workgroup 1
    int dh_c; int64_t nBt;                 // the multicomponent map of AggBnArgs (one block: dh_c = d, nBt = B)
};
template <int QPW, int RR, bool BN>
__global__ __launch_bounds__(1024) void k_bn_agg_bwd(BnAggBwdArgs q) {
    constexpr int kQLanes = 1024 / QPW;
    __shared__ float4 red[16][2][4];
    if ((int)blockIdx.x * 4 * QPW >= q.b.d) {   // the workgroup behind the columns': what sums over the rows of the batch, in workgroup order
        if (!q.part) return;
        // four threads per output, each over a quarter of the row blocks in order, joined as ((q0 + q1) + (q2 + q3)): a fixed tree
        const int n_out = q.tN + q.t, sub = threadIdx.x & 3, per = (q.n_part + 3) / 4;
        for (int i0 = 0; i0 <= n_out; i0 += 256) {
            const int i = i0 + (threadIdx.x >> 2);
            const gemm::rsrc_t rP = gemm::make_rsrc(q.part, gemm::clamp_bytes((int64_t)q.n_part * q.part_stride * 4));
            float v[16];   // (n_part <= kRowsMaxB / 16 = 64 row blocks)
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int w = sub * per + u;
                v[u] = col_ldf(rP, i <= n_out && u < per && w < q.n_part, (int64_t)w * q.part_stride + i);
            }
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u) s += v[u];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            if (sub != 0 || i > n_out) continue;
            if (i < q.tN) { if (q.gW1) q.gW1[i] = s; }
            else if (i < n_out) { if (q.gb1) q.gb1[i - q.tN] = s; }
            else {   // the loss: sum / count (no finite target: 0 / 0 = NaN, like the reference)
                const float cnt = q.part[n_out + 1];
                q.loss_out[0] = s / cnt;
                q.loss_out[1] = cnt;
            }
        }
        return;
    }
    const BnBwdArgs& a = q.b;
    const int tq = threadIdx.x % QPW, ty = threadIdx.x / QPW;
    const int c = (blockIdx.x * QPW + tq) * 4;
    const bool ok = c < a.d;
    const int comp = ok ? c / q.dh_c : 0;
    const int cv = c - comp * q.dh_c;   // (this quad's column in H_v's rows)
    const int64_t mo = (int64_t)comp * a.B, nBt = q.nBt;
    int n_stamp = 0;
    auto stamp = [&]() {
        if (q.dbg && blockIdx.x == 1 && threadIdx.x == 0 && n_stamp < 6) q.dbg[n_stamp] = (long long)__builtin_readcyclecounter();
        ++n_stamp;
    };
    stamp();  // 0 entry
    // every request of the kernel first (buffer loads: no branch, no wait in between)
    float4 gs[RR], xr[RR];
    int v0[RR], v1[RR];
    const gemm::rsrc_t rBd = gemm::make_rsrc(q.bounds, (unsigned)((3 * nBt + 4) * 4));
    const gemm::rsrc_t rG = gemm::make_rsrc(a.gY, gemm::clamp_bytes(a.B * a.ldgy * 4)), rX = gemm::make_rsrc(a.X, gemm::clamp_bytes(a.B * a.ldx * 4));
#pragma unroll
    for (int i = 0; i < RR; ++i) {
        const int64_t r = ty + (int64_t)kQLanes * i;
        const bool in = ok && r < a.B;
        gs[i] = gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(rG, in ? (unsigned)(r * a.ldgy + c) * 4u : gemm::kOOB, 0, 0));
        xr[i] = BN ? gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(rX, in ? (unsigned)(r * a.ldx + c) * 4u : gemm::kOOB, 0, 0)) : make_float4(0.f, 0.f, 0.f, 0.f);
        v0[i] = col_ldi(rBd, r < a.B, mo + r);
        v1[i] = col_ldi(rBd, r < a.B, nBt + mo + r);
    }
    const int flag = col_ldi(rBd, true, 2 * nBt);
    auto ldq = [&](const float* p) {
        return gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(col_buf(p, (int64_t)a.d * 4, q.bounds), (BN && ok) ? (unsigned)c * 4u : gemm::kOOB, 0, 0));
    };
    const float4 mean = ldq(a.training ? a.save_mean : a.run_mean), is0 = ldq(a.training ? a.save_invstd : a.run_var), gam0 = ldq(a.gamma);
    stamp();  // 1 requests out
    if constexpr (BN) {
        const float4 invstd = a.training ? is0 : make_float4(1.f / sqrtf(is0.x + a.eps), 1.f / sqrtf(is0.y + a.eps), 1.f / sqrtf(is0.z + a.eps), 1.f / sqrtf(is0.w + a.eps));
        float4 xh[RR], s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            const bool in = ok && ty + (int64_t)kQLanes * i < a.B;
            xh[i] = in ? make_float4((xr[i].x - mean.x) * invstd.x, (xr[i].y - mean.y) * invstd.y, (xr[i].z - mean.z) * invstd.z, (xr[i].w - mean.w) * invstd.w)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
            s1 = f4_add(s1, gs[i]);
            s2 = f4_add(s2, make_float4(gs[i].x * xh[i].x, gs[i].y * xh[i].y, gs[i].z * xh[i].z, gs[i].w * xh[i].w));
        }
        stamp();  // 2 data here
        quad_col_sum2<QPW>(red, tq, s1, s2);
        stamp();  // 3 column sums
        if (ok && ty == 0) {
            if (a.g_gamma) *reinterpret_cast<float4*>(a.g_gamma + c) = s2;
            if (a.g_beta) *reinterpret_cast<float4*>(a.g_beta + c) = s1;
        }
        const float4 gam = a.gamma ? gam0 : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 k = make_float4(gam.x * invstd.x, gam.y * invstd.y, gam.z * invstd.z, gam.w * invstd.w);
        const float invB = 1.f / (float)a.B;
#pragma unroll
        for (int i = 0; i < RR; ++i)
            gs[i] = a.training ? make_float4(k.x * (gs[i].x - invB * s1.x - xh[i].x * invB * s2.x), k.y * (gs[i].y - invB * s1.y - xh[i].y * invB * s2.y),
                                             k.z * (gs[i].z - invB * s1.z - xh[i].z * invB * s2.z), k.w * (gs[i].w - invB * s1.w - xh[i].w * invB * s2.w))
                               : make_float4(k.x * gs[i].x, k.y * gs[i].y, k.z * gs[i].z, k.w * gs[i].w);
    }
    if (!ok) return;
    const float nanv = __int_as_float(0x7fc00000);
    if (flag) {   // an invalid `batch`: every row NaN (atoms outside every molecule's range included)
        for (int64_t v = ty; v < q.nV; v += kQLanes) *reinterpret_cast<float4*>(q.gHv + v * q.ldg + cv) = make_float4(nanv, nanv, nanv, nanv);
        return;
    }
#pragma unroll
    for (int i = 0; i < RR; ++i) {
        const int64_t r = ty + (int64_t)kQLanes * i;
        if (r >= a.B) continue;
        float4 g = gs[i];
        if (q.agg_mode == DMPNN_MOLAGG_MEAN) { const float n = (float)(v1[i] - v0[i]); g = make_float4(g.x / n, g.y / n, g.z / n, g.w / n); }
        if (q.agg_mode == DMPNN_MOLAGG_NORM) g = make_float4(g.x / q.agg_norm, g.y / q.agg_norm, g.z / q.agg_norm, g.w / q.agg_norm);
        for (int v = v0[i]; v < v1[i]; ++v) *reinterpret_cast<float4*>(q.gHv + (int64_t)v * q.ldg + cv) = g;
    }
    stamp();  // 4 (2 without batch norm) rows issued
}

struct RowsArgs {
    const float* Z; int64_t ldz;           // [B, K] the predictor's input
    SplitW W0f, W0b;                       // W0 [N, K] as N rows over K (forward) and as K rows over N (data gradient; see HeadSplit)
    const float* b0; const float* W1; const float* b1;   // [N] | NULL, [t, N], [t] | NULL
    float* A1;                             // [B, N] the hidden layer's output tau(Z W0^T + b0): written by PH 1, read by PH 2
    float* preds;                          // [B, t]
    const float* T; const float* w; const float* tw; const unsigned char* lt; const unsigned char* gt; int kind;
    float* gA1; float* gZ;                 // [B, N], [B, Kg]
    float* part; int part_stride;          // per row block: gW1 [t][N] | gb1 [t] | loss sum | number of finite targets
    int64_t B; int N, K, t, act; float slope;
    long long* dbg;                        // optional cycle stamps of workgroup (1, 1)
    int Kg;                                // columns of dl/dZ formed: K, or d_h with molecule descriptors (Z's first d_h columns)
    FfnDrop drop;                          // the predictor's dropout on A1 (the output layer's input)
};
// The predictor + criterion + their backward as TWO launches over (row block of 16 molecules) x (slice of 64 columns):
//   PH 1  A1[:, slice] = tau(Z W0^T + b0)                                                          160 workgroups at 512 x 300
//   PH 2  everything that is local to a row, redone by each of the row block's slices from the whole rows of A1 (16 x N values:
//         cheaper than a launch): P = A1 W1^T + b1, the criterion (every workgroup counts the finite targets of the WHOLE batch
//         itself), dl/dP, dl/dA1 — then ITS slice of dl/dZ = dl/dA1 . W0, of dl/dA1 (for the hidden layer's weight gradient) and
//         of the row block's partial of gW1; slice 0 also writes the predictions and the partials of gb1 and of the loss.
// Both contractions on the f16 pipe (3-product split, fp32 accumulation: the block's arithmetic), the weight fragments of a wave's 16
// columns requested in one go at kernel entry.  (ONE launch per row block holding whole rows was built first: 27-33 us — a CU pulls
// its 820 KB of weight fragments at ~55 GB/s, profiles/r05_head_rowblock_stamps.txt; sliced, a workgroup needs 82 KB per contraction.)
template <int WNT, int PH>
__global__ __launch_bounds__(256) void k_head_rows(RowsArgs a) {
    constexpr int BN = 64 * WNT, NCH = BN / 32, TS = NCH * 128 + 16, LDA = BN + 4;
    __shared__ __attribute__((aligned(16))) unsigned char As[16 * TS];   // split operand tile: the rows of Z (PH 1) / of dl/dA1 (PH 2)
    __shared__ __attribute__((aligned(16))) float A1s[PH == 2 ? 16 * LDA : 4];   // fp32 tile: A1, later dl/dA1
    __shared__ float inv_s[16];                                          // 1 / scale of the split tile's rows
    __shared__ float Ps[16][kOutMaxTasks];
    __shared__ __attribute__((aligned(16))) float gPs[16][kOutMaxTasks];
    __shared__ float W1s[kOutMaxTasks][PH == 2 ? BN : 1];                // W1 [t, N], zero beyond
    __shared__ float red2[2][4];
    __shared__ float tot[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    const int cs = blockIdx.y;                  // column slice; wave w owns the 16 columns of tile T
    const int T = cs * 4 + wave, col = T * 16 + li;
    const int nrows = (int)(a.B - row0 < 16 ? a.B - row0 : 16);
    const int t = a.t;
    int n_stamp = 0;
    auto stamp = [&]() {
        if (a.dbg && blockIdx.x == 1 && blockIdx.y == 1 && threadIdx.x == 0 && n_stamp < 8) a.dbg[n_stamp] = (long long)__builtin_readcyclecounter();
        ++n_stamp;
    };
    stamp();  // 0 entry
    // (buffer loads: an offset out of range reads 0 without a branch or a select on the data — nothing in the request section consumes a
    //  loaded value, so every request is out before the first wait; a NULL array is a zero-length buffer)
    auto buf = [&](const void* ptr, int64_t bytes) { return gemm::make_rsrc(ptr ? ptr : a.Z, ptr ? (unsigned)bytes : 0u); };
    auto ldf = [&](gemm::rsrc_t r, bool ok, int64_t idx) {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, ok ? (unsigned)idx * 4u : gemm::kOOB, 0, 0));
    };
    // rows of an fp32 [B, width] tensor: thread (row i = tid >> 4, p = tid & 15) takes columns 4 p + 64 j
    auto load_rows = [&](const float* X, int64_t ld, int width, float4 (&x)[WNT]) {
        const int i = tid >> 4, p = tid & 15;
        const gemm::rsrc_t rX = gemm::make_rsrc(X + row0 * ld, (unsigned)(nrows * ld * 4));
#pragma unroll
        for (int j = 0; j < WNT; ++j) {
            const int c4 = 4 * p + 64 * j;
            x[j] = gemm::as_f4(__builtin_amdgcn_raw_buffer_load_b128(rX, (i < nrows && c4 < width) ? (unsigned)(i * ld + c4) * 4u : gemm::kOOB, 0, 0));
        }
    };
    // fp32 rows -> split tile (the row's maximum by four shuffles)
    auto split_rows = [&](const float4 (&x)[WNT]) {
        const int i = tid >> 4, p = tid & 15;
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < WNT; ++j)
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(x[j].x), fabsf(x[j].y))), fmaxf(fabsf(x[j].z), fabsf(x[j].w)));
        for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        const float sr = mega16::scale_for(mx);
        if (p == 0) inv_s[i] = 1.f / sr;
#pragma unroll
        for (int j = 0; j < WNT; ++j) {
            const int c4 = 4 * p + 64 * j;
            h4 hi, lo;
            mega16::split4(x[j], sr, hi, lo);
            unsigned char* d = As + i * TS + (c4 >> 5) * 128 + (c4 & 31) * 2;
            *reinterpret_cast<h4*>(d) = hi;
            *reinterpret_cast<h4*>(d + 64) = lo;
        }
    };
    // the wave's weight fragments: every chunk of column tile T (chunks beyond W.nc and tiles beyond n_out: out of range, 0)
    h8 wh[NCH], wl[NCH];
    auto request = [&](const SplitW& W, int n_out) {
        const gemm::rsrc_t rW = gemm::make_rsrc(W.p, (unsigned)(((n_out + 15) / 16) * W.nc * 2048));
        const unsigned o0 = (unsigned)T * (unsigned)(W.nc * 2048) + (unsigned)lane * 16u;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const unsigned o = (c < W.nc && T * 16 < n_out) ? o0 + (unsigned)c * 2048u : gemm::kOOB;
            wh[c] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(rW, o, 0, 0));
            wl[c] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(rW, o == gemm::kOOB ? o : o + 1024u, 0, 0));
        }
    };
    auto contract = [&]() {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();   // the split tile (and inv_s) is complete
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const unsigned char* pa = As + li * TS + c * 128 + lg * 16;
            const h8 ah = *reinterpret_cast<const h8*>(pa), al = *reinterpret_cast<const h8*>(pa + 64);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wh[c], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wl[c], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wh[c], acc, 0, 0, 0);
        }
        return acc;
    };

    if constexpr (PH == 1) {
        float4 zx[WNT];
        load_rows(a.Z, a.ldz, a.K, zx);
        const float isw = ldf(gemm::make_rsrc(a.W0f.inv_scale, (unsigned)(a.N * 4)), col < a.N, col);
        const float bv = ldf(buf(a.b0, a.N * 4), col < a.N, col);
        request(a.W0f, a.N);
        __builtin_amdgcn_sched_barrier(0);   // (requests above, consumers below)
        stamp();  // 1 requests out
        split_rows(zx);
        const f32x4 acc = contract();
        stamp();  // 2 contraction issued
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * lg + r;
            const float y = apply_act_small(acc[r] * (isw * inv_s[i]) + bv, a.act, a.slope);   // (dropout: A1 = mask tau / (1 - p))
            if (col < a.N && i < nrows) a.A1[(row0 + i) * a.N + col] = a.drop.on ? y * (a.drop.keep(row0 + i, col) ? a.drop.scale : 0.f) : y;
        }
        stamp();  // 3 end
        return;
    } else {
        // ---- requests: the rows of A1, the criterion's inputs (element (row ei, task ej) of this row block on thread tid < 16 t; the
        // targets of the WHOLE batch — B t <= 4 096 values, 16 per thread — for the count of finite ones), W1, 1 / s_n of W0's rows for
        // the thread's columns of dl/dA1 (n = tid, tid + 256), the fragments of the wave's 16 columns of W0 ----
        float4 ax[WNT];
        load_rows(a.A1, a.N, a.N, ax);
        const int ei = tid / t, ej = tid - ei * t;
        const bool elem = tid < 16 * t && ei < nrows;
        const int64_t egi = (row0 + ei) * t + ej;
        const gemm::rsrc_t rT = buf(a.T, a.B * t * 4);
        const float ey = ldf(rT, elem, egi);
        const float ewv = ldf(buf(a.w, a.B * 4), elem, row0 + ei), etv = ldf(buf(a.tw, t * 4), elem, ej);
        const unsigned char elt = __builtin_amdgcn_raw_buffer_load_b8(buf(a.lt, a.B * t), elem ? (unsigned)egi : gemm::kOOB, 0, 0);
        const unsigned char egt = __builtin_amdgcn_raw_buffer_load_b8(buf(a.gt, a.B * t), elem ? (unsigned)egi : gemm::kOOB, 0, 0);
        constexpr int NCNT = (int)(kRowsMaxB * kOutMaxTasks / 256);
        float cv[NCNT];
#pragma unroll
        for (int u = 0; u < NCNT; ++u) cv[u] = ldf(rT, tid + 256 * u < a.B * t, tid + 256 * u);
        constexpr int NW1 = kOutMaxTasks * BN / 256;
        float w1v[NW1];
        const gemm::rsrc_t rW1 = gemm::make_rsrc(a.W1, (unsigned)(t * a.N * 4));
#pragma unroll
        for (int u = 0; u < NW1; ++u) {
            const int idx = tid + 256 * u, j = idx / BN, n = idx - j * BN;
            w1v[u] = ldf(rW1, j < t && n < a.N, j * a.N + n);
        }
        const gemm::rsrc_t rIS = gemm::make_rsrc(a.W0f.inv_scale, (unsigned)(a.N * 4));
        constexpr int NCOL = (BN + 255) / 256;
        float isn[NCOL];
#pragma unroll
        for (int u = 0; u < NCOL; ++u) isn[u] = ldf(rIS, tid + 256 * u < a.N, tid + 256 * u);
        float b1v[kOutMaxTasks];
#pragma unroll
        for (int j = 0; j < kOutMaxTasks; ++j) b1v[j] = ldf(buf(a.b1, t * 4), j < t, j);
        request(a.W0b, a.Kg);
        __builtin_amdgcn_sched_barrier(0);   // (requests above, consumers below)
        stamp();  // 1 requests out
#pragma unroll
        for (int u = 0; u < NW1; ++u) { const int idx = tid + 256 * u; W1s[idx / BN][idx % BN] = w1v[u]; }   // (read by every row of the tile, twice)
        // dl/dP as 16 x 4: columns beyond t must be ZERO (they meet W1's zero rows below) — all of the tile first, the t live columns
        // after the criterion.  (Round 5 zeroed them with the threads 16 t .. 63 only: the columns >= t of the rows below 4 t kept whatever
        // the LDS held — 0 x a finite leftover on a warm box, NaN on a cold one; found in round 6 with DMPNN_DEBUG_LDS_POISON)
        if (tid < 16 * kOutMaxTasks) gPs[tid / kOutMaxTasks][tid % kOutMaxTasks] = 0.f;
#pragma unroll
        for (int j = 0; j < WNT; ++j) *reinterpret_cast<float4*>(A1s + (tid >> 4) * LDA + 4 * (tid & 15) + 64 * j) = ax[j];   // (zero beyond N and beyond the batch)
        __syncthreads();
        stamp();  // 2 A1 in the tile
        // ---- P = A1 W1^T + b1: thread (row i, part p) sums the columns n = p mod 16 ----
        {
            const int i = tid >> 4, p = tid & 15;
            float sp[kOutMaxTasks] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < BN / 16; ++q) {   // (columns beyond N: zeros in both tiles)
                const int n = p + 16 * q;
                const float x = A1s[i * LDA + n];
#pragma unroll
                for (int j = 0; j < kOutMaxTasks; ++j) sp[j] += x * W1s[j][n];
            }
#pragma unroll
            for (int j = 0; j < kOutMaxTasks; ++j) {
                for (int off = 1; off < 16; off <<= 1) sp[j] += __shfl_xor(sp[j], off);
                if (p == 0 && j < t) {
                    const float v = sp[j] + b1v[j];
                    Ps[i][j] = v;
                    if (cs == 0 && i < nrows) a.preds[(row0 + i) * t + j] = v;
                }
            }
        }
        // ---- criterion (k_loss's arithmetic per element): this row block's rows; the count over the whole batch ----
        float sm = 0.f, sl = 0.f;
#pragma unroll
        for (int u = 0; u < NCNT; ++u) sm += (tid + 256 * u < a.B * t && isfinite(cv[u])) ? 1.f : 0.f;
        __syncthreads();   // Ps
        float ef = 0.f, ep = 0.f;
        const bool efin = elem && isfinite(ey);
        if (elem) {
            ep = Ps[ei][ej];
            if ((elt && ep < ey) || (egt && ep > ey)) ep = ey;
            ef = (a.w ? ewv : 1.f) * (a.tw ? etv : 1.f);
            if (efin) sl = loss_value(a.kind, ep, ey) * ef;
        }
        for (int off = 32; off > 0; off >>= 1) { sl += __shfl_xor(sl, off); sm += __shfl_xor(sm, off); }
        if (lane == 0) { red2[0][wave] = sl; red2[1][wave] = sm; }
        __syncthreads();
        if (tid == 0) {
            tot[0] = (red2[0][0] + red2[0][1]) + (red2[0][2] + red2[0][3]);
            tot[1] = (red2[1][0] + red2[1][1]) + (red2[1][2] + red2[1][3]);
            if (cs == 0) {
                float* pp = a.part + (int64_t)blockIdx.x * a.part_stride + t * a.N + t;
                pp[0] = tot[0]; pp[1] = tot[1];
            }
        }
        __syncthreads();
        if (tid < 16 * t) gPs[ei][ej] = efin ? loss_deriv(a.kind, ep, ey) * ef * (1.f / tot[1]) : 0.f;   // (columns beyond t: zeroed above)
        __syncthreads();
        stamp();  // 3 criterion
        // ---- the output layer's backward on this row block: thread = column n of A1 (all of them: the operand of the contraction below) ----
        //   dl/dA1[i][n] = (sum_j gP[i][j] W1[j][n]) tau'(A1[i][n]),  partial gW1[j][n] = sum_i gP[i][j] A1[i][n],  partial gb1[j] = sum_i gP[i][j]
        // (with the predictor's dropout A1 is the masked output and the factor is mask / (1 - p) tau': FfnDrop::act_grad)
        // what leaves for memory is the slice's: columns [64 cs, 64 cs + 64)
        // (the 16 rows of a column in registers, dl/dP as 16-byte rows: straight-line code — a loop with the activation's switch inside
        //  waited for every LDS round trip, 6 us)
        const bool simple_act = !act_is_smooth(a.act);
        const float neg = a.act == DMPNN_ACT_NONE ? 1.f : (a.act == DMPNN_ACT_RELU ? 0.f : a.slope);   // tau' for y <= 0 (ReLU class)
        float4 gp4[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) gp4[i] = *reinterpret_cast<const float4*>(&gPs[i][0]);
#pragma unroll
        for (int u = 0; u < NCOL; ++u) {
            const int n = tid + 256 * u;
            if (n >= BN) break;
            const bool okn = n < a.N, mine = okn && (n >> 6) == cs;
            const float isn_c = isn[u];
            const float4 w1 = make_float4(W1s[0][n], W1s[1][n], W1s[2][n], W1s[3][n]);   // (rows beyond t are zero)
            float xv[16], gv[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) xv[i] = A1s[i * LDA + n];
            float4 gw = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float4 gp = gp4[i];   // (columns beyond t are zero)
                const float g = ((gp.x * w1.x + gp.y * w1.y) + gp.z * w1.z) + gp.w * w1.w;
                gw.x += gp.x * xv[i]; gw.y += gp.y * xv[i]; gw.z += gp.z * xv[i]; gw.w += gp.w * xv[i];
                float dv = simple_act ? (xv[i] > 0.f ? 1.f : neg) : act_grad_from_out(a.drop.on ? xv[i] * a.drop.unscale : xv[i], a.act, a.slope);
                if (a.drop.on) dv *= a.drop.keep(row0 + i, n) ? a.drop.scale : 0.f;
                gv[i] = okn ? g * dv : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                A1s[i * LDA + n] = gv[i] * isn_c;   // (the operand of dl/dA1 . W0 carries W0's row scales on its reduction index: see HeadSplit)
                if (mine && i < nrows) a.gA1[(row0 + i) * a.N + n] = gv[i];
            }
            if (mine) {
                const float gwv[4] = {gw.x, gw.y, gw.z, gw.w};
                for (int j = 0; j < t; ++j) a.part[(int64_t)blockIdx.x * a.part_stride + (int64_t)j * a.N + n] = gwv[j];
            }
        }
        if (cs == 0 && tid < t) {
            float sb = 0.f;
            for (int i = 0; i < 16; ++i) sb += gPs[i][tid];
            a.part[(int64_t)blockIdx.x * a.part_stride + t * a.N + tid] = sb;
        }
        __syncthreads();
        stamp();  // 4 output layer's backward
        // ---- dl/dZ[:, slice] = dl/dA1 . W0 ----
        {
            float4 gx[WNT];
#pragma unroll
            for (int j = 0; j < WNT; ++j) gx[j] = *reinterpret_cast<const float4*>(A1s + (tid >> 4) * LDA + 4 * (tid & 15) + 64 * j);
            split_rows(gx);
        }
        const f32x4 acc = contract();
        stamp();  // 5 contraction issued
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * lg + r;
            if (col < a.Kg && i < nrows) a.gZ[(row0 + i) * a.Kg + col] = acc[r] * inv_s[i];
        }
        stamp();  // 6 end
    }
}

// out[c][r] = in[r][c] for a weight matrix (<= a few hundred KB)
__global__ void k_head_transpose(const float* __restrict__ in, int64_t ldi, float* __restrict__ out, int64_t ldo, int rows, int cols) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = by + j, c = bx + threadIdx.x;
        tile[j][threadIdx.x] = (r < rows && c < cols) ? in[(int64_t)r * ldi + c] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int c = bx + j, r = by + threadIdx.x;
        if (c < cols && r < rows) out[(int64_t)c * ldo + r] = tile[threadIdx.x][j];
    }
}
// g[r][c] *= tau'(Y[r][c])   (Y = the activated output the next layer consumed; with the predictor's dropout Y is masked and the factor
// is FfnDrop::act_grad)
__global__ void k_head_act_bwd(float* __restrict__ g, int64_t ldg, const float* __restrict__ Y, int64_t ldy, int64_t rows, int cols,
                               int act, float slope, FfnDrop drop) {
    const int64_t n = rows * cols;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols; const int c = (int)(i - r * cols);
        const float y = Y[r * ldy + c];
        g[r * ldg + c] *= drop.on ? drop.act_grad(r, c, y, act, slope) : act_grad_from_out(y, act, slope);
    }
}

}  // namespace
}  // namespace dmpnn
