// f1, the fourth aggregation: AttentiveAggregation (chemprop/nn/agg.py:116-133) as two kernels and a small reduce.
//
// Reference: s = exp(W h_v + b); Z = scatter-sum of s; alpha = s / Z[batch]; out = scatter-sum of alpha h_v — a chain of seven
// launches around two [V, d_h] temporaries.  Here, for molecule m with atoms [first[m], end[m]) of the dmpnn_molagg_bounds table:
//
//   k_attn_fwd     one wave per molecule.  Rows up to kAttnNarrowQuads column groups per lane (1 024 columns as 16-byte quads, 256 as
//                  single floats) stay in registers: the row is read ONCE, its logit is a wave reduction, and Z += s, acc += s h_v run in
//                  increasing atom order; out = acc / Z with a true division (plain exp, no max subtraction: the reference's arithmetic up
//                  to where the division sits).  Wider rows take column passes: the logits first (kept in LDS for the first
//                  kAttnStageAtoms atoms of the molecule, recomputed beyond), then one pass per 64 lanes of columns; the second read of
//                  a row comes from L2.  Kept for the backward pass: s [n_atoms] and Z [n_mols], nothing else.
//   k_attn_bwd     one wave per molecule (a wave walks molecules wave, wave + n_waves, ...):  a_v = g_m h_v, c_m = sum alpha_v a_v,
//                  dl_v = alpha_v (a_v - c_m), gH[v] = alpha_v g_m + dl_v w, and the wave's own partial row of gW = sum dl_v h_v | gb.
//                  H is read twice (the second sweep recomputes a_v from the row it holds anyway).
//   k_attn_reduce  the partial rows summed in a fixed order: no floating-point atomics, the same bits on every call.
//
// An invalid batch vector (the table's flag) poisons out / gH / gW / gb with NaN; a molecule without atoms gives a zero row.
#include "dmpnn_common.hpp"

namespace dmpnn {
namespace {

constexpr int kAttnNarrowQuads = 4;    // column groups per lane of a row that stays in registers
constexpr int kAttnStageAtoms = 128;   // atoms of a molecule whose logit term stays in LDS on the column-pass form
constexpr int kAttnMaxWaves = 1024;    // partial rows of the backward pass
constexpr int kAttnUnroll = 4;         // atoms in flight on the register form

struct AttnArgs {
    const float* H; int64_t ldh;
    const int* bounds;
    const float* W; const float* b;
    float* out; int64_t ldo;
    float* keep_s; float* keep_Z;
    const float* gout; int64_t ldgo;
    float* gH; int64_t ldgh;
    float* part; int part_ld; int n_waves;
    int64_t n_atoms, n_mols;
    int d;
    int* id_bounds; int64_t* id_batch;   // the head: a bounds table and a batch vector of n_mols one-atom molecules, written on the side
};

__device__ __forceinline__ float wave_sum(float x) {   // butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

template <int VEC>
__device__ __forceinline__ void ld_cols(const float* __restrict__ p, int c, int d, float* x) {
    if (VEC == 4) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < d) q = *reinterpret_cast<const float4*>(p + c);   // (d % 4 == 0: a quad that starts inside the row ends inside it)
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = c < d ? p[c] : 0.f;
    }
}

template <int VEC>
__device__ __forceinline__ void st_cols(float* __restrict__ p, int c, int d, const float* x) {
    if (c >= d) return;
    if (VEC == 4) *reinterpret_cast<float4*>(p + c) = make_float4(x[0], x[1], x[2], x[3]);
    else p[c] = x[0];
}

// the dot product of row `r` with row `q` over all d columns, in column passes (the same order whenever it is asked again)
template <int VEC>
__device__ __forceinline__ float row_dot(const float* __restrict__ r, const float* __restrict__ q, int d, int lane) {
    float p = 0.f;
    for (int c0 = 0; c0 < d; c0 += 64 * VEC) {
        float x[VEC], y[VEC];
        ld_cols<VEC>(r, c0 + lane * VEC, d, x);
        ld_cols<VEC>(q, c0 + lane * VEC, d, y);
#pragma unroll
        for (int t = 0; t < VEC; ++t) p += x[t] * y[t];
    }
    return wave_sum(p);
}

// NQ > 0: the register form (rows of up to 64 VEC NQ columns); NQ == 0: the column-pass form
template <int VEC, int NQ>
__global__ __launch_bounds__(256) void k_attn_fwd(AttnArgs a) {
    __shared__ float stage[4][kAttnStageAtoms];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t m = blockIdx.x * 4ll + wv;
    if (m >= a.n_mols) return;
    const int d = a.d;
    const int flag = a.bounds[2 * a.n_mols];
    if (a.id_bounds && lane == 0) {
        a.id_bounds[m] = (int)m;
        a.id_bounds[a.n_mols + m] = (int)m + 1;
        a.id_bounds[2 * a.n_mols + 4 + m] = 0;
        if (m == 0) for (int i = 0; i < 4; ++i) a.id_bounds[2 * a.n_mols + i] = 0;
        a.id_batch[m] = m;
    }
    float* out = a.out + m * a.ldo;
    const float nanv = __int_as_float(0x7fc00000);
    if (flag) {
        for (int c = lane; c < d; c += 64) out[c] = nanv;
        if (a.keep_Z && lane == 0) a.keep_Z[m] = nanv;
        return;
    }
    const int v0 = a.bounds[m], v1 = a.bounds[a.n_mols + m];
    const float bias = a.b[0];
    float Z = 0.f;
    if constexpr (NQ > 0) {
        constexpr int Q = NQ * VEC, U = kAttnUnroll;
        float w[Q], acc[Q];
#pragma unroll
        for (int j = 0; j < NQ; ++j) ld_cols<VEC>(a.W, (lane + 64 * j) * VEC, d, w + j * VEC);
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0.f;
        for (int v = v0; v < v1; v += U) {
            float x[U][Q], p[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int vv = v + u < v1 ? v + u : v1 - 1;   // (the tail reads the molecule's last row again: in bounds, not used)
                const float* row = a.H + (int64_t)vv * a.ldh;
#pragma unroll
                for (int j = 0; j < NQ; ++j) ld_cols<VEC>(row, (lane + 64 * j) * VEC, d, x[u] + j * VEC);
                p[u] = 0.f;
#pragma unroll
                for (int q = 0; q < Q; ++q) p[u] += x[u][q] * w[q];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) p[u] = wave_sum(p[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (v + u < v1) {
                    const float s = expf(p[u] + bias);
                    Z += s;
#pragma unroll
                    for (int q = 0; q < Q; ++q) acc[q] += s * x[u][q];
                    if (a.keep_s && lane == 0) a.keep_s[v + u] = s;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            float y[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) y[t] = v1 > v0 ? acc[j * VEC + t] / Z : 0.f;
            st_cols<VEC>(out, (lane + 64 * j) * VEC, d, y);
        }
    } else {
        for (int v = v0; v < v1; ++v) {
            const float s = expf(row_dot<VEC>(a.H + (int64_t)v * a.ldh, a.W, d, lane) + bias);
            Z += s;
            if (v - v0 < kAttnStageAtoms) stage[wv][v - v0] = s;   // (every lane writes the same value, and reads back what it wrote)
            if (a.keep_s && lane == 0) a.keep_s[v] = s;
        }
        for (int c0 = 0; c0 < d; c0 += 64 * VEC) {
            const int c = c0 + lane * VEC;
            float acc[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) acc[t] = 0.f;
            for (int v = v0; v < v1; ++v) {
                const float* row = a.H + (int64_t)v * a.ldh;
                const float s = v - v0 < kAttnStageAtoms ? stage[wv][v - v0] : expf(row_dot<VEC>(row, a.W, d, lane) + bias);
                float x[VEC];
                ld_cols<VEC>(row, c, d, x);
#pragma unroll
                for (int t = 0; t < VEC; ++t) acc[t] += s * x[t];
            }
#pragma unroll
            for (int t = 0; t < VEC; ++t) acc[t] = v1 > v0 ? acc[t] / Z : 0.f;
            st_cols<VEC>(out, c, d, acc);
        }
    }
    if (a.keep_Z && lane == 0) a.keep_Z[m] = Z;
}

template <int VEC, int NQ>
__global__ __launch_bounds__(256) void k_attn_bwd(AttnArgs a) {
    __shared__ float stage[4][kAttnStageAtoms];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wave = blockIdx.x * 4ll + wv;
    const int d = a.d;
    if (a.bounds[2 * a.n_mols]) {   // an invalid batch vector: every row of gH is NaN (the reduce poisons gW / gb)
        const float nanv = __int_as_float(0x7fc00000);
        for (int64_t v = wave; v < a.n_atoms; v += gridDim.x * 4ll)
            for (int c = lane; c < d; c += 64) a.gH[v * a.ldgh + c] = nanv;
        return;
    }
    if (wave >= a.n_waves) return;
    float* part = a.part ? a.part + wave * (int64_t)a.part_ld : nullptr;
    const int dpad = a.part_ld - 4;
    float gb = 0.f;
    if constexpr (NQ > 0) {
        constexpr int Q = NQ * VEC, U = kAttnUnroll;
        float w[Q], gw[Q], g[Q];
#pragma unroll
        for (int j = 0; j < NQ; ++j) ld_cols<VEC>(a.W, (lane + 64 * j) * VEC, d, w + j * VEC);
#pragma unroll
        for (int q = 0; q < Q; ++q) gw[q] = 0.f;
        for (int64_t m = wave; m < a.n_mols; m += a.n_waves) {
            const int v0 = a.bounds[m], v1 = a.bounds[a.n_mols + m];
            if (v1 <= v0) continue;
            const float Z = a.keep_Z[m];
#pragma unroll
            for (int j = 0; j < NQ; ++j) ld_cols<VEC>(a.gout + m * a.ldgo, (lane + 64 * j) * VEC, d, g + j * VEC);
            float cm = 0.f;
            for (int sweep = 0; sweep < 2; ++sweep) {   // 0: c_m;  1: the gradients (a_v again from the row it reads anyway: the same bits)
                for (int v = v0; v < v1; v += U) {
                    float x[U][Q], p[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int vv = v + u < v1 ? v + u : v1 - 1;
                        const float* row = a.H + (int64_t)vv * a.ldh;
#pragma unroll
                        for (int j = 0; j < NQ; ++j) ld_cols<VEC>(row, (lane + 64 * j) * VEC, d, x[u] + j * VEC);
                        p[u] = 0.f;
#pragma unroll
                        for (int q = 0; q < Q; ++q) p[u] += x[u][q] * g[q];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) p[u] = wave_sum(p[u]);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (v + u < v1) {
                            const float al = a.keep_s[v + u] / Z;
                            if (sweep == 0) {
                                cm += al * p[u];
                            } else {
                                const float dl = al * (p[u] - cm);
                                gb += dl;
                                float* grow = a.gH + (int64_t)(v + u) * a.ldgh;
#pragma unroll
                                for (int j = 0; j < NQ; ++j) {
                                    float y[VEC];
#pragma unroll
                                    for (int t = 0; t < VEC; ++t) {
                                        const int q = j * VEC + t;
                                        gw[q] += dl * x[u][q];
                                        y[t] = al * g[q] + dl * w[q];
                                    }
                                    st_cols<VEC>(grow, (lane + 64 * j) * VEC, d, y);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (part) {
#pragma unroll
            for (int j = 0; j < NQ; ++j) st_cols<VEC>(part, (lane + 64 * j) * VEC, d, gw + j * VEC);
        }
    } else {
        if (part) {   // the wave's partial row: every lane owns its columns for the whole launch
            float z[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) z[t] = 0.f;
            for (int c0 = 0; c0 < d; c0 += 64 * VEC) st_cols<VEC>(part, c0 + lane * VEC, d, z);
        }
        for (int64_t m = wave; m < a.n_mols; m += a.n_waves) {
            const int v0 = a.bounds[m], v1 = a.bounds[a.n_mols + m];
            if (v1 <= v0) continue;
            const float Z = a.keep_Z[m];
            const float* grow_m = a.gout + m * a.ldgo;
            float cm = 0.f;
            for (int v = v0; v < v1; ++v) {
                const float av = row_dot<VEC>(a.H + (int64_t)v * a.ldh, grow_m, d, lane);
                if (v - v0 < kAttnStageAtoms) stage[wv][v - v0] = av;
                cm += (a.keep_s[v] / Z) * av;
            }
            for (int c0 = 0; c0 < d; c0 += 64 * VEC) {
                const int c = c0 + lane * VEC;
                float g[VEC], w[VEC], gw[VEC];
                ld_cols<VEC>(grow_m, c, d, g);
                ld_cols<VEC>(a.W, c, d, w);
#pragma unroll
                for (int t = 0; t < VEC; ++t) gw[t] = 0.f;
                if (part) ld_cols<VEC>(part, c, d, gw);
                for (int v = v0; v < v1; ++v) {
                    const float* row = a.H + (int64_t)v * a.ldh;
                    const float av = v - v0 < kAttnStageAtoms ? stage[wv][v - v0] : row_dot<VEC>(row, grow_m, d, lane);
                    const float al = a.keep_s[v] / Z;
                    const float dl = al * (av - cm);
                    if (c0 == 0) gb += dl;
                    float x[VEC], y[VEC];
                    ld_cols<VEC>(row, c, d, x);
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        gw[t] += dl * x[t];
                        y[t] = al * g[t] + dl * w[t];
                    }
                    st_cols<VEC>(a.gH + (int64_t)v * a.ldgh, c, d, y);
                }
                if (part) st_cols<VEC>(part, c, d, gw);
            }
        }
    }
    if (part && lane == 0) part[dpad] = gb;
}

// gW[c] (c < d) and gb (c == d): the partial rows in four contiguous groups, each summed in row order, the four sums added in order
__global__ __launch_bounds__(256) void k_attn_reduce(const float* __restrict__ part, int part_ld, int n_rows, int d, const int* __restrict__ flag,
                                                     float* __restrict__ gW, float* __restrict__ gb) {
    __shared__ float sm[4][64];
    const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int per = (n_rows + 3) / 4;
    const int r0 = grp * per, r1 = r0 + per < n_rows ? r0 + per : n_rows;
    float s = 0.f;
    if (c <= d) {
        const float* p = part + (c < d ? c : part_ld - 4);
        for (int r = r0; r < r1; ++r) s += p[(int64_t)r * part_ld];
    }
    sm[grp][cl] = s;
    __syncthreads();
    if (grp == 0 && c <= d) {
        float t = ((sm[0][cl] + sm[1][cl]) + sm[2][cl]) + sm[3][cl];
        if (flag[0]) t = __int_as_float(0x7fc00000);
        if (c < d) { if (gW) gW[c] = t; }
        else if (gb) gb[0] = t;
    }
}

inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
inline int attn_waves(int64_t n_mols) { return (int)(n_mols < kAttnMaxWaves ? (n_mols > 0 ? n_mols : 0) : kAttnMaxWaves); }
inline int attn_part_ld(int64_t d) { return (int)align4(d) + 4; }
inline size_t attn_table_bytes(const dmpnn_molagg_attn_args& a) { return a.bounds ? 0 : al256(dmpnn_molagg_ws_bytes(a.n_mols)); }

int attn_check(const dmpnn_molagg_attn_args* ap, bool bwd) {
    const char* who = bwd ? "molagg_attn_bwd" : "molagg_attn_fwd";
    DMPNN_CHECK_ARG(ap != nullptr, "%s: null args", who);
    const dmpnn_molagg_attn_args& a = *ap;
    DMPNN_CHECK_ARG(a.n_atoms >= 0 && a.n_mols >= 0 && a.n_atoms < (1ll << 31) && a.n_mols < (1ll << 30), "%s: sizes out of range", who);
    DMPNN_CHECK_ARG(a.d_h >= 1 && a.d_h < (1 << 24), "%s: d_h (%lld) outside 1 .. 2^24", who, (long long)a.d_h);
    DMPNN_CHECK_ARG(a.ldh >= a.d_h, "%s: ldh (%lld) < d_h (%lld)", who, (long long)a.ldh, (long long)a.d_h);
    DMPNN_CHECK_ARG((a.keep_s == nullptr) == (a.keep_Z == nullptr), "%s: keep_s and keep_Z go together", who);
    const bool work = a.n_atoms > 0 && a.n_mols > 0;
    if (!bwd) {
        DMPNN_CHECK_ARG(a.ldo >= a.d_h, "%s: ldo (%lld) < d_h (%lld)", who, (long long)a.ldo, (long long)a.d_h);
        DMPNN_CHECK_ARG(a.n_mols == 0 || (a.out && a.W && a.b && (a.bounds || a.batch || a.n_atoms == 0)), "%s: NULL out / W / b / bounds and batch", who);
        DMPNN_CHECK_ARG(a.n_atoms == 0 || a.n_mols == 0 || a.H, "%s: H is NULL", who);
    } else {
        DMPNN_CHECK_ARG(a.ldgo >= a.d_h && a.ldgh >= a.d_h, "%s: ldgo (%lld) / ldgh (%lld) < d_h (%lld)", who, (long long)a.ldgo, (long long)a.ldgh,
                        (long long)a.d_h);
        DMPNN_CHECK_ARG(a.n_atoms == 0 || a.gH, "%s: gH is NULL", who);
        DMPNN_CHECK_ARG(!work || (a.H && a.W && a.gout && a.keep_s && a.keep_Z), "%s: NULL H / W / gout / keep_s / keep_Z", who);
    }
    const size_t need = bwd ? dmpnn_molagg_attn_ws_bytes(ap) : attn_table_bytes(a);
    if (a.n_mols > 0 && need > 0 && (bwd ? (a.gW || a.gb || !a.bounds) : true) && (!a.ws || a.ws_bytes < need)) {
        set_error("%s: workspace missing or too small (%zu < %zu bytes)", who, a.ws ? a.ws_bytes : (size_t)0, need);
        return DMPNN_ENOSPC;
    }
    DMPNN_CHECK_ARG(!a.ws || aligned16(a.ws), "%s: workspace must be 16-byte aligned", who);
    return DMPNN_OK;
}

AttnArgs attn_kernel_args(const dmpnn_molagg_attn_args& a) {
    AttnArgs k;
    memset(&k, 0, sizeof(k));
    k.H = a.H; k.ldh = a.ldh;
    k.bounds = static_cast<const int*>(a.bounds ? a.bounds : a.ws);
    k.W = a.W; k.b = a.b;
    k.out = a.out; k.ldo = a.ldo; k.keep_s = a.keep_s; k.keep_Z = a.keep_Z;
    k.gout = a.gout; k.ldgo = a.ldgo; k.gH = a.gH; k.ldgh = a.ldgh;
    k.n_atoms = a.n_atoms; k.n_mols = a.n_mols; k.d = (int)a.d_h;
    return k;
}

#define DMPNN_ATTN_LAUNCH(KERNEL, VECOK, D, GRID, STREAM, ARGS)                                                                  \
    do {                                                                                                                        \
        const int64_t groups_ = (VECOK) ? ((D) / 4 + 63) / 64 : ((D) + 63) / 64;                                                \
        if (VECOK) {                                                                                                            \
            if (groups_ <= 1) hipLaunchKernelGGL((KERNEL<4, 1>), GRID, dim3(256), 0, STREAM, ARGS);                             \
            else if (groups_ <= 2) hipLaunchKernelGGL((KERNEL<4, 2>), GRID, dim3(256), 0, STREAM, ARGS);                        \
            else if (groups_ <= kAttnNarrowQuads) hipLaunchKernelGGL((KERNEL<4, kAttnNarrowQuads>), GRID, dim3(256), 0, STREAM, ARGS); \
            else hipLaunchKernelGGL((KERNEL<4, 0>), GRID, dim3(256), 0, STREAM, ARGS);                                          \
        } else {                                                                                                                \
            if (groups_ <= 1) hipLaunchKernelGGL((KERNEL<1, 1>), GRID, dim3(256), 0, STREAM, ARGS);                             \
            else if (groups_ <= 2) hipLaunchKernelGGL((KERNEL<1, 2>), GRID, dim3(256), 0, STREAM, ARGS);                        \
            else if (groups_ <= kAttnNarrowQuads) hipLaunchKernelGGL((KERNEL<1, kAttnNarrowQuads>), GRID, dim3(256), 0, STREAM, ARGS); \
            else hipLaunchKernelGGL((KERNEL<1, 0>), GRID, dim3(256), 0, STREAM, ARGS);                                          \
        }                                                                                                                       \
    } while (0)

}  // namespace

int attn_fwd_impl(const dmpnn_molagg_attn_args* ap, int* id_bounds, int64_t* id_batch, void* stream) {
    DMPNN_TRY(attn_check(ap, false));
    const dmpnn_molagg_attn_args& a = *ap;
    if (a.n_mols == 0) return DMPNN_OK;
    if (!a.bounds) DMPNN_TRY(dmpnn_molagg_bounds(a.batch, a.n_atoms, a.n_mols, a.ws, a.ws_bytes, stream));
    AttnArgs k = attn_kernel_args(a);
    k.id_bounds = id_bounds; k.id_batch = id_batch;
    const bool vec = a.d_h % 4 == 0 && a.ldh % 4 == 0 && a.ldo % 4 == 0 && aligned16(a.H) && aligned16(a.out) && aligned16(a.W);
    const dim3 grid((unsigned)((a.n_mols + 3) / 4));
    DMPNN_ATTN_LAUNCH(k_attn_fwd, vec, a.d_h, grid, static_cast<hipStream_t>(stream), k);
    DMPNN_CHECK_LAUNCH("k_attn_fwd");
    return DMPNN_OK;
}

int attn_bwd_impl(const dmpnn_molagg_attn_args* ap, void* stream) {
    DMPNN_TRY(attn_check(ap, true));
    const dmpnn_molagg_attn_args& a = *ap;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.n_atoms == 0 || a.n_mols == 0) {   // nothing to differentiate: the requested gradients are zero
        bool ok = true;
        if (a.gW) ok = ok && hipMemsetAsync(a.gW, 0, (size_t)a.d_h * sizeof(float), s) == hipSuccess;
        if (a.gb) ok = ok && hipMemsetAsync(a.gb, 0, sizeof(float), s) == hipSuccess;
        if (a.n_atoms > 0) ok = ok && hipMemset2DAsync(a.gH, (size_t)a.ldgh * sizeof(float), 0, (size_t)a.d_h * sizeof(float), (size_t)a.n_atoms, s) == hipSuccess;
        if (!ok) { set_error("molagg_attn_bwd: hipMemsetAsync failed"); return DMPNN_EHIP; }
        return DMPNN_OK;
    }
    AttnArgs k = attn_kernel_args(a);
    const bool want_w = a.gW || a.gb;
    k.n_waves = attn_waves(a.n_mols);
    k.part_ld = attn_part_ld(a.d_h);
    k.part = want_w ? reinterpret_cast<float*>(static_cast<unsigned char*>(a.ws) + attn_table_bytes(a)) : nullptr;
    const bool vec = a.d_h % 4 == 0 && a.ldh % 4 == 0 && a.ldgo % 4 == 0 && a.ldgh % 4 == 0 && aligned16(a.H) && aligned16(a.gout) && aligned16(a.gH) &&
                     aligned16(a.W);
    const dim3 grid((unsigned)((k.n_waves + 3) / 4));
    DMPNN_ATTN_LAUNCH(k_attn_bwd, vec, a.d_h, grid, s, k);
    DMPNN_CHECK_LAUNCH("k_attn_bwd");
    if (want_w) {
        hipLaunchKernelGGL(k_attn_reduce, dim3((unsigned)((a.d_h + 1 + 63) / 64)), dim3(256), 0, s, k.part, k.part_ld, k.n_waves, k.d,
                           k.bounds + 2 * a.n_mols, a.gW, a.gb);
        DMPNN_CHECK_LAUNCH("k_attn_reduce");
    }
    return DMPNN_OK;
}

}  // namespace dmpnn

extern "C" {

// [the bounds table when a->bounds == NULL] | the backward pass's partial rows: min(n_mols, 1 024) x (align4(d_h) + 4) floats
size_t dmpnn_molagg_attn_ws_bytes(const dmpnn_molagg_attn_args* a) {
    if (!a || a->n_mols < 0 || a->d_h < 1 || a->d_h >= (1 << 24)) return 0;
    return dmpnn::attn_table_bytes(*a) + dmpnn::al256((size_t)dmpnn::attn_waves(a->n_mols) * dmpnn::attn_part_ld(a->d_h) * sizeof(float));
}

int dmpnn_molagg_attn_fwd(const dmpnn_molagg_attn_args* a, void* stream) { return dmpnn::attn_fwd_impl(a, nullptr, nullptr, stream); }

int dmpnn_molagg_attn_bwd(const dmpnn_molagg_attn_args* a, void* stream) { return dmpnn::attn_bwd_impl(a, stream); }

}  // extern "C"
