// K6, input side — gradients of the block with respect to its INPUTS V, E and V_d (what autograd does through mixins.py:8-9 and
// base.py:180-188 when a feature tensor requires grad: attributions on a frozen model, a learned featurizer in front of the block).
//
// The per-step general route of backward_impl (dmpnn_backward.hip) ends with two tensors in its workspace, both in the caller's
// row order:  GO = dL/d(W_o [V || Mv] + b_o)  [n_atoms, ldh]  and  G0 = dL/d(W_i [V[src] || E] + b_i)  [n_edges, ldh].  With them
//
//     gE   = G0 . W_i[:, d_v:]                                   [n_edges, d_e]
//     S[v] = sum_{e: src(e) = v} G0[e] = sum_{e': dst(e') = v} G0[rev(e')]
//     gV   = GO . W_o[:, :d_v] + S . W_i[:, :d_v]                [n_atoms, d_v]
//     gV_d = gout . W_d[:, d_h:]                                 [n_atoms, d_vd]
//
// Sum first, then contract: S has n_atoms rows, the [n_edges, d_v + d_e] product is never formed.  The second form of S is the
// incoming-edge CSR of the plan read through rev — one wave per atom, a fixed summation order (increasing edge id of the incoming
// edges), no atomics — and holds on a symmetric graph only: on a plan whose header says otherwise S is NaN, and gV with it.
// gV is ONE kernel, k_input_grad_v: a workgroup per tile of kIgTA atoms stages [GO[v] || S[v]] in LDS — S[v] summed there from
// G0[rev(.)], never written to memory — in K-chunks of kIgKC columns, each split into f16 pairs under its own row scale, and
// contracts them with the pre-split [W_o[:, :d_v] ; W_i[:, :d_v]] on the f16 pipe (3 products, fp32 accumulation).  Where that kernel
// does not take the call (input_grad_v_fused: d_v, alignment) the host composes gV instead: k_src_sum, then the row kernels over the
// transposed, stacked slices.  gE and gV_d run on the row kernels (k_rows16 where its gate takes the call — the pre-split reads the
// slice transposed in place — else the fp32 MFMA kernel over a transposed copy).
#include "dmpnn_common.hpp"
#include "dmpnn_mega16_impl.hpp"   // (scale_for / split4 / h8: the operand split of the f16 pipe)

namespace dmpnn {

namespace {

inline size_t align64(size_t x) { return (x + 63) & ~size_t(63); }

// S[v][0:h] = sum over the incoming edges e' of v (CSR order) of G[rev(e')][0:h];  NaN rows on a plan without a usable rev
// (asymmetric graph, light plan, tile plan).  Columns >= h of S are never written.
template <int VEC>
__global__ __launch_bounds__(256) void k_src_sum(PlanView pv, int nV, int nE, int h, const float* __restrict__ G, int64_t ldg,
                                                 float* __restrict__ S, int64_t lds) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_waves = gridDim.x * 4;
    const bool bad = (pv.hdr[DMPNN_HDR_FLAGS] & (PLAN_ASYMMETRIC | PLAN_TILES_ONLY)) != 0 || pv.hdr[DMPNN_HDR_LIGHT] != 0;
    const int n_cols = h / VEC;
    const float qnan = __int_as_float(0x7FC00000);
    for (int v = wave; v < nV; v += n_waves) {
        int beg = 0, d = 0;
        bool poison = bad;
        if (!bad) {
            beg = pv.row_ptr[v];
            d = pv.row_ptr[v + 1] - beg;
            if (beg < 0 || d < 0 || beg + d > nE) { d = 0; poison = true; }   // (a plan that is not this batch's: read nothing, NaN)
        }
        for (int cg = lane; cg < n_cols; cg += 64) {
            const int c = cg * VEC;
            float acc[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) acc[t] = 0.f;
            for (int i0 = 0; i0 < d; i0 += 4) {
                // four rows per round: their index loads, then their row loads, are issued together; the adds stay in CSR order
                // (an index out of range is read at a clamped position, for the bounds alone, and the row comes out NaN)
                int er[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = pv.perm[beg + (i0 + j < d ? i0 + j : i0)];
                    const int r = pv.rev[e < 0 ? 0 : (e >= nE ? nE - 1 : e)];
                    poison |= e < 0 || e >= nE || r < 0 || r >= nE;
                    er[j] = r < 0 ? 0 : (r >= nE ? nE - 1 : r);
                }
                float row[4][VEC];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* p = G + (int64_t)er[j] * ldg + c;
                    if constexpr (VEC == 4) {
                        const float4 q = *reinterpret_cast<const float4*>(p);
                        row[j][0] = q.x; row[j][1] = q.y; row[j][2] = q.z; row[j][3] = q.w;
                    } else {
                        row[j][0] = *p;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (i0 + j < d) {
#pragma unroll
                        for (int t = 0; t < VEC; ++t) acc[t] += row[j][t];
                    }
                }
            }
            if (poison) {
#pragma unroll
                for (int t = 0; t < VEC; ++t) acc[t] = qnan;
            }
            float* o = S + (int64_t)v * lds + c;
            if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else *o = acc[0];
        }
    }
}

// ---- gV in one kernel ------------------------------------------------------------------------------------------------------------
// gV[v] = GO[v] . W_o[:, :d_v] + S[v] . W_i[:, :d_v] for a tile of kIgTA atoms per workgroup (256 threads, 4 waves).  The operand row
// [GO[v] || S[v]] passes through LDS in K-chunks of kIgKC columns (first those of GO, then those of S), so that any d_h fits: thread
// (row i = tid >> 4, p = tid & 15) holds the quads 4 p + 64 j of its row's chunk — for S it adds the rows G0[rev(e')] of the atom's
// incoming edges in CSR order, k_src_sum's order — the 16 threads of a row agree on the chunk's maximum by four shuffles, and the
// chunk is stored as f16 pairs x s = hi + lo under that power-of-two scale (mega16::split4).  Wave w owns the column tiles w, w + 4,
// ... (kIgCT of them at most: d_v <= kIgMaxDv) and reads its weight fragments from the pre-split matrices (fragment-major, one
// 16-byte load per lane, k_split_weights); a chunk's products go to a fresh accumulator that is folded into the fp32 total with the
// chunk's row scale and the column's scale.  A plan without a usable rev, or an index out of range: NaN rows.
constexpr int kIgTA = 16;       // atoms per tile: one MFMA row tile
constexpr int kIgKC = 256;      // columns of GO or of S per K-chunk (8 MFMA steps of 32)
constexpr int kIgCT = 4;        // column tiles per wave
constexpr int kIgMaxDv = 4 * kIgCT * 16;
typedef float ig_f32x4 __attribute__((ext_vector_type(4)));
struct IgVArgs {
    PlanView pv; int nV, nE, h, dv;
    const float* GO; const float* G0; int64_t ldh;
    const unsigned char* Wp[2]; const float* isw[2]; int nc;   // pre-split W_o[:, :d_v] and W_i[:, :d_v] as d_v rows over d_h (read transposed)
    float* gV; int64_t ldgv;
};
__global__ __launch_bounds__(256) void k_input_grad_v(IgVArgs a) {
    using mega16::h4; using mega16::h8;
    constexpr int NCH = kIgKC / 32, TS = NCH * 128 + 16, NQ = kIgKC / 64;
    __shared__ __attribute__((aligned(16))) unsigned char As[kIgTA * TS];   // the split chunk: row i, 32-column group c: 64 B hi | 64 B lo
    __shared__ float inv_s[kIgTA];                                         // 1 / scale of the chunk's rows (NaN: a poisoned row)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int i = tid >> 4, p = tid & 15;
    const int64_t row0 = (int64_t)blockIdx.x * kIgTA;
    const int nrows = (int)(a.nV - row0 < kIgTA ? a.nV - row0 : kIgTA);
    const bool live = i < nrows;
    const int64_t v = row0 + i;
    const float qnan = __int_as_float(0x7FC00000);
    const bool with_s = a.nE > 0;
    bool poison = false;
    int beg = 0, d = 0;
    if (with_s) {
        poison = (a.pv.hdr[DMPNN_HDR_FLAGS] & (PLAN_ASYMMETRIC | PLAN_TILES_ONLY)) != 0 || a.pv.hdr[DMPNN_HDR_LIGHT] != 0;
        if (live && !poison) {
            beg = a.pv.row_ptr[v];
            d = a.pv.row_ptr[v + 1] - beg;
            if (beg < 0 || d < 0 || beg + d > a.nE) { d = 0; poison = true; }
        }
    }
    ig_f32x4 tot[kIgCT];
#pragma unroll
    for (int ct = 0; ct < kIgCT; ++ct) tot[ct] = ig_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int part = 0; part < (with_s ? 2 : 1); ++part) {
        for (int k0 = 0; k0 < a.h; k0 += kIgKC) {
            // ---- the thread's quads of the chunk (a.ldh % 4 == 0: a quad that begins below d_h ends inside the row) ----
            float4 x[NQ];
#pragma unroll
            for (int j = 0; j < NQ; ++j) x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (part == 0) {
                if (live) {
#pragma unroll
                    for (int j = 0; j < NQ; ++j) {
                        const int c4 = k0 + 4 * p + 64 * j;
                        if (c4 < a.h) x[j] = *reinterpret_cast<const float4*>(a.GO + v * a.ldh + c4);
                    }
                }
            } else {
                for (int i0 = 0; i0 < d; i0 += 2) {   // two rows per round: index loads, then row loads, together; adds in CSR order
                    int er[2];
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int e = a.pv.perm[beg + (i0 + t < d ? i0 + t : i0)];
                        const int r = a.pv.rev[e < 0 ? 0 : (e >= a.nE ? a.nE - 1 : e)];
                        poison |= e < 0 || e >= a.nE || r < 0 || r >= a.nE;
                        er[t] = r < 0 ? 0 : (r >= a.nE ? a.nE - 1 : r);
                    }
                    float4 q[2][NQ];
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
#pragma unroll
                        for (int j = 0; j < NQ; ++j) {
                            const int c4 = k0 + 4 * p + 64 * j;
                            q[t][j] = c4 < a.h ? *reinterpret_cast<const float4*>(a.G0 + (int64_t)er[t] * a.ldh + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
                        }
                    }
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        if (i0 + t < d) {
#pragma unroll
                            for (int j = 0; j < NQ; ++j) { x[j].x += q[t][j].x; x[j].y += q[t][j].y; x[j].z += q[t][j].z; x[j].w += q[t][j].w; }
                        }
                    }
                }
            }
            float mx = 0.f;
#pragma unroll
            for (int j = 0; j < NQ; ++j) {   // columns >= d_h of the last quad are padding: whatever they hold, the operand has zeros there
                const int c4 = k0 + 4 * p + 64 * j;
                if (c4 + 1 >= a.h) x[j].y = 0.f;
                if (c4 + 2 >= a.h) x[j].z = 0.f;
                if (c4 + 3 >= a.h) x[j].w = 0.f;
                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(x[j].x), fabsf(x[j].y))), fmaxf(fabsf(x[j].z), fabsf(x[j].w)));
            }
            for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            const float sr = mega16::scale_for(mx);
            __syncthreads();   // the previous chunk's contraction has read As and inv_s
            if (p == 0) inv_s[i] = poison ? qnan : 1.f / sr;
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int c4 = 4 * p + 64 * j;
                h4 hi, lo;
                mega16::split4(x[j], sr, hi, lo);
                unsigned char* dp = As + i * TS + (c4 >> 5) * 128 + (c4 & 31) * 2;
                *reinterpret_cast<h4*>(dp) = hi;
                *reinterpret_cast<h4*>(dp + 64) = lo;
            }
            __syncthreads();   // the split chunk (and inv_s) is complete
            // ---- contraction: the chunk's 32-column groups that exist (cg < nc) against the wave's column tiles ----
            const int cg0 = k0 >> 5;
            const int n_ch = a.nc - cg0 < NCH ? a.nc - cg0 : NCH;
#pragma unroll
            for (int ct = 0; ct < kIgCT; ++ct) {
                const int T = wave + 4 * ct;
                if (T * 16 < a.dv) {   // (wave-uniform)
                    const int col = T * 16 + li;
                    const unsigned char* wp = a.Wp[part] + ((int64_t)T * a.nc + cg0) * 2048 + lane * 16;
                    ig_f32x4 acc = ig_f32x4{0.f, 0.f, 0.f, 0.f};
                    for (int c = 0; c < n_ch; ++c) {
                        const h8 wh = *reinterpret_cast<const h8*>(wp + c * 2048), wl = *reinterpret_cast<const h8*>(wp + c * 2048 + 1024);
                        const unsigned char* pa = As + li * TS + c * 128 + lg * 16;
                        const h8 ah = *reinterpret_cast<const h8*>(pa), al = *reinterpret_cast<const h8*>(pa + 64);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wh, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wl, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wh, acc, 0, 0, 0);
                    }
                    const float isw = col < a.dv ? a.isw[part][col] : 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) tot[ct][r] += acc[r] * (isw * inv_s[4 * lg + r]);
                }
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < kIgCT; ++ct) {
        const int col = (wave + 4 * ct) * 16 + li;
        if (col < a.dv) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ii = 4 * lg + r;
                if (ii < nrows) a.gV[(row0 + ii) * a.ldgv + col] = tot[ct][r];
            }
        }
    }
}

// THE dispatch rule of gV: what k_input_grad_v takes — any n_atoms, n_edges, d_h and d_e; at most kIgMaxDv columns (kIgCT column tiles
// per wave); GO and G0 as rows of whole 16-byte quads.  Everything else is composed on the host (k_src_sum + the row kernels).
bool input_grad_v_fused(int64_t dv, int64_t ldh, const float* GO, const float* G0) {
    return dv >= 1 && dv <= kIgMaxDv && ldh % 4 == 0 && aligned16(GO) && aligned16(G0);
}

// out[c][r] = in[r][c] for up to four weight slices in one launch (a few hundred KB in all)
struct TrJob { const float* in; int64_t ldi; float* out; int64_t ldo; int rows, cols; };
struct TrJobs { TrJob job[4]; int n; };
__global__ __launch_bounds__(256) void k_transpose_slices(TrJobs a) {
    const TrJob j = a.job[blockIdx.y];
    const int64_t total = (int64_t)j.rows * j.cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i / j.rows), r = (int)(i - (int64_t)c * j.rows);
        j.out[(int64_t)c * j.ldo + r] = j.in[(int64_t)r * j.ldi + c];
    }
}

// C[M, N] = [A1 || A2] . Wt^T  (Wt [N, K1 + K2] fp32, row stride ldw): the f16 pipe where the row kernel's gate takes the call
int contract(int64_t M, int64_t N, const float* A1, int64_t lda1, int64_t K1, const float* A2, int64_t lda2, int64_t K2, const float* Wt, int64_t ldw,
             float* C, int64_t ldc, bool use16, float* w16, const int* poison_flags, int poison_mask, hipStream_t s, const SplitWView* view = nullptr) {
    if (M == 0 || N == 0) return DMPNN_OK;
    dmpnn_gemm_args g;
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.K1 = K1; g.A1 = A1; g.lda1 = lda1; g.K2 = K2; g.A2 = K2 ? A2 : nullptr; g.lda2 = K2 ? lda2 : 0;
    g.W = Wt; g.ldw = ldw; g.C = C; g.ldc = ldc; g.act = DMPNN_ACT_NONE;
    if (view) return launch_linear16_view(g, *view, poison_flags, poison_mask, s);   // (the slice was pre-split in place, read transposed)
    if (use16 && linear16_ok(g)) {
        SplitWView w;
        DMPNN_TRY(split_weights_view(Wt, ldw, N, K1 + K2, 0, w16, &w, s));
        return launch_linear16_view(g, w, poison_flags, poison_mask, s);
    }
    GemmExtra x;
    memset(&x, 0, sizeof(x));
    x.poison_flags = poison_flags; x.poison_mask = poison_mask;
    return launch_linear_ex(g, x, s);
}

struct IgLayout { size_t wt_v, wt_e, wt_d, w16_v, w16_e, w16_d, total; };
IgLayout ig_layout(const dmpnn_fwd_args& f) {
    const int64_t h = f.d_h, dv = f.d_v, de = f.d_e, dvd = f.W_d ? f.d_vd : 0;
    IgLayout L;
    size_t o = 0;
    L.wt_v = o; o += align64((size_t)dv * 2 * h);
    L.wt_e = o; o += align64((size_t)de * h);
    L.wt_d = o; o += align64((size_t)dvd * (h + dvd));
    // (gV: the stacked [d_v, 2 d_h] matrix of the composed form, or the two [d_v, d_h] halves k_input_grad_v reads)
    const size_t stacked = linear16_wsplit_bytes(dv > 0 ? dv : 1, 2 * h), half = linear16_wsplit_bytes(dv > 0 ? dv : 1, h);
    L.w16_v = o; o += align64(((stacked > 2 * half ? stacked : 2 * half) + 3) / 4);
    L.w16_e = o; o += align64((linear16_wsplit_bytes(de > 0 ? de : 1, h) + 3) / 4);
    L.w16_d = o; o += align64((linear16_wsplit_bytes(dvd > 0 ? dvd : 1, h + dvd) + 3) / 4);
    L.total = o;
    return L;
}

}  // namespace

int launch_src_sum(const PlanView& pv, int64_t nV, int64_t nE, int64_t h, const float* G, int64_t ldg, float* S, int64_t lds, hipStream_t s) {
    if (nV == 0 || h == 0) return DMPNN_OK;
    int64_t blocks = (nV + 3) / 4;
    if (blocks > 256 * 32) blocks = 256 * 32;
    // (no edges: every row is a row of zeros, and G — which is then never read — may be anything, NULL included)
    const bool vec = h % 4 == 0 && ldg % 4 == 0 && lds % 4 == 0 && aligned16(G) && aligned16(S);
    if (vec) hipLaunchKernelGGL(k_src_sum<4>, dim3((unsigned)blocks), dim3(256), 0, s, pv, (int)nV, (int)nE, (int)h, G, ldg, S, lds);
    else hipLaunchKernelGGL(k_src_sum<1>, dim3((unsigned)blocks), dim3(256), 0, s, pv, (int)nV, (int)nE, (int)h, G, ldg, S, lds);
    DMPNN_CHECK_LAUNCH("k_src_sum");
    return DMPNN_OK;
}

size_t input_grads_ws_floats(const dmpnn_fwd_args& f) { return ig_layout(f).total; }

int input_grads(const dmpnn_fwd_args& f, const InputGrads& ig, const float* gout, int64_t ldgout, const float* GO, const float* G0, float* S,
                bool use16, hipStream_t s) {
    const int64_t nV = f.n_atoms, nE = f.n_edges, h = f.d_h, dv = f.d_v, de = f.d_e, dvd = f.W_d ? f.d_vd : 0, ldh = f.ldh;
    const bool want_v = ig.gV && nV > 0 && dv > 0, want_e = ig.gE && nE > 0 && de > 0, want_d = ig.gV_d && nV > 0 && dvd > 0;
    if (!want_v && !want_e && !want_d) return DMPNN_OK;
    const IgLayout L = ig_layout(f);
    float* w = ig.ws;
    // which kernel forms which gradient: gV in k_input_grad_v where it takes the call; gE and gV_d on k_rows16 where ITS gate does, over
    // a pre-split that reads the slice transposed in place.  Whatever is left is composed over transposed copies of the slices.
    auto rows16_takes = [&](int64_t M, int64_t N, const float* A, int64_t lda, int64_t K) {
        dmpnn_gemm_args g;
        memset(&g, 0, sizeof(g));
        g.M = M; g.N = N; g.K1 = K; g.A1 = A; g.lda1 = lda;
        return use16 && linear16_ok(g);
    };
    const bool v_fused = want_v && input_grad_v_fused(dv, ldh, GO, G0);
    const bool e16 = want_e && rows16_takes(nE, de, G0, ldh, h), d16 = want_d && rows16_takes(nV, dvd, gout, ldgout, h + dvd);
    SplitWJob sj[4];
    SplitWView sv[4];
    int n_sj = 0, i_vo = -1, i_e = -1, i_d = -1;
    if (v_fused) {   // (element (n, k) of each is W[k ldw + n]: tr = 1)
        i_vo = n_sj;
        sj[n_sj++] = SplitWJob{f.W_o, dv + h, dv, h, 1, w + L.w16_v};
        sj[n_sj++] = SplitWJob{f.W_i, dv + de, dv, h, 1, w + L.w16_v + linear16_wsplit_bytes(dv, h) / 4};   // (unused without edges)
    }
    if (e16) { i_e = n_sj; sj[n_sj++] = SplitWJob{f.W_i + dv, dv + de, de, h, 1, w + L.w16_e}; }
    if (d16) { i_d = n_sj; sj[n_sj++] = SplitWJob{f.W_d + h, h + dvd, dvd, h + dvd, 1, w + L.w16_d}; }
    DMPNN_TRY(split_weights_views(sj, n_sj, sv, s));
    TrJobs tj;
    memset(&tj, 0, sizeof(tj));
    int max_elems = 0;
    auto add = [&](const float* in, int64_t ldi, float* out, int64_t ldo, int64_t rows, int64_t cols) {
        tj.job[tj.n++] = TrJob{in, ldi, out, ldo, (int)rows, (int)cols};
        if (rows * cols > max_elems) max_elems = (int)(rows * cols);
    };
    if (want_v && !v_fused) {   // Wt_v [d_v][2 d_h] = [W_o[:, :d_v]^T || W_i[:, :d_v]^T]
        add(f.W_o, dv + h, w + L.wt_v, 2 * h, h, dv);
        if (nE > 0) add(f.W_i, dv + de, w + L.wt_v + h, 2 * h, h, dv);
    }
    if (want_e && !e16) add(f.W_i + dv, dv + de, w + L.wt_e, h, h, de);                       // Wt_e [d_e][d_h]
    if (want_d && !d16) add(f.W_d + h, h + dvd, w + L.wt_d, h + dvd, h + dvd, dvd);          // Wt_d [d_vd][d_h + d_vd]
    if (tj.n > 0) {
        int blocks = (max_elems + 255) / 256;
        if (blocks > 256) blocks = 256;
        hipLaunchKernelGGL(k_transpose_slices, dim3((unsigned)blocks, (unsigned)tj.n), dim3(256), 0, s, tj);
        DMPNN_CHECK_LAUNCH("k_transpose_slices");
    }
    if (want_d) DMPNN_TRY(contract(nV, dvd, gout, ldgout, h + dvd, nullptr, 0, 0, w + L.wt_d, h + dvd, ig.gV_d, ig.ldgvd, use16, w + L.w16_d, nullptr, 0, s, d16 ? &sv[i_d] : nullptr));
    if (want_e) DMPNN_TRY(contract(nE, de, G0, ldh, h, nullptr, 0, 0, w + L.wt_e, h, ig.gE, ig.ldge, use16, w + L.w16_e, nullptr, 0, s, e16 ? &sv[i_e] : nullptr));
    if (v_fused) {
        IgVArgs a;
        memset(&a, 0, sizeof(a));
        a.pv = plan_view(f.plan, nV, nE); a.nV = (int)nV; a.nE = (int)nE; a.h = (int)h; a.dv = (int)dv;
        a.GO = GO; a.G0 = G0; a.ldh = ldh;
        a.Wp[0] = sv[i_vo].p; a.isw[0] = sv[i_vo].inv_scale; a.Wp[1] = sv[i_vo + 1].p; a.isw[1] = sv[i_vo + 1].inv_scale; a.nc = sv[i_vo].nc;
        a.gV = ig.gV; a.ldgv = ig.ldgv;
        hipLaunchKernelGGL(k_input_grad_v, dim3((unsigned)((nV + kIgTA - 1) / kIgTA)), dim3(256), 0, s, a);
        DMPNN_CHECK_LAUNCH("k_input_grad_v");
    } else if (want_v) {
        const PlanView pv = plan_view(f.plan, nV, nE);
        if (nE > 0) DMPNN_TRY(launch_src_sum(pv, nV, nE, h, G0, ldh, S, ldh, s));
        // (the contraction's own poisoning as well: a NaN operand row need not survive the operand split as a NaN)
        DMPNN_TRY(contract(nV, dv, GO, ldh, h, S, ldh, nE > 0 ? h : 0, w + L.wt_v, 2 * h, ig.gV, ig.ldgv, use16, w + L.w16_v,
                           nE > 0 ? pv.hdr + DMPNN_HDR_FLAGS : nullptr, PLAN_ASYMMETRIC, s));
    }
    return DMPNN_OK;
}

}  // namespace dmpnn

using namespace dmpnn;

extern "C" {

int dmpnn_src_sum(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h, const float* G, int64_t ldg, float* S, int64_t lds,
                  void* stream) {
    DMPNN_CHECK_ARG(plan && n_atoms >= 0 && n_edges >= 0 && d_h >= 1 && ldg >= d_h && lds >= d_h, "src_sum: bad arguments");
    DMPNN_CHECK_ARG(n_atoms < (int64_t(1) << 31) && n_edges < (int64_t(1) << 31), "src_sum: size out of range");
    DMPNN_CHECK_ARG((n_edges == 0 || G) && (n_atoms == 0 || S), "src_sum: null tensor");
    return launch_src_sum(plan_view(plan, n_atoms, n_edges), n_atoms, n_edges, d_h, G, ldg, S, lds, static_cast<hipStream_t>(stream));
}

size_t dmpnn_backward_inputs_ws_bytes(const dmpnn_fwd_args* f) {
    if (!f) return 0;
    return (align64(dmpnn_backward_ws_bytes(f) / sizeof(float)) + input_grads_ws_floats(*f)) * sizeof(float);
}

int dmpnn_backward_inputs(const dmpnn_bwd_inputs_args* a, void* stream) {
    DMPNN_CHECK_ARG(a != nullptr, "backward_inputs: null args");
    const dmpnn_bwd_args& b = a->b;
    const dmpnn_fwd_args& f = b.f;
    // every check of this entry and of the route it takes in backward_impl, before any device work
    DMPNN_CHECK_ARG(!(f.flags & (DMPNN_F_FUSED | DMPNN_F_MEGA | DMPNN_F_TILE_PLAN | DMPNN_F_ATOM)),
                    "backward_inputs: input gradients are provided on the per-step general route, bond messages (a kept forward without "
                    "DMPNN_F_FUSED / DMPNN_F_MEGA / DMPNN_F_TILE_PLAN / DMPNN_F_ATOM)");
    DMPNN_CHECK_ARG(f.act != DMPNN_ACT_PRELU, "backward_inputs: PReLU has no fused backward (use the row kernels)");
    DMPNN_CHECK_ARG(f.act >= DMPNN_ACT_RELU && f.act <= DMPNN_ACT_SELU, "backward_inputs: activation %d has no fused backward (use the row kernels)", f.act);
    DMPNN_CHECK_ARG(f.plan && f.d_h > 0 && f.d_v > 0 && f.d_e >= 0 && f.depth >= 1 && f.n_atoms >= 0 && f.n_edges >= 0 && f.ldh >= f.d_h,
                    "backward_inputs: bad forward description");
    DMPNN_CHECK_ARG(f.W_i && f.W_o && (f.depth < 2 || f.n_edges == 0 || f.W_h), "backward_inputs: null weights");
    DMPNN_CHECK_ARG(!b.g_edge, "backward_inputs: g_edge is taken by the backward tile kernel only");
    const bool has_vd = f.W_d != nullptr;
    DMPNN_CHECK_ARG(!a->gV_d || (has_vd && f.d_vd > 0 && f.V_d), "backward_inputs: gV_d needs a block with W_d (b.f.W_d, d_vd > 0)");
    DMPNN_CHECK_ARG(!a->gV || a->ldgv >= f.d_v, "backward_inputs: leading dimension below its width (ldgv < d_v)");
    DMPNN_CHECK_ARG(!a->gE || a->ldge >= f.d_e, "backward_inputs: leading dimension below its width (ldge < d_e)");
    DMPNN_CHECK_ARG(!a->gV_d || a->ldgvd >= f.d_vd, "backward_inputs: leading dimension below its width (ldgvd < d_vd)");
    DMPNN_CHECK_ARG(f.n_atoms == 0 || (b.gout && b.ldgout >= f.d_h + (has_vd ? f.d_vd : 0)), "backward_inputs: null gout, or ldgout below its width");
    DMPNN_CHECK_ARG(f.n_atoms == 0 || (f.V && f.out && f.Mv && (!has_vd || f.Hv)), "backward_inputs: the forward's tensors are missing (V, out, Mv, Hv)");
    DMPNN_CHECK_ARG(f.n_edges == 0 || (f.H0 && (f.d_e == 0 || f.E) && (f.depth < 2 || (f.Hs && f.Ms))), "backward_inputs: the forward's kept tensors are missing");
    if (f.dropout_p != 0.f) {   // (what backward_impl asks of a forward with the mask in the row kernels)
        DMPNN_CHECK_ARG(f.dropout_p > 0.f && f.dropout_p < 1.f && (f.flags & DMPNN_F_SPLIT16) && (f.flags & DMPNN_F_KEEP) && !has_vd && f.d_h <= 1024 &&
                        (!(f.flags & DMPNN_F_UNDIRECTED) || (f.flags & DMPNN_F_UNDIRECTED_MASK)),
                        "backward_inputs: in-kernel dropout on the per-step general route needs DMPNN_F_SPLIT16 | DMPNN_F_KEEP, no W_d, d_h <= 1024 "
                        "(undirected: DMPNN_F_UNDIRECTED_MASK)");
    }
    DMPNN_CHECK_ARG(!(f.flags & DMPNN_F_UNDIRECTED_MASK) || (f.flags & DMPNN_F_UNDIRECTED), "backward_inputs: DMPNN_F_UNDIRECTED_MASK only goes with DMPNN_F_UNDIRECTED");
    const size_t need = dmpnn_backward_inputs_ws_bytes(&f);
    if (!b.ws || b.ws_bytes < need) {
        set_error("backward_inputs: workspace too small (%zu < %zu bytes: dmpnn_backward_inputs_ws_bytes)", b.ws_bytes, need);
        return DMPNN_ENOSPC;
    }
    InputGrads ig{a->gV, a->ldgv, a->gE, a->ldge, a->gV_d, a->ldgvd, b.ws + align64(dmpnn_backward_ws_bytes(&f) / sizeof(float))};
    return backward_impl(&b, stream, nullptr, nullptr, &ig);
}

}  // extern "C"
