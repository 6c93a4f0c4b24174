// The atom-descriptor layer H_v' = W_d cat(H_v, V_d) + b_d (message_passing/base.py: the layer behind finalize of a block built with
// d_vd > 0) as a stage of its own between the block and the head: dmpnn_vd_forward / dmpnn_vd_backward (include/dmpnn.h).
//
// Arithmetic: the f16 matrix pipe with the project's exact 3-term operand split (dmpnn_mega16_impl.hpp: x s = hi + lo, products
// hi hi + hi lo + lo hi, fp32 accumulation) — fp32-class.
//   k_vd_split   W_d [D, D] (D = d_h + d_vd) -> a ROW-MAJOR split image hi[Dp][Dp] | lo[Dp][Dp] (Dp = D rounded up to 32, zero padded),
//                row n under its own power-of-two scale s_n, 1 / s_n beside it.  One wave per row.  Nothing about the weights is kept
//                between steps: the image is rebuilt by the forward, and by a backward that does not directly follow it.
//   k_vd_gemm<false>  forward: out = cat(Hv, V_d) . W_d^T + b_d.  A workgroup owns 32 rows and ALL columns: its operand rows are
//                read element by element (any width, any row stride: zero-padded inside the split), scaled per row and split into LDS;
//                the image streams through LDS in chunks of 32 reduction columns, each requested into registers one chunk ahead; a
//                lane's weight fragment is 4 consecutive k of one image row (a plain 8-byte LDS read).
//   k_vd_gemm<true>   data gradient: gHv = gout . W_d[:, :d_h].  The reduction now runs over the image's ROW index, so nothing is
//                transposed in memory: the same image streams through LDS in chunks of 32 ROWS as they are, and the fragments leave
//                LDS through gfx950's transposed read (ds_read_b64_tr_b16: lane i of a 16-lane group receives column i of the 4 x 16
//                block the group addresses).  The rows' scales s_k lie along the reduction here: 1 / s_k (an exact power of two) is
//                folded into column k of gout before its rows are scaled and split.
//   weight gradient   gW_d = gout^T . [Hv || V_d || 1]: the library's weight-gradient product (dmpnn_linear_wgrad: on the f16 pipe
//                from 1 024 rows on when D is even — operand split, product, reduce —, its fp32 kernel below that and for odd D).
//   dropout      dmpnn_vd_args.dropout_p in (0, 1): the block's nn.Dropout once more behind this layer (base.py:185-188), the hash mask of
//                the other homes at site DMPNN_DROP_SITE_VD, keyed on (atom, column of out).  Second instantiations k_vd_gemm<., true>:
//                the forward masks in its epilogue (kept: the p = 0 value times 1.f / (1.f - p); dropped: +0); the data gradient masks
//                gout as it reads it — each element is read by exactly one lane of one workgroup — and writes the masked rows back IN
//                PLACE, so the weight gradient launched behind it on the same stream reads the masked gradient too.  No new launch, no
//                workspace; the p = 0 instantiations are the code they were.
// Launches: forward 2 (split, product); backward 1 (data gradient; + the split when the image is not the forward's) + the weight
// gradient's (3 on the f16 pipe).  Shapes: any d_vd >= 1 with D <= DMPNN_VD_MAX_WIDTH (the operand tile and one image chunk share the
// LDS of a CU); any n_atoms.
#include <string.h>

#include "dmpnn_mega16_impl.hpp"

namespace dmpnn {
namespace vd {

using mega16::h4;
using mega16::scale_for;
using gemm::f32x4;

constexpr int kRowTile = 16, RT = 2;   // a workgroup owns RT row tiles of 16 rows
constexpr int kMaxNTW = 9;       // 16-column tiles per wave: ceil(ceil(544 / 16) / 4)
constexpr int kMaxKJ = 9;        // operand elements per lane and row: ceil(544 / 64)
constexpr int kMaxPieces = 9;    // 16-byte pieces of an image chunk's hi (and lo) part per thread: ceil(4 * 544 / 256)

struct VdK {
    int M, K1, K2, N;                       // rows; columns of A1 and A2 (the reduction is K1 + K2 long); output columns
    const float* A1; long long lda1;
    const float* A2; long long lda2;        // (K2 == 0: unused)
    const float* kscale;                    // multiplies column k of [A1 || A2] before the split (the image rows' 1 / s_k), or null
    const _Float16* Wh; const _Float16* Wl; int Dp;   // split image, row-major [Dp][Dp]
    const float* nscale;                    // multiplies output column n (the image rows' 1 / s_n), or null
    const float* bias;                      // or null
    float* C; long long ldc;
    // DROP instantiations only (dmpnn_vd_args.dropout_p): keep(m, c) = drop_hash(seed, DMPNN_DROP_SITE_VD, m, c) >= drop_thr.
    //   TR = false: the mask lies on C's columns;  TR = true: on A1's (gout), and the masked rows are written back through A1w
    unsigned drop_thr, seed_lo, seed_hi; float drop_scale; float* A1w;
};

struct VdSplit { const float* W; int D, Dp; _Float16* Wh; _Float16* Wl; float* inv; };

__global__ __launch_bounds__(256) void k_vd_split(VdSplit a) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= a.Dp) return;
    const bool live = n < a.D;
    const float* row = a.W + (long long)(live ? n : 0) * a.D;
    float mx = 0.f;
    for (int k = lane; k < a.D; k += 64) mx = fmaxf(mx, fabsf(row[k]));
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float s = live ? scale_for(mx) : 0.f;
    if (lane == 0) a.inv[n] = live ? 1.f / s : 0.f;
    for (int k = lane; k < a.Dp; k += 64) {
        const float x = (live && k < a.D) ? row[k] * s : 0.f;
        const _Float16 hi = (_Float16)x;
        a.Wh[(long long)n * a.Dp + k] = hi;
        a.Wl[(long long)n * a.Dp + k] = (_Float16)(x - (float)hi);
    }
}

typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 f16x4_t;
__device__ __forceinline__ h4 lds_tr4(const _Float16* p) {
    const f16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) f16x4_t*)(p));
    return __builtin_bit_cast(h4, v);
}

// LDS (halfs): A hi [16 RT][Kp + 8] | A lo | image chunk hi | image chunk lo | (floats) 1 / row scale [16 RT]
//   image chunk, TR = false: [Np][40]  (32 reduction columns of every image row; 80-byte rows)
//                TR = true:  [32][Np + 8]  (32 image rows as they are)
static_assert(DMPNN_VD_MAX_WIDTH <= 64 * kMaxKJ && DMPNN_VD_MAX_WIDTH <= 64 * kMaxNTW && 4 * DMPNN_VD_MAX_WIDTH <= 256 * kMaxPieces, "register arrays are sized for the widest layer");
inline size_t vd_lds_bytes(int Kp, int Np, bool tr, int rows) {
    const size_t a = (size_t)2 * rows * (Kp + 8) * 2;
    const size_t w = tr ? (size_t)2 * 32 * (Np + 8) * 2 : (size_t)2 * Np * 40 * 2;
    return a + w + rows * sizeof(float);
}

// DROP is a second instantiation, not a run-time branch: the p = 0 kernels stay the code they were (the operand rows already hold
// 4 x kMaxKJ live registers per lane beside the prefetched image chunk; the hash's temporaries are not added to that build).
template <bool TR, bool DROP>
__global__ __launch_bounds__(256) void k_vd_gemm(VdK a) {
    constexpr int kBM = kRowTile * RT;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int K = a.K1 + a.K2;
    const int Kp = (K + 31) & ~31, Np = (a.N + 15) & ~15, NT = Np >> 4;
    const int lda = Kp + 8;                              // halfs per row of the operand tile
    const int ldw = TR ? Np + 8 : 40;                    // halfs per row of the image chunk
    const int wrows = TR ? 32 : Np;
    _Float16* Ah = reinterpret_cast<_Float16*>(lds);
    _Float16* Al = Ah + kBM * lda;
    _Float16* Bh = Al + kBM * lda;
    _Float16* Bl = Bh + wrows * ldw;
    float* rinv = reinterpret_cast<float*>(Bl + wrows * ldw);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const long long m0 = (long long)blockIdx.x * kBM;

    // ---- the image chunks: 4 Np 16-byte pieces of hi and of lo each; piece `idx` of a chunk -> (global offset, LDS offset) in halfs.
    // A chunk is requested into registers one chunk AHEAD — the loads are in flight under the previous chunk's products — and goes
    // to LDS between two barriers (a workgroup is alone on its CU: nothing else would cover the round trip to L2).
    typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
    const int n_pieces = 4 * Np;
    u32x4v pre_h[kMaxPieces], pre_l[kMaxPieces];
    auto piece = [&](int idx, int k0, long long& src, int& dst) {
        if constexpr (TR) {          // image rows k0 .. k0 + 31 as they are, columns [0, Np)
            const int ppr = Np >> 3, r = idx / ppr, p = idx - r * ppr;
            src = (long long)(k0 + r) * a.Dp + 8 * p; dst = r * ldw + 8 * p;
        } else {                     // columns k0 .. k0 + 31 of the image rows [0, Np)
            const int n = idx >> 2, p = idx & 3;
            src = (long long)n * a.Dp + k0 + 8 * p; dst = n * ldw + 8 * p;
        }
    };
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < kMaxPieces; ++i) {
            const int idx = tid + 256 * i;
            if (idx < n_pieces) {
                long long src; int dst;
                piece(idx, k0, src, dst);
                pre_h[i] = *reinterpret_cast<const u32x4v*>(a.Wh + src);
                pre_l[i] = *reinterpret_cast<const u32x4v*>(a.Wl + src);
            }
        }
    };
    auto stash = [&](int k0) {
#pragma unroll
        for (int i = 0; i < kMaxPieces; ++i) {
            const int idx = tid + 256 * i;
            if (idx < n_pieces) {
                long long src; int dst;
                piece(idx, k0, src, dst);
                *reinterpret_cast<u32x4v*>(Bh + dst) = pre_h[i];
                *reinterpret_cast<u32x4v*>(Bl + dst) = pre_l[i];
            }
        }
    };
    fetch(0);   // (in flight under the operand rows below)

    // ---- the workgroup's operand rows: scaled per row, split, zero-padded to Kp columns (rows beyond M: zeros); four rows' loads
    // are requested together ----
    float ks[kMaxKJ];   // the columns' multipliers of this lane, once
#pragma unroll
    for (int j = 0; j < kMaxKJ; ++j) {
        const int c = lane + 64 * j;
        ks[j] = (a.kscale && c < K) ? a.kscale[c] : 1.f;
    }
    for (int r0 = wave; r0 < kBM; r0 += 16) {   // (rows r0, r0 + 4, r0 + 8, r0 + 12)
        float v[4][kMaxKJ];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long m = m0 + r0 + 4 * q;
            const bool live = m < a.M;
#pragma unroll
            for (int j = 0; j < kMaxKJ; ++j) {
                const int c = lane + 64 * j;
                float x = 0.f;
                if (live && c < a.K1) x = a.A1[m * a.lda1 + c];
                else if (live && c < K) x = a.A2[m * a.lda2 + (c - a.K1)];
                if constexpr (DROP && TR) {
                    // the masked gradient g' = keep ? gout / (1 - p) : +0 feeds this product AND the weight gradient behind it: this
                    // lane is the only reader of the element in the launch, so it goes back in place
                    if (live && c < K) {
                        x = drop_hash(a.seed_lo, a.seed_hi, (unsigned)DMPNN_DROP_SITE_VD, (unsigned)m, (unsigned)c) >= a.drop_thr ? x * a.drop_scale : 0.f;
                        a.A1w[m * a.lda1 + c] = x;
                    }
                }
                v[q][j] = x;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + 4 * q;
            float mx = 0.f;
#pragma unroll
            for (int j = 0; j < kMaxKJ; ++j) {
                v[q][j] *= ks[j];
                mx = fmaxf(mx, fabsf(v[q][j]));
            }
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            const float s = scale_for(mx);
#pragma unroll
            for (int j = 0; j < kMaxKJ; ++j) {
                const int c = lane + 64 * j;
                if (c < Kp) {
                    const float y = v[q][j] * s;
                    const _Float16 hi = (_Float16)y;
                    Ah[r * lda + c] = hi;
                    Al[r * lda + c] = (_Float16)(y - (float)hi);
                }
            }
            if (lane == 0) rinv[r] = 1.f / s;
        }
    }

    f32x4 acc[RT][kMaxNTW];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < kMaxNTW; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < Kp; k0 += 32) {
        __syncthreads();   // (the previous chunk's fragments are read; first pass: the operand tile is complete)
        stash(k0);
        __syncthreads();
        if (k0 + 32 < Kp) fetch(k0 + 32);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            h4 ah[RT], al[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int o = (rt * 16 + li) * lda + k0 + kk * 16 + 4 * lg;
                ah[rt] = *reinterpret_cast<const h4*>(Ah + o);
                al[rt] = *reinterpret_cast<const h4*>(Al + o);
            }
#pragma unroll
            for (int t = 0; t < kMaxNTW; ++t) {
                const int nt = wave + 4 * t;   // (a scalar: the branch keeps every lane of the wave — the transposed read needs them all)
                if (nt < NT) {
                    h4 bh, bl;
                    if constexpr (TR) {
                        // group lg reads the block of rows kk 16 + 4 lg .. + 3, columns nt 16 .. + 15: lane 4 q + p supplies row q, columns 4 p ..
                        const int o = (kk * 16 + 4 * lg + (li >> 2)) * ldw + nt * 16 + 4 * (li & 3);
                        bh = lds_tr4(Bh + o);
                        bl = lds_tr4(Bl + o);
                    } else {
                        const int o = (nt * 16 + li) * ldw + kk * 16 + 4 * lg;
                        bh = *reinterpret_cast<const h4*>(Bh + o);
                        bl = *reinterpret_cast<const h4*>(Bl + o);
                    }
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah[rt], bh, acc[rt][t], 0, 0, 0);
                        acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah[rt], bl, acc[rt][t], 0, 0, 0);
                        acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(al[rt], bh, acc[rt][t], 0, 0, 0);
                    }
                }
            }
        }
    }
    // ---- epilogue: register j of a lane is row 4 lg + j, column li of its tile ----
#pragma unroll
    for (int t = 0; t < kMaxNTW; ++t) {
        const int nt = wave + 4 * t;
        if (nt >= NT) continue;
        const int n = nt * 16 + li;
        if (n >= a.N) continue;
        const float ns = a.nscale ? a.nscale[n] : 1.f;
        const float bv = a.bias ? a.bias[n] : 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = rt * 16 + 4 * lg + j;
                const long long m = m0 + r;
                if (m < a.M) {
                    const float y = acc[rt][t][j] * rinv[r] * ns + bv;
                    if constexpr (DROP && !TR)
                        a.C[m * a.ldc + n] = drop_hash(a.seed_lo, a.seed_hi, (unsigned)DMPNN_DROP_SITE_VD, (unsigned)m, (unsigned)n) >= a.drop_thr ? y * a.drop_scale : 0.f;
                    else
                        a.C[m * a.ldc + n] = y;
                }
            }
    }
}

static size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
struct VdLayout { size_t wh, wl, inv, wgrad, wgrad_bytes, total; int D, Dp; };
static VdLayout vd_layout(const dmpnn_vd_args& a) {
    VdLayout L;
    L.D = (int)(a.d_h + a.d_vd); L.Dp = (L.D + 31) & ~31;
    size_t o = 0;
    L.wh = o; o += al256((size_t)L.Dp * L.Dp * 2);
    L.wl = o; o += al256((size_t)L.Dp * L.Dp * 2);
    L.inv = o; o += al256((size_t)L.Dp * 4);
    const size_t w1 = dmpnn_linear_wgrad_ws_bytes(a.n_atoms, L.D, L.D, 1), w0 = dmpnn_linear_wgrad_ws_bytes(a.n_atoms, L.D, L.D, 0);
    L.wgrad = o; L.wgrad_bytes = al256(w1 > w0 ? w1 : w0);   // (with or without gb_d: the product's plan differs)
    L.total = o + L.wgrad_bytes;
    return L;
}

// every check of both entry points (before any device work); bwd: the backward's fields as well
static int vd_check(const dmpnn_vd_args* a, bool bwd) {
    DMPNN_CHECK_ARG(a != nullptr, "vd: null args");
    DMPNN_CHECK_ARG(a->n_atoms >= 0 && a->d_h >= 1, "vd: bad sizes (n_atoms %lld, d_h %lld)", (long long)a->n_atoms, (long long)a->d_h);
    DMPNN_CHECK_ARG(a->d_vd >= 1, "vd: d_vd (%lld) must be >= 1", (long long)a->d_vd);
    DMPNN_CHECK_ARG(a->d_h + a->d_vd <= DMPNN_VD_MAX_WIDTH, "vd: d_h + d_vd = %lld is beyond the %d columns this layer takes",
                    (long long)(a->d_h + a->d_vd), DMPNN_VD_MAX_WIDTH);
    DMPNN_CHECK_ARG(a->n_atoms < (int64_t(1) << 31) - 64, "vd: too many atoms");
    DMPNN_CHECK_ARG(a->dropout_p >= 0.f && a->dropout_p < 1.f, "vd: dropout_p (%g) must be in [0, 1)", (double)a->dropout_p);
    const bool rows = a->n_atoms > 0;   // (a batch without atoms has no row tensors to point at)
    DMPNN_CHECK_ARG(a->W_d && (!rows || (a->Hv && a->V_d)), "vd: null Hv / V_d / W_d");
    DMPNN_CHECK_ARG(a->ldhv >= a->d_h && a->ldvd >= a->d_vd, "vd: a leading dimension below its width (ldhv %lld, ldvd %lld)",
                    (long long)a->ldhv, (long long)a->ldvd);
    if (!bwd) {
        DMPNN_CHECK_ARG(a->b_d && (!rows || a->out), "vd forward: null b_d / out");
        DMPNN_CHECK_ARG(a->ldout >= a->d_h + a->d_vd, "vd forward: ldout (%lld) below d_h + d_vd", (long long)a->ldout);
    } else {
        DMPNN_CHECK_ARG(!rows || (a->gout && a->gHv), "vd backward: null gout / gHv");
        DMPNN_CHECK_ARG(a->ldgout >= a->d_h + a->d_vd && a->ldghv >= a->d_h, "vd backward: a leading dimension below its width (ldgout %lld, ldghv %lld)",
                        (long long)a->ldgout, (long long)a->ldghv);
    }
    DMPNN_CHECK_ARG(a->ws != nullptr && (reinterpret_cast<uintptr_t>(a->ws) & 15u) == 0, "vd: null or unaligned workspace");
    const VdLayout L = vd_layout(*a);
    if (a->ws_bytes < L.total) {
        set_error("vd: workspace too small (%zu < %zu bytes)", a->ws_bytes, L.total);
        return DMPNN_ENOSPC;
    }
    return DMPNN_OK;
}

static int vd_split(const dmpnn_vd_args& a, const VdLayout& L, hipStream_t s) {
    unsigned char* ws = static_cast<unsigned char*>(a.ws);
    VdSplit sp{a.W_d, L.D, L.Dp, reinterpret_cast<_Float16*>(ws + L.wh), reinterpret_cast<_Float16*>(ws + L.wl), reinterpret_cast<float*>(ws + L.inv)};
    hipLaunchKernelGGL(k_vd_split, dim3((unsigned)((L.Dp + 3) / 4)), dim3(256), 0, s, sp);
    DMPNN_CHECK_LAUNCH("k_vd_split");
    return DMPNN_OK;
}

// the mask of dmpnn_vd_args.dropout_p into the kernel's arguments; false: no mask (p == 0, or so small that floor(p 2^32) == 0)
static bool vd_drop(const dmpnn_vd_args& a, VdK& k) {
    if (!(a.dropout_p > 0.f) || drop_threshold(a.dropout_p) == 0u) return false;
    k.drop_thr = drop_threshold(a.dropout_p); k.drop_scale = 1.f / (1.f - a.dropout_p);
    k.seed_lo = (unsigned)(a.dropout_seed & 0xFFFFFFFFull); k.seed_hi = (unsigned)(a.dropout_seed >> 32);
    return true;
}

template <bool TR, bool DROP>
static int vd_launch(const VdK& k, hipStream_t s) {
    constexpr int BM = kRowTile * RT;
    const int K = k.K1 + k.K2, Kp = (K + 31) & ~31, Np = (k.N + 15) & ~15;
    const size_t lds = vd_lds_bytes(Kp, Np, TR, BM);
    // (the most dynamic LDS a workgroup may ask for: an attribute of the kernel on ONE device — set once per instantiation and device)
    static bool attr[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || !attr[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vd_gemm<TR, DROP>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) {
            set_error("hipFuncSetAttribute(k_vd_gemm): %s", hipGetErrorString(e));
            return DMPNN_EHIP;
        }
        if (dev >= 0 && dev < 64) attr[dev] = true;
    }
    hipLaunchKernelGGL((k_vd_gemm<TR, DROP>), dim3((unsigned)((k.M + BM - 1) / BM)), dim3(256), lds, s, k);
    DMPNN_CHECK_LAUNCH(TR ? "k_vd_gemm<dgrad>" : "k_vd_gemm<fwd>");
    return DMPNN_OK;
}
}  // namespace vd

int vd_check_args(const dmpnn_vd_args* a, bool bwd) { return vd::vd_check(a, bwd); }

int vd_forward_impl(const dmpnn_vd_args* a, void* stream) {
    DMPNN_TRY(vd::vd_check(a, false));
    if (a->n_atoms == 0) return DMPNN_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const vd::VdLayout L = vd::vd_layout(*a);
    DMPNN_TRY(vd::vd_split(*a, L, s));
    unsigned char* ws = static_cast<unsigned char*>(a->ws);
    vd::VdK k;
    memset(&k, 0, sizeof(k));
    k.M = (int)a->n_atoms; k.K1 = (int)a->d_h; k.K2 = (int)a->d_vd; k.N = L.D;
    k.A1 = a->Hv; k.lda1 = a->ldhv; k.A2 = a->V_d; k.lda2 = a->ldvd;
    k.Wh = reinterpret_cast<const _Float16*>(ws + L.wh); k.Wl = reinterpret_cast<const _Float16*>(ws + L.wl); k.Dp = L.Dp;
    k.nscale = reinterpret_cast<const float*>(ws + L.inv); k.bias = a->b_d;
    k.C = a->out; k.ldc = a->ldout;
    return vd::vd_drop(*a, k) ? vd::vd_launch<false, true>(k, s) : vd::vd_launch<false, false>(k, s);
}

// split_ready: the workspace still holds this step's image of W_d (dmpnn_train_step: the forward ran in the same call)
int vd_backward_impl(const dmpnn_vd_args* a, void* stream, bool split_ready) {
    DMPNN_TRY(vd::vd_check(a, true));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const vd::VdLayout L = vd::vd_layout(*a);
    const int64_t D = L.D;
    if (a->n_atoms == 0) {
        hipError_t e = hipSuccess;
        if (a->gW_d) e = hipMemsetAsync(a->gW_d, 0, (size_t)(D * D) * sizeof(float), s);
        if (a->gb_d && e == hipSuccess) e = hipMemsetAsync(a->gb_d, 0, (size_t)D * sizeof(float), s);
        if (e != hipSuccess) {
            set_error("vd backward: hipMemsetAsync: %s", hipGetErrorString(e));
            return DMPNN_EHIP;
        }
        return DMPNN_OK;
    }
    unsigned char* ws = static_cast<unsigned char*>(a->ws);
    if (!split_ready) DMPNN_TRY(vd::vd_split(*a, L, s));
    vd::VdK k;
    memset(&k, 0, sizeof(k));
    k.M = (int)a->n_atoms; k.K1 = (int)D; k.K2 = 0; k.N = (int)a->d_h;
    k.A1 = a->gout; k.lda1 = a->ldgout;
    k.kscale = reinterpret_cast<const float*>(ws + L.inv);
    k.Wh = reinterpret_cast<const _Float16*>(ws + L.wh); k.Wl = reinterpret_cast<const _Float16*>(ws + L.wl); k.Dp = L.Dp;
    k.C = a->gHv; k.ldc = a->ldghv;
    if (vd::vd_drop(*a, k)) {   // (gout leaves the launch as the masked gradient: what the weight gradient below reads)
        k.A1w = const_cast<float*>(a->gout);
        DMPNN_TRY((vd::vd_launch<true, true>(k, s)));
    } else {
        DMPNN_TRY((vd::vd_launch<true, false>(k, s)));
    }
    if (a->gW_d || a->gb_d) {
        dmpnn_gemm_args g;
        memset(&g, 0, sizeof(g));
        g.M = a->n_atoms; g.N = D; g.K1 = a->d_h; g.K2 = a->d_vd;
        g.A1 = a->Hv; g.lda1 = a->ldhv; g.A2 = a->V_d; g.lda2 = a->ldvd;
        DMPNN_TRY(dmpnn_linear_wgrad(&g, a->gout, a->ldgout, a->gW_d, D, a->gb_d, ws + L.wgrad, L.wgrad_bytes, stream));
    }
    return DMPNN_OK;
}

}  // namespace dmpnn

using namespace dmpnn;

extern "C" {

size_t dmpnn_vd_ws_bytes(const dmpnn_vd_args* a) {
    if (!a || a->d_h < 1 || a->d_vd < 1 || a->n_atoms < 0 || a->d_h + a->d_vd > DMPNN_VD_MAX_WIDTH) return 0;
    return vd::vd_layout(*a).total;
}
int dmpnn_vd_forward(const dmpnn_vd_args* a, void* stream) { return vd_forward_impl(a, stream); }
int dmpnn_vd_backward(const dmpnn_vd_args* a, void* stream) { return vd_backward_impl(a, stream, false); }

}  // extern "C"
