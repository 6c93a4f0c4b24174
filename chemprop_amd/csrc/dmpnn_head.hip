// f4: what chemprop.models.MPNN does AFTER the message-passing block in a training step, as kernels chained
// by ONE C call — and the whole step (K0 + forward + this + backward + optimizer) as one more (dmpnn_train_step):
//
//     H   = agg(H_v, batch)                     models/model.py:131      nn/agg.py:66-113     (dmpnn_molagg_*)
//     Z   = bn(H)                               models/model.py:132      nn.BatchNorm1d, batch statistics in training
//     P   = ffn(Z)                              models/model.py:146,155  nn/ffn.py:24-68, nn/predictors.py:161-169
//     l   = sum(L w_i t_j mask) / sum(mask)     models/model.py:156      nn/metrics.py:78-127 (MSE :137-141, MAE :146-148,
//                                                                         bounded variants :157-163)
// and the gradients of l with respect to every parameter above and to H_v (the `gout` of dmpnn_backward).
//
// The reference runs this as ~60 ATen launches from Python (forward + autograd); at 512 molecules every one of them is
// launch latency.  Here: segment reduction, one batch-norm kernel, one fp32-MFMA contraction per layer (activation fused),
// one loss kernel that also emits dl/dP; backward: per layer one weight-gradient product (+ reduce), one transposed
// contraction with the activation derivative fused into a small elementwise pass, one batch-norm kernel, one gather.
#include "dmpnn_head_kernels.hpp"   // (every kernel this file launches, their argument structs and size constants)

namespace dmpnn {
namespace {

struct HeadLayout {
    size_t bounds, Hm, Z, mean, invstd, act[DMPNN_MAX_FFN_LAYERS], gP, gA, gB, Wt, wgrad, gHm, total;
    size_t Zx;                             // with molecule descriptors: the fingerprint cat(bn(H), X_d) [B, Kp] (zero-padded to Kp)
    int64_t Kp;
    size_t wgrad_bytes;
    int64_t maxd;
    // the four-launch form (rows_shape): the hidden layer's split weight in both orientations, their row scales, the row kernel's partials
    size_t W0f, W0b, isf, isb, part;
    int part_stride, n_part;
    // agg_mode == DMPNN_MOLAGG_ATTENTIVE (behind everything else: the other offsets do not move): the aggregate A [B, d] and its gradient,
    // the batch vector of B one-atom molecules, the bounds table of the real batch, the kept s [n_atoms] | Z [B], the attention's own scratch
    size_t att_A, att_gA, att_idb, att_bounds, att_s, att_Z, att_ws, att_ws_bytes;
    // the spectral criteria (in front of the attentive part: the inner head's layout stays the front of the outer one): per row the
    // loss and the count of finite targets, k_spectral_rows to k_spectral_finish
    size_t spec_loss, spec_cnt;
    // the binary MCC criterion (in front of the attentive part as well): per block of kMccRows molecule rows the four sums of every task
    // [n_blocks][4][t] and per (row block, column block) the count of finite targets, k_mcc_cols to k_mcc_finish
    size_t mcc_part, mcc_cnt;
    int mcc_blocks, mcc_cb;
};
inline bool spectral_loss(int loss) { return loss == DMPNN_LOSS_SID || loss == DMPNN_LOSS_WASSERSTEIN; }
// the criteria that run as a stage of their own (head_criterion) and not in k_loss — so not inside k_out_all's launch either
inline bool staged_loss(int loss) { return spectral_loss(loss) || loss == DMPNN_LOSS_MCC; }
// the shapes the four-launch form takes (training or not is the caller's business): one hidden layer, a handful of outputs
// (with molecule descriptors the first layer's reduction may be up to kRowsMaxK wide: d_h + d_xd; its data gradient stays d_h wide)
// components of a multicomponent fingerprint (dmpnn_head_args.n_components: 0 and 1 are one block)
inline int64_t head_ncomp(const dmpnn_head_args& h) { return h.n_components > 1 ? h.n_components : 1; }
// (loss <= DMPNN_LOSS_BCE: k_head_rows evaluates the per-element criteria MSE / MAE / BCE itself — which keeps DMPNN_LOSS_MCC, a
//  reduction down the columns, out of this form as it keeps the spectral criteria out)
bool rows_shape(const dmpnn_head_args& h) {
    return h.n_layers == 2 && h.dims[2] <= kOutMaxTasks && h.dims[2] >= 1 && h.loss <= DMPNN_LOSS_BCE && h.n_mols <= kRowsMaxB &&
           h.dims[0] <= (h.X_d ? kRowsMaxK : kRowsMaxWidth) && head_ncomp(h) * h.d_h <= kRowsMaxWidth && h.dims[1] <= kRowsMaxWidth && h.dims[0] % 4 == 0;
}
HeadLayout head_layout(const dmpnn_head_args& h) {
    HeadLayout L;
    memset(&L, 0, sizeof(L));
    // d: the width of the block part of the fingerprint (n_components d_h); the bounds table covers every component's molecules
    const int64_t B = h.n_mols > 0 ? h.n_mols : 0, d = head_ncomp(h) * h.d_h;
    size_t o = 0;
    L.bounds = o; o += al256(dmpnn_molagg_ws_bytes(head_ncomp(h) * B));
    L.Hm = o; o += al256((size_t)B * d * 4);
    L.Z = o; o += al256(h.bn_weight ? (size_t)B * d * 4 : 0);
    L.mean = o; o += al256((size_t)d * 4);
    L.invstd = o; o += al256((size_t)d * 4);
    L.Kp = h.X_d ? (h.dims[0] + 3) & ~int64_t(3) : d;
    L.Zx = o; o += al256(h.X_d ? (size_t)B * L.Kp * 4 : 0);
    int64_t maxd = h.X_d && L.Kp > d ? L.Kp : d;   // (the chain's scratch for layer 0: its data gradient [B, Kp], its unwanted weight gradient)
    for (int l = 0; l < h.n_layers; ++l) {
        if (h.dims[l + 1] > maxd) maxd = h.dims[l + 1];
        L.act[l] = o;
        if (l + 1 < h.n_layers) o += al256((size_t)B * h.dims[l + 1] * 4);   // (the last layer writes `preds`)
    }
    L.maxd = maxd;
    const int64_t t = h.n_layers > 0 ? h.dims[h.n_layers] : d;
    L.gP = o; o += al256((size_t)B * t * 4);
    L.gA = o; o += al256((size_t)B * maxd * 4);
    L.gB = o; o += al256((size_t)B * maxd * 4);
    L.Wt = o; o += al256((size_t)maxd * maxd * 4);
    size_t wg = 0;
    for (int l = 0; l < h.n_layers; ++l) {
        const size_t b = dmpnn_linear_wgrad_ws_bytes(B, h.dims[l + 1], h.dims[l], 1);
        if (b > wg) wg = b;
    }
    if (h.n_layers > 0) {  // (the first layer's weight gradient may ride in the block's backward launches: its split operands + slabs)
        const size_t b = extra_wgrad_ws_floats(B, (int)h.dims[1], (int)h.dims[0] + 1) * sizeof(float);
        if (b > wg) wg = b;
    }
    L.wgrad = o; L.wgrad_bytes = al256(wg); o += L.wgrad_bytes;
    L.gHm = o; o += al256((size_t)B * d * 4);
    if (h.n_layers == 2 && rows_shape(h)) {
        const int64_t N = h.dims[1], K = h.dims[0], t = h.dims[2];
        L.W0f = o; o += al256((size_t)((N + 15) / 16) * ((K + 31) / 32) * 2048);
        L.W0b = o; o += al256((size_t)((d + 15) / 16) * ((N + 31) / 32) * 2048);   // (the backward orientation: the first d_h columns)
        L.isf = o; o += al256((size_t)N * 4);
        L.isb = o; o += al256((size_t)K * 4);
        L.n_part = (int)((B + 15) / 16);
        L.part_stride = (int)(t * N + t + 2);
        L.part = o; o += al256((size_t)L.n_part * L.part_stride * 4);
    }
    if (spectral_loss(h.loss)) {
        L.spec_loss = o; o += al256((size_t)B * 4);
        L.spec_cnt = o; o += al256((size_t)B * 4);
    }
    if (h.loss == DMPNN_LOSS_MCC) {
        const int64_t tc = t > 0 ? t : 0;
        L.mcc_blocks = (int)(B > kMccRows ? (B + kMccRows - 1) / kMccRows : 1);
        L.mcc_cb = (int)(tc > kMccThreads ? (tc + kMccThreads - 1) / kMccThreads : 1);
        L.mcc_part = o; o += al256((size_t)L.mcc_blocks * tc * 4 * 4);
        L.mcc_cnt = o; o += al256((size_t)L.mcc_blocks * L.mcc_cb * 4);
    }
    if (h.agg_mode == DMPNN_MOLAGG_ATTENTIVE) {
        const int64_t nV = h.n_atoms > 0 ? h.n_atoms : 0;
        L.att_A = o; o += al256((size_t)B * d * 4);
        L.att_gA = o; o += al256((size_t)B * d * 4);
        L.att_idb = o; o += al256((size_t)B * 8);
        L.att_bounds = o; o += al256(dmpnn_molagg_ws_bytes(B));
        L.att_s = o; o += al256((size_t)nV * 4);
        L.att_Z = o; o += al256((size_t)B * 4);
        dmpnn_molagg_attn_args q;
        memset(&q, 0, sizeof(q));
        q.n_mols = B; q.d_h = d; q.bounds = &q;   // (a table is given: the partial rows alone)
        L.att_ws_bytes = dmpnn_molagg_attn_ws_bytes(&q);
        L.att_ws = o; o += al256(L.att_ws_bytes);
    }
    L.total = o;
    return L;
}

}  // namespace
}  // namespace dmpnn

using namespace dmpnn;

extern "C" {

size_t dmpnn_head_ws_bytes(const dmpnn_head_args* h) {
    if (!h || h->n_layers < 0 || h->n_layers > DMPNN_MAX_FFN_LAYERS || h->d_h <= 0 || h->n_components < 0 || h->n_components > DMPNN_MAX_COMPONENTS) return 0;
    return head_layout(*h).total;
}

}  // extern "C"

namespace {
inline unsigned char* ws_at(const dmpnn_head_args& h, size_t off) { return static_cast<unsigned char*>(h.ws) + off; }
inline float* ws_f(const dmpnn_head_args& h, size_t off) { return reinterpret_cast<float*>(ws_at(h, off)); }

// outputs per task of an output transform and of a criterion
int transform_per_task(int transform, int n_classes) {
    if (transform == DMPNN_PT_DIRICHLET_BINARY || transform == DMPNN_PT_DIRICHLET_MULTICLASS) return n_classes;
    return transform == DMPNN_PT_SOFTMAX ? n_classes : (transform == DMPNN_PT_EVIDENTIAL ? 4 : ((transform == DMPNN_PT_MVE || transform == DMPNN_PT_QUANTILE) ? 2 : 1));
}
int loss_per_task(const dmpnn_head_args& h) {
    return (h.loss == DMPNN_LOSS_CE || h.loss == DMPNN_LOSS_DIRICHLET) ? h.n_classes : (h.loss == DMPNN_LOSS_EVIDENTIAL ? 4 : ((h.loss == DMPNN_LOSS_MVE || h.loss == DMPNN_LOSS_QUANTILE) ? 2 : 1));
}

// the criterion is one this library knows: a value of enum dmpnn_loss — and no class dimension beside the spectral criteria, whose one
// output per task is a bin of the spectrum (with n_classes set, 8 / 9 name nothing: older callers probe 8 as the first unknown value)
// DMPNN_LOSS_MCC = 11 likewise; 10 names nothing (probed as the first unknown value since the spectral criteria)
inline bool known_criterion(const dmpnn_head_args& h) {
    if (h.loss == DMPNN_LOSS_MCC) return h.n_classes == 0;
    return h.loss >= DMPNN_LOSS_MSE && h.loss <= DMPNN_LOSS_WASSERSTEIN && !(spectral_loss(h.loss) && h.n_classes != 0);
}
// every argument rule of dmpnn_head (head_attentive: its own, then these on the head behind the attention), before the workspace rule
int head_check(const dmpnn_head_args& h, const float* Hv, int64_t ldhv) {
    DMPNN_CHECK_ARG(h.n_components >= 0 && h.n_components <= DMPNN_MAX_COMPONENTS, "head: n_components (%d) outside 0..%d", (int)h.n_components,
                    DMPNN_MAX_COMPONENTS);
    DMPNN_CHECK_ARG(h.ffn_dropout_p >= 0.f && h.ffn_dropout_p < 1.f, "head: ffn_dropout_p (%g) outside [0, 1)", (double)h.ffn_dropout_p);
    // a multicomponent fingerprint: ncomp blocks of dc columns each, side by side (d = ncomp dc); the table of molecule bounds covers nBt
    const int64_t dc = h.d_h, d = head_ncomp(h) * dc, B = h.n_mols, nV = h.n_atoms;
    const int Ln = h.n_layers;
    DMPNN_CHECK_ARG(B >= 0 && nV >= 0 && dc > 0 && ldhv >= dc, "head: bad sizes");
    DMPNN_CHECK_ARG(Ln >= 1 && Ln <= DMPNN_MAX_FFN_LAYERS, "head: 1..%d predictor layers", DMPNN_MAX_FFN_LAYERS);
    // molecule descriptors: the predictor's input is cat(bn(agg(H_v)), X_d), dims[0] = d_h + d_xd
    const bool xd = h.X_d != nullptr;
    DMPNN_CHECK_ARG(xd ? h.dims[0] > d : h.dims[0] == d, xd ? "head: with X_d, dims[0] = n_components d_h + d_xd > n_components d_h"
                                                           : "head: dims[0] == d_h (times n_components) without X_d");
    DMPNN_CHECK_ARG(!xd || h.ld_xd >= h.dims[0] - d, "head: ld_xd (%lld) < d_xd (%lld)", (long long)h.ld_xd, (long long)(h.dims[0] - d));
    for (int l = 0; l < Ln; ++l) DMPNN_CHECK_ARG(h.W[l] && h.dims[l + 1] > 0, "head: layer %d has no weight / width", l);
    DMPNN_CHECK_ARG(h.act >= DMPNN_ACT_NONE && h.act <= DMPNN_ACT_SELU && h.act != DMPNN_ACT_PRELU, "head: activation %d is not built in", h.act);
    DMPNN_CHECK_ARG(known_criterion(h), "head: unknown criterion %d (n_classes %d)", h.loss, (int)h.n_classes);
    DMPNN_CHECK_ARG(h.loss <= DMPNN_LOSS_MAE || (!h.lt_mask && !h.gt_mask), "head: only the MSE / MAE criteria have bounds (lt_mask / gt_mask)");
    if (spectral_loss(h.loss)) {
        DMPNN_CHECK_ARG(h.spectral_act == 0 || h.spectral_act == 1, "head: unknown spectral_act %d (0 softplus, 1 exp)", (int)h.spectral_act);
        DMPNN_CHECK_ARG(std::isfinite(h.spectral_threshold) && h.spectral_threshold >= 0.f, "head: spectral_threshold (%g) must be finite and >= 0 (0: none)",
                        (double)h.spectral_threshold);
    }
    DMPNN_CHECK_ARG((h.loss != DMPNN_LOSS_MVE && h.loss != DMPNN_LOSS_QUANTILE) || h.dims[Ln] % 2 == 0, "head: the MVE / quantile criteria need an output layer 2 n_tasks wide");
    DMPNN_CHECK_ARG(h.loss != DMPNN_LOSS_QUANTILE || (h.quantile_alpha > 0.f && h.quantile_alpha < 1.f), "head: the quantile criterion needs 0 < quantile_alpha < 1");
    DMPNN_CHECK_ARG(h.loss != DMPNN_LOSS_EVIDENTIAL || h.dims[Ln] % 4 == 0, "head: the evidential criterion needs an output layer 4 n_tasks wide");
    DMPNN_CHECK_ARG(h.loss != DMPNN_LOSS_CE || (h.n_classes >= 2 && h.dims[Ln] % h.n_classes == 0), "head: cross entropy needs n_classes >= 2 dividing the output width");
    DMPNN_CHECK_ARG(h.loss != DMPNN_LOSS_DIRICHLET || (h.n_classes >= 2 && h.dims[Ln] % h.n_classes == 0), "head: the Dirichlet criterion needs n_classes >= 2 dividing the output width");
    DMPNN_CHECK_ARG(h.preds && (nV == 0 || (Hv && h.batch)), "head: null H_v / batch / preds");
    DMPNN_CHECK_ARG(!h.bn_weight || (h.bn_running_mean && h.bn_running_var), "head: batch norm without running statistics");
    // (torch.nn.BatchNorm1d in training mode — hence the reference — raises "Expected more than 1 value per channel": a batch of one
    //  molecule has no variance, and the output would silently be beta)
    DMPNN_CHECK_ARG(!(h.bn_weight && h.bn_training) || B != 1, "head: batch norm in training mode needs more than 1 molecule per batch");
    DMPNN_CHECK_ARG(!h.gHv || (h.targets && h.loss_out && h.ldg >= dc), "head: gradients need targets, loss_out and ldg >= d_h");
    return DMPNN_OK;
}
// the workspace rule, behind the argument rules: there, large enough for the layout L, 16-byte aligned.  who: "head" | "predict_head"
int head_ws_check(const dmpnn_head_args& h, const HeadLayout& L, const char* who) {
    if (!h.ws || h.ws_bytes < L.total) {
        set_error("%s: workspace missing or too small (%zu < %zu bytes)", who, h.ws_bytes, L.total);
        return DMPNN_ENOSPC;
    }
    DMPNN_CHECK_ARG(aligned16(h.ws), "head: workspace must be 16-byte aligned");
    return DMPNN_OK;
}

// ---- the route of one call -----------------------------------------------------------------------------------------------------------
// What a whole training step did in front of the head.  bounds_done: K0 wrote the bounds table (attentive: the REAL batch's, at att_bounds).
// agg_rode: the forward tile kernel wrote the aggregate of the molecules it carried into the workspace's H and marked them in done[] (AggRide)
struct HeadPre { bool bounds_done, agg_rode; };
// Which kernels a call takes: decided once per call by head_route, the only reader of DMPNN_HEAD, DMPNN_HEAD_AGG and DMPNN_HEAD_QPW — on
// every call: tests flip them inside one process
struct HeadRoute {
    bool cols_fused;           // the column kernels k_agg_bn_fwd / k_bn_agg_bwd take aggregation and batch norm (else the chain's kernels)
    bool want_rows, rows;      // DMPNN_HEAD=rows (tests: a training call that takes the chain is an error, not a silent chain); the four-launch form
    bool own_bounds;           // the inference head: the column kernel takes the bounds from the batch vector itself — no table, two launches less
    bool fuse_agg;             // the aggregation inside k_agg_bn_fwd (else dmpnn_molagg_fwd — every CU — runs in front)
    int qpw;                   // quads per workgroup of the column kernels
    bool small_out, out_all;   // the output layer as dot products (k_out_fwd / k_out_bwd); its backward and the criterion as ONE launch (k_out_all)
    bool agg_may_ride;         // dmpnn_train_step: the aggregate may leave with the forward tile kernel's tiles (head_ride_slots)
    HeadPre pre;
};
// predict: the inference head (dmpnn_predict_head), which alone goes without a bounds table
HeadRoute head_route(const dmpnn_head_args& h, const float* Hv, int64_t ldhv, HeadPre pre, bool predict) {
    const char *head_env = getenv("DMPNN_HEAD"), *agg_env = getenv("DMPNN_HEAD_AGG"), *qpw_env = getenv("DMPNN_HEAD_QPW");
    const bool chain = head_env && !strcmp(head_env, "chain"), want_grad = h.gHv != nullptr;
    const int64_t B = h.n_mols, nV = h.n_atoms;
    const int Ln = h.n_layers;
    HeadRoute R{};
    R.pre = pre;
    // the column kernels move 16-byte quads: widths and strides in multiples of 4 floats, 16-byte aligned rows (a multicomponent
    // fingerprint: a quad must not straddle two components — d_h % 4 == 0 — or the chain takes it)
    R.cols_fused = !chain && B <= kRowsMaxB && nV > 0 && h.d_h % 4 == 0 && ldhv % 4 == 0 && aligned16(Hv) &&
                   (!want_grad || (h.ldg % 4 == 0 && aligned16(h.gHv))) && (int64_t)nV * ldhv < (1ll << 29) &&
                   (!h.bn_weight || (aligned16(h.bn_weight) && aligned16(h.bn_bias) && aligned16(h.bn_running_mean) && aligned16(h.bn_running_var) &&
                                     (!h.g_bn_weight || aligned16(h.g_bn_weight)) && (!h.g_bn_bias || aligned16(h.g_bn_bias))));
    R.want_rows = head_env && !strcmp(head_env, "rows");
    R.rows = R.cols_fused && want_grad && h.targets && rows_shape(h) && aligned16(h.W[0]);
    R.own_bounds = predict && !pre.bounds_done && R.cols_fused && head_ncomp(h) * B <= kOwnBoundsMols;
    // the aggregation inside the column kernel's launch up to 512 molecules (one launch less: 159 against 166 us per step at 64 molecules,
    // 221 against 220 at 512 — the column workgroups pull H_v at ~55 GB/s each, 5.5 MB over 38 of them); beyond that dmpnn_molagg_fwd runs
    // in front (DMPNN_HEAD_AGG=fused | split: the A/B switch).  (rode: only what the tile kernel left is summed there)
    R.fuse_agg = pre.agg_rode || R.own_bounds || (agg_env ? !strcmp(agg_env, "fused") : B <= kFuseAggMols);
    // (4, 1 molecule per thread) up to 256 molecules, (2, 1) up to 512, (2, 2) up to 1 024 (DMPNN_HEAD_QPW=4 | 2: the A/B switch)
    R.qpw = (qpw_env && !strcmp(qpw_env, "4")) ? 4 : ((qpw_env && !strcmp(qpw_env, "2")) ? 2 : (B <= 256 ? 4 : 2));
    R.small_out = Ln >= 1 && Ln <= DMPNN_MAX_FFN_LAYERS && h.dims[Ln] <= kOutMaxTasks;
    R.out_all = R.small_out && want_grad && h.targets && B <= kOutAllMaxRows && loss_per_task(h) == 1 && !staged_loss(h.loss);   // (k_loss's criteria)
    // The ride's own conditions — NOT cols_fused: no alignment terms.  (with descriptors and no batch norm the aggregate goes into the fingerprint's
    // rows, not into H; the attentive aggregate needs every atom's logit first; DMPNN_HEAD_AGG=fused | split switches the ride off)
    R.agg_may_ride = h.agg_mode != DMPNN_MOLAGG_ATTENTIVE && B <= kRowsMaxB && h.d_h % 4 == 0 && !chain && (!h.X_d || h.bn_weight) &&
                     !(agg_env && strcmp(agg_env, "tile"));
    return R;
}
// dmpnn_train_step's one question: where in this head's workspace (NULL: too small) do the bounds table K0 fills on the side (attentive:
// the REAL batch's, at att_bounds) and H live, and may the aggregate ride with the forward tile kernel?
struct HeadRideSlots { int* bounds; float* Hm; bool may_ride; };
HeadRideSlots head_ride_slots(const dmpnn_head_args& h, const float* Hv, int64_t ldhv) {
    const HeadLayout L = head_layout(h);
    if (!h.ws || h.ws_bytes < L.total) return HeadRideSlots{nullptr, nullptr, false};
    return HeadRideSlots{reinterpret_cast<int*>(ws_at(h, h.agg_mode == DMPNN_MOLAGG_ATTENTIVE ? L.att_bounds : L.bounds)), ws_f(h, L.Hm),
                         head_route(h, Hv, ldhv, HeadPre{false, false}, false).agg_may_ride};
}
#define DMPNN_COL_LAUNCH(KERNEL, QPW_V, B_V, BN_V, GRID, STREAM, ARGS)                                                   \
    do {                                                                                                                \
        const int rr_ = (int)(((B_V) * (QPW_V) + 1023) / 1024);                                                          \
        if ((QPW_V) == 4 && rr_ <= 1) { if (BN_V) hipLaunchKernelGGL((KERNEL<4, 1, true>), GRID, dim3(1024), 0, STREAM, ARGS); else hipLaunchKernelGGL((KERNEL<4, 1, false>), GRID, dim3(1024), 0, STREAM, ARGS); } \
        else if ((QPW_V) == 4 && rr_ <= 2) { if (BN_V) hipLaunchKernelGGL((KERNEL<4, 2, true>), GRID, dim3(1024), 0, STREAM, ARGS); else hipLaunchKernelGGL((KERNEL<4, 2, false>), GRID, dim3(1024), 0, STREAM, ARGS); } \
        else if ((QPW_V) == 4) { if (BN_V) hipLaunchKernelGGL((KERNEL<4, 4, true>), GRID, dim3(1024), 0, STREAM, ARGS); else hipLaunchKernelGGL((KERNEL<4, 4, false>), GRID, dim3(1024), 0, STREAM, ARGS); } \
        else if (rr_ <= 1) { if (BN_V) hipLaunchKernelGGL((KERNEL<2, 1, true>), GRID, dim3(1024), 0, STREAM, ARGS); else hipLaunchKernelGGL((KERNEL<2, 1, false>), GRID, dim3(1024), 0, STREAM, ARGS); } \
        else { if (BN_V) hipLaunchKernelGGL((KERNEL<2, 2, true>), GRID, dim3(1024), 0, STREAM, ARGS); else hipLaunchKernelGGL((KERNEL<2, 2, false>), GRID, dim3(1024), 0, STREAM, ARGS); } \
    } while (0)
// k_bn_fwd / k_bn_bwd: `reg`, the build that keeps a thread's rows in registers, up to kBnRegRows * kBnLanes molecules (the caller checks the launch)
template <class Args>
void launch_bn(void (*reg)(Args), void (*mem)(Args), const Args& a, hipStream_t s) {
    hipLaunchKernelGGL((a.B <= kBnRegRows * kBnLanes ? reg : mem), dim3((unsigned)((a.d + kBnCols - 1) / kBnCols)), dim3(1024), 0, s, a);
}
int launch_bn_agg_bwd(const BnAggBwdArgs& q, bool bn, int qpw, hipStream_t s) {
    const dim3 grid((unsigned)((q.b.d + 4 * qpw - 1) / (4 * qpw)) + (q.part ? 1u : 0u));   // (+ 1: the row kernels' partials)
    DMPNN_COL_LAUNCH(k_bn_agg_bwd, qpw, q.b.B, bn, grid, s, q);
    DMPNN_CHECK_LAUNCH("k_bn_agg_bwd");
    return DMPNN_OK;
}
// The front of a head call's forward, behind the bounds table: H = agg(H_v) [B, ldH], Z = bn(H) and the X_d columns — the predictor's
// input Z [B, ldz] — into the workspace.  R.cols_fused: ONE column kernel, in whose launch the hidden layer's weight split rides when
// `split` is given (the four-launch form); else the chain's kernels.  Shared by head_run and the inference head.
struct HeadFront { const float* Z; int64_t ldz; float* Hm; int64_t ldH; };
int head_front(const dmpnn_head_args& h, const HeadLayout& L, const HeadRoute& R, const float* Hv, int64_t ldhv, void* stream, const HeadSplit* split,
               HeadFront* out) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t ncomp = head_ncomp(h), dc = h.d_h;
    const int64_t B = h.n_mols, d = ncomp * dc, nV = h.n_atoms, nBt = ncomp * B;
    const bool xd = h.X_d != nullptr, bn = h.bn_weight != nullptr;
    // H = agg(H_v) [B, ldH] and bn(H) [B, ldY]; with descriptors bn(H) — or H itself without batch norm — is written straight into the
    // first d_h columns of the fingerprint Zx [B, Kp], whose other columns are X_d and zeros (XdFill)
    const int64_t Kp = L.Kp, ldH = (xd && !bn) ? Kp : d, ldY = xd ? Kp : d;
    float* Zx = xd ? ws_f(h, L.Zx) : nullptr;
    float* Hm = (xd && !bn) ? Zx : ws_f(h, L.Hm);
    float* Ybn = xd ? Zx : ws_f(h, L.Z);
    const XdFill xf{h.X_d, h.ld_xd, Zx, Kp, B, (int)d, (int)(Kp - d), (int)(h.dims[0] - d), 4096};
    const BnArgs b{Hm, ldH, Ybn, ldY, h.bn_weight, h.bn_bias, h.bn_running_mean, h.bn_running_var, ws_f(h, L.mean), ws_f(h, L.invstd),
                   B, (int)d, h.bn_eps, h.bn_momentum, h.bn_training, h.bn_num_batches_tracked};
    *out = bn ? HeadFront{Ybn, ldY, Hm, ldH} : HeadFront{Hm, ldH, Hm, ldH};
    if (R.cols_fused) {
        AggBnArgs q{};
        q.b = b;
        q.use_done = R.pre.agg_rode ? 1 : 0;
        if (!R.fuse_agg) DMPNN_TRY(molagg_fwd_rows(Hv, ldhv, nV, dc, nBt, ws_at(h, L.bounds), h.agg_mode, h.agg_norm, Hm, ldH, B, stream));
        q.Hv = R.fuse_agg ? Hv : nullptr; q.ldhv = ldhv; q.nV = nV; q.bounds = reinterpret_cast<const int*>(ws_at(h, L.bounds)); q.agg_mode = h.agg_mode; q.agg_norm = h.agg_norm;
        q.n_col_blocks = (int)((d + 4 * R.qpw - 1) / (4 * R.qpw));
        q.dbg = g_debug_stamps ? g_debug_stamps + 80 : nullptr;
        q.dh_c = (int)dc; q.nBt = nBt;
        q.batch = h.batch;
        if (split) q.split = *split;
        q.n_split_blocks = split ? split->ncb : 0;
        const int xd_blocks = xd ? xd_fill_blocks(xf) : 0;   // (the descriptor columns of Zx: the launch's last workgroups)
        q.xd = xf;
        const dim3 grid((unsigned)(q.n_col_blocks + q.n_split_blocks + xd_blocks));
        if (R.own_bounds) DMPNN_COL_LAUNCH(k_agg_bn_fwd_own_bounds, R.qpw, B, bn, grid, s, q);
        else if (R.fuse_agg || bn || q.n_split_blocks || xd_blocks) DMPNN_COL_LAUNCH(k_agg_bn_fwd, R.qpw, B, bn, grid, s, q);
        DMPNN_CHECK_LAUNCH("k_agg_bn_fwd");
        return DMPNN_OK;
    }
    DMPNN_TRY(molagg_fwd_rows(Hv, ldhv, nV, dc, nBt, ws_at(h, L.bounds), h.agg_mode, h.agg_norm, Hm, ldH, B, stream));
    if (xd) {
        hipLaunchKernelGGL(k_xd_fill, dim3((unsigned)xd_fill_blocks(xf)), dim3(1024), 0, s, xf);
        DMPNN_CHECK_LAUNCH("k_xd_fill");
    }
    if (bn) {
        launch_bn(k_bn_fwd<true>, k_bn_fwd<false>, b, s);
        DMPNN_CHECK_LAUNCH("k_bn_fwd");
    }
    return DMPNN_OK;
}
// PH 1 of the row kernel — a hidden layer tau(Z W0^T + b0) from its split image — by the widest row a wave holds; the caller checks the launch
void launch_head_rows_ph1(const RowsArgs& r, dim3 grid, int width, hipStream_t s) {
    if (width <= 128) hipLaunchKernelGGL((k_head_rows<2, 1>), grid, dim3(256), 0, s, r);
    else if (width <= kRowsMaxWidth) hipLaunchKernelGGL((k_head_rows<5, 1>), grid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL((k_head_rows<8, 1>), grid, dim3(256), 0, s, r);
}
// the grid of the elementwise kernels k_ffn_drop / k_head_act_bwd over n elements (grid-stride loops)
dim3 elementwise_grid(int64_t n) { return dim3((unsigned)(n > 1024 * 256 ? 1024 : (n + 255) / 256)); }
// layer l as a contraction call: tau(A W_l^T + b_l) into C   (sigma of the NEXT block fused here, ffn.py:49-58)
dmpnn_gemm_args ffn_layer(const dmpnn_head_args& h, int l, int64_t M, const float* A, int64_t lda, float* C) {
    dmpnn_gemm_args g{};
    g.M = M; g.N = h.dims[l + 1]; g.K1 = h.dims[l]; g.A1 = A; g.lda1 = lda;
    g.W = h.W[l]; g.ldw = h.dims[l]; g.bias = h.b[l];
    g.C = C; g.ldc = h.dims[l + 1]; g.act = h.act; g.act_slope = h.act_slope;
    return g;
}
// the criterion's argument block on raw outputs h.preds `ldp` wide, nc of them per task; gP (or NULL): where dl/dP goes, in rows of ldp
LossArgs loss_args(const dmpnn_head_args& h, int ldp, int nc, float* gP) {
    const int t = ldp / nc;   // tasks (= columns of `targets`)
    return LossArgs{h.preds, ldp, h.targets, t, h.weights, h.task_weights, h.lt_mask, h.gt_mask, gP, ldp, h.loss_out, h.n_mols, t, h.loss, nc,
                    h.evid_v_kl, h.evid_eps, h.quantile_alpha, h.loss == DMPNN_LOSS_DIRICHLET ? (float)std::lgamma((double)nc) : 0.f};
}
// the criterion of h.preds into loss_out, its gradient into gP (or NULL): one launch (the spectral criteria and binary MCC: their own
// stages, two launches each)
int head_criterion(const dmpnn_head_args& h, const HeadLayout& L, float* gP, hipStream_t s) {
    if (h.loss == DMPNN_LOSS_MCC) {
        const int64_t t = h.dims[h.n_layers];
        int lgC = 0;
        while ((1 << lgC) < kMccThreads && (1 << lgC) < t) ++lgC;   // (C: the smallest power of two >= min(t, kMccThreads))
        const MccArgs q{h.preds, t, h.targets, t, h.weights, h.task_weights, gP, t, h.loss_out, h.n_mols, (int)t, lgC, L.mcc_blocks, L.mcc_cb,
                        ws_f(h, L.mcc_part), reinterpret_cast<int*>(ws_at(h, L.mcc_cnt))};
        hipLaunchKernelGGL(k_mcc_cols, dim3((unsigned)((int64_t)L.mcc_blocks * L.mcc_cb)), dim3(kMccThreads), 0, s, q);
        DMPNN_CHECK_LAUNCH("k_mcc_cols");
        // (without a gradient: the sums alone, one workgroup; with one: a workgroup per row block up to kMccFinishMaxBlocks)
        const int fin = gP ? (L.mcc_blocks > kMccFinishMaxBlocks ? kMccFinishMaxBlocks : L.mcc_blocks) : 1;
        hipLaunchKernelGGL(k_mcc_finish, dim3((unsigned)fin), dim3(kMccThreads), 0, s, q);
        DMPNN_CHECK_LAUNCH("k_mcc_finish");
        return DMPNN_OK;
    }
    if (spectral_loss(h.loss)) {
        const int64_t t = h.dims[h.n_layers], n = h.n_mols * t;
        const SpectralArgs q{h.preds, t, h.targets, t, h.weights, h.task_weights, gP, t, h.loss_out, h.n_mols, (int)t, h.loss, h.spectral_act,
                             h.spectral_threshold, ws_f(h, L.spec_loss), reinterpret_cast<int*>(ws_at(h, L.spec_cnt))};
        hipLaunchKernelGGL(k_spectral_rows, dim3((unsigned)h.n_mols), dim3(kSpecCols), 0, s, q);
        DMPNN_CHECK_LAUNCH("k_spectral_rows");
        const int64_t blocks = gP ? (n + 4 * kSpecCols - 1) / (4 * kSpecCols) : 1;   // (four elements per thread; without a gradient: the sums alone)
        hipLaunchKernelGGL(k_spectral_finish, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(kSpecCols), 0, s, q);
        DMPNN_CHECK_LAUNCH("k_spectral_finish");
        return DMPNN_OK;
    }
    const LossArgs q = loss_args(h, (int)h.dims[h.n_layers], loss_per_task(h), gP);
    hipLaunchKernelGGL(k_loss, dim3(1), dim3(1024), 0, s, q);
    DMPNN_CHECK_LAUNCH("k_loss");
    return DMPNN_OK;
}
// Layer l's weight gradient gW[l] = gZ^T A and gb[l] = colsum(gZ): a product of its own.  defer (a whole training step, the FIRST layer):
// not launched but described in *defer — it rides in the block's backward launches (ExtraWgrad), its inputs stay in the workspace until then
int head_wgrad(const dmpnn_head_args& h, const HeadLayout& L, int l, const float* gZ, const float* A, int64_t lda, ExtraWgrad* defer, void* stream) {
    if (!h.gW[l] && !h.gb[l]) return DMPNN_OK;
    const int64_t N = h.dims[l + 1], K = h.dims[l];
    float* gb = h.b[l] ? h.gb[l] : nullptr;
    if (defer && l == 0 && h.gW[l] && N % 2 == 0 && K % 2 == 0) {
        *defer = ExtraWgrad{gZ, N, A, lda, h.n_mols, (int)N, (int)K, h.b[l] ? 1 : 0, h.gW[l], K, gb, ws_f(h, L.wgrad)};
        return DMPNN_OK;
    }
    dmpnn_gemm_args g{};
    g.M = h.n_mols; g.N = N; g.K1 = K; g.A1 = A; g.lda1 = lda;
    float* gw = h.gW[l] ? h.gW[l] : ws_f(h, L.Wt);   // (the product writes both; an unwanted one lands in scratch)
    return dmpnn_linear_wgrad(&g, gZ, N, gw, K, gb, ws_at(h, L.wgrad), L.wgrad_bytes, stream);
}
// The back end's block: q.b — batch norm backward on dl/dZ = gZ [B, d] (rows of ldgz) and H, no gX (k_bn_bwd: the caller sets it) —
// and the broadcast to the atoms' rows.  rows (the four-launch form): k_bn_agg_bwd also sums the row kernel's partials
BnAggBwdArgs bn_agg_bwd_args(const dmpnn_head_args& h, const HeadLayout& L, const HeadFront& fr, const float* gZ, int64_t ldgz, bool rows) {
    const int64_t d = head_ncomp(h) * h.d_h;
    BnAggBwdArgs q{};
    q.b = BnBwdArgs{gZ, ldgz, fr.Hm, fr.ldH, nullptr, d, h.bn_weight, ws_f(h, L.mean), ws_f(h, L.invstd), h.bn_running_mean, h.bn_running_var,
                    h.g_bn_weight, h.g_bn_bias, h.n_mols, (int)d, h.bn_eps, h.bn_training};
    q.gHv = h.gHv; q.ldg = h.ldg; q.bounds = reinterpret_cast<const int*>(ws_at(h, L.bounds)); q.nV = h.n_atoms; q.agg_mode = h.agg_mode; q.agg_norm = h.agg_norm;
    q.dh_c = (int)h.d_h; q.nBt = head_ncomp(h) * h.n_mols;
    if (!rows) return q;
    q.t = (int)h.dims[2] / loss_per_task(h); q.tN = q.t * (int)h.dims[1];
    q.part = ws_f(h, L.part); q.n_part = L.n_part; q.part_stride = L.part_stride;
    q.gW1 = h.gW[1]; q.gb1 = h.b[1] ? h.gb[1] : nullptr; q.loss_out = h.loss_out;
    q.dbg = g_debug_stamps ? g_debug_stamps + 96 : nullptr;
    return q;
}
// The four-launch form (round 5, see k_agg_bn_fwd) behind its front, in whose launch the hidden layer's split weight rode (head_split): the whole
// predictor + criterion + their backward as the row kernel's two launches, the hidden layer's weight gradient; the back end takes the partials
HeadSplit head_split(const dmpnn_head_args& h, const HeadLayout& L) {
    return HeadSplit{h.W[0], (int)h.dims[1], (int)h.dims[0], ws_at(h, L.W0f), ws_at(h, L.W0b), ws_f(h, L.isf), (int)((h.dims[0] + 31) / 32),
                     (int)((h.dims[1] + 31) / 32), (int)(head_ncomp(h) * h.d_h)};
}
int head_rows(const dmpnn_head_args& h, const HeadLayout& L, const HeadFront& fr, const HeadSplit& sp, ExtraWgrad* defer, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int N = (int)h.dims[1], K = (int)h.dims[0], t = (int)h.dims[2] / loss_per_task(h);
    const int Kg = (int)(head_ncomp(h) * h.d_h);   // dl/dZ: the first d_h columns (= K without descriptors)
    float* gA1 = ws_f(h, L.gA);
    RowsArgs r{fr.Z, fr.ldz, SplitW{sp.fwd, sp.inv_scale, sp.ncf}, SplitW{sp.bwd, ws_f(h, L.isb), sp.ncb}, h.b[0], h.W[1], h.b[1], ws_f(h, L.act[0]), h.preds, h.targets, h.weights, h.task_weights,
               h.lt_mask, h.gt_mask, h.loss, gA1, ws_f(h, L.gB), ws_f(h, L.part), L.part_stride, h.n_mols, N, K, t, h.act, h.act_slope,
               g_debug_stamps ? g_debug_stamps + 64 : nullptr, Kg, ffn_drop(h, 1)};
    // PH 1 reduces over K, PH 2 holds rows of N and forms Kg columns; without descriptors K == Kg and both take the wider of N, K
    const int widest = N > Kg ? N : Kg, w1 = h.X_d ? K : (N > K ? N : K);
    const dim3 g1((unsigned)L.n_part, (unsigned)((N + 63) / 64)), g2((unsigned)L.n_part, (unsigned)((widest + 63) / 64));
    launch_head_rows_ph1(r, g1, w1, s);
    if (r.dbg) r.dbg += 8;
    if (widest <= 128) hipLaunchKernelGGL((k_head_rows<2, 2>), g2, dim3(256), 0, s, r);
    else hipLaunchKernelGGL((k_head_rows<5, 2>), g2, dim3(256), 0, s, r);
    DMPNN_CHECK_LAUNCH("k_head_rows");
    return head_wgrad(h, L, 0, gA1, fr.Z, fr.ldz, defer, stream);
}
// The chain's layers read A[l] [B, dims[l]] in rows of chain_ld: A[0] = the fingerprint Z, A[l] = layer l - 1's activated (and masked) output
inline int64_t chain_ld(const dmpnn_head_args& h, const HeadFront& fr, int l) { return l == 0 ? fr.ldz : h.dims[l]; }
// the chain's forward, filling A: per layer one contraction with the activation fused (+ the dropout mask); R.small_out: the last as dot products
int head_chain_forward(const dmpnn_head_args& h, const HeadLayout& L, const HeadRoute& R, const HeadFront& fr, const float** A, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t B = h.n_mols;
    const int Ln = h.n_layers;
    A[0] = fr.Z;
    for (int l = 0; l < Ln; ++l) {
        if (R.small_out && l == Ln - 1) {
            OutFwdArgs q{A[l], chain_ld(h, fr, l), h.W[l], h.b[l], h.preds, B, (int)h.dims[l], (int)h.dims[Ln]};
            hipLaunchKernelGGL(k_out_fwd, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, q);
            DMPNN_CHECK_LAUNCH("k_out_fwd");
            A[l + 1] = h.preds;
            break;
        }
        float* out = l + 1 < Ln ? ws_f(h, L.act[l]) : h.preds;
        dmpnn_gemm_args g = ffn_layer(h, l, B, A[l], chain_ld(h, fr, l), out);
        if (l + 1 == Ln) g.act = DMPNN_ACT_NONE;
        DMPNN_TRY(dmpnn_linear_fwd(&g, stream));
        const FfnDrop dr = ffn_drop(h, l + 1);   // (the next layer's input: mask behind tau)
        if (dr.on) {
            hipLaunchKernelGGL(k_ffn_drop, elementwise_grid(B * h.dims[l + 1]), dim3(256), 0, s, out, h.dims[l + 1], B, (int)h.dims[l + 1], dr);
            DMPNN_CHECK_LAUNCH("k_ffn_drop");
        }
        A[l + 1] = out;
    }
    return DMPNN_OK;
}
// the chain's backward from dl/dP = gP (R.out_all: formed here, with the criterion, in the output layer's launch): per layer the weight
// gradient (head_wgrad) and the data gradient, down to *gZ [B, d]: the gradient w.r.t. the fingerprint's first d_h columns
struct HeadGradZ { const float* g; int64_t ld; };
int head_chain_backward(const dmpnn_head_args& h, const HeadLayout& L, const HeadRoute& R, const HeadFront& fr, const float* const* A, const float* gP,
                        ExtraWgrad* defer, HeadGradZ* gZ, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t B = h.n_mols, d = head_ncomp(h) * h.d_h;
    const int Ln = h.n_layers;
    float* bufs[2] = {ws_f(h, L.gA), ws_f(h, L.gB)};
    float* Wt = ws_f(h, L.Wt);
    const float* g_cur = gP;          // gradient w.r.t. the pre-activation of layer l's output
    int64_t ld_cur = h.dims[Ln];      // (its row stride)
    int pp = 0;
    for (int l = Ln - 1; l >= 0; --l) {
        const int64_t N = h.dims[l + 1], K = h.dims[l];
        // the data gradient of layer 0 is wanted for the block's d_h columns only (none flows to the descriptors)
        const int64_t Kout = l == 0 ? d : K, lda = chain_ld(h, fr, l);
        float* out = bufs[pp]; pp ^= 1;
        if (R.small_out && l == Ln - 1) {
            // (l == 0: no activation in front of the only layer — the derivative factor is 1; every column's gradient is formed, in rows of
            //  chain_ld(0) — Kp with descriptors, 16-byte rows for the column kernels)
            OutBwdArgs q{g_cur, A[l], lda, h.W[l], out, lda, h.gW[l], h.b[l] ? h.gb[l] : nullptr, B, (int)K, (int)N, l > 0 ? h.act : DMPNN_ACT_NONE, h.act_slope,
                         ffn_drop(h, l)};
            const dim3 grid((unsigned)((K + kBnCols - 1) / kBnCols));
            if (R.out_all) {
                OutAllArgs qa{q, loss_args(h, (int)N, 1, nullptr)};
                qa.l.v_kl = qa.l.eps = qa.l.q_alpha = 0.f;   // (its criteria, one output per task, have no constants: zeros as ever)
                qa.o.gP = nullptr;
                hipLaunchKernelGGL(k_out_all, grid, dim3(1024), 0, s, qa);
                DMPNN_CHECK_LAUNCH("k_out_all");
            } else {
                hipLaunchKernelGGL(k_out_bwd, grid, dim3(1024), 0, s, q);
                DMPNN_CHECK_LAUNCH("k_out_bwd");
            }
            g_cur = out; ld_cur = lda;
            continue;
        }
        DMPNN_TRY(head_wgrad(h, L, l, g_cur, A[l], lda, defer, stream));
        // data gradient: gA[l] = g . W_l   (the contraction kernel on W_l^T; layer 0 with descriptors: its first d_h columns)
        hipLaunchKernelGGL(k_head_transpose, dim3((unsigned)((Kout + 31) / 32), (unsigned)((N + 31) / 32)), dim3(32, 8), 0, s, h.W[l], K, Wt, N, (int)N, (int)Kout);
        DMPNN_CHECK_LAUNCH("k_head_transpose");
        dmpnn_gemm_args g{};
        g.M = B; g.N = Kout; g.K1 = N; g.A1 = g_cur; g.lda1 = ld_cur; g.W = Wt; g.ldw = N;
        g.C = out; g.ldc = Kout; g.act = DMPNN_ACT_NONE;
        DMPNN_TRY(dmpnn_linear_fwd(&g, stream));
        const FfnDrop dr = ffn_drop(h, l);
        if (l > 0 && (h.act != DMPNN_ACT_NONE || dr.on)) {
            hipLaunchKernelGGL(k_head_act_bwd, elementwise_grid(B * K), dim3(256), 0, s, out, K, A[l], K, B, (int)K, h.act, h.act_slope, dr);
            DMPNN_CHECK_LAUNCH("k_head_act_bwd");
        }
        g_cur = out; ld_cur = Kout;
    }
    *gZ = HeadGradZ{g_cur, ld_cur};
    return DMPNN_OK;
}
// the back end: batch norm backward and the broadcast of dl/dH to the atoms' rows — ONE column kernel, or k_bn_bwd and dmpnn_molagg_bwd
// (Running the hidden layers' weight-gradient products and the molecule bounds on a second stream of the library's own was
//  built and measured: each fork / join pair costs ~6 us of cross-queue synchronisation on this runtime — the step got 12 us
//  SLOWER, profiles/r03_side_stream_ab.txt.  One stream.)
int head_back_end(const dmpnn_head_args& h, const HeadLayout& L, const HeadRoute& R, const HeadFront& fr, const float* gZ, int64_t ldgz, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    BnAggBwdArgs q = bn_agg_bwd_args(h, L, fr, gZ, ldgz, R.rows);
    if (R.cols_fused) return launch_bn_agg_bwd(q, h.bn_weight != nullptr, R.qpw, s);
    if (h.bn_weight) {
        q.b.gX = ws_f(h, L.gHm);
        launch_bn(k_bn_bwd<true>, k_bn_bwd<false>, q.b, s);
        DMPNN_CHECK_LAUNCH("k_bn_bwd");
        gZ = q.b.gX; ldgz = q.b.ldgx;
    }
    return molagg_bwd_rows(gZ, ldgz, h.batch, h.n_atoms, h.d_h, head_ncomp(h) * h.n_mols, ws_at(h, L.bounds), h.agg_mode, h.agg_norm, h.gHv, h.ldg,
                           h.n_mols, stream);
}

int head_attentive(const dmpnn_head_args& h, const float* Hv, int64_t ldhv, void* stream, HeadPre pre, ExtraWgrad* defer, const dmpnn_predict_args* pred);
// dmpnn_head, and the head of dmpnn_train_step (pre, defer: what the step did in front, what it takes over behind — HeadPre, head_wgrad)
int head_run(const dmpnn_head_args* hp, const float* Hv, int64_t ldhv, void* stream, HeadPre pre, ExtraWgrad* defer) {
    DMPNN_CHECK_ARG(hp != nullptr, "head: null args");
    const dmpnn_head_args& h = *hp;
    if (h.agg_mode == DMPNN_MOLAGG_ATTENTIVE) return head_attentive(h, Hv, ldhv, stream, pre, defer, nullptr);
    DMPNN_TRY(head_check(h, Hv, ldhv));
    const HeadLayout L = head_layout(h);
    DMPNN_TRY(head_ws_check(h, L, "head"));
    if (h.n_mols == 0) return DMPNN_OK;
    const bool want_grad = h.gHv != nullptr;
    const HeadRoute R = head_route(h, Hv, ldhv, pre, false);
    DMPNN_CHECK_ARG(!R.want_rows || R.rows || !want_grad, "head: DMPNN_HEAD=rows, but this shape takes the chain");
    const int64_t nBt = head_ncomp(h) * h.n_mols;
    if (!pre.bounds_done) DMPNN_TRY(dmpnn_molagg_bounds(h.batch, h.n_atoms, nBt, ws_at(h, L.bounds), dmpnn_molagg_ws_bytes(nBt), stream));
    const HeadSplit split = head_split(h, L);   // (used by the four-launch form alone)
    HeadFront fr;
    DMPNN_TRY(head_front(h, L, R, Hv, ldhv, stream, R.rows ? &split : nullptr, &fr));
    if (R.rows) {   // dl/dZ [B, d]: the row kernel's gZ, in rows of d
        DMPNN_TRY(head_rows(h, L, fr, split, defer, stream));
        return head_back_end(h, L, R, fr, ws_f(h, L.gB), head_ncomp(h) * h.d_h, stream);
    }
    const float* A[DMPNN_MAX_FFN_LAYERS + 1];
    DMPNN_TRY(head_chain_forward(h, L, R, fr, A, stream));
    if (!h.targets) return DMPNN_OK;
    DMPNN_CHECK_ARG(h.loss_out != nullptr, "head: targets without loss_out");
    float* gP = ws_f(h, L.gP);
    if (!R.out_all) DMPNN_TRY(head_criterion(h, L, want_grad ? gP : nullptr, static_cast<hipStream_t>(stream)));
    if (!want_grad) return DMPNN_OK;
    HeadGradZ gZ;
    DMPNN_TRY(head_chain_backward(h, L, R, fr, A, gP, defer, &gZ, stream));
    return head_back_end(h, L, R, fr, gZ.g, gZ.ld, stream);
}

// ---- the inference head: dmpnn_predict_head (dmpnn.h) --------------------------------------------------------------------------------
// bytes of layer l's slot in dmpnn_predict_args.wsplit: its split image where the f16 row kernel takes the layer's shape — a rule of
// the widths alone (the rows it reads live in the workspace: 16-byte aligned, strides Kp | d | dims[l]), so the slots of a model
// do not move with the batch — else 0
size_t predict_slot_bytes(const dmpnn_head_args& h, const HeadLayout& L, int l) {
    const int64_t ld0 = h.X_d ? L.Kp : head_ncomp(h) * h.d_h;
    const dmpnn_gemm_args g = ffn_layer(h, l, 1, reinterpret_cast<const float*>(uintptr_t(256)), l == 0 ? ld0 : h.dims[l], nullptr);
    return linear16_ok(g) ? linear16_wsplit_bytes(g.N, g.K1) : 0;
}
inline bool known_transform(int t) {
    return (t >= DMPNN_PT_NONE && t <= DMPNN_PT_QUANTILE) || t == DMPNN_PT_SPECTRAL || t == DMPNN_PT_DIRICHLET_BINARY || t == DMPNN_PT_DIRICHLET_MULTICLASS;
}
bool predict_sizes_ok(const dmpnn_predict_args* p) {
    return p && p->head.n_layers >= 1 && p->head.n_layers <= DMPNN_MAX_FFN_LAYERS && p->head.d_h > 0 && p->head.n_mols >= 0 && p->head.n_components >= 0 &&
           p->head.n_components <= DMPNN_MAX_COMPONENTS && known_transform(p->transform);
}
size_t predict_wsplit_total(const dmpnn_head_args& h, const HeadLayout& L) {
    size_t n = 0;
    for (int l = 0; l + 1 < h.n_layers; ++l)
        if (h.dims[l] > 0 && h.dims[l + 1] > 0) n += predict_slot_bytes(h, L, l);
    return n;
}
// every rule of dmpnn.h that is the inference head's own (dmpnn_head's follow in predict_core), before any device work
int predict_check(const dmpnn_predict_args* pp) {
    DMPNN_CHECK_ARG(pp != nullptr, "predict_head: null args");
    const dmpnn_predict_args& p = *pp;
    const dmpnn_head_args& h = p.head;
    bool grads = h.gHv || h.g_bn_weight || h.g_bn_bias || h.g_att_W || h.g_att_b;
    for (int l = 0; l < DMPNN_MAX_FFN_LAYERS; ++l) grads = grads || h.gW[l] || h.gb[l];
    DMPNN_CHECK_ARG(!grads, "predict_head: inference only — head.gHv and every head.g* gradient pointer must be NULL");
    DMPNN_CHECK_ARG(h.bn_training == 0, "predict_head: inference only — head.bn_training must be 0 (running statistics)");
    DMPNN_CHECK_ARG(h.ffn_dropout_p == 0.f, "predict_head: inference only — head.ffn_dropout_p must be 0 (got %g)", (double)h.ffn_dropout_p);
    DMPNN_CHECK_ARG((p.out_mean == nullptr) == (p.out_scale == nullptr), "predict_head: out_mean and out_scale come together (both or neither)");
    DMPNN_CHECK_ARG(known_transform(p.transform), "predict_head: unknown transform %d", (int)p.transform);
    DMPNN_CHECK_ARG(p.transform != DMPNN_PT_SPECTRAL || (!p.out_mean && (h.spectral_act == 0 || h.spectral_act == 1)),
                    "predict_head: the spectral transform takes no out_mean / out_scale and head.spectral_act 0 (softplus) or 1 (exp), got %d", (int)h.spectral_act);
    DMPNN_CHECK_ARG(h.n_layers >= 1 && h.n_layers <= DMPNN_MAX_FFN_LAYERS, "predict_head: 1..%d predictor layers", DMPNN_MAX_FFN_LAYERS);
    const int64_t n_out = h.dims[h.n_layers];
    DMPNN_CHECK_ARG(n_out > 0 && n_out < (int64_t(1) << 24), "predict_head: bad output width %lld", (long long)n_out);
    DMPNN_CHECK_ARG(p.transform != DMPNN_PT_SOFTMAX || (h.n_classes >= 2 && n_out % h.n_classes == 0),
                    "predict_head: the softmax transform needs head.n_classes >= 2 dividing the output width (%d, %lld)", (int)h.n_classes, (long long)n_out);
    DMPNN_CHECK_ARG((p.transform != DMPNN_PT_MVE && p.transform != DMPNN_PT_QUANTILE) || n_out % 2 == 0,
                    "predict_head: the MVE / quantile transforms need an output layer 2 n_tasks wide (got %lld)", (long long)n_out);
    DMPNN_CHECK_ARG(p.transform != DMPNN_PT_EVIDENTIAL || n_out % 4 == 0, "predict_head: the evidential transform needs an output layer 4 n_tasks wide (got %lld)",
                    (long long)n_out);
    // (k_predict_tail reads x(2 j + 1) and x(c0 + k) without a bounds test: these two rules keep it inside the row)
    DMPNN_CHECK_ARG(p.transform != DMPNN_PT_DIRICHLET_BINARY || (h.n_classes == 2 && n_out % 2 == 0),
                    "predict_head: the binary Dirichlet transform needs head.n_classes == 2 and an output layer 2 n_tasks wide (%d, %lld)", (int)h.n_classes,
                    (long long)n_out);
    DMPNN_CHECK_ARG(p.transform != DMPNN_PT_DIRICHLET_MULTICLASS || (h.n_classes >= 2 && n_out % h.n_classes == 0),
                    "predict_head: the multiclass Dirichlet transform needs head.n_classes >= 2 dividing the output width (%d, %lld)", (int)h.n_classes,
                    (long long)n_out);
    DMPNN_CHECK_ARG((p.transform != DMPNN_PT_DIRICHLET_BINARY && p.transform != DMPNN_PT_DIRICHLET_MULTICLASS) || !p.out_mean,
                    "predict_head: the Dirichlet transforms take no out_mean / out_scale (probabilities are not unscaled)");
    if (h.targets) {
        DMPNN_CHECK_ARG(known_criterion(h), "head: unknown criterion %d (n_classes %d)", h.loss, (int)h.n_classes);
        DMPNN_CHECK_ARG(loss_per_task(h) == transform_per_task(p.transform, h.n_classes),
                        "predict_head: the criterion (%d) and the transform (%d) disagree on the outputs per task (%d against %d)", (int)h.loss, (int)p.transform,
                        loss_per_task(h), transform_per_task(p.transform, h.n_classes));
        DMPNN_CHECK_ARG(h.loss_out != nullptr, "predict_head: targets without loss_out");
    }
    DMPNN_CHECK_ARG(!p.fingerprint || p.ld_fp >= h.dims[0], "predict_head: ld_fp (%lld) < dims[0] (%lld)", (long long)p.ld_fp, (long long)h.dims[0]);
    DMPNN_CHECK_ARG(!p.wsplit || aligned16(p.wsplit), "predict_head: wsplit must be 16-byte aligned");
    return DMPNN_OK;
}
int predict_wsplit_check(const dmpnn_predict_args& p, const dmpnn_head_args& h, const HeadLayout& L) {
    if (p.wsplit && p.wsplit_bytes < predict_wsplit_total(h, L)) {
        set_error("predict_head: wsplit too small (%zu < %zu bytes)", p.wsplit_bytes, predict_wsplit_total(h, L));
        return DMPNN_ENOSPC;
    }
    return DMPNN_OK;
}
// hidden layer l of the inference head into `out`: the f16 row kernel on the layer's cached split image at `slot` (NULL: none), or fp32
int predict_hidden_layer(const dmpnn_predict_args& p, const dmpnn_head_args& h, int l, const float* A, int64_t lda, float* out, unsigned char* slot, hipStream_t s) {
    const int64_t B = h.n_mols;
    const dmpnn_gemm_args g = ffn_layer(h, l, B, A, lda, out);
    if (!slot || !linear16_ok(g)) return launch_linear(g, s);
    SplitWView w = split_weights_view_of(slot, g.N, g.K1);
    if (!p.wsplit_ready) DMPNN_TRY(split_weights_view(g.W, g.ldw, g.N, g.K1, 0, slot, &w, s));
    // up to kRowsMaxB molecules the training head's row kernel takes the layer (k_head_rows<., 1>: 16 molecules x 64 columns per
    // workgroup, 160 workgroups at 512 x 300, from the same split image) where its loads fit — a reduction width of whole quads up
    // to kRowsMaxK, 16-byte rows: k_rows16's 48-row tiles are 11 workgroups there (31 us against the fp32 contraction's 10.5)
    if (!(B <= kRowsMaxB && g.K1 % 4 == 0 && g.K1 <= kRowsMaxK && lda % 4 == 0 && aligned16(A))) return launch_linear16_view(g, w, nullptr, 0, s);
    RowsArgs r{};
    r.Z = A; r.ldz = lda; r.W0f = SplitW{w.p, w.inv_scale, w.nc}; r.b0 = g.bias; r.A1 = out;
    r.B = B; r.N = (int)g.N; r.K = (int)g.K1; r.act = h.act; r.slope = h.act_slope;
    launch_head_rows_ph1(r, dim3((unsigned)((B + 15) / 16), (unsigned)((g.N + 63) / 64)), (int)g.K1, s);
    DMPNN_CHECK_LAUNCH("k_head_rows");
    return DMPNN_OK;
}
// the inference head on the model `h` — p.head, or the attentive mode's head on one-atom molecules
int predict_core(const dmpnn_predict_args& p, const dmpnn_head_args& h, const float* Hv, int64_t ldhv, void* stream, HeadPre pre) {
    if (h.agg_mode == DMPNN_MOLAGG_ATTENTIVE) return head_attentive(h, Hv, ldhv, stream, pre, nullptr, &p);
    DMPNN_TRY(head_check(h, Hv, ldhv));   // dmpnn_head's argument rules
    const HeadLayout L = head_layout(h);
    DMPNN_TRY(predict_wsplit_check(p, h, L));
    DMPNN_TRY(head_ws_check(h, L, "predict_head"));
    const int64_t B = h.n_mols, nBt = head_ncomp(h) * B;
    if (B == 0) return DMPNN_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ln = h.n_layers;
    const HeadRoute R = head_route(h, Hv, ldhv, pre, true);
    if (!pre.bounds_done && !R.own_bounds) DMPNN_TRY(dmpnn_molagg_bounds(h.batch, h.n_atoms, nBt, ws_at(h, L.bounds), dmpnn_molagg_ws_bytes(nBt), stream));
    HeadFront fr;
    DMPNN_TRY(head_front(h, L, R, Hv, ldhv, stream, nullptr, &fr));
    const float* A = fr.Z;
    int64_t lda = fr.ldz;
    unsigned char* slot = static_cast<unsigned char*>(p.wsplit);
    for (int l = 0; l + 1 < Ln; ++l) {
        float* out = ws_f(h, L.act[l]);
        const size_t bytes = predict_slot_bytes(h, L, l);
        DMPNN_TRY(predict_hidden_layer(p, h, l, A, lda, out, (p.wsplit && bytes) ? slot : nullptr, s));
        if (p.wsplit) slot += bytes;
        A = out; lda = h.dims[l + 1];
    }
    // the output layer, the transform and every store: one launch (beyond DMPNN_PREDICT_MAX_OUT outputs the layer is a contraction of
    // its own and the launch transforms its rows)
    const int n_out = (int)h.dims[Ln], per = transform_per_task(p.transform, h.n_classes);
    PredictTail q{A, lda, (int)h.dims[Ln - 1], h.W[Ln - 1], h.b[Ln - 1], n_out, B, h.preds, p.preds, p.transform, n_out / per, per, p.out_mean, p.out_scale,
                  p.fingerprint, p.ld_fp, fr.Z, fr.ldz, (int)h.dims[0], h.spectral_act};
    if (n_out > DMPNN_PREDICT_MAX_OUT) {
        dmpnn_gemm_args g = ffn_layer(h, Ln - 1, B, A, lda, h.preds);
        g.act = DMPNN_ACT_NONE;
        DMPNN_TRY(launch_linear(g, s));
        q.W = nullptr;
    }
    if (q.W || q.preds || q.fp) DMPNN_TRY(launch_predict_tail(q, s));
    if (!h.targets) return DMPNN_OK;
    return head_criterion(h, L, nullptr, s);
}
// agg_mode == DMPNN_MOLAGG_ATTENTIVE: the attention forward into the aggregate A, the head as it is on A — B one-atom molecules under SUM,
// a one-row sum is the row itself, so every form of the head is taken unchanged (pred: the inference head of *pred instead of head_run) — and
// the attention backward from A's gradient into the caller's gHv / g_att_W / g_att_b.  pre.bounds_done: K0 wrote the REAL batch's table.
int head_attentive(const dmpnn_head_args& h, const float* Hv, int64_t ldhv, void* stream, HeadPre pre, ExtraWgrad* defer, const dmpnn_predict_args* pred) {
    const int64_t B = h.n_mols, d = h.d_h, nV = h.n_atoms;
    DMPNN_CHECK_ARG(h.att_W && h.att_b, "head: DMPNN_MOLAGG_ATTENTIVE needs att_W and att_b");
    DMPNN_CHECK_ARG(h.n_components <= 1, "head: DMPNN_MOLAGG_ATTENTIVE takes one component (n_components %d)", (int)h.n_components);
    DMPNN_CHECK_ARG(B >= 0 && nV >= 0 && d > 0 && ldhv >= d, "head: bad sizes");
    DMPNN_CHECK_ARG(nV == 0 || (Hv && h.batch), "head: null H_v / batch / preds");
    const bool want_grad = h.gHv != nullptr;
    DMPNN_CHECK_ARG(!want_grad || h.ldg >= d, "head: gradients need targets, loss_out and ldg >= d_h");
    const HeadLayout L = head_layout(h);
    unsigned char* ws = static_cast<unsigned char*>(h.ws);
    dmpnn_head_args hi = h;   // the head on A: its layout is the front of this one
    hi.agg_mode = DMPNN_MOLAGG_SUM; hi.n_atoms = B;
    hi.batch = ws ? reinterpret_cast<const int64_t*>(ws + L.att_idb) : reinterpret_cast<const int64_t*>(&hi);   // (no workspace: a non-NULL stand-in for the checks)
    hi.gHv = want_grad ? (ws ? reinterpret_cast<float*>(ws + L.att_gA) : reinterpret_cast<float*>(&hi)) : nullptr; hi.ldg = d;
    hi.att_W = hi.att_b = nullptr; hi.g_att_W = hi.g_att_b = nullptr;
    const float* A = ws ? reinterpret_cast<const float*>(ws + L.att_A) : reinterpret_cast<const float*>(&hi);
    // every other argument rule, then this mode's own (larger) workspace — the inner head's is its front — before any device work
    DMPNN_TRY(head_check(hi, A, d));
    if (pred) DMPNN_TRY(predict_wsplit_check(*pred, hi, L));   // (L: the descriptors' padded width is the inner head's too)
    DMPNN_TRY(head_ws_check(h, L, "head"));
    if (B == 0) return DMPNN_OK;
    if (!pre.bounds_done) DMPNN_TRY(dmpnn_molagg_bounds(h.batch, nV, B, ws + L.att_bounds, dmpnn_molagg_ws_bytes(B), stream));
    dmpnn_molagg_attn_args q{};
    q.n_atoms = nV; q.n_mols = B; q.d_h = d; q.H = Hv; q.ldh = ldhv; q.batch = h.batch; q.bounds = ws + L.att_bounds;
    q.W = h.att_W; q.b = h.att_b;
    q.out = reinterpret_cast<float*>(ws + L.att_A); q.ldo = d;
    if (want_grad) { q.keep_s = reinterpret_cast<float*>(ws + L.att_s); q.keep_Z = reinterpret_cast<float*>(ws + L.att_Z); }
    q.gout = reinterpret_cast<const float*>(ws + L.att_gA); q.ldgo = d; q.gH = h.gHv; q.ldgh = h.ldg;
    q.gW = h.g_att_W; q.gb = h.g_att_b;
    q.ws = ws + L.att_ws; q.ws_bytes = L.att_ws_bytes;
    DMPNN_TRY(attn_fwd_impl(&q, reinterpret_cast<int*>(ws + L.bounds), reinterpret_cast<int64_t*>(ws + L.att_idb), stream));
    const HeadPre inner{true, false};   // (the attention's forward wrote the table of the one-atom molecules)
    DMPNN_TRY(pred ? predict_core(*pred, hi, A, d, stream, inner) : head_run(&hi, A, d, stream, inner, defer));
    if (want_grad) DMPNN_TRY(attn_bwd_impl(&q, stream));
    return DMPNN_OK;
}

constexpr AggRide kNoAggRide = {nullptr, 0, nullptr, nullptr, 0, 0, 0.f, false};

// (round 6: on a tile plan built in the step from the batch vector, the tile kernels' launches are bounded by the batch's molecule count — a
//  tile holds at least one molecule — instead of the layout's bound: 512 instead of 745 workgroups at 512 molecules, forward and backward;
//  a plan that turns out to hold more tiles than that comes back NaN from both kernels)
void bound_tile_launch(dmpnn_fwd_args& f, int64_t n_mols) {
    if ((f.flags & DMPNN_F_TILE_PLAN) && f.n_tiles_launch == 0 && n_mols > 0) f.n_tiles_launch = n_mols;
}

// One component of a training step (`c`: dmpnn_step_args for component 0, a dmpnn_step_component for `comp` > 0): K0 unless its plan is
// ready, then the keeping forward `f` — with DMPNN_F_WSPLIT_READY when the weight pre-split rode in K0's launch.  `mb` / `mb_mols`: the
// aggregation's bounds table for the planner to fill on the side (pre->bounds_done: it did); `ride` then goes with the forward
// (pre->agg_rode: taken).
template <class Comp>
int plan_and_forward(const Comp& c, dmpnn_fwd_args f, int comp, int* mb, int64_t mb_mols, const AggRide& ride, HeadPre* pre, void* stream) {
    bool wrote = false, split = false;
    if (!c.plan_ready) {
        char who[32] = "";
        if (comp > 0) snprintf(who, sizeof(who), "component %d: ", comp);
        DMPNN_CHECK_ARG(f.n_edges == 0 || (c.edge_index && c.rev_edge_index), "train_step: %snull index arrays", who);
        if (f.flags & DMPNN_F_TILE_PLAN)   // (the tile table alone: the kept tensors stay in the caller's edge order, dmpnn.h)
            DMPNN_TRY(prepare_tiles_and_bounds(c.edge_index, c.rev_edge_index, c.batch, f.n_atoms, f.n_edges, const_cast<void*>(f.plan), c.plan_bytes,
                                               mb, mb_mols, stream, &wrote, &f, &split));
        else
            DMPNN_TRY(dmpnn_prepare_with_batch(c.edge_index, c.rev_edge_index, c.batch, f.n_atoms, f.n_edges, const_cast<void*>(f.plan), c.plan_bytes,
                                               stream));
    }
    if (split) f.flags |= DMPNN_F_WSPLIT_READY;
    if (wrote) g_agg_ride = ride;   // (K0 wrote the bounds table and zeroed its done[])
    const int rc = dmpnn_forward(&f, stream);
    if (pre) *pre = HeadPre{wrote, g_agg_ride.taken};
    g_agg_ride = kNoAggRide;
    return rc;
}
// how the step's parts must fit: the block (bw), the atom-descriptor layer between it and the head (a->vd), further components, the head
int step_check(const dmpnn_step_args* a, const dmpnn_bwd_args& bw) {
    const dmpnn_fwd_args& f = bw.f;
    const dmpnn_vd_args* vd = a->vd;
    DMPNN_CHECK_ARG((f.flags & DMPNN_F_KEEP) != 0, "train_step: the forward must keep its tensors (DMPNN_F_KEEP)");
    if (vd) {
        DMPNN_CHECK_ARG(f.W_d == nullptr, "train_step: with the atom-descriptor stage the block itself carries no W_d");
        DMPNN_CHECK_ARG(a->n_extra == 0 && a->head.n_components <= 1, "train_step: the atom-descriptor stage takes one block, one component");
        DMPNN_CHECK_ARG(f.out == vd->Hv && f.ldout == vd->ldhv && bw.gout == vd->gHv && bw.ldgout == vd->ldghv,
                        "train_step: the block's out / gout must be the atom-descriptor stage's Hv / gHv");
        DMPNN_CHECK_ARG(a->head.gHv == vd->gout && a->head.ldg == vd->ldgout, "train_step: head.gHv must be the atom-descriptor stage's gout");
        DMPNN_CHECK_ARG(a->head.d_h == f.d_h + vd->d_vd && vd->d_h == f.d_h, "train_step: head, block and atom-descriptor widths differ");
        DMPNN_CHECK_ARG(a->head.n_atoms == vd->n_atoms && vd->n_atoms == f.n_atoms, "train_step: head, block and atom-descriptor atom counts differ");
        // (one nn.Dropout module in the reference: the mask behind W_d is drawn with the block's p and seed)
        DMPNN_CHECK_ARG(!(vd->dropout_p > 0.f) || (f.dropout_p == vd->dropout_p && f.dropout_seed == vd->dropout_seed),
                        "train_step: the atom-descriptor stage's dropout (p %g) must be the block's (p %g) under the same seed", (double)vd->dropout_p,
                        (double)f.dropout_p);
        DMPNN_TRY(vd_check_args(vd, false));
        DMPNN_TRY(vd_check_args(vd, true));
    } else {
        DMPNN_CHECK_ARG(a->head.gHv == a->bwd.gout && a->head.ldg == a->bwd.ldgout, "train_step: head.gHv must be the backward's gout");
        DMPNN_CHECK_ARG(a->head.d_h == f.d_h + (f.W_d ? f.d_vd : 0), "train_step: head and block sizes differ");
    }
    int64_t n_atoms_all = f.n_atoms;
    for (int e = 0; e < a->n_extra; ++e) {   // every further block writes the rows behind the previous one's in H_v, reads them in gHv
        const dmpnn_bwd_args& eb = a->extra[e].bwd;
        DMPNN_CHECK_ARG((eb.f.flags & DMPNN_F_KEEP) && eb.f.d_h == a->head.d_h && !eb.f.W_d, "train_step: component %d: a keeping forward of d_h %lld, no V_d",
                        e + 1, (long long)a->head.d_h);
        DMPNN_CHECK_ARG(eb.f.ldout == f.ldout && eb.f.out == f.out + n_atoms_all * f.ldout && eb.ldgout == bw.ldgout && eb.gout == bw.gout + n_atoms_all * bw.ldgout,
                        "train_step: component %d: its H_v / gHv rows must follow the previous component's", e + 1);
        n_atoms_all += eb.f.n_atoms;
    }
    DMPNN_CHECK_ARG(a->head.n_atoms == n_atoms_all, "train_step: head and block sizes differ (%lld atoms against %lld)", (long long)a->head.n_atoms,
                    (long long)n_atoms_all);
    return DMPNN_OK;
}
// the step's forward stage: every component's K0 + keeping forward, the atom-descriptor layer, the head (defer: head_wgrad)
int step_forward(const dmpnn_step_args* a, const dmpnn_fwd_args& f, ExtraWgrad* defer, void* stream) {
    const dmpnn_head_args& h = a->head;
    const dmpnn_vd_args* vd = a->vd;
    const float* Hv = vd ? vd->out : f.out;   // what the head reads
    const int64_t ldhv = vd ? vd->ldout : f.ldout;
    // component 0: the planner already holds every molecule's atom range — it writes the aggregation's bounds table on the side (bounds_done);
    // the block's aggregate then leaves with the tile kernel's tiles (AggRide) when the head is going to take its column kernels on this shape
    HeadPre pre{false, false};
    int* mb = nullptr;
    AggRide ride = kNoAggRide;
    if (!a->plan_ready && (f.flags & DMPNN_F_TILE_PLAN) && h.ws && h.n_mols > 0 && h.batch == a->batch && h.n_atoms == f.n_atoms && h.n_components <= 1) {
        const HeadRideSlots hs = head_ride_slots(h, Hv, ldhv);
        mb = hs.bounds;
        if (mb && hs.may_ride && h.d_h == f.d_h && !f.W_d && !vd)
            ride = AggRide{hs.Hm, (int)h.d_h, a->batch, mb, (int)h.n_mols, h.agg_mode, h.agg_norm, false};
    }
    DMPNN_TRY(plan_and_forward(*a, f, 0, mb, h.n_mols, ride, &pre, stream));
    for (int e = 0; e < a->n_extra; ++e) {   // the further blocks, each into its rows of H_v
        dmpnn_fwd_args fe = a->extra[e].bwd.f;
        bound_tile_launch(fe, h.n_mols);
        DMPNN_TRY(plan_and_forward(a->extra[e], fe, e + 1, nullptr, 0, kNoAggRide, nullptr, stream));
    }
    if (vd) DMPNN_TRY(vd_forward_impl(vd, stream));   // H_v' = W_d cat(H_v, V_d) + b_d
    return head_run(&h, Hv, ldhv, stream, pre, defer);
}
}  // namespace

extern "C" {

int dmpnn_head(const dmpnn_head_args* hp, const float* Hv, int64_t ldhv, void* stream) { return head_run(hp, Hv, ldhv, stream, HeadPre{false, false}, nullptr); }

// K0 + forward (kept tensors) + the head above + backward + optimizer: one training step of models/model.py:148-161 with
// torch.optim.Adam (model.py:208-231), every kernel enqueued by this one call.
int dmpnn_train_step(const dmpnn_step_args* a, void* stream) {
    DMPNN_CHECK_ARG(a != nullptr, "train_step: null args");
    // a multicomponent model: ncomp > 1 components in the head's fingerprint, either ONE shared block over the merged batch (n_extra = 0:
    // its batch vector numbers ncomp B molecules) or one block per component (n_extra = ncomp - 1: each batch holds B molecules)
    const int64_t ncomp = a->head.n_components > 1 ? a->head.n_components : 1;
    const int n_extra = a->n_extra;
    DMPNN_CHECK_ARG(n_extra >= 0 && (n_extra == 0 || (a->extra && n_extra + 1 == ncomp)), "train_step: n_extra (%d) must be 0 or head.n_components - 1",
                    n_extra);
    dmpnn_bwd_args bw = a->bwd;
    // (the tile kernels' launches are bounded by the molecules of the block's OWN batch: a shared block over the merged batch holds ncomp B)
    const int64_t blk_mols = a->head.batch == a->batch ? ncomp * a->head.n_mols : (n_extra > 0 ? a->head.n_mols : 0);
    bound_tile_launch(bw.f, blk_mols);
    DMPNN_TRY(step_check(a, bw));
    const int stages = a->stages ? a->stages : (DMPNN_STEP_FORWARD | DMPNN_STEP_BACKWARD | DMPNN_STEP_UPDATE);
    // (a whole step in one call: the first predictor layer's weight gradient rides in the block's backward launches; a staged
    //  step — data parallel — has the head's gradients final after the forward stage, so nothing is deferred there)
    ExtraWgrad rider{};
    if (stages & DMPNN_STEP_FORWARD) DMPNN_TRY(step_forward(a, bw.f, (stages & DMPNN_STEP_BACKWARD) ? &rider : nullptr, stream));
    if (stages & DMPNN_STEP_BACKWARD) {
        bool rode = false;
        // (the layer's gradients lie in the block's slice of the flat buffer: this stage; the image of W_d is the forward's when that ran in this call)
        if (a->vd) DMPNN_TRY(vd_backward_impl(a->vd, stream, (stages & DMPNN_STEP_FORWARD) != 0));
        DMPNN_TRY(backward_impl(&bw, stream, rider.Z ? &rider : nullptr, &rode));   // (the rider: in component 0's launches only)
        for (int e = 0; e < n_extra; ++e) {
            dmpnn_bwd_args be = a->extra[e].bwd;
            bound_tile_launch(be.f, a->head.n_mols);
            DMPNN_TRY(backward_impl(&be, stream, nullptr, nullptr));
        }
        // (the backward pass did not take the f16 products: the product of its own, as dmpnn_head would have run it)
        if (rider.Z && !rode) DMPNN_TRY(head_wgrad(a->head, head_layout(a->head), 0, rider.Z, rider.A, rider.lda, nullptr, stream));
    }
    if ((stages & DMPNN_STEP_UPDATE) && a->n_params > 0 && a->clip_val > 0.f)   // Trainer(gradient_clip_val): between backward and update
        DMPNN_TRY(dmpnn_clip_grad(const_cast<float*>(a->g), a->n_params, a->clip_val, a->clip_mode, a->grad_scale > 0.f ? a->grad_scale : 1.f,
                                  a->clip_ws, stream));
    if ((stages & DMPNN_STEP_UPDATE) && a->n_params > 0)
        DMPNN_TRY(dmpnn_adam_step(a->p, a->g, a->m, a->v, a->n_params, a->lr, a->beta1, a->beta2, a->eps, a->weight_decay, a->bias_corr1,
                                  a->sqrt_bias_corr2, a->grad_scale, a->dev_scalars, stream));
    return DMPNN_OK;
}

size_t dmpnn_predict_head_ws_bytes(const dmpnn_predict_args* p) { return predict_sizes_ok(p) ? head_layout(p->head).total : 0; }
size_t dmpnn_predict_head_wsplit_bytes(const dmpnn_predict_args* p) { return predict_sizes_ok(p) ? predict_wsplit_total(p->head, head_layout(p->head)) : 0; }
int dmpnn_predict_head(const dmpnn_predict_args* p, const float* Hv, int64_t ldhv, void* stream) {
    reset_launch_count();
    DMPNN_TRY(predict_check(p));
    return predict_core(*p, p->head, Hv, ldhv, stream, HeadPre{false, false});
}

}  // extern "C"

// ---- one validation step: the inference head, then the metric stage (dmpnn_metrics.hip) on its preds ---------------------------------
namespace {
// the transforms that feed a metric kind (dmpnn.h); NONE goes behind every transform
bool metric_kind_fits(int kind, int transform) {
    switch (kind) {
        case DMPNN_METRIC_NONE: return true;
        case DMPNN_METRIC_REGRESSION:
            return transform == DMPNN_PT_NONE || transform == DMPNN_PT_UNSCALE || transform == DMPNN_PT_MVE || transform == DMPNN_PT_EVIDENTIAL ||
                   transform == DMPNN_PT_QUANTILE;
        case DMPNN_METRIC_BINARY: return transform == DMPNN_PT_SIGMOID || transform == DMPNN_PT_DIRICHLET_BINARY;
        case DMPNN_METRIC_MULTICLASS: return transform == DMPNN_PT_SOFTMAX || transform == DMPNN_PT_DIRICHLET_MULTICLASS;
        default: return false;
    }
}
// every rule of dmpnn_validate_head that is its own, and the stage's arguments into *m: the partials behind the head's layout in head.ws
int validate_check(const dmpnn_validate_args* vp, dmpnn_metric_args* m) {
    DMPNN_CHECK_ARG(vp != nullptr, "validate_head: null args");
    const dmpnn_validate_args& v = *vp;
    const dmpnn_predict_args& p = v.predict;
    const dmpnn_head_args& h = p.head;
    DMPNN_TRY(predict_check(&p));
    DMPNN_CHECK_ARG(predict_sizes_ok(&p), "validate_head: bad sizes (d_h, n_mols, n_components)");
    DMPNN_CHECK_ARG(h.targets && h.loss_out && p.preds, "validate_head: head.targets, head.loss_out and predict.preds are required");
    DMPNN_CHECK_ARG(v.metric_kind >= DMPNN_METRIC_NONE && v.metric_kind <= DMPNN_METRIC_MULTICLASS, "validate_head: unknown metric_kind %d", (int)v.metric_kind);
    DMPNN_CHECK_ARG(metric_kind_fits(v.metric_kind, p.transform), "validate_head: metric_kind %d does not go with transform %d (outputs per task, or a spectral head)",
                    (int)v.metric_kind, (int)p.transform);
    const int per = transform_per_task(p.transform, h.n_classes);
    const int64_t n_out = h.dims[h.n_layers], t = n_out / per;
    memset(m, 0, sizeof(*m));
    m->kind = v.metric_kind; m->n_mols = h.n_mols; m->n_tasks = t; m->n_classes = h.n_classes; m->group = per; m->threshold = v.threshold;
    m->preds = p.preds; m->ld_p = n_out;
    m->targets = v.metric_targets ? v.metric_targets : h.targets; m->ld_t = v.metric_targets ? v.ld_mt : t;
    m->lt_mask = h.lt_mask; m->gt_mask = h.gt_mask;
    m->loss = h.loss_out; m->stats = v.stats; m->stats_bytes = v.stats_bytes;
    // the stage's argument rules first (a stand-in for its workspace: that rule is the next one, on head.ws as a whole)
    m->ws = m; m->ws_bytes = ~size_t(0);
    DMPNN_TRY(metric_check(*m));
    const size_t front = head_layout(h).total, need = front + metric_ws_bytes(*m);
    if (!h.ws || h.ws_bytes < need) {
        set_error("validate_head: workspace missing or too small (%zu < %zu bytes)", h.ws_bytes, need);
        return DMPNN_ENOSPC;
    }
    m->ws = static_cast<unsigned char*>(h.ws) + front; m->ws_bytes = h.ws_bytes - front;
    return DMPNN_OK;
}
}  // namespace

extern "C" {

size_t dmpnn_validate_head_ws_bytes(const dmpnn_validate_args* v) {
    if (!v || !predict_sizes_ok(&v->predict)) return 0;
    const dmpnn_head_args& h = v->predict.head;
    const int per = transform_per_task(v->predict.transform, h.n_classes);
    if (per < 1) return 0;
    dmpnn_metric_args m{};
    m.kind = v->metric_kind; m.n_mols = h.n_mols; m.n_tasks = h.dims[h.n_layers] / per; m.n_classes = h.n_classes;
    return head_layout(h).total + metric_ws_bytes(m);
}
int dmpnn_validate_head(const dmpnn_validate_args* v, const float* Hv, int64_t ldhv, void* stream) {
    dmpnn_metric_args m;
    DMPNN_TRY(validate_check(v, &m));   // (every refusal of its own in front of the count's reset: dmpnn_last_launch_count() stays as it was)
    reset_launch_count();
    DMPNN_TRY(predict_core(v->predict, v->predict.head, Hv, ldhv, stream, HeadPre{false, false}));
    return launch_metric_stats(m, static_cast<hipStream_t>(stream));
}

// the same step, then the batch's (key, label) rows into the epoch's rank buffer (dmpnn_rank.hip): one launch more
size_t dmpnn_validate_head_ranked_ws_bytes(const dmpnn_validate_rank_args* r) { return r ? dmpnn_validate_head_ws_bytes(&r->validate) : 0; }
int dmpnn_validate_head_ranked(const dmpnn_validate_rank_args* r, const float* Hv, int64_t ldhv, void* stream) {
    DMPNN_CHECK_ARG(r != nullptr, "validate_head_ranked: null args");
    const dmpnn_validate_args& v = r->validate;
    dmpnn_metric_args m;
    DMPNN_TRY(validate_check(&v, &m));
    DMPNN_CHECK_ARG(v.metric_kind == DMPNN_METRIC_BINARY, "validate_head_ranked: metric_kind %d — ranks are kept for DMPNN_METRIC_BINARY alone", (int)v.metric_kind);
    dmpnn_rank_append_args ap{};
    ap.n_mols = m.n_mols; ap.n_tasks = m.n_tasks; ap.group = m.group;
    ap.preds = m.preds; ap.ld_p = m.ld_p; ap.targets = m.targets; ap.ld_t = m.ld_t;
    ap.keys = r->keys; ap.labels = r->labels; ap.capacity = r->capacity; ap.row0 = r->row0;
    DMPNN_TRY(rank_append_check(ap));
    reset_launch_count();
    DMPNN_TRY(predict_core(v.predict, v.predict.head, Hv, ldhv, stream, HeadPre{false, false}));
    DMPNN_TRY(launch_metric_stats(m, static_cast<hipStream_t>(stream)));
    return launch_rank_append(ap, static_cast<hipStream_t>(stream));
}

}  // extern "C"
