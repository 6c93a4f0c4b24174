/*
 * dmpnn.h — C ABI of the MI355X (gfx950) D-MPNN bond-message-passing engine.
 *
 * This is the drop-in boundary for ONE path of chemprop (v2.3.1):
 *     chemprop.nn.BondMessagePassing.forward        chemprop/nn/message_passing/base.py:196-212
 *       initialize / message (mixin)                chemprop/nn/message_passing/mixins.py:8-18
 *       update                                      chemprop/nn/message_passing/base.py:135-141
 *       finalize                                    chemprop/nn/message_passing/base.py:180-194
 * chemprop has no native code and no FFI of its own (it issues ATen ops); the binding a maintainer
 * would add is a ctypes (or pybind) stub inside a BondMessagePassing subclass — see INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross this boundary.
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors in practice) unless it
 *     is a pointer to one of the argument structs below (host memory).
 *   - matrices are row-major with an explicit leading dimension (elements, not bytes);
 *     weights are in nn.Linear layout [out_features, in_features].
 *   - all work is enqueued on the hipStream_t passed as `stream` (void*); no call synchronises,
 *     allocates or frees device memory, so every call is hipGraph-capture safe.
 *   - every function returns 0 on success, a negative DMPNN_E* code otherwise, never throws,
 *     never exits; dmpnn_last_error_string() describes the last failure on the calling thread.
 *   - tensors are fp32; the contractions accumulate in fp32: on the f16 matrix pipe with the exact 3-term operand
 *     split (v_mfma_f32_16x16x32_f16; DMPNN_F_SPLIT16, the default of the host side) or on the exact fp32 MFMA
 *     (v_mfma_f32_16x16x4_f32) — both fp32-class, see DESIGN.md section 3.
 */
#ifndef DMPNN_H
#define DMPNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (dmpnn_version()): 8 — round 3: dmpnn_head / dmpnn_train_step, active dropout (dmpnn_fwd_args.dropout_p / dropout_seed),
 * DMPNN_F_ATOM, the route rule (dmpnn_forward_route).  9 — end of round 3: dmpnn_head_args.bn_num_batches_tracked, DMPNN_F_TILE_PLAN
 * (training on a tile plan), dmpnn_fwd_args.keep_bits / keep_bits_bytes + dmpnn_forward_keep_bits_bytes.  Structs only ever grow at
 * their end; a host built against another version is refused by its own check of dmpnn_version() (chemprop_amd/_lib.py).
 * 10 — round 4: `keep_bits` also on DMPNN_F_FUSED | DMPNN_F_SPLIT16 | DMPNN_F_KEEP (the LEAN training forward of the per-step fused
 * route: split message rows of every step in `msplit`, sign bits, no fp32 copies) and the backward step kernels that read it;
 * in-kernel dropout no longer takes PReLU; dmpnn_backward refuses a dropout forward it cannot scale.
 * 11 — round 4: DMPNN_F_ATOM also with DMPNN_F_KEEP (atom messages TRAIN on the tile kernels; `msplit` keeps the bond-feature half of
 * the messages) and dmpnn_backward for it (gW_i [d_h, d_v], gW_h [d_h, d_h + d_e]); dmpnn_bwd_args.g_edge (a second gradient input, with
 * respect to the kept H^(depth-1): the edge read-out of the mol-atom-bond blocks); `msplit` on the tile kernel's training forward: M^(t)
 * kept as split rows, every weight-gradient product of dmpnn_backward on split rows.
 * 12 — round 5: dmpnn_clip_grad / dmpnn_clip_grad_ws_bytes (Lightning's Trainer(gradient_clip_val), cli/train.py:1937, over the flat
 * gradient buffer) and dmpnn_step_args.clip_val / clip_mode / clip_ws (the clip between the backward pass and the update of ONE call); DMPNN_LOSS_BCE;
 * dmpnn_train_route (the training-plan / kept-form rule beside dmpnn_forward_route); dmpnn_fwd_args.h0_bytes + dmpnn_forward_h0_bytes
 * (H0 kept as row quads on the per-step fused route's inference forward).
 * 13 — round 6: dmpnn_tile_waves (which form of the tile kernels a launch of these shapes takes); dmpnn_prepare_tiles with a batch
 * vector runs over several workgroups and uses the plan's unused arrays as hand-off scratch (nothing for the caller to do).
 * 14 — round 6: DMPNN_LOSS_MVE / DMPNN_LOSS_EVIDENTIAL / DMPNN_LOSS_QUANTILE in dmpnn_head (evid_v_kl / evid_eps / quantile_alpha).
 * 15 — round 6: DMPNN_F_STORE16 also with DMPNN_F_MEGA (the whole-forward tile kernel on f16 operands: one MFMA pass, opt-in, not
 * fp32-class; it was DMPNN_EINVAL there).  Grown at its end, same version: dmpnn_head_args.X_d / ld_xd (molecule descriptors behind
 * the batch norm; the two fields are zero in a caller built before them, which is the NULL they default to); dmpnn_head_args.n_components
 * and dmpnn_step_args.n_extra / extra (multicomponent models: zero in an older caller, which is one block); dmpnn_head_args.ffn_dropout_p /
 * ffn_dropout_seed (the predictor's dropout as a hash mask: zero in an older caller, which is no dropout); DMPNN_MOLAGG_ATTENTIVE with
 * dmpnn_molagg_attn_fwd / _bwd / _ws_bytes and dmpnn_head_args.att_W / att_b / g_att_W / g_att_b (zero in an older caller); DMPNN_F_UNDIRECTED_MASK
 * (a flag bit no older caller sets: dropout_p > 0 with DMPNN_F_UNDIRECTED on the per-step general route, DMPNN_EINVAL without it).
 * Added, same version (new entries only; no existing struct or entry changes): dmpnn_backward_inputs / dmpnn_backward_inputs_ws_bytes /
 * dmpnn_bwd_inputs_args (gradients with respect to V, E and V_d on the per-step general route) and dmpnn_src_sum.
 * Grown, same version: DMPNN_LOSS_SID / DMPNN_LOSS_WASSERSTEIN and DMPNN_PT_SPECTRAL (new accepted values) with
 * dmpnn_head_args.spectral_act / spectral_threshold at its end (zero in an older caller: read by the new values alone).
 * Grown, same version: DMPNN_ACT_SELU (a new accepted value of every `act` that took DMPNN_ACT_ELU; no struct changes).
 * Grown, same version: DMPNN_LOSS_MCC = 11 (a new accepted value of dmpnn_head_args.loss; 10 stays unknown; no struct changes;
 * dmpnn_head_ws_bytes() grows with that value only).
 * Grown, same version: DMPNN_PT_DIRICHLET_BINARY = 10 / DMPNN_PT_DIRICHLET_MULTICLASS = 11 (new accepted values of
 * dmpnn_predict_args.transform; 7 and 9 stay unknown; no struct changes). */
#define DMPNN_ABI_VERSION 15

enum dmpnn_status {
    DMPNN_OK = 0,
    DMPNN_EINVAL = -1,  /* bad argument (null pointer, negative size, unsupported option)        */
    DMPNN_EHIP = -2,    /* a HIP runtime call failed; see dmpnn_last_error_string()             */
    DMPNN_ENOSPC = -3   /* caller-provided workspace too small                                   */
};

/* tau of chemprop/nn/utils.py:19-55.  DMPNN_ACT_NONE lets the caller apply an arbitrary nn.Module
 * itself (the kernels then emit pre-activations). */
enum dmpnn_activation {
    DMPNN_ACT_NONE = 0,
    DMPNN_ACT_RELU = 1,
    DMPNN_ACT_LEAKYRELU = 2, /* slope = act_slope (chemprop uses 0.1, nn/utils.py:47)            */
    DMPNN_ACT_PRELU = 3,     /* slope read on device from *act_slope_ptr (single learnable scalar) */
    DMPNN_ACT_TANH = 4,
    DMPNN_ACT_ELU = 5,       /* alpha = 1                                                         */
    DMPNN_ACT_SELU = 6       /* lambda (z > 0 ? z : alpha expm1(z)), torch's constants:
                                alpha = 1.6732632423543772848170429916717, lambda = 1.0507009873554804934193349852946 */
};

enum dmpnn_flags {
    DMPNN_F_UNDIRECTED = 1u << 0, /* base.py:202-203: H <- (H + H[rev]) / 2 before every message() */
    DMPNN_F_UNDIRECTED_MASK = 1u << 12, /* with DMPNN_F_UNDIRECTED | DMPNN_F_SPLIT16 | DMPNN_F_KEEP, without DMPNN_F_FUSED (a training
                                     forward of the per-step general route on the f16 pipe): dropout_p in (0, 1) is taken for
                                     undirected messages too — the row kernels' mask does not care about direction, and
                                     dmpnn_backward, which reads the flag from the forward's block, regenerates it behind the
                                     reverse-edge average (keyed on the row of H^(t), as in the forward).  Opt-in: without it
                                     dropout_p > 0 with DMPNN_F_UNDIRECTED stays DMPNN_EINVAL.  With dropout_p == 0 it is accepted
                                     and ignored.  Without DMPNN_F_UNDIRECTED, or with DMPNN_F_FUSED / DMPNN_F_MEGA /
                                     DMPNN_F_TILE_PLAN / DMPNN_F_ATOM: DMPNN_EINVAL before any device work                       */
    DMPNN_F_FUSED = 1u << 1,      /* dmpnn_forward / dmpnn_backward: edge tensors live in CSR-row
                                     order and the segment sums are formed in the contraction
                                     epilogues (molecular graphs: symmetric, in-degree <= 24;
                                     not with DMPNN_F_UNDIRECTED)                                   */
    DMPNN_F_MEGA = 1u << 2,       /* with DMPNN_F_FUSED: the whole forward of a tile of whole molecules
                                     (<= 48 edge rows, <= 32 atoms) in ONE launch, H / M never leave the
                                     CU (dmpnn_forward_can_fuse returns 2 when the shapes allow it)   */
    DMPNN_F_KEEP = 1u << 3,       /* dmpnn_backward will follow: H0, H^(t), M^(t), Mv are written to
                                     the workspace (always the case outside DMPNN_F_MEGA)             */
    DMPNN_F_SPLIT16 = 1u << 4,    /* with DMPNN_F_MEGA: contractions on the f16 matrix pipe with the exact
                                     3-term split (x s = hi + lo, fp32 accumulate): fp32-class accuracy at
                                     5.3x the fp32-MFMA rate; needs the `wsplit` workspace                */
    DMPNN_F_WSPLIT_READY = 1u << 5, /* with DMPNN_F_SPLIT16: `wsplit` still holds the pre-split an earlier
                                     dmpnn_forward wrote for exactly these W_i / W_h / W_o values and shapes
                                     (the CALLER vouches for it, e.g. inference with frozen weights): the
                                     pre-split launch is skipped                                          */
    DMPNN_F_LOADER_TILES = 1u << 6, /* `plan` carries molecule tiles for a batch of ANY size: a tile plan
                                     (dmpnn_prepare_tiles_from_table, or dmpnn_prepare_tiles with a batch vector where
                                     dmpnn_tile_plan_any_size()) or a full plan with tiles (dmpnn_prepare_with_batch):
                                     DMPNN_F_MEGA is not limited to batches the single-workgroup plan takes     */
    DMPNN_F_H0_RESIDUAL = 1u << 8,  /* with DMPNN_F_FUSED | DMPNN_F_SPLIT16 (the per-step fused route): the residual H0 = W_i x + b_i is
                                     written once by K1 and read back in every step, instead of being recomputed per step from the
                                     exactly split K1 operand (the default for d_h <= 320).  Implied by DMPNN_F_KEEP and for d_h > 320 */
    DMPNN_F_ROW_FINALIZE = 1u << 9, /* the same route: the finalize on the row kernel from an fp32 Mv, instead of on the step kernel
                                     over 48-atom tiles fed by split rows (the default from depth 2 on).  Implied by DMPNN_F_KEEP    */
    DMPNN_F_ATOM = 1u << 10,      /* AtomMessagePassing (base.py:254-289, mixins.py:21-30) instead of the bond variant: W_i is [d_h, d_v]
                                     (H0 = W_i V[src]), W_h is [d_h, d_h + d_e], the message is M[e] = (sum_{e': dst e' = src e} [H[e'] || E[e']])
                                     — no reverse-edge term.  With DMPNN_F_FUSED | DMPNN_F_MEGA | DMPNN_F_SPLIT16, d_e <= 16: the
                                     whole-forward tile kernel — the bond-feature half of the message is constant over the depth loop,
                                     so W_h[:, d_h:] (sum E)[src] is formed once per tile and joins the residual.  With DMPNN_F_KEEP
                                     (ABI 11: training; even d_v / d_e / d_h, no W_d, no in-kernel dropout) that half, ME[e] =
                                     (sum_{e': dst e' = src e} E[e']), is kept as depth - 1 identical slots of [n_edges][16] fp32 rows
                                     in `msplit` (>= (depth - 1) * n_edges * 64 bytes; row order = the kept M^(t) rows') so that
                                     dmpnn_backward's W_h product reads [M^(t) || ME] as one operand; H0 is kept as W_i V[src] (+ b_i)
                                     alone.  A molecule beyond the tile comes back NaN (forward and gradients).
                                     WITHOUT DMPNN_F_FUSED (the per-step general route; fp32 or DMPNN_F_SPLIT16, inference or
                                     DMPNN_F_KEEP, any molecule size, any d_h, depth >= 1; directed, no W_d, 1 <= d_e <= 16): ME is
                                     formed once per call by the atom mode of the message kernel into ONE slot of [n_edges][16]
                                     zero-padded fp32 rows in `msplit` (>= n_edges * 64 bytes, 16-byte aligned, caller's edge order:
                                     kept with DMPNN_F_KEEP, scratch otherwise), every step's message is the atom mode of the same
                                     kernel, and the update is ONE contraction W_h [M^(t) || ME]; dropout_p as for the bond block
                                     on that route (DMPNN_F_SPLIT16 | DMPNN_F_KEEP, additionally even d_e); dmpnn_backward reads
                                     the same block (gW_h [d_h, d_h + d_e], all zero at depth 1).  Any other combination — the
                                     per-step fused routes, the lean route, W_d, undirected, d_e > 16: DMPNN_EINVAL                  */
    DMPNN_F_TILE_PLAN = 1u << 11, /* with DMPNN_F_FUSED | DMPNN_F_MEGA | DMPNN_F_SPLIT16 | DMPNN_F_KEEP: `plan` is a TILE plan
                                     (dmpnn_prepare_tiles: K0 is the 11 us tile table instead of the 28 us CSR plan at 512 molecules)
                                     — the kept tensors H0 / Hs / Ms are in the CALLER's edge order and dmpnn_backward runs on
                                     the tile kernel with the caller's index arrays (edge_index, rev_edge_index: required).  The
                                     host cannot see what kind of plan a device buffer holds: this flag is how dmpnn_backward
                                     (and dmpnn_train_step's K0) are told.  A backward pass the tile kernel cannot take
                                     (frozen W_i and W_h, odd leading dimensions) is DMPNN_EINVAL with this flag, never a
                                     silent use of CSR tables that are not there                                           */
    DMPNN_F_STORE16 = 1u << 7     /* OPT-IN, NOT fp32-class.  With DMPNN_F_FUSED | DMPNN_F_SPLIT16 (the per-step fused route):
                                     the message tensor between the depth steps is stored as ONE f16 per element with a
                                     power-of-two row scale (2 bytes instead of the exact hi + lo pair of 4) and contracted
                                     in two MFMA passes a_hi (w_hi + w_lo) instead of three.  Every message element is
                                     rounded to an 11-bit significand once per step (bf16, which BASELINE configs[1] names,
                                     has 8): outputs differ from the fp32 reference by ~1e-4 relative, the tests hold
                                     2e-3.  H0, the weights, every accumulation and the output stay fp32 / exact-split.
                                     Same workspace layout as without the flag (the slots are simply not filled).
                                     With DMPNN_F_FUSED | DMPNN_F_MEGA | DMPNN_F_SPLIT16 (ABI 15, the whole-forward tile
                                     kernel, which has no messages in memory): EVERY matrix product runs on the hi halves
                                     alone — operand rows, messages, weights and the H of the incidence products as one f16
                                     per element under the exact split's power-of-two scales, ONE MFMA pass instead of
                                     three and half the weight stream; accumulation, residual, bias, activation and the
                                     output stay fp32.  ~3e-4 .. 9e-4 relative against the fp32 reference (the reference
                                     under torch's bf16 autocast: 4e-3 .. 9e-3), the tests hold 2e-3; a molecule beyond the
                                     tile still takes the generic fp32 path.  Inference only, bond messages: with
                                     DMPNN_F_KEEP or DMPNN_F_ATOM it is DMPNN_EINVAL                                     */
};

/* ---------------------------------------------------------------------------------------------
 * K0  graph plan.  Replaces nothing in the reference (which rebuilds a dense [E,h] int64 index on
 * every call, mixins.py:12 / base.py:208).  Converts the int64 COO arrays of a BatchMolGraph
 * (chemprop/data/collate.py:13-73) to int32, builds the stable incoming-edge CSR by destination
 * atom (row order = increasing edge id = the reference's sequential scatter order) and validates
 * the graph invariants on device.  The plan is an opaque int32 blob in caller-owned device memory.
 * ------------------------------------------------------------------------------------------- */
size_t dmpnn_plan_bytes(int64_t n_atoms, int64_t n_edges);

int dmpnn_prepare(const int64_t* edge_index, /* [2, n_edges] row 0 = src atom, row 1 = dst atom */
                  const int64_t* rev_edge_index, /* [n_edges]                                   */
                  int64_t n_atoms, int64_t n_edges, void* plan, size_t plan_bytes, void* stream);
/* The same, writing only what a FORWARD of the fused routes reads (row_ptr, perm, srcp, revp, the tile
 * tables, the header): for inference.  dmpnn_backward, the general route and the row kernels need the
 * full plan.  Batches beyond the single-workgroup plan (6144 atoms / 10240 edges) get the full plan. */
int dmpnn_prepare_light(const int64_t* edge_index, const int64_t* rev_edge_index, int64_t n_atoms, int64_t n_edges,
                        void* plan, size_t plan_bytes, void* stream);

/* The TILE plan: only the piece-tile tables and the header — for an inference dmpnn_forward with
 * DMPNN_F_FUSED | DMPNN_F_MEGA | DMPNN_F_SPLIT16 (no DMPNN_F_KEEP) whose dmpnn_fwd_args carry the caller's own
 * edge_index / rev_edge_index.  The tile kernel then takes the rows of a tile to be its edges in the caller's order
 * (the reference's collate keeps the edges of a molecule together, data/collate.py:48-62), reads src / dst / rev straight
 * from those int64 arrays — no sort, no CSR, no permutation is built — and verifies per tile that the tile is closed
 * (a tile that is not writes NaN to its atoms).  No other entry point may be given a tile plan (their kernels return
 * NaN where they check the header, and are otherwise undefined).  Batches beyond the single-workgroup plan get the
 * full plan (header word LIGHT says which one was written).
 * `batch` (BatchMolGraph.batch, [n_atoms] int64, may be NULL): with it the tiles are made of whole MOLECULES found by
 * binary search in the (non-decreasing) batch vector and in batch[dst[.]] — no histogram, no scan, no connectivity
 * analysis; without it of whole connected pieces as in the full plan.                                            */
int dmpnn_prepare_tiles(const int64_t* edge_index, const int64_t* rev_edge_index, const int64_t* batch, int64_t n_atoms,
                        int64_t n_edges, void* plan, size_t plan_bytes, void* stream);
/* 1 when dmpnn_prepare_tiles WITH a batch vector writes a tile plan for a batch of this size even beyond the
 * single-workgroup plan (three multi-workgroup launches; their scratch must fit the plan's unused arrays): a forward on
 * it passes DMPNN_F_LOADER_TILES ("tile plan of any batch size") like one on a loader table.  Without a batch vector, or
 * when this returns 0, a batch beyond the single-workgroup plan gets the full plan, which has no piece tiles. */
int dmpnn_tile_plan_any_size(int64_t n_atoms, int64_t n_edges);

/* The FULL plan (as dmpnn_prepare) WITH molecule tiles at any batch size — what TRAINING on the tile kernels needs
 * (DMPNN_F_MEGA | DMPNN_F_KEEP, then dmpnn_backward) beyond the single-workgroup plan, whose connectivity analysis stops
 * at 10240 directed edges.  `batch` as for dmpnn_prepare_tiles.  Within the single-workgroup plan, or with batch == NULL,
 * or where !dmpnn_tile_plan_any_size(): exactly dmpnn_prepare.  Otherwise the tiles come from the batch vector (the
 * multi-workgroup planner of dmpnn_prepare_tiles) and the full plan's last kernel verifies, on the device, what a full
 * plan's tiles must satisfy: every tile is the row range [row_ptr[first atom], row_ptr[end atom]) (true when the edges
 * come in molecule order, data/collate.py:51-56) and every row's source atom lies in the tile of its destination; a
 * violation sets DMPNN_PLAN_NO_PIECE_TILES (the tile kernels return NaN; every other route is unaffected).  A forward
 * on such a plan passes DMPNN_F_LOADER_TILES.                                                                       */
int dmpnn_prepare_with_batch(const int64_t* edge_index, const int64_t* rev_edge_index, const int64_t* batch, int64_t n_atoms,
                             int64_t n_edges, void* plan, size_t plan_bytes, void* stream);
/* 1 when dmpnn_prepare_with_batch (batch != NULL) leaves molecule tiles in the full plan of a batch of this size — within the
 * single-workgroup plan always (piece tiles), beyond it where the multi-workgroup planner's scratch fits — i.e. when a forward on
 * that plan may pass DMPNN_F_MEGA (| DMPNN_F_LOADER_TILES beyond the single-workgroup plan); 0: plain dmpnn_prepare, no tiles. */
int dmpnn_full_plan_keeps_tiles(int64_t n_atoms, int64_t n_edges);

/* Plan header words (int32) readable by the caller after a stream sync (diagnostics/tests). */
enum dmpnn_plan_hdr {
    DMPNN_HDR_FLAGS = 0,   /* bit0: graph is NOT symmetric (rev is not an involution with
                              src(rev e)==dst(e)): the general edge-form message kernel runs;
                              bit1: an index was out of range (clamped; results undefined);
                              bit2: an in-degree exceeds what the fused row tiling supports (24).
                              Any of bits 0-2 set: a forward with DMPNN_F_FUSED returns NaN (loud) —
                              run such graphs without DMPNN_F_FUSED;
                              bit3: no piece tiles (the batch is too large for the single-workgroup plan and no
                              batch vector was given, or the batch vector / the edge order is not the one collate
                              produces): DMPNN_F_MEGA returns NaN.  A piece (molecule) of more than 48 rows / 32 atoms
                              is NOT an error: it becomes a tile of its own, counted in DMPNN_HDR_NSPILL, and the tile
                              kernels carry it through their generic fp32 path (csrc/dmpnn_spill_impl.hpp);
                              bit4: tile plan; bit5: the 16 words behind the header are check words of K0's validation
                              workgroups (dmpnn_forward_tiles with a host table AND the batch vector)                    */
    DMPNN_HDR_MAXDEG = 1,
    DMPNN_HDR_NATOMS = 2,
    DMPNN_HDR_NEDGES = 3,
    DMPNN_HDR_NTILES = 4,  /* fused row tiles actually used (<= the launch bound)                */
    DMPNN_HDR_TILE_STRIDE = 5,
    DMPNN_HDR_NMTILES = 6, /* piece tiles actually used                                            */
    DMPNN_HDR_LIGHT = 7,   /* 1: light plan (dmpnn_prepare_light): src / dst / rev / inv / dstp / ident
                              were NOT written — valid for forwards of the fused routes only;
                              2: tile plan (dmpnn_prepare_tiles): only the piece-tile tables were written  */
    DMPNN_HDR_NSPILL = 8,  /* piece tiles that exceed the matrix-pipe tile (48 rows / 32 atoms): slow but exact;
                              the host reads it asynchronously to move datasets of large molecules to the per-step routes */
    DMPNN_HDR_WORDS = 16
};
/* Word offsets of the arrays inside the plan (for tests):
 *   [0..4]  src, dst, rev, row_ptr, perm                  (original edge ids)
 *   [5..8]  inv, srcp, dstp, revp                         (CSR-row coordinates: row i = edge perm[i])
 *   [9..10] tile_row, tile_atom                           (row tiles of whole atoms, fused forward)
 *   [11]    number of tile slots (launch bound)
 *   [12..13] mtile_row, mtile_atom                        (row tiles of whole connected pieces)
 *   [14]    number of piece-tile slots (launch bound)                                            */
#define DMPNN_PLAN_NOFFSETS 15
int dmpnn_plan_layout(int64_t n_atoms, int64_t n_edges, int64_t offsets_out[DMPNN_PLAN_NOFFSETS]);

/* ---------------------------------------------------------------------------------------------
 * Row kernels (each replaces the reference lines cited; exported for per-row parity tests and
 * roofline measurement; dmpnn_forward below chains them).
 * ------------------------------------------------------------------------------------------- */

/* K2  mixins.py:11-18 (+ base.py:200 tau-on-load, + base.py:202-203 undirected):
 *     Hin' = tau_in(Hin) [averaged with its reverse if undirected];
 *     M[e] = sum_{e': dst(e') = src(e)} Hin'[e'] - Hin'[rev(e)]
 * flags: DMPNN_F_UNDIRECTED, or DMPNN_F_ATOM — the atom message (mixins.py:21-30), the same sum without the reverse row:
 *     M[e] = sum_{e': dst(e') = src(e)} Hin'[e']      (same kernel, same summation order; both flags together: DMPNN_EINVAL)     */
int dmpnn_message_fwd(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h,
                      const float* Hin, int64_t ld_in, float* M, int64_t ld_m,
                      int act_on_load, float act_slope, const float* act_slope_ptr,
                      unsigned flags, void* stream);

/* K4  base.py:208-211:  Mv[v] = sum_{e': dst(e') = v} tau_in(Hin[e'])                            */
int dmpnn_aggregate_fwd(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h,
                        const float* Hin, int64_t ld_in, float* Mv, int64_t ld_mv,
                        int act_on_load, float act_slope, const float* act_slope_ptr, void* stream);

/* Shared contraction (fp32 MFMA):
 *     C[r, :] = act( [A1[g(r), 0:K1] || A2[r, 0:K2]] . W^T + bias + Cadd[r, :] ),  g = gather or id
 *   K1  mixins.py:8-9     A1 = V gathered by src, A2 = E, W = W_i          act = none (H0 is pre-act)
 *   K3  base.py:135-141   A1 = M, W = W_h, Cadd = H0                        act = tau
 *   K5  base.py:180-183   A1 = V, A2 = Mv, W = W_o, bias = b_o              act = tau
 *       base.py:185-188   A1 = H_v, A2 = V_d, W = W_d, bias = b_d           act = none
 * Zpre (optional) receives the pre-activation (needed by the backward of PReLU / custom tau).
 * Leading dimensions count floats and are at least the width they carry: lda1 >= K1 (when K1 > 0), lda2 >= K2 (when
 * K2 > 0), ldw >= K1 + K2, and ldcadd / ldc / ldz >= N for each of Cadd / C / Zpre that is given; a smaller one is
 * DMPNN_EINVAL before anything is launched or written (dmpnn_linear_fwd and dmpnn_linear16_fwd, its wsplit included).
 * M == 0 is DMPNN_OK and writes no output; at least one of C and Zpre must be given.
 * gather1: int32 row indices into A1, one per output row.  An index >= gather1_rows reads a row of ZEROS (the hardware
 * range check of the operand's buffer descriptor; nothing behind the gather1_rows x lda1 floats of A1 is touched), so
 * the output row is that of A1's part absent; with gather1_rows == 0 (unknown) no index is out of range and every
 * index must be valid.  Indices are not negative.                                                                */
typedef struct dmpnn_gemm_args {
    int64_t M, N, K1, K2;
    const float* A1; int64_t lda1; const int32_t* gather1; /* gather1 may be NULL                */
    int64_t gather1_rows;                                   /* rows of the A1 tensor when gather1 is given
                                                               (bounds the hardware range check; 0 = unknown) */
    const float* A2; int64_t lda2;                          /* A2 may be NULL iff K2 == 0         */
    const float* W;  int64_t ldw;                           /* [N, K1+K2]                         */
    const float* bias;                                      /* [N] or NULL                        */
    const float* Cadd; int64_t ldcadd;                      /* [M, N] or NULL                     */
    float* C; int64_t ldc;                                  /* [M, N]                             */
    float* Zpre; int64_t ldz;                               /* [M, N] or NULL                     */
    int act; float act_slope; const float* act_slope_ptr;
} dmpnn_gemm_args;
int dmpnn_linear_fwd(const dmpnn_gemm_args* a, void* stream);
/* The same contraction on the f16 matrix pipe with the exact 3-term operand split (x s = hi + lo, fp32 accumulate:
 * fp32-class accuracy, see DMPNN_F_SPLIT16).  `wsplit` (>= dmpnn_linear16_wsplit_bytes(N, K1 + K2) bytes, caller-owned)
 * receives the pre-split weights; wsplit_ready != 0: it still holds them from an earlier call with the same W.
 * dmpnn_linear16_ok: 1 when the shapes / alignments are taken (even K1, K2 and row strides, 8-byte aligned operands,
 * a non-NULL operand for every live width, a gathered A1 below 2 GiB), else the caller stays on dmpnn_linear_fwd;
 * dmpnn_linear16_fwd refuses what it refuses (DMPNN_EINVAL) before the weight split writes into wsplit.          */
size_t dmpnn_linear16_wsplit_bytes(int64_t N, int64_t K);
int dmpnn_linear16_ok(const dmpnn_gemm_args* a);
int dmpnn_linear16_fwd(const dmpnn_gemm_args* a, void* wsplit, size_t wsplit_bytes, int wsplit_ready, void* stream);
/* dmpnn_linear16_fwd with the dropout mask of dmpnn_fwd_args.dropout_p on C: C[r][c] = keep ? act(z) / (1 - p) : +0 with
 * keep = hash(seed, site, r, c) >= floor(p 2^32) (dmpnn_dropout_keep); Zpre stays the unmasked pre-activation.  0 < p < 1,
 * site >= 0, N <= 1024 and an output C, else DMPNN_EINVAL (before the weight split writes into wsplit). */
int dmpnn_linear16_dropout_fwd(const dmpnn_gemm_args* a, void* wsplit, size_t wsplit_bytes, int wsplit_ready, float p, uint64_t seed,
                               int32_t site, void* stream);

/* K3 + K2 (or + K4) fused — ONE per-depth update of the fused route, the dominant kernel of the path:
 *     H'      = tau(H0 + M . W_h^T + b_h)                                   base.py:135-141
 *     M_next[rev(r)] = S[dst(r)] - H'[r],  S[v] = sum_{rows r of v} H'[r]   mixins.py:11-18   (if M_next)
 *     Mv[v]   = S[v]                                                        base.py:208-211   (if Mv)
 * Rows are the plan's CSR-row order (row i = edge perm[i]); the segment sums are formed from the
 * LDS-resident output tile in the epilogue of the fp32-MFMA contraction.  H_out may be NULL
 * (inference).  Needs d_h % 4 == 0, d_h <= 320, 16-byte aligned tensors, ld % 4 == 0, ld >= d_h;
 * anything else is DMPNN_EINVAL before a byte is written.                                        */
int dmpnn_update_fwd(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h,
                     const float* M, int64_t ld_m, const float* H0, int64_t ld_h0,
                     const float* W_h, const float* b_h,
                     float* H_out, int64_t ld_hout, float* M_next, int64_t ld_mnext,
                     float* Mv, int64_t ld_mv,
                     int act, float act_slope, const float* act_slope_ptr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole forward: base.py:196-212 for BondMessagePassing (graph_transform / V_d_transform /
 * dropout are applied by the caller: they are torch modules outside the kernels).
 * ------------------------------------------------------------------------------------------- */
typedef struct dmpnn_fwd_args {
    /* graph */
    const void* plan; int64_t n_atoms, n_edges;
    /* dimensions and options */
    int64_t d_v, d_e, d_h, d_vd; int32_t depth; uint32_t flags;
    int32_t act; float act_slope; const float* act_slope_ptr;
    /* inputs */
    const float* V; int64_t ldv;      /* [n_atoms, d_v]                                           */
    const float* E; int64_t lde;      /* [n_edges, d_e]                                           */
    const float* V_d; int64_t ldvd;   /* [n_atoms, d_vd] or NULL                                  */
    /* parameters, nn.Linear layout */
    const float* W_i; const float* b_i;   /* [d_h, d_v+d_e], [d_h] or NULL                        */
    const float* W_h; const float* b_h;   /* [d_h, d_h],     [d_h] or NULL                        */
    const float* W_o; const float* b_o;   /* [d_h, d_v+d_h], [d_h]                                */
    const float* W_d; const float* b_d;   /* [d_h+d_vd, d_h+d_vd] or NULL                         */
    /* caller-owned workspace, all with leading dimension ldh >= d_h:
     *   H0      [n_edges, ldh]            pre-activation W_i(...)                                 *
     *   Hs      n_hslots x [n_edges, ldh] H^(t) lives in slot (t-1) % n_hslots (t = 1..depth-1);  *
     *                                     n_hslots = depth-1 keeps every H^(t) for backward.      *
     *                                     General route: required (n_hslots >= 1).  Fused route:  *
     *                                     optional — NULL skips the H^(t) stores (inference)      *
     *   Ms      n_mslots x [n_edges, ldh] message M^(t) in slot (t-1) % n_mslots; n_mslots =      *
     *                                     depth-1 keeps them for backward; the fused route needs  *
     *                                     >= 2 slots when depth > 2 (M^(t+1) is produced while    *
     *                                     M^(t) is consumed)                                      *
     *   Mv      [n_atoms, ldh]                                                                    *
     *   Hv      [n_atoms, ldh]            only when W_d != NULL (tau(W_o(.)) before W_d)          *
     * With DMPNN_F_FUSED the rows of H0 / Hs / Ms are in the plan's CSR-row order (row i = edge   *
     * perm[i]); without it they are in the caller's edge order.  Mv, Hv, out are per atom.        */
    int64_t ldh; float* H0; float* Hs; int32_t n_hslots; float* Ms; int32_t n_mslots;
    float* Mv; float* Hv;
    /* output [n_atoms, d_h (+ d_vd)] */
    float* out; int64_t ldout;
    /* DMPNN_F_SPLIT16: caller-owned scratch for the pre-split weights, >= dmpnn_forward_wsplit_bytes() */
    void* wsplit; size_t wsplit_bytes;
    /* the caller's own index arrays (device): required when `plan` is a tile plan (dmpnn_prepare_tiles), else ignored */
    const int64_t* edge_index; const int64_t* rev_edge_index;
    /* DMPNN_F_MEGA: number of tile workgroups to launch when the caller knows the tile count (loader tiles) or an upper
     * bound of it (the batch's molecule count: a tile holds at least one molecule); 0 = the launch bound of the batch
     * size (workgroups beyond the table's tiles exit at once — 745 workgroups for the 230 tiles of 512 QM9-shaped
     * molecules, 1 us of a 30 us launch when the real tiles leave only 25 CUs for them).  A plan that turns out to hold
     * MORE tiles than this: every output NaN */
    int64_t n_tiles_launch;
    /* DMPNN_F_MEGA without DMPNN_F_KEEP: scratch of >= dmpnn_forward_spill_bytes() bytes for molecules larger than a
     * tile (generic in-kernel path; with DMPNN_F_KEEP the kept tensors serve).  NULL: such a molecule's atoms come back
     * NaN (never a silently wrong number). */
    float* spill_ws; size_t spill_bytes;
    /* DMPNN_F_FUSED | DMPNN_F_SPLIT16 | DMPNN_F_KEEP (training on the per-step fused route, molecules of any size): the two
     * ping-pong slots of split message rows (n_edges * dmpnn_split_row_floats(d_h) floats each) live HERE, and H0 / Hs / Ms /
     * Mv are the fp32 tensors dmpnn_backward reads (n_hslots = n_mslots = depth - 1, rows in the plan's CSR-row order):
     * every step writes its H^(t) and the fp32 copy of its message beside the split rows the next step consumes. */
    /* ... ABI 11, DMPNN_F_FUSED | DMPNN_F_MEGA | DMPNN_F_SPLIT16 | DMPNN_F_KEEP (a training forward of the TILE kernel, bond messages,
     * depth >= 2): given (depth - 1) * n_edges * dmpnn_split_row_floats(d_h) floats here (16-byte aligned), the kernel keeps M^(t) as
     * split rows in it (slot t - 1; rows in the kept tensors' order) INSTEAD of the fp32 rows in Ms — which then hold the rows of
     * molecules beyond the tile only — and dmpnn_backward, handed the same block, runs every weight-gradient product on split rows
     * (csrc/dmpnn_wgrad16.hip: k_wgrad16r; faster from ~30 000 message rows on: the host's rule).  NULL: fp32 rows.
     * With DMPNN_F_ATOM the same field holds the kept bond-feature half of the messages (see the flag). */
    void* msplit; size_t msplit_bytes;
    /* ACTIVE DROPOUT inside the kernels (base.py:135-141 `self.dropout(H_t)` after every update, :182 after the finalize's tau):
     * with DMPNN_F_MEGA | DMPNN_F_SPLIT16 | DMPNN_F_KEEP (a training forward of the tile kernel), a ReLU-class activation
     * (none / relu / leakyrelu / prelu) and no W_d: dropout_p in (0, 1) zeroes every element of H^(t), t >= 1, and of the
     * finalize output with probability p and scales the rest by 1 / (1 - p).  The mask is a counter-based hash of
     * (dropout_seed, site, row, column) — site = t - 1 for the update steps, depth - 1 for the finalize; row = the CALLER's
     * edge id (edge sites: the same mask on a CSR plan and on a tile plan) / the atom (finalize) — restated in oracle/dropout_hash.py; dmpnn_backward regenerates nothing: the
     * kept tensors are post-dropout, and for a ReLU-class activation their sign carries the mask.  0: no dropout.
     * The second home of the same mask: the LEAN training forward of the per-step fused route (DMPNN_F_FUSED | DMPNN_F_SPLIT16 |
     * DMPNN_F_KEEP with `keep_bits`, below) — molecules beyond the tile — with relu / leakyrelu and that form's own conditions.
     * There the kept bit stays the sign of tau(z) BEFORE dropout (one bit cannot also say "dropped") and the backward step kernels
     * regenerate the mask from the hash; the finalize output is post-dropout and carries it in its sign.  The route rules
     * (dmpnn_forward_route / dmpnn_train_route) never choose this form for dropout_p > 0: the caller asks for it.
     * The third home: the training forward of the per-step GENERAL route on the f16 pipe (DMPNN_F_SPLIT16 | DMPNN_F_KEEP without
     * DMPNN_F_FUSED) — any molecule size, d_h <= 1024 (the hash key is row * 1024 + col), depth >= 1 (depth 1: the finalize site
     * only), activation none / relu / leakyrelu / tanh / elu / selu, directed (or, the fourth admitted case, DMPNN_F_UNDIRECTED with
     * DMPNN_F_UNDIRECTED_MASK: the same mask sites, behind the reverse-edge average in dmpnn_backward), no W_d, and an update and a finalize contraction that
     * dmpnn_linear16_ok takes (they run on the row kernel k_rows16, whose epilogue applies the mask; the hash row is the output row:
     * the edge tensors of this route are in the caller's edge order).  The kept H^(t) and the output are post-dropout;
     * dmpnn_backward regenerates the mask from the hash for EVERY activation (for tanh / elu / selu / none a zero does not say "dropped")
     * and uses m / (1 - p) * tau'(y (1 - p)).  The route rules never choose a route for dropout_p > 0 here either: the caller asks.
     * Any other route / activation with dropout_p != 0: DMPNN_EINVAL (the caller runs its own dropout between the row kernels). */
    float dropout_p; uint64_t dropout_seed;
    /* DMPNN_F_TILE_PLAN with a ReLU-class activation (none / relu / leakyrelu) and dropout_p == 0: what the backward tile kernel
     * needs of H0 and H^(t) is the SIGN of every element (tau' is a step).  With `keep_bits` (>= dmpnn_forward_keep_bits_bytes()
     * bytes, 16-byte aligned) the forward stores one bit per element — 2 KB per tile and tensor, straight from the matrix-pipe
     * fragments — instead of the fp32 rows (57.6 KB per tile and tensor through an LDS transpose); H0 / Hs must still be there:
     * a molecule beyond the tile keeps its fp32 rows in them (the kernels' generic path).  NULL: fp32 rows as before. */
    /* DMPNN_F_FUSED | DMPNN_F_SPLIT16 | DMPNN_F_KEEP with `keep_bits` (ABI 10; ReLU-class activation, no W_d, no dropout, d_h <= 320,
     * depth 2 .. 8, ldh == d_h — the backward step kernels read their rows as one contiguous run; a padded ldh makes
     * dmpnn_forward_keep_bits_bytes() 0 —, a full plan): the LEAN training forward of the per-step fused route.  `msplit` then holds depth - 1 slots of split
     * message rows (M^(t) of every step, CSR-row order: nothing is copied to fp32), `H0` holds the split K1 operand [V[src] || E]
     * — rows of ceil((d_v + d_e) / 32) * 128 + 16 bytes, so the buffer must span n_edges * max(4 ldh, that) bytes — (no H0
     * tensor: the residual is recomputed per step), `keep_bits` one bit per element of H0 and of
     * every H^(t) as rows of block_cols(d_h) / 8 bytes per site (site 0: H0), `Mv` the fp32 per-atom sums; Hs / Ms are not used.
     * dmpnn_backward then runs the backward STEP kernels over the plan's tiles (csrc/dmpnn_bstep16.hip).
     * With dropout_p in (0, 1) (relu / leakyrelu only; on request — the route rules keep "lean implies no dropout") the same sizes
     * hold and the bits mean the same: [tau(z) > 0] before the mask, which both step kernels compute from the hash. */
    void* keep_bits; size_t keep_bits_bytes;
    /* ABI 12, DMPNN_F_FUSED | DMPNN_F_SPLIT16 without DMPNN_F_KEEP (inference on the per-step fused route): the size of the buffer
     * behind `H0`.  With >= dmpnn_forward_h0_bytes() bytes there the route keeps H0 = W_i x + b_i in the layout of the step kernel's
     * accumulator fragments (row QUADS: [quad][column][4 rows], a tile's quads at ((first row + 3) >> 2) + tile index), written by K1
     * straight from its registers and read back by every depth step as 15 coalesced 16-byte loads per lane — instead of recomputing it
     * from the split K1 operand in every step (d_h <= 320: 135 MFMAs and ~140 KB of operand / weight fragments through the CU's L1
     * path per 48-row tile) or reading fp32 rows through 48-60 scattered 4-byte loads per lane (d_h > 320).  0 (or too small): the
     * forms of ABI <= 11. */
    size_t h0_bytes;
} dmpnn_fwd_args;
size_t dmpnn_forward_wsplit_bytes(const dmpnn_fwd_args* a);
/* bytes of `keep_bits` for this forward (0: the forward does not qualify — see the field) */
size_t dmpnn_forward_keep_bits_bytes(const dmpnn_fwd_args* a);
/* bytes of the `H0` buffer with which an inference forward of the per-step fused route on the f16 pipe keeps H0 as row quads
 * (dmpnn_fwd_args.h0_bytes); 0: these shapes / flags do not take that form. */
size_t dmpnn_forward_h0_bytes(const dmpnn_fwd_args* a);
/* DMPNN_F_FUSED | DMPNN_F_SPLIT16 (without DMPNN_F_MEGA): the per-step fused route on the f16 matrix pipe — inference
 * forward of batches of ANY molecule size (d_h <= 640): one launch per depth step, the message tensor kept between the
 * steps as SPLIT rows (per row: chunks of [hi 32 halfs | lo 32 halfs] + a 16-byte tail with the row's power-of-two scale;
 * x s = hi + lo exactly as in DMPNN_F_SPLIT16's contractions).  `Ms` must then hold n_mslots >= 2 slots of
 * n_edges * dmpnn_split_row_floats(d_h) floats each (instead of n_edges * ldh); plan: dmpnn_prepare
 * or dmpnn_prepare_light.  `Mv` ([n_atoms, ldh] floats) and `H0` ([n_edges, ldh] floats) are this route's SCRATCH: from depth 2
 * on the finalize runs on the step kernel, fed by per-atom sums kept as split rows in a message slot, and `Mv` holds the split
 * rows of V (DMPNN_F_ROW_FINALIZE: fp32 Mv and the row kernel); for d_h <= 320 and depth >= 2 it holds the
 * exactly split K1 operand [V[src] || E] of every row (the residual W_i x + b_i is recomputed inside every step), not
 * H0 — a caller that wants the H0 tensor of this route passes DMPNN_F_H0_RESIDUAL. */
int64_t dmpnn_split_row_floats(int64_t d_h);
/* 1 when the shapes of `a` allow DMPNN_F_FUSED | DMPNN_F_SPLIT16 (inference, directed, d_h % 4 == 0, d_h <= 640, even d_v / d_e) */
int dmpnn_forward_can_fuse16(const dmpnn_fwd_args* a);
/* (3 n_edges + n_atoms) * ldh floats: H0 | H^(t) | M^(t) | Mv of the generic path, indexed by the batch's own rows */
size_t dmpnn_forward_spill_bytes(const dmpnn_fwd_args* a);
int dmpnn_forward(const dmpnn_fwd_args* a, void* stream);
/* K0 + forward of the steady inference path in ONE call (one foreign-function transition instead of two on a path whose host
 * side is as long as its device side): the tile plan of `a->plan` — from the loader's table when tile_row / tile_atom (n_tiles
 * entries + 1) are given (dmpnn_prepare_tiles_from_table), else from the batch vector / connectivity (dmpnn_prepare_tiles with
 * a->edge_index, a->rev_edge_index, `batch`) — then dmpnn_forward(a).  `a` as for an inference dmpnn_forward on a tile plan.
 * BOTH `batch` and a table (of dmpnn_pack_tiles_blocked, made where the batch was made): K0 copies the table and validates the
 * batch vector beside it in the same launch — ids and destinations in range, batch and batch[dst] non-decreasing, every tile start
 * a molecule boundary — one check word per validation workgroup behind the header (header flag bit5), which the tile kernel reads:
 * any bit set and the output is NaN, as for bits 1 / 3 of the header.  a->n_tiles_launch may then be n_tiles. */
int dmpnn_forward_tiles(const dmpnn_fwd_args* a, const int64_t* batch, const int* tile_row, const int* tile_atom, int64_t n_tiles,
                        size_t plan_bytes, void* stream);
/* 1 when the shapes / alignment of `a` allow DMPNN_F_FUSED (d_h % 4 == 0, d_h <= 320, even d_v and
 * d_e, directed), 2 when they also allow DMPNN_F_MEGA (batch within the single-workgroup plan:
 * <= 6144 atoms, <= 10240 edges — any size with DMPNN_F_LOADER_TILES), else 0.  Graph properties (symmetry, in-degree <= 24) are decided on the device by
 * dmpnn_prepare: a fused forward on a graph that violates them returns NaN and leaves the plan flags
 * set (DMPNN_HDR_FLAGS) — run such graphs without DMPNN_F_FUSED. */
int dmpnn_forward_can_fuse(const dmpnn_fwd_args* a);
/* The route the default policy takes for these shapes — ONE rule, in the library (the measured crossovers are its constants):
 *   keep       != 0: a training forward (dmpnn_backward will follow)
 *   max_level  cap from what the caller knows about the batch: 2 whole-forward tile kernel allowed, 1 per-step fused routes,
 *              0 general route only (a graph the fused kernels cannot represent; molecules beyond the tile: 1)
 *   plan_kind  0 full plan, 1 light plan (dmpnn_prepare_light), 2 tile plan (dmpnn_prepare_tiles*)
 *   arith      0: contractions on the f16 pipe with the exact operand split (default), 1: exact fp32 MFMA
 * Returns an enum dmpnn_route, or -1 when no route serves the combination (a tile plan without the tile kernel, a light plan for
 * the general route or for training).  The flags of `a` other than DMPNN_F_UNDIRECTED / DMPNN_F_LOADER_TILES are ignored. */
enum dmpnn_route { DMPNN_ROUTE_GENERAL = 0, DMPNN_ROUTE_GENERAL16 = 1, DMPNN_ROUTE_FUSED = 2, DMPNN_ROUTE_FUSED16 = 3,
                   DMPNN_ROUTE_MEGA = 4, DMPNN_ROUTE_MEGA16 = 5 };
int dmpnn_forward_route(const dmpnn_fwd_args* a, int keep, int max_level, int plan_kind, int arith);
/* v13 — waves per workgroup of the whole-forward / backward tile kernels (base.py:196-212 per tile of whole molecules) for a batch of
 * these sizes: 8 — ONE tile per 512-thread workgroup, its 20 column tiles split 3+3+3+3+2+2+2+2 over the waves (two waves per SIMD
 * out of one tile) — when the launch has at most one tile per CU and 128 < d_h <= 320; else 4 (two 256-thread workgroups per CU).
 * `n_tiles`: the tile count where the host knows it (a loader's table), else 0.  DMPNN_TILE_WAVES=4|8 in the environment overrides. */
int dmpnn_tile_waves(int64_t n_atoms, int64_t n_edges, int64_t d_h, int64_t n_tiles);

/* v12 — the TRAINING side of that rule, also in the library (round-4 VERDICT weak #10: it lived in three places of the host code): for a
 * training forward of these shapes — `a`: sizes, depth, act, DMPNN_F_UNDIRECTED / DMPNN_F_ATOM, W_d (non-NULL: the block has one),
 * dropout_p — which PLAN K0 builds, which route the forward then takes, and in what FORM the backward pass gets its tensors:
 *   n_mols     molecules of the batch (0: unknown)
 *   have       bit 0: the batch vector (BatchMolGraph.batch) is there; bit 1: a loader's tile table came with the batch
 *   oversize   what the host knows about molecules beyond the tile (48 directed edges / 32 atoms): 1 yes, 0 no, -1 unknown
 *   max_level, arith   as for dmpnn_forward_route (the caller's cap: validation verdicts, DMPNN_MEGA / DMPNN_GENERAL; DMPNN_MFMA)
 *   keep_rows  DMPNN_KEEP_ROWS: -1 the size rule (DMPNN_KEEP_ROWS_MIN message rows), 0 never, 1 always
 * plan_kind 2 (the tile plan, DMPNN_F_TILE_PLAN: K0 = the tile table alone, kept tensors in the caller's edge order) needs the tile
 * kernels' shapes (d_h % 4 == 0, d_h <= 320, even d_v / d_e, or DMPNN_F_ATOM's), a directed block without W_d and with a built-in
 * activation other than PReLU, dropout only with a ReLU-class activation, no molecule known to exceed the tile, at most 30 directed
 * edges per molecule on average, and a planner that can build it (the single-workgroup plan, a loader's table, or the batch vector
 * for the multi-workgroup planner); everything else trains on the full plan (plan_kind 0).  Returns 0, or DMPNN_EINVAL. */
#define DMPNN_KEEP_ROWS_MIN 4096
typedef struct dmpnn_train_route_info {
    int32_t plan_kind;      /* 0 | 2                                                                                          */
    int32_t route;          /* enum dmpnn_route of the training forward on that plan (dmpnn_forward_route with keep)           */
    int32_t keep_rows;      /* 1: the tile kernel keeps M^(t) as split rows in `msplit` (every weight gradient on k_wgrad16r);
                               a size rule, answered whatever `route` is — and only where the kernel's tile row is the kept row:
                               d_h <= 128 or 256 < d_h <= 320 (in between the messages stay fp32 rows in `Ms`)               */
    int32_t keep_bits;      /* 1: H0 / H^(t) leave as sign bits (`keep_bits`): the tile plan or the lean route, ReLU-class, no dropout */
    int32_t lean;           /* 1: the per-step fused route's LEAN training forward (split rows of every step + sign bits)      */
} dmpnn_train_route_info;
int dmpnn_train_route(const dmpnn_fwd_args* a, int64_t n_mols, int32_t have, int32_t oversize, int32_t max_level, int32_t arith,
                      int32_t keep_rows, dmpnn_train_route_info* out);

/* ---------------------------------------------------------------------------------------------
 * K6  backward.  The reference has no backward code of its own: gradients come from torch autograd
 * through the ATen ops of base.py:196-212 / mixins.py:8-18 (training: models/model.py:148-161).
 * These entry points are what a torch.autograd.Function around the forward calls.
 * dmpnn_backward produces the gradients of the parameters (in training, features are data); dmpnn_backward_inputs (below) also
 * those of the inputs V, E and V_d, on the per-step general route.  Indices are data everywhere.
 * ------------------------------------------------------------------------------------------- */
typedef struct dmpnn_bwd_args {
    dmpnn_fwd_args f;                    /* the forward call, with its KEPT workspace
                                            (n_hslots = n_mslots = depth-1) and its output         */
    const float* gout; int64_t ldgout;   /* dL/d out  [n_atoms, d_h (+ d_vd)]                       */
    /* outputs, dense nn.Linear layout; any may be NULL (not needed / frozen)                      */
    float* gW_i; float* gb_i; float* gW_h; float* gb_h;
    float* gW_o; float* gb_o; float* gW_d; float* gb_d;
    float* ws; size_t ws_bytes;          /* caller-owned scratch, >= dmpnn_backward_ws_bytes(&f)   */
    /* ABI 11.  A second gradient input: dL/dH^(depth-1) [n_edges, ld_gedge >= d_h] from a consumer of the kept edge states themselves
     * (Hs slot depth - 2; H0 through tau for depth 1) — the edge read-out of the mol-atom-bond blocks, mol_atom_bond.py:221-264 — in the
     * row order of the kept tensors (the caller's edge order with DMPNN_F_TILE_PLAN, else the plan's CSR-row order).  Taken by the
     * backward tile kernel only (a forward with DMPNN_F_MEGA | DMPNN_F_SPLIT16 | DMPNN_F_KEEP; 16-byte aligned, ld_gedge % 4 == 0).
     * NULL: none. */
    const float* g_edge; int64_t ld_gedge;
} dmpnn_bwd_args;
size_t dmpnn_backward_ws_bytes(const dmpnn_fwd_args* f);
int dmpnn_backward(const dmpnn_bwd_args* a, void* stream);

/* K6 with the gradients of the block's INPUTS (attributions on a frozen model, a learned featurizer or descriptor network in front of
 * the block).  dmpnn_backward's chain ends with GO = dL/d(W_o [V || Mv] + b_o) and G0 = dL/d(W_i [V[src] || E] + b_i); from them
 *     gE   = G0 . W_i[:, d_v:]
 *     gV   = GO . W_o[:, :d_v] + S . W_i[:, :d_v],   S[v] = sum_{e: src(e) = v} G0[e]     (dmpnn_src_sum: sum first, then contract)
 *     gV_d = gout . W_d[:, d_h:]
 * Per-step general route only: b.f is a kept forward WITHOUT DMPNN_F_FUSED / DMPNN_F_MEGA / DMPNN_F_TILE_PLAN / DMPNN_F_ATOM (bond
 * messages, directed or DMPNN_F_UNDIRECTED, with or without W_d, every built-in activation but PReLU); anything else, gV_d without
 * b.f.W_d, or a leading dimension below its width is DMPNN_EINVAL before any device work.  The parameter gradients of `b` are written
 * exactly as dmpnn_backward writes them (any may be NULL — all of them: the data-gradient chain still runs for gV / gE).  Outputs
 * are overwritten, not accumulated.  n_edges == 0: gV = GO . W_o[:, :d_v], gE is empty; n_atoms == 0: nothing is written.  S holds
 * on a symmetric graph only: on a plan whose header says otherwise (DMPNN_HDR_FLAGS bit 0) gV is NaN, never silently wrong.
 * b.ws / b.ws_bytes: >= dmpnn_backward_inputs_ws_bytes(&b.f) (dmpnn_backward's workspace + the pre-split / transposed weight slices);
 * DMPNN_ENOSPC otherwise. */
typedef struct dmpnn_bwd_inputs_args {
    dmpnn_bwd_args b;                 /* as for dmpnn_backward; any parameter-gradient pointer may be NULL */
    float* gV;   int64_t ldgv;        /* [n_atoms, d_v]  or NULL */
    float* gE;   int64_t ldge;        /* [n_edges, d_e]  or NULL; rows in the caller's edge order */
    float* gV_d; int64_t ldgvd;       /* [n_atoms, d_vd] or NULL (needs b.f.W_d) */
} dmpnn_bwd_inputs_args;
size_t dmpnn_backward_inputs_ws_bytes(const dmpnn_fwd_args* f);
int dmpnn_backward_inputs(const dmpnn_bwd_inputs_args* a, void* stream);
/* S[v, 0:d_h] = sum_{e': dst(e') = v} G[rev(e'), 0:d_h] — on a symmetric graph the sum of G over the edges that LEAVE v, the transpose
 * of the gather A[src(e)] (mixins.py:8-9).  One pass over the plan's incoming-edge CSR in its fixed order (no atomics: the same bits
 * on every call), 16-byte row quads where d_h, the strides and the pointers allow it; any d_h >= 1, ldg / lds >= d_h, columns beyond
 * d_h are never written.  A full plan (dmpnn_prepare); on an asymmetric graph, a light plan or a tile plan every row is NaN. */
int dmpnn_src_sum(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h, const float* G, int64_t ldg, float* S, int64_t lds,
                  void* stream);

/* Row-level backward (used when the activation / dropout modules run in torch between kernels).
 *   message_bwd    gH[e'] = sum_{e: src(e)=dst(e')} gM[e] - gM[rev(e')]   (transpose of K2, directed)
 *   atom_message_bwd   gH[e'] = sum_{e: src(e)=dst(e')} gM[e]             (transpose of K2 with DMPNN_F_ATOM; NaN on an asymmetric plan)
 *   aggregate_bwd  gH[e]  = gMv[dst(e)]                                   (transpose of K4)
 *   linear_wgrad   gW = gZ^T . [A1[gather] || A2],  gb = colsum(gZ)       (g describes the FORWARD
 *                  operands A1/A2/gather/M/N/K1/K2; W, C, act fields are ignored)
 * The data gradient of a contraction is dmpnn_linear_fwd on the transposed weight.               */
int dmpnn_message_bwd(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h,
                      const float* gM, int64_t ld_gm, float* gH, int64_t ld_gh, void* stream);
int dmpnn_atom_message_bwd(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h,
                           const float* gM, int64_t ld_gm, float* gH, int64_t ld_gh, void* stream);
int dmpnn_aggregate_bwd(const void* plan, int64_t n_atoms, int64_t n_edges, int64_t d_h,
                        const float* gMv, int64_t ld_gmv, float* gH, int64_t ld_gh, void* stream);
size_t dmpnn_linear_wgrad_ws_bytes(int64_t M, int64_t N, int64_t K, int has_bias);
int dmpnn_linear_wgrad(const dmpnn_gemm_args* g, const float* gZ, int64_t ldgz, float* gW, int64_t ldgw,
                       float* gb, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * f1 (the step right after the path): per-molecule aggregation of the atom representations.
 * Replaces chemprop/nn/agg.py:66-113 (MeanAggregation / SumAggregation / NormAggregation.forward: an
 * [V, h] int64 index, a host read of batch.max() and scatter_reduce_) by a segment reduction over the
 * SORTED `batch` vector (data/collate.py:48-62).  `n_mols` is the caller's (the reference reads it back
 * from the device).  Molecules without atoms give zero rows (agg.py:44-46).  An invalid `batch` (id out of
 * range, or decreasing) is detected on device and poisons the outputs with NaN.
 *   dmpnn_molagg_bounds  first / one-past-last atom of every molecule + the validity flag -> ws
 *                        (ws: int first[n_mols] | end[n_mols] | flag, 3 words of padding | done[n_mols] — done[] is zeroed here and
 *                        used only inside dmpnn_train_step, where the forward tile kernel marks the molecules whose aggregate it
 *                        wrote itself; dmpnn_molagg_ws_bytes() covers it)
 *   dmpnn_molagg_fwd     out[m] = sum_{v in m} H[v]   (MEAN: / count, NORM: / norm; true divisions)
 *   dmpnn_molagg_bwd     gH[v]  = gOut[batch[v]]      (MEAN: / count, NORM: / norm)
 * ------------------------------------------------------------------------------------------- */
enum dmpnn_molagg_mode { DMPNN_MOLAGG_SUM = 0, DMPNN_MOLAGG_MEAN = 1, DMPNN_MOLAGG_NORM = 2,
                         DMPNN_MOLAGG_ATTENTIVE = 3 /* dmpnn_head_args.agg_mode only (att_W / att_b); dmpnn_molagg_fwd / _bwd answer
                                                       DMPNN_EINVAL for it: the attentive aggregation has its own entry points below */ };
size_t dmpnn_molagg_ws_bytes(int64_t n_mols);
int dmpnn_molagg_bounds(const int64_t* batch, int64_t n_atoms, int64_t n_mols, void* ws, size_t ws_bytes, void* stream);
int dmpnn_molagg_fwd(const float* H, int64_t ldh, int64_t n_atoms, int64_t d_h, int64_t n_mols, const void* ws, int mode,
                     float norm, float* out, int64_t ldo, void* stream);
int dmpnn_molagg_bwd(const float* gout, int64_t ldg, const int64_t* batch, int64_t n_atoms, int64_t d_h, int64_t n_mols,
                     const void* ws, int mode, float norm, float* gH, int64_t ldgh, void* stream);

/* AttentiveAggregation (chemprop/nn/agg.py:116-133), W = nn.Linear(d_h, 1):
 *   s_v = exp(W h_v + b)   Z_m = sum_{v in m} s_v   out[m] = (sum_{v in m} s_v h_v) / Z_m     (atoms in increasing order; plain exp, no max
 *                                                                                              subtraction, a true division)
 *   a_v = gout[m] h_v   alpha_v = s_v / Z_m   c_m = sum alpha_v a_v   dl_v = alpha_v (a_v - c_m)
 *   gH[v] = alpha_v gout[m] + dl_v W     gW = sum_v dl_v h_v     gb = sum_v dl_v   (analytically zero: what comes back is rounding)
 * dmpnn_molagg_attn_fwd: ONE launch, every row of H read once; keep_s [n_atoms] / keep_Z [n_mols] (both or neither; NULL: inference)
 * are all the backward pass needs beside H.  dmpnn_molagg_attn_bwd: one launch for gH and per-wave partial rows of gW | gb, one small
 * launch that adds the rows in a fixed order (gW == gb == NULL: not run) — no floating-point atomics, the same bits on every call.
 * Any d_h >= 1, any row stride >= d_h (columns beyond d_h are never written); rows move as 16-byte quads when d_h, every stride and
 * every base pointer allow it, as single floats otherwise.  `bounds`: the table dmpnn_molagg_bounds wrote; NULL: the forward pass
 * builds it from `batch` at the head of `ws` (one more launch) and the backward pass on the same `ws` finds it there.  Its flag (an
 * invalid batch vector) poisons out, gH, gW and gb with NaN; a molecule without atoms gives a zero row.  n_atoms == 0 or n_mols == 0
 * in the backward pass: the requested gradients are zeroed.  Every argument check runs before any device work (DMPNN_EINVAL;
 * DMPNN_ENOSPC for ws: the forward pass needs it only for the table, the backward pass also for gW / gb). */
typedef struct dmpnn_molagg_attn_args {
    int64_t n_atoms, n_mols, d_h;
    const float* H; int64_t ldh;            /* [n_atoms, ldh]                                                      */
    const int64_t* batch;                   /* [n_atoms], read only when bounds == NULL                             */
    const void* bounds;                     /* dmpnn_molagg_bounds' table for (batch, n_mols), or NULL              */
    const float* W; const float* b;         /* [d_h], [1]: the nn.Linear(d_h, 1)                                    */
    float* out; int64_t ldo;                /* forward: out [n_mols, ldo]                                           */
    float* keep_s; float* keep_Z;           /* forward: out, [n_atoms] / [n_mols] or NULL; backward: in             */
    const float* gout; int64_t ldgo;        /* backward: in [n_mols, ldgo]                                          */
    float* gH; int64_t ldgh;                /* backward: out [n_atoms, ldgh]                                        */
    float* gW; float* gb;                   /* backward: out [d_h], [1]; NULL: not wanted                           */
    void* ws; size_t ws_bytes;              /* >= dmpnn_molagg_attn_ws_bytes(), 16-byte aligned                     */
} dmpnn_molagg_attn_args;
size_t dmpnn_molagg_attn_ws_bytes(const dmpnn_molagg_attn_args* a);
int dmpnn_molagg_attn_fwd(const dmpnn_molagg_attn_args* a, void* stream);
int dmpnn_molagg_attn_bwd(const dmpnn_molagg_attn_args* a, void* stream);

/* f2 (atom messages, mixins.py:21-30): out[i] = X[idx[i]], i < n_out (an index outside [0, n_src) gives a NaN
 * row).  M[e] = S[src(e)] with S = dmpnn_aggregate_fwd of the edge rows; its transpose is
 * dmpnn_aggregate_fwd of the rows gathered through rev(e) (symmetric graphs).                           */
int dmpnn_gather_rows(const float* X, int64_t ldx, int64_t n_src, const int* idx, int64_t n_out, int64_t d,
                      float* out, int64_t ldo, void* stream);

/* f3 (batching, data/collate.py:37-62): the three int64 index tensors of a BatchMolGraph from molecule-LOCAL int32
 * indices and the running offsets (all device pointers; the loader packs them, with V and E, into one buffer and
 * ships it with one copy — chemprop_amd/data.py PackedBatch):
 *   edge_index[0][e] = src[e] + atom_off[m], edge_index[1][e] = dst[e] + atom_off[m], rev_edge_index[e] = rev[e] + edge_off[m]
 *   for edge_off[m] <= e < edge_off[m+1];  batch[a] = m for atom_off[m] <= a < atom_off[m+1].
 * atom_off / edge_off have n_mols + 1 non-decreasing entries starting at 0 and ending at n_atoms / n_edges;
 * edge_index is [2, n_edges] row-major.  Local ids are not validated here: dmpnn_prepare* flags what they break. */
int dmpnn_collate(const int* atom_off, const int* edge_off, int64_t n_mols, const int* src, const int* dst, const int* rev,
                  int64_t n_atoms, int64_t n_edges, int64_t* edge_index, int64_t* rev_edge_index, int64_t* batch,
                  void* stream);

/* f3, second half ("pre-built tiles from the DataLoader worker feed K0 for free"): the tile plan of dmpnn_prepare_tiles
 * from a table the loader made while packing the batch.
 *   dmpnn_pack_tiles      HOST function (host pointers, no device work): greedy packing of consecutive whole molecules
 *                         into tiles of <= 48 directed edges / <= 32 atoms from the running offsets; tile_row / tile_atom
 *                         receive n_tiles + 1 entries; returns n_tiles, -1 if a molecule alone exceeds a tile, -2 on a
 *                         bad argument / `cap` too small.  dmpnn_max_tiles(n_atoms, n_edges) + 1 entries always suffice.
 *   dmpnn_prepare_tiles_from_table   device pointers: copies the table into `plan` (>= dmpnn_plan_bytes) and writes a
 *                         tile-plan header; order / size violations set DMPNN_PLAN_NO_PIECE_TILES (NaN from the tile
 *                         kernel), and the tile kernel checks on the batch's own index arrays that every tile is closed.
 * A forward on such a plan passes DMPNN_F_LOADER_TILES (no batch-size limit from the single-workgroup plan) and may give
 * n_tiles_launch = n_tiles so that only that many workgroups are launched.                                          */
int64_t dmpnn_pack_tiles(const int* atom_off, const int* edge_off, int64_t n_mols, int* tile_row, int* tile_atom, int64_t cap);
/* HOST function: the packing of the DEVICE planners (K0 from the batch vector) — greedy as dmpnn_pack_tiles, except that a tile also
 * starts at every block of 64 consecutive molecules and that a molecule without atoms or edges starts a tile where the walk meets
 * it.  A batch that carries THIS table (with its batch vector: dmpnn_forward_tiles given both) gets the tiles, the tile scales and
 * every output bit K0 would have given it from the batch vector.  Arguments, outputs and errors as dmpnn_pack_tiles. */
int64_t dmpnn_pack_tiles_blocked(const int* atom_off, const int* edge_off, int64_t n_mols, int* tile_row, int* tile_atom, int64_t cap);
int64_t dmpnn_max_tiles(int64_t n_atoms, int64_t n_edges);
int dmpnn_prepare_tiles_from_table(const int* tile_row, const int* tile_atom, int64_t n_tiles, int64_t n_atoms,
                                   int64_t n_edges, void* plan, size_t plan_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Misc
 * ------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------
 * f4: the optimizer step of the training loop (chemprop/models/model.py:208-231 trains with torch.optim.Adam) as ONE
 * launch over flat buffers: `p`, `g`, `m`, `v` are [n] fp32, n % 4 == 0, 16-byte aligned (the parameters of a model as
 * views of one buffer, their gradients as views of another: distributed.GradSync).  Arithmetic of torch.optim.Adam
 * (amsgrad = false):  g' = grad_scale * g + weight_decay * p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
 * p -= (lr / bias_corr1) * m / (sqrt(v) / sqrt_bias_corr2 + eps).  With `dev_scalars` (4 device floats: lr, bias_corr1,
 * sqrt_bias_corr2, grad_scale) those four come from memory instead of the arguments, so that a captured graph replays
 * with the values of its own step.
 * ------------------------------------------------------------------------------------------- */
int dmpnn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, float bias_corr1, float sqrt_bias_corr2, float grad_scale, const float* dev_scalars,
                    void* stream);

/* Gradient clipping over the flat gradient buffer — what `chemprop train --grad-clip` asks Lightning for
 * (cli/train.py:1937 `gradient_clip_val`; lightning's precision plugin then calls torch.nn.utils.clip_grad_norm_ /
 * clip_grad_value_ between the backward pass and optimizer.step).  DMPNN_CLIP_NORM: total = grad_scale * ||g||_2 over the whole
 * buffer, g *= min(1, clip_val / (total + 1e-6)); the total norm is left in ws[256] (device).  DMPNN_CLIP_VALUE: every element
 * of grad_scale * g clamped to [-clip_val, clip_val].  `grad_scale` is the factor dmpnn_adam_step will apply (1 / world after a
 * SUM all-reduce): the clipped quantity is the averaged gradient, as under DDP.  No host read, two launches (norm) / one (value).
 * `ws`: dmpnn_clip_grad_ws_bytes() of device scratch, 16-byte aligned (norm only). */
enum dmpnn_clip_mode { DMPNN_CLIP_NORM = 0, DMPNN_CLIP_VALUE = 1 };
size_t dmpnn_clip_grad_ws_bytes(void);
int dmpnn_clip_grad(float* g, int64_t n, float clip_val, int32_t mode, float grad_scale, float* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * f4, the rest of the model: what chemprop.models.MPNN does after the block in a training step (models/model.py:126-134,
 * 148-161) as ONE call —  H = agg(H_v, batch) (nn/agg.py:66-113);  Z = bn(H) (nn.BatchNorm1d, model.py:94,132);
 * P = ffn(Z) (nn/ffn.py:24-68 under nn/predictors.py:161-169: Linear, then (act, dropout, Linear) blocks; the dropout is the hash
 * mask of dmpnn_head_args.ffn_dropout_p);
 * loss = sum(L w_i t_j mask) / sum(mask), mask = isfinite(targets) (model.py:152-156, nn/metrics.py:78-127; L: MSE :137-141,
 * MAE :146-148, with lt_mask / gt_mask the bounded variants :157-163) — and, when gHv != NULL, the gradients of the loss
 * with respect to every parameter and to H_v (the `gout` of dmpnn_backward).  All pointers device pointers, fp32, dense
 * row-major (ld = width) unless an ld is given.  bn_training != 0: batch statistics, running statistics updated in place
 * (momentum; unbiased variance); 0: running statistics.  The reference's nn.BatchNorm1d also counts num_batches_tracked: the
 * caller's business (an int64 buffer that does not enter the arithmetic with a fixed momentum).
 * ------------------------------------------------------------------------------------------- */
#define DMPNN_MAX_FFN_LAYERS 8
#define DMPNN_MAX_COMPONENTS 8             /* dmpnn_head_args.n_components: at most this many blocks side by side in the fingerprint */
#define DMPNN_DROP_SITE_FFN 0x10000        /* dmpnn_head_args.ffn_dropout_p: the predictor's mask sites start here (the block's are 0 .. depth-1) */
enum dmpnn_loss { DMPNN_LOSS_MSE = 0, DMPNN_LOSS_MAE = 1,
                  DMPNN_LOSS_BCE = 2, /* v12: binary cross entropy with logits (nn/metrics.py:292-295; predictors.py:235-247) */
                  DMPNN_LOSS_CE = 3,  /* v12: cross entropy over dmpnn_head_args.n_classes logits per task (nn/metrics.py:298-304;
                                         MulticlassClassificationFFN.train_step, predictors.py:271-314): the output layer is
                                         [n_tasks * n_classes] wide, `targets` holds class indices as floats */
                  DMPNN_LOSS_MVE = 4, /* v14: mean-variance estimation (MVELoss, nn/metrics.py:203-219, on MveFFN.train_step,
                                         predictors.py:173-190): the output layer is [2 n_tasks] wide — columns [0, t) the means,
                                         [t, 2t) the raw variances, var = softplus(raw);  L = (mean - y)^2 / (2 var) + log(2 pi var) / 2 */
                  DMPNN_LOSS_EVIDENTIAL = 5, /* v14: deep evidential regression (EvidentialLoss, nn/metrics.py:222-262, on
                                         EvidentialFFN.train_step, predictors.py:193-212): the output layer is [4 n_tasks] wide — mean |
                                         raw v | raw alpha | raw beta, v = softplus, alpha = softplus + 1, beta = softplus;
                                         L = L_nll + evid_v_kl (L_reg - evid_eps) */
                  DMPNN_LOSS_QUANTILE = 6, /* v14: the interval pinball loss (QuantileLoss, nn/metrics.py:589-610, on QuantileFFN.train_step,
                                         predictors.py:215-232): the output layer is [2 n_tasks] wide — lower | upper bounds;
                                         L = pinball(y - lower; alpha / 2) + pinball(y - upper; 1 - alpha / 2), alpha = quantile_alpha */
                  DMPNN_LOSS_DIRICHLET = 7 /* v15 growth: evidential classification (DirichletLoss, nn/metrics.py, on BinaryDirichletFFN /
                                         MulticlassDirichletFFN.train_step, nn/predictors.py): the output layer is [n_tasks * n_classes]
                                         wide in the layout of DMPNN_LOSS_CE — column j K + k is class k of task j, K = n_classes (>= 2,
                                         dividing the width; 2 for the binary head) — and `targets` holds class indices c as floats (outside
                                         [0, K): a NaN loss).  alpha = softplus(raw) + 1, S = sum_k alpha_k, p = alpha / S, y = one_hot(c):
                                         L_mse = sum_k (y_k - p_k)^2 + sum_k p_k (1 - p_k) / (S + 1);
                                         alpha~ = y + (1 - y) alpha, S~ = sum_k alpha~_k:
                                         L_kl = lgamma(S~) - sum_k lgamma(alpha~_k) - lgamma(K) + sum_k (alpha~_k - 1) (psi(alpha~_k) - psi(S~));
                                         L = L_mse + evid_v_kl L_kl (evid_v_kl: DirichletLoss.v_kl).  No bounds */
                  , DMPNN_LOSS_SID = 8, DMPNN_LOSS_WASSERSTEIN = 9
                                      /* v15 growth: the spectral criteria (SID / Wasserstein, nn/metrics.py, on SpectralFFN.train_step,
                                         nn/predictors.py) — see "The spectral criteria" below.  One output per task; preds holds the raw x.
                                         n_classes != 0 beside them is no criterion this library knows ("unknown criterion":
                                         DMPNN_EINVAL), bounds masks beside them: DMPNN_EINVAL */
                  , DMPNN_LOSS_MCC = 11
                                      /* v15 growth: the binary Matthews-correlation criterion (BinaryMCCLoss, nn/metrics.py, on
                                         BinaryClassificationFFN.train_step) — see "The binary MCC criterion" below.  One output per task;
                                         preds holds the raw logits.  10 stays a value this library does not know (older callers probe it
                                         as the first unknown criterion), and so does 11 with n_classes != 0 ("unknown criterion":
                                         DMPNN_EINVAL); bounds masks beside it: DMPNN_EINVAL.  No struct field: the 1e-8 is a constant */ };
/* The spectral criteria.  These formulas are the contract: they restate chemprop 2.3.1 (nn/predictors.py: SpectralFFN; nn/metrics.py:
 * SID, Wasserstein, ChempropMetric.update / compute) from memory and were NOT run against that source.
 *   x [B, t] the MLP's raw output; T [B, t] the targets, m = isfinite(T), y = T where finite, else 0; w [B] row weights, tw [t] task
 *   weights; thr = spectral_threshold (the criterion's `threshold`; None there = 0 here = no clamp).
 * Predictor (SpectralFFN.forward, which is also its train_step):
 *   a = softplus(x) (beta 1, threshold 20) for spectral_act 0, a = exp(x) for spectral_act 1 (spectral_activation="exp");
 *   p = a / sum_j a_ij, summed over ALL columns.  (The reference appends the activation module to `ffn` as a child named
 *   spectral_activation; it is not a layer of the MLP.)
 * Both criteria:  c = max(p, thr) if thr is given, else p;  Z_i = sum_j m_ij c_ij;  q = c / Z_i.
 *   SID:          L_ij = q log(q / y) + y log(y / q) where m, 0 elsewhere (the reference fills masked q and y with 1).
 *   Wasserstein:  L_ij = | sum_{k<=j} y_ik - sum_{k<=j} q_ik |.  The running sum of q INCLUDES the masked columns' q; only y is 0
 *                 there (no masked_fill in that criterion, as recalled).  Consequence: masked columns get a non-zero gradient; in
 *                 SID without a threshold their gradient is analytically zero (and exactly 0 here).
 *   Reduction (update + compute):  loss = sum L w_i tw_j m / sum m;  loss_out = [loss, sum m], as for every other criterion.
 * Declared behaviour at the edges:
 *   - no finite target anywhere: NaN loss, as for every criterion;
 *   - a row with no finite target while others have some: loss_out[0] is NaN.  (The reference's Wasserstein loss is NaN there, and its
 *     SID gradient is NaN there (0 / 0) beside a finite loss: a declared deviation in favour of "never silently wrong");
 *   - a finite target of 0 in SID: NaN as in the reference (0 log 0); not special-cased;
 *   - exp: the kernels subtract the row maximum before exponentiating — identical in exact arithmetic for p, and finite where exp(x)
 *     alone overflows float32;
 *   - thr: 0 means none (p > 0, so a clamp at 0 is a no-op); the clamp's derivative is 1 for p >= thr, as torch's; negative or
 *     non-finite: DMPNN_EINVAL.  An unknown spectral_act: DMPNN_EINVAL.
 * The stage (k_spectral_rows + k_spectral_finish, two launches in place of k_loss's one): a grid over molecule rows, sums and scans in a
 * fixed order, no floating-point atomics — loss_out and the gradients are bit-identical from call to call. */
/* The binary MCC criterion (DMPNN_LOSS_MCC).  These formulas are the contract: they restate chemprop 2.3.1 (nn/metrics.py: BinaryMCCLoss,
 * on the logits BinaryClassificationFFN.train_step hands over) and were NOT run against that source.
 *   x [B, t] the output layer's raw logits; T [B, t] the targets, m = isfinite(T), y = T where finite, else 0 (used as the float it
 *   is; 0 / 1 are expected, as for DMPNN_LOSS_BCE); w [B] row weights, tw [t] task weights (1 where NULL).
 *   p = sigmoid(x),  a_ij = w_i m_ij, and per task j, over ALL molecules of the batch:
 *     TP_j = sum_i a y p        FP_j = sum_i a (1 - y) p        TN_j = sum_i a (1 - y) (1 - p)        FN_j = sum_i a y (1 - p)
 *     D_j = (TP + FP) (TP + FN) (TN + FP) (TN + FN),   MCC_j = (TP TN - FP FN) / sqrt(D_j + 1e-8)
 *   loss = 1 - (1 / t) sum_j tw_j MCC_j;   loss_out = [loss, sum m].
 * The gradient, two coefficients per task:  S = sqrt(D + 1e-8), N = TP TN - FP FN, A = TP + FP, Bq = TP + FN, C = TN + FP, E = TN + FN,
 *   g(dN, dD) = dN / S - N dD / (2 S^3),
 *   alpha_j = g(TN, Bq C E + A C E) - g(-FP, A C E + A Bq C)        (d/dTP - d/dFN)
 *   beta_j  = g(-FN, Bq C E + A Bq E) - g(TP, A Bq E + A Bq C)      (d/dFP - d/dTN)
 *   dloss/dx_ij = -(tw_j / t) a_ij (y_ij alpha_j + (1 - y_ij) beta_j) p_ij (1 - p_ij).
 * Declared deviations and behaviour at the edges:
 *   - the reference applies the sigmoid only when some prediction lies outside [0, 1] (a test on the data); here it is always applied:
 *     the predictor's train_step hands over logits;
 *   - the mean runs over all t tasks: a task without a finite target has MCC_j = 0 and a gradient of exactly 0; a batch without any
 *     finite target has loss 1.0 — NOT the NaN of the sum / count criteria — and loss_out[1] = 0;
 *   - a task whose finite targets are all of one class (0 or 1) has MCC_j = 0 and a gradient of exactly 0, not merely a small one (N and
 *     the dN, dD of the class that is present vanish exactly in the form above; the other coefficient meets a factor y or 1 - y of 0);
 *   - rows of weight 0 take no part; no lt_mask / gt_mask (DMPNN_EINVAL), as for every criterion but MSE / MAE;
 *   - several devices: every rank forms the sums over its own shard, as the reference's training loss does.
 * The stage (k_mcc_cols + k_mcc_finish, two launches in place of k_loss's one): k_mcc_cols, a grid over blocks of molecule rows (and of
 * 256 task columns), leaves each block's four sums per task in the workspace; k_mcc_finish adds the blocks' sums per task in block order
 * (in double), forms MCC_j, alpha_j, beta_j and writes dloss/dx (gP == NULL inside the library: the loss alone, what dmpnn_predict_head
 * takes with targets); workgroup 0 writes loss_out.  Any B >= 1, any t >= 1; no atomics, no order that depends on scheduling — loss_out
 * and the gradients are bit-identical from call to call.  The four-launch row form and the one-launch output-layer-plus-criterion form
 * are not taken with it.  dmpnn_predict_head: with DMPNN_PT_SIGMOID. */
typedef struct dmpnn_head_args {
    int64_t n_atoms, n_mols, d_h;           /* rows of H_v, molecules, width of H_v                              */
    const int64_t* batch;                   /* [n_atoms] molecule of every atom, non-decreasing (BatchMolGraph.batch) */
    int32_t agg_mode; float agg_norm;       /* enum dmpnn_molagg_mode; the norm of NormAggregation                  */
    const float* bn_weight; const float* bn_bias;  /* [d_h] each; bn_weight == NULL: no batch norm (nn.Identity)   */
    float* bn_running_mean; float* bn_running_var; /* [d_h] each, updated in place when bn_training               */
    float bn_eps, bn_momentum; int32_t bn_training;
    int32_t n_layers; int32_t act; float act_slope;       /* Linear layers of the predictor; enum dmpnn_activation */
    const float* W[DMPNN_MAX_FFN_LAYERS];   /* W[l]: [dims[l+1], dims[l]]  (nn.Linear layout)                       */
    const float* b[DMPNN_MAX_FFN_LAYERS];   /* [dims[l+1]] or NULL                                                  */
    int64_t dims[DMPNN_MAX_FFN_LAYERS + 1]; /* dims[0] = d_h (+ d_xd with X_d) ... dims[n_layers] = n_tasks    */
    int32_t loss;                           /* enum dmpnn_loss                                                      */
    const float* targets;                   /* [n_mols, n_tasks], NaN / inf = missing; NULL: predictions only       */
    const float* weights;                   /* [n_mols] or NULL (ones)                                              */
    const float* task_weights;              /* [n_tasks] or NULL (ones)                                             */
    const unsigned char* lt_mask; const unsigned char* gt_mask;  /* [n_mols, n_tasks] bytes or NULL (unbounded)    */
    float* preds;                           /* out [n_mols, n_tasks]                                                */
    float* loss_out;                        /* out, 2 floats: the loss, the number of finite targets                */
    float* gW[DMPNN_MAX_FFN_LAYERS]; float* gb[DMPNN_MAX_FFN_LAYERS];  /* out (NULL: not wanted), nn.Linear layout  */
    float* g_bn_weight; float* g_bn_bias;   /* out [d_h] or NULL                                                    */
    float* gHv; int64_t ldg;                /* out [n_atoms, ldg] dloss / dH_v; NULL: forward (and loss) only       */
    void* ws; size_t ws_bytes;              /* caller-owned scratch, >= dmpnn_head_ws_bytes()                       */
    int64_t* bn_num_batches_tracked;        /* nn.BatchNorm1d's counter: += 1 on device when bn_training (NULL: not kept) — v9 */
    int32_t n_classes;                      /* v12, DMPNN_LOSS_CE (and DMPNN_LOSS_DIRICHLET): classes per task (>= 2); the last layer's width is n_tasks * n_classes */
    float evid_v_kl, evid_eps;              /* v14, DMPNN_LOSS_EVIDENTIAL: EvidentialLoss.v_kl (0.2) and .eps (1e-8); DMPNN_LOSS_DIRICHLET reads
                                               evid_v_kl as DirichletLoss.v_kl (0.2) and ignores evid_eps                              */
    float quantile_alpha;                   /* v14, DMPNN_LOSS_QUANTILE: QuantileLoss.alpha (0.1)                                      */
    const float* X_d; int64_t ld_xd;        /* v15 growth: [n_mols, d_xd] molecule descriptors, row stride ld_xd >= d_xd, or NULL (none).
                                               d_xd = dims[0] - d_h: the predictor's input is cat(bn(agg(H_v)), X_d) (models/model.py,
                                               fingerprint) and W[0] is [dims[1], d_h + d_xd]; no gradient flows to X_d               */
    int32_t n_components;                   /* v15 growth: 0 or 1 — one block; n > 1 — a multicomponent model (models/multi.py): H_v
                                               holds the atoms of n B molecules (component 0's first), `batch` numbers molecule i of
                                               component c as c B + i, n_mols = B (target rows); the fingerprint is
                                               cat(agg(H_v^0), ..., agg(H_v^(n-1))) [B, n d_h] before batch norm (bn_* are n d_h long),
                                               dims[0] = n d_h (+ d_xd); d_h stays one block's width and gHv [n_atoms, ldg] holds every
                                               component's rows */
    float ffn_dropout_p; uint64_t ffn_dropout_seed;  /* v15 growth: the predictor's nn.Dropout (nn/ffn.py:49-58: act, dropout, Linear) as a
                                               hash mask; 0 (what a caller built before the fields passes): none; outside [0, 1): DMPNN_EINVAL.
                                               Layer l (1 <= l < n_layers) reads N = dims[l] columns: its input element (r, c) — r the
                                               target row (the molecule, also of a multicomponent model) — is KEPT, and scaled by 1 / (1 - p),
                                               when drop_hash(seed, DMPNN_DROP_SITE_FFN + l, r ceil(N / 1024) + c / 1024, c % 1024) >=
                                               floor(p 2^32) (the hash of dmpnn_fwd_args.dropout_p; dmpnn_dropout_keep).  Applied whenever
                                               p > 0: the caller decides when training is on.  No mask is stored: the backward pass
                                               regenerates it */
    const float* att_W; const float* att_b; float* g_att_W; float* g_att_b;  /* v15 growth: agg_mode == DMPNN_MOLAGG_ATTENTIVE —
                                               AttentiveAggregation's W [d_h] and b [1] (both required, else DMPNN_EINVAL) and their
                                               gradients (out, NULL: not wanted; final when dmpnn_head returns, like the predictor's).
                                               The aggregate is formed by dmpnn_molagg_attn_fwd into the workspace, the head runs on it
                                               as on a batch of one-atom molecules, dmpnn_molagg_attn_bwd carries its input gradient back
                                               to gHv.  n_components > 1 with it: DMPNN_EINVAL.  Zero in an older caller; ignored in the
                                               other modes.  dmpnn_head_ws_bytes() grows in this mode only */
    int32_t spectral_act; float spectral_threshold;  /* v15 growth: DMPNN_LOSS_SID / _WASSERSTEIN and DMPNN_PT_SPECTRAL — SpectralFFN's
                                               activation (0 softplus, 1 exp) and the criterion's threshold (0: none).  Zero in an older
                                               caller; ignored by every other criterion and transform */
} dmpnn_head_args;
size_t dmpnn_head_ws_bytes(const dmpnn_head_args* h);
int dmpnn_head(const dmpnn_head_args* h, const float* Hv, int64_t ldhv, void* stream);

/* The same model behind the block at INFERENCE, as one call with kernels of its own: what MPNN.forward / fingerprint do in eval mode
 * after message_passing (models/model.py:126-146) and what validation_step adds (the criterion on the raw outputs: val_loss) —
 * aggregation, eval-mode batch norm and the X_d columns (k_agg_bn_fwd, or the chain's kernels where the column kernel does not take
 * the shape), every hidden layer on the f16 pipe from its split image, activation fused (up to 1 024 molecules the training head's row
 * kernel k_head_rows<., 1>, 16 molecules x 64 columns per workgroup, where the reduction width is whole quads up to 512; k_rows16
 * otherwise; a layer whose shape dmpnn_linear16_ok refuses — odd widths, unaligned rows — runs as dmpnn_linear_fwd), then ONE launch
 * (k_predict_tail) for the output layer, the predictor's output
 * transform and every store, and k_loss when targets are given (the spectral criteria and binary MCC: their stages of two launches).  The usual model (sum / mean / norm aggregation, batch norm, one hidden
 * layer, <= DMPNN_PREDICT_MAX_OUT outputs, <= 1 024 molecules, widths in whole quads) with a ready split: three launches, four with
 * targets (dmpnn_last_launch_count()).  Output layers wider than DMPNN_PREDICT_MAX_OUT run on the contraction kernels and
 * k_predict_tail transforms their rows.
 *
 * Inference only — each of these is DMPNN_EINVAL before any device work: head.gHv or any head.g* pointer non-NULL; head.bn_training
 * != 0; head.ffn_dropout_p != 0; only one of out_mean / out_scale; an unknown transform; DMPNN_PT_SOFTMAX with head.n_classes < 2 or
 * n_classes not dividing n_out = head.dims[head.n_layers]; DMPNN_PT_MVE / _QUANTILE with n_out % 2 != 0, DMPNN_PT_EVIDENTIAL with
 * n_out % 4 != 0; DMPNN_PT_DIRICHLET_BINARY with head.n_classes != 2 or an odd n_out, DMPNN_PT_DIRICHLET_MULTICLASS with head.n_classes < 2
 * or n_classes not dividing n_out, either of the two with out_mean / out_scale; with head.targets, a head.loss whose outputs per task
 * (cross entropy / Dirichlet: n_classes; MVE / quantile: 2; evidential: 4; else 1) disagree with the transform's (softmax and the two
 * Dirichlet transforms: n_classes; MVE / quantile: 2; evidential: 4; else 1), or no head.loss_out; and
 * whatever dmpnn_head refuses.  A workspace (head.ws) or wsplit that is too small: DMPNN_ENOSPC.  The running statistics and
 * bn_num_batches_tracked are never written.  head.targets != NULL also writes head.loss_out: the criterion on the RAW outputs
 * (chemprop's val_loss), k_loss's arithmetic unchanged.  n_components > 1 and DMPNN_MOLAGG_ATTENTIVE are taken as dmpnn_head takes
 * them (attentive: dmpnn_molagg_attn_fwd into the workspace, then this head on one-atom molecules).
 *
 * Transforms — x a raw row, t = n_tasks, s / m = out_scale[j] / out_mean[j] (1 / 0 when NULL), softplus = F.softplus (beta 1,
 * threshold 20):  NONE p[j] = x[j];  UNSCALE p[j] = x[j] s + m;  SIGMOID p[j] = 1 / (1 + exp(-x[j]));  SOFTMAX p[j][k] =
 * softmax_k(x[j nc + k]) (the maximum subtracted first);  MVE p[j] = (x[j] s + m, softplus(x[t+j]) s^2);  EVIDENTIAL p[j] = (x[j] s
 * + m, softplus(x[t+j]), softplus(x[2t+j]) + 1, softplus(x[3t+j]) s^2);  QUANTILE lo = x[j] s + m, up = x[t+j] s + m: p[j] = ((lo +
 * up) / 2, up - lo);  SPECTRAL p[j] = a(x[j]) / sum_k a(x[k]) (below the enum);  with alpha[c] = softplus(x[c]) + 1 (the alphas of
 * DMPNN_LOSS_DIRICHLET):  DIRICHLET_BINARY S = alpha[2j] + alpha[2j+1]: p[j] = (alpha[2j+1] / S, 2 / S);  DIRICHLET_MULTICLASS p[j][k] =
 * alpha[j nc + k] / sum_m alpha[j nc + m] (both below the enum).  These are the eval-mode forward of nn/predictors.py with
 * UnscaleTransform / transform_variance.
 *
 * wsplit: the f16 split images of the hidden layers' weights, one slot per layer l < n_layers - 1 in layer order, each
 * dmpnn_linear16_wsplit_bytes(dims[l+1], dims[l]) long — 0 for a layer that runs as dmpnn_linear_fwd — kept by the caller between
 * calls (the convention of dmpnn_linear16_fwd): wsplit_ready == 0 splits every layer first (one launch each), != 0 says the images
 * are current and launches nothing for them; whether they are is the caller's business.  wsplit == NULL: no cache, the hidden
 * layers run as dmpnn_linear_fwd (fp32 contraction).  dmpnn_predict_head_ws_bytes() / _wsplit_bytes(): 0 for a NULL or malformed
 * struct. */
enum dmpnn_predict_transform { DMPNN_PT_NONE = 0, DMPNN_PT_UNSCALE, DMPNN_PT_SIGMOID, DMPNN_PT_SOFTMAX,
                               DMPNN_PT_MVE, DMPNN_PT_EVIDENTIAL, DMPNN_PT_QUANTILE };
#define DMPNN_PT_SPECTRAL 8
/* DMPNN_PT_SPECTRAL (v15 growth; a further value of dmpnn_predict_args.transform beside the enumerators, which stay as they were —
 * 7 stays an unknown transform): SpectralFFN.forward — preds [n_mols, n_tasks] = p = a / sum_row a, a = softplus(x) | exp(x - max_row x)
 * by head.spectral_act ("The spectral criteria" above); the row's sum (and maximum) once per row.  With out_mean / out_scale, or an
 * unknown head.spectral_act: DMPNN_EINVAL. */
#define DMPNN_PT_DIRICHLET_BINARY 10
#define DMPNN_PT_DIRICHLET_MULTICLASS 11
/* DMPNN_PT_DIRICHLET_BINARY / _MULTICLASS (v15 growth; further values of dmpnn_predict_args.transform — 7 and 9 stay unknown transforms):
 * the eval-mode forward of the evidential-classification predictors on alpha[c] = softplus(x[c]) + 1, the alphas DMPNN_LOSS_DIRICHLET forms.
 * BINARY — BinaryDirichletFFN: raw column 2 j + k is the evidence of class k of task j, head.n_classes == 2 and an even n_out; preds
 * [n_mols, n_tasks, 2] = (alpha[2j+1] / S, 2 / S) with S = alpha[2j] + alpha[2j+1]: the probability of class 1 and the uncertainty.
 * MULTICLASS — MulticlassDirichletFFN: cross entropy's layout, head.n_classes >= 2 dividing n_out; preds [n_mols, n_tasks, n_classes] =
 * alpha[j nc + k] / sum_m alpha[j nc + m].  Both count n_classes outputs per task (head.targets: with DMPNN_LOSS_DIRICHLET).  Any other
 * n_classes / n_out, or out_mean / out_scale with either: DMPNN_EINVAL before any device work — the kernel gathers a task's columns
 * without a bounds test of its own. */
#define DMPNN_PREDICT_MAX_OUT 64
typedef struct dmpnn_predict_args {
    dmpnn_head_args head;          /* the model behind the block, as dmpnn_head reads it. head.preds = the RAW outputs
                                      [n_mols, n_out] (predictor.train_step's, in the MLP's column layout), required */
    int32_t transform;             /* enum dmpnn_predict_transform */
    const float* out_mean; const float* out_scale;   /* [n_tasks] each, or both NULL (identity): UnscaleTransform in eval mode */
    float* preds;                  /* out, transformed: [n_mols, n_tasks] | [n_mols, n_tasks, n_classes] | [n_mols, n_tasks, 2 or 4]; NULL: not wanted */
    float* fingerprint; int64_t ld_fp;   /* out or NULL: the predictor's input cat(bn(agg(H_v)), X_d) [n_mols, dims[0]], ld_fp >= dims[0] */
    void* wsplit; size_t wsplit_bytes; int32_t wsplit_ready;   /* f16 split images of the hidden layers' weights, kept by the caller
                                      between calls (the convention of dmpnn_linear16_fwd); NULL: no cache, fp32 contraction */
} dmpnn_predict_args;
size_t dmpnn_predict_head_ws_bytes(const dmpnn_predict_args* p);
size_t dmpnn_predict_head_wsplit_bytes(const dmpnn_predict_args* p);
int    dmpnn_predict_head(const dmpnn_predict_args* p, const float* Hv, int64_t ldhv, void* stream);

/* Epoch metric statistics (v15 growth: new entry points, every existing struct and call as it was).  Every metric a validation epoch
 * reports — MSE / RMSE / MAE / R2 and their bounded forms, binary accuracy / F1 / MCC, multiclass accuracy / MCC, the epoch's val_loss —
 * is a function of a few per-task SUMS over the (molecule, task) pairs with a finite target, and sums add across batches.  This stage
 * adds one batch's sums into a persistent device buffer `stats` of doubles; the epoch ends with ONE copy of it to the host.
 *
 * stats = header[4] | task 0 | task 1 | ... (dmpnn_metric_stats_doubles() doubles; the caller zeroes it at the start of an epoch):
 *   header: [0] += loss[0] loss[1] and [1] += loss[1] — `loss` is the [loss, n_finite] pair a criterion wrote on the same stream
 *           (dmpnn_predict_head's loss_out), read by the stage's last launch; skipped when loss == NULL or loss[1] is not > 0, so the
 *           epoch's val_loss = stats[0] / stats[1] is the count-weighted mean over batches; [2] += 1 (calls); [3] += n_mols.
 *   DMPNN_METRIC_NONE: the header alone.
 *   DMPNN_METRIC_REGRESSION, 8 doubles per task: with m = target finite, e = p - t (p and t converted to double first), e_b = e but 0
 *           where (lt_mask and p < t) or (gt_mask and p > t) — BoundedMixin (nn/metrics.py:157-163), restated — the sums over m of
 *           1, e^2, |e|, t, t^2, e_b^2, |e_b|, and one reserved slot that is written as 0.  p = preds[i][j group]: element 0 of task
 *           j's group (group 1: plain / unscaled, 2: MVE / quantile, 4: evidential).
 *   DMPNN_METRIC_BINARY, 8 doubles per task: n, TP, FP, TN, FN and three reserved slots (written as 0).  Predicted class: p > threshold
 *           (strictly: torchmetrics' convention, restated); positive target: t > 0.5.  p = preds[i][j group] (group 1: sigmoid; 2:
 *           DMPNN_PT_DIRICHLET_BINARY, whose column 0 is p_1).
 *   DMPNN_METRIC_MULTICLASS, n_classes^2 doubles per task: the confusion counts [target class][argmax_k preds[i][j n_classes + k]];
 *           argmax takes the lowest index among equal maxima; a finite target is truncated to int, one outside [0, n_classes) is
 *           skipped like a NaN one.  2 <= n_classes <= DMPNN_METRIC_MAX_CLASSES, group is ignored.
 * Declared deviation — restated from chemprop 2.3.1 and not run against it: the statistics are UNWEIGHTED (validation and test run
 * with unit weights in the reference); head.weights and task_weights go into val_loss only.
 *
 * Two launches at most: a column reduction (row blocks of 128 molecules x column blocks of tasks; each leaves its partial sums in ws
 * [n_row_blocks][n_tasks per_task] doubles) and a finish that adds the partials in block order in double — exactly one thread performs
 * stats[k] += batch_sum for each slot, no floating-point atomics: the buffer after a call is bitwise reproducible for the same inputs
 * and the same starting contents.  DMPNN_METRIC_NONE is the finish alone.  n_mols == 0 launches nothing and leaves stats as it was.
 * DMPNN_EINVAL before any device work: an unknown kind; n_mols or n_tasks < 0; n_classes outside 2..DMPNN_METRIC_MAX_CLASSES
 * (multiclass); group outside {1, 2, 4}; a threshold that is not finite (binary); NULL preds / targets (kind != NONE) or stats; ld_p
 * below n_tasks group (multiclass: n_tasks n_classes) or ld_t below n_tasks; stats not 8-byte aligned; stats_bytes below 8
 * dmpnn_metric_stats_doubles().  DMPNN_ENOSPC: ws missing (where bytes are needed) or below dmpnn_metric_stats_ws_bytes(). */
enum dmpnn_metric_kind { DMPNN_METRIC_NONE = 0, DMPNN_METRIC_REGRESSION, DMPNN_METRIC_BINARY, DMPNN_METRIC_MULTICLASS };
#define DMPNN_METRIC_MAX_CLASSES 16
#define DMPNN_METRIC_HEADER 4              /* doubles in front of the tasks */
typedef struct dmpnn_metric_args {
    int32_t kind;                          /* enum dmpnn_metric_kind */
    int64_t n_mols, n_tasks;
    int32_t n_classes, group;              /* multiclass: classes per task; regression / binary: preds elements per task (1 | 2 | 4) */
    float threshold;                       /* binary: predicted class = p > threshold */
    const float* preds; int64_t ld_p;      /* [n_mols, n_tasks, group | n_classes], rows of ld_p floats */
    const float* targets; int64_t ld_t;    /* [n_mols, n_tasks], NaN = missing, rows of ld_t floats */
    const unsigned char* lt_mask; const unsigned char* gt_mask;   /* regression: [n_mols, n_tasks] bytes or NULL */
    const float* loss;                     /* device [loss, n_finite] of this batch or NULL */
    double* stats; size_t stats_bytes;     /* device, in / out */
    void* ws; size_t ws_bytes;             /* the row blocks' partials */
} dmpnn_metric_args;
size_t dmpnn_metric_stats_doubles(int32_t kind, int64_t n_tasks, int32_t n_classes);   /* 0: an unknown kind / bad sizes */
size_t dmpnn_metric_stats_ws_bytes(const dmpnn_metric_args* a);
int    dmpnn_metric_stats(const dmpnn_metric_args* a, void* stream);

/* One validation step behind the block as one call: predict_core exactly as dmpnn_predict_head runs it (same kernels, same bits), then
 * the stage above on predict.preds with loss = predict.head.loss_out — dmpnn_predict_head's launches plus at most two.  The stage's
 * partials live behind the head's layout in predict.head.ws: dmpnn_validate_head_ws_bytes() = dmpnn_predict_head_ws_bytes() + the
 * stage's.  n_tasks = n_out / (the transform's outputs per task), group = those outputs, n_classes = predict.head.n_classes; the
 * bounds are predict.head.lt_mask / gt_mask.  DMPNN_EINVAL before any device work (dmpnn_last_launch_count() as it was): whatever
 * dmpnn_predict_head refuses; no predict.head.targets, predict.head.loss_out or predict.preds; a kind the transform does not feed —
 * REGRESSION wants NONE / UNSCALE / MVE / EVIDENTIAL / QUANTILE, BINARY wants SIGMOID / DIRICHLET_BINARY, MULTICLASS wants SOFTMAX /
 * DIRICHLET_MULTICLASS with 2 <= n_classes <= DMPNN_METRIC_MAX_CLASSES, DMPNN_PT_SPECTRAL takes DMPNN_METRIC_NONE alone; ld_mt below
 * n_tasks; stats_bytes too small.  A workspace that is too small: DMPNN_ENOSPC.  n_mols == 0 launches nothing. */
typedef struct dmpnn_validate_args {
    dmpnn_predict_args predict;            /* as dmpnn_predict_head reads it */
    int32_t metric_kind;                   /* enum dmpnn_metric_kind */
    float threshold;                       /* DMPNN_METRIC_BINARY */
    const float* metric_targets; int64_t ld_mt;   /* [n_mols, n_tasks] the targets the metrics compare with, or NULL: predict.head.targets
                                              (a caller whose criterion's targets are scaled while the metrics' are not) */
    double* stats; size_t stats_bytes;
} dmpnn_validate_args;
size_t dmpnn_validate_head_ws_bytes(const dmpnn_validate_args* v);
int    dmpnn_validate_head(const dmpnn_validate_args* v, const float* Hv, int64_t ldhv, void* stream);

/* Epoch rank metrics (v15 growth: new entry points and structs, every existing struct and call as it was).  ROC-AUC and PRC-AUC of a
 * binary head are functions of RANKS, not of sums, so the epoch keeps every (score, label) pair — on the device, in a buffer the
 * caller owns — and the epoch ends with one all-pairs count and one copy of 8 (n_tasks + pooled) doubles.  No sort, no atomics of any
 * kind, a fixed order of additions: `out` is bitwise reproducible.
 *
 * The buffer: keys uint32 [capacity, n_tasks] and labels uint8 [capacity, n_tasks], contiguous, leading dimension n_tasks.  Row r is
 * the r-th molecule appended this epoch; the caller counts the rows on the host (every batch's n_mols is known there).
 *   key    the order-preserving uint32 image of the float32 score: -0.0 becomes +0.0, then sign bit set -> ~bits, else bits |
 *          0x80000000.  Compares are integer compares: flushing denormals can neither merge nor split ties.  A finite score never
 *          maps to 0; key 0 is "not ranked".
 *   label  0 negative, 1 positive (t > 0.5, DMPNN_METRIC_BINARY's rule); not ranked, with key 0: 2 where the target is NaN or not
 *          finite, 3 where the target is finite and the prediction is not — counted per task as n_skipped (a declared deviation: the
 *          reference would rank the garbage).
 * For one column, over its ranked elements, with s the score, for element i and all elements j (j = i included in the "equal" counts):
 *   gp_i, gn_i  positives / negatives with s_j > s_i;   ep_i, en_i  positives / negatives with s_j == s_i;
 *   first_i     no j < i (row order) has s_j == s_i: one representative per distinct threshold.
 *   ROC-AUC = U2 / (2 P N), U2 = sum over negative i of (2 gp_i + ep_i) — an integer, twice the Mann-Whitney count with ties counted
 *             half: the trapezoid under torchmetrics' BinaryAUROC(thresholds=None) curve.
 *   PRC-AUC = (1 / P) sum over i with first_i of ep_i (P_i + Pprev_i) / 2, P_i = (gp_i + ep_i) / (gp_i + ep_i + gn_i + en_i), Pprev_i =
 *             gp_i / (gp_i + gn_i), or 1 where nothing is strictly greater (the curve's appended point, recall 0 and precision 1):
 *             chemprop 2.3.1's BinaryAUPRC — auc(recall, precision) over BinaryPrecisionRecallCurve, trapezoid, no truncation.
 * Declared deviations — restated from chemprop 2.3.1 and not run against it: unweighted; a column without positives or without
 * negatives gives NaN for both (the reference warns and returns 0); n_skipped above.  The cost is quadratic in the keys ranked
 * together, bounded by DMPNN_RANK_MAX_ROWS (which also keeps the uint32 counters safe). */
#define DMPNN_RANK_MAX_ROWS 262144         /* keys ranked together (one column; the pooled column: rows n_tasks) */
#define DMPNN_RANK_TILE 2048               /* (key, label) pairs k_rank_pairs stages through LDS at a time */
#define DMPNN_RANK_OUT 8                   /* doubles per row of `out` */

/* One launch (k_rank_append, one thread per (molecule, task)): rows [row0, row0 + n_mols) of the buffer from preds [n_mols, n_tasks
 * group] (the score is element 0 of the task's group; group 1: sigmoid, 2: DMPNN_PT_DIRICHLET_BINARY, whose column 0 is p_1) and
 * targets [n_mols, n_tasks].  DMPNN_EINVAL before any device work: NULL pointers, negative sizes, group outside {1, 2}, ld_p below
 * n_tasks group or ld_t below n_tasks, n_mols n_tasks beyond one launch (2^31).  DMPNN_ENOSPC before any device work: row0 + n_mols >
 * capacity.  n_mols == 0 (or n_tasks == 0) launches nothing. */
typedef struct dmpnn_rank_append_args {
    int64_t n_mols, n_tasks;
    int32_t group;                         /* preds elements per task: 1 | 2 */
    const float* preds; int64_t ld_p;      /* rows of ld_p floats */
    const float* targets; int64_t ld_t;    /* NaN = missing, rows of ld_t floats */
    uint32_t* keys; unsigned char* labels; /* the epoch's buffer */
    int64_t capacity, row0;                /* rows the buffer holds; the first row this call writes */
} dmpnn_rank_append_args;
int    dmpnn_rank_append(const dmpnn_rank_append_args* a, void* stream);

/* dmpnn_validate_head exactly as it runs (same kernels, same bits in preds / raw / loss / stats), then the append launch on
 * predict.preds and metric_targets (predict.head.targets where that is NULL): dmpnn_validate_head's launches plus one.  It takes
 * metric_kind == DMPNN_METRIC_BINARY only.  DMPNN_EINVAL before any device work (dmpnn_last_launch_count() as it was): whatever
 * dmpnn_validate_head refuses, another metric_kind, NULL keys / labels, negative capacity / row0; DMPNN_ENOSPC: a workspace that is
 * too small (dmpnn_validate_head_ranked_ws_bytes() = dmpnn_validate_head_ws_bytes(): the append needs none) or row0 + n_mols >
 * capacity. */
typedef struct dmpnn_validate_rank_args {
    dmpnn_validate_args validate;          /* as dmpnn_validate_head reads it */
    uint32_t* keys; unsigned char* labels;
    int64_t capacity, row0;
} dmpnn_validate_rank_args;
size_t dmpnn_validate_head_ranked_ws_bytes(const dmpnn_validate_rank_args* r);
int    dmpnn_validate_head_ranked(const dmpnn_validate_rank_args* r, const float* Hv, int64_t ldhv, void* stream);

/* The epoch's end: out = double [n_tasks + pooled][8] = n_pos, n_neg, n_skipped, n_thresholds, U2, roc, prc, 0 per task column — counts
 * and U2 exact integers held in doubles, roc = U2 / (2 P N) (one division of exact integers), prc as above, both NaN where P == 0 or
 * N == 0.  pooled = 1 adds a last row that ranks all rows n_tasks pairs as ONE column (ClassificationMixin.update flattens
 * preds[mask] over tasks: the reference's pooling) — the same kernels on the contiguous buffer read as [rows n_tasks, 1]; its
 * n_skipped is the sum over tasks.  k_rank_pairs (one workgroup per 256 rows i and task; the column's j staged through LDS in tiles
 * of DMPNN_RANK_TILE; one partial per workgroup into ws) and k_rank_finish (one thread per column, the partials in block order): two
 * launches for the per-task rows, two more for the pooled row; rows == 0 launches nothing and leaves zeros for the counts and NaN
 * for roc / prc.  DMPNN_EINVAL before any device work: NULL keys / labels / out, out or ws not 8-byte aligned, rows < 0, n_tasks
 * outside [1, 65535], pooled outside {0, 1}, more than DMPNN_RANK_MAX_ROWS keys ranked together (rows, and rows n_tasks with pooled: a
 * caller above it passes pooled = 0).  DMPNN_ENOSPC: ws missing or below dmpnn_rank_metrics_ws_bytes(). */
typedef struct dmpnn_rank_args {
    const uint32_t* keys; const unsigned char* labels;
    int64_t rows, n_tasks;
    int32_t pooled;                        /* 0 | 1 */
    double* out;                           /* device, [n_tasks + pooled][DMPNN_RANK_OUT] */
    void* ws; size_t ws_bytes;             /* the workgroups' partials */
} dmpnn_rank_args;
size_t dmpnn_rank_metrics_ws_bytes(const dmpnn_rank_args* a);
int    dmpnn_rank_metrics(const dmpnn_rank_args* a, void* stream);

/* One training step of models/model.py:148-161 with torch.optim.Adam (model.py:208-231), every kernel enqueued by ONE call:
 * K0 (dmpnn_prepare_with_batch into bwd.f.plan unless plan_ready) -> dmpnn_forward(&bwd.f) (DMPNN_F_KEEP) -> dmpnn_head on
 * bwd.f.out (head.gHv must be bwd.gout) -> dmpnn_backward(&bwd) -> dmpnn_adam_step over the flat buffers (n_params == 0: no
 * optimizer step).  The argument structs are exactly those of the separate entry points; nothing is allocated. */
enum dmpnn_step_stage {                     /* dmpnn_step_args.stages: which part of the step this call enqueues (0 = all)  */
    DMPNN_STEP_FORWARD = 1,                 /* K0 + the block's forward + the head (forward AND backward: the head's gradients
                                               are final after this stage — a data-parallel job exchanges them while ...)    */
    DMPNN_STEP_BACKWARD = 2,                /* ... the block's backward pass runs                                             */
    DMPNN_STEP_UPDATE = 4                   /* the optimizer step                                                             */
};
typedef struct dmpnn_step_component {     /* a further block of a multicomponent model (one block per component): its batch */
    const int64_t* edge_index; const int64_t* rev_edge_index; const int64_t* batch; size_t plan_bytes; int32_t plan_ready;
    dmpnn_bwd_args bwd;                     /* bwd.f.out / bwd.gout: this component's rows of head's H_v / gHv (the rows after the
                                               previous component's, same row stride); every block's d_h is head.d_h             */
} dmpnn_step_component;

/* The atom-descriptor layer behind a block's finalize step (message_passing/base.py: H_v' = W_d cat(H_v, V_d) + b_d, no activation)
 * as a stage of its own (dmpnn_vd.hip): the block in front of it is then the plain W_d-free block.  The forward and the data
 * gradient: f16 matrix pipe, exact 3-term operand split, fp32 accumulation, at every shape.  The weight gradient gW_d / gb_d is
 * dmpnn_linear_wgrad's product: on the f16 pipe (operand split, product, reduce) from 1 024 atoms on when d_h + d_vd, ldhv, ldvd and
 * ldgout are even and the operands 8-byte aligned; otherwise its fp32 kernel plus the reduce (fp32-class either way).  Any d_vd >= 1 and any leading dimension >= its width (operands are read element by element and
 * zero-padded inside the split: odd widths and unaligned row strides included); d_h + d_vd <= DMPNN_VD_MAX_WIDTH, else DMPNN_EINVAL.
 * No gradient flows to V_d.  forward reads Hv V_d W_d b_d, writes out; backward reads gout Hv V_d W_d, writes gHv and (when not
 * NULL) gW_d [d_h+d_vd, d_h+d_vd] dense and gb_d.  n_atoms == 0: the requested gradients are zeroed.  Every argument check runs
 * before any device work.
 * dropout_p in (0, 1) (v15 growth; 0 — what a zero-filled block of an older caller carries — is no mask): the block's nn.Dropout once
 * more behind this layer (message_passing/base.py:185-188).  Element (atom r, column c) of out is kept iff
 * drop_hash(dropout_seed, DMPNN_DROP_SITE_VD, r, c) >= floor(p 2^32) (dmpnn_dropout_keep; c < d_h + d_vd <= 544 < 1024, the hash's
 * column range): forward writes out = keep ? (the p = 0 value) * (1.f / (1.f - p)) : +0.  Nothing of the mask is stored: backward
 * regenerates it and OVERWRITES gout IN PLACE with the masked gradient g' = keep ? gout * (1.f / (1.f - p)) : +0 (whether or not gW_d /
 * gb_d are asked for); gHv, gW_d and gb_d are all formed from g'.  A second dmpnn_vd_backward on the same gout would therefore mask
 * twice: the caller refills gout first.  A dropout_p so small that floor(p 2^32) == 0 (0 < p < 2^-32) keeps every element and its
 * float scale is 1: such a call is the p = 0 call (no mask, no scale, gout not written), as in the other homes.  dropout_p outside
 * [0, 1): DMPNN_EINVAL. */
#define DMPNN_VD_MAX_WIDTH 544
#define DMPNN_DROP_SITE_VD 0x8000          /* dmpnn_vd_args.dropout_p: the mask site behind W_d (the block's sites are 0 .. depth-1, the predictor's start at DMPNN_DROP_SITE_FFN) */
typedef struct dmpnn_vd_args {
    int64_t n_atoms, d_h, d_vd;            /* rows; width of H_v; width of V_d (>= 1)                    */
    const float* Hv;  int64_t ldhv;        /* [n_atoms, d_h]   the block's output                        */
    const float* V_d; int64_t ldvd;        /* [n_atoms, d_vd]  already through V_d_transform             */
    const float* W_d; const float* b_d;    /* [d_h+d_vd, d_h+d_vd] nn.Linear layout; [d_h+d_vd]          */
    float* out; int64_t ldout;             /* [n_atoms, d_h+d_vd]  = cat(Hv, V_d) . W_d^T + b_d (no act) */
    const float* gout; int64_t ldgout;     /* backward: dL/dout (dropout_p > 0: WRITTEN, see above)      */
    float* gHv; int64_t ldghv;             /* backward: dL/dHv [n_atoms, d_h] = gout . W_d[:, :d_h]      */
    float* gW_d; float* gb_d;              /* backward: out, or NULL (not wanted)                        */
    void* ws; size_t ws_bytes;             /* >= dmpnn_vd_ws_bytes()                                     */
    float dropout_p; uint64_t dropout_seed; /* v15 growth: the mask on out / gout (0: none)               */
} dmpnn_vd_args;
size_t dmpnn_vd_ws_bytes(const dmpnn_vd_args* a);
int dmpnn_vd_forward(const dmpnn_vd_args* a, void* stream);
int dmpnn_vd_backward(const dmpnn_vd_args* a, void* stream);

typedef struct dmpnn_step_args {
    const int64_t* edge_index; const int64_t* rev_edge_index; const int64_t* batch; size_t plan_bytes; int32_t plan_ready;
    int32_t stages;
    dmpnn_bwd_args bwd;                     /* bwd.f: the forward of the block                                     */
    dmpnn_head_args head;
    float* p; const float* g; float* m; float* v; int64_t n_params;   /* flat parameter / gradient / moment buffers */
    float lr, beta1, beta2, eps, weight_decay, bias_corr1, sqrt_bias_corr2, grad_scale; const float* dev_scalars;
    float clip_val; int32_t clip_mode; float* clip_ws;   /* v12: clip_val > 0: dmpnn_clip_grad(g, ...) before the update (g is then written) */
    int32_t n_extra; const dmpnn_step_component* extra;  /* v15 growth: a multicomponent model with head.n_components = 1 + n_extra blocks
                                               (component 0 is the fields above); each block's K0 and forward, the head once on the
                                               merged batch, each block's backward.  n_extra = 0 with head.n_components > 1: ONE shared
                                               block over the merged batch (the components' graphs as one BatchMolGraph)             */
    const dmpnn_vd_args* vd;                /* v15 growth: NULL (what an older caller passes): none.  Else the atom-descriptor layer between
                                               the block and the head: K0 -> block forward into vd->Hv -> dmpnn_vd_forward -> the head on
                                               vd->out -> dmpnn_vd_backward into bwd.gout -> block backward -> update.  Requires
                                               bwd.f.W_d == NULL, bwd.f.out == vd->Hv, bwd.gout == vd->gHv, head.gHv == vd->gout,
                                               head.d_h == bwd.f.d_h + vd->d_vd, equal atom counts, n_extra == 0, head.n_components <= 1.
                                               vd->dropout_p > 0 requires bwd.f.dropout_p == vd->dropout_p and the same seed (one
                                               nn.Dropout module in the reference), else DMPNN_EINVAL.
                                               Staged: the layer's forward belongs to DMPNN_STEP_FORWARD, its backward to
                                               DMPNN_STEP_BACKWARD (its gradients lie in the block's slice of the flat buffer) */
} dmpnn_step_args;
int dmpnn_train_step(const dmpnn_step_args* a, void* stream);

/* The dropout mask of dmpnn_fwd_args.dropout_p as a HOST function (tests pin oracle/dropout_hash.py on it): 1 when element
 * (site, row, col) is kept under `seed` and `p`. */
int dmpnn_dropout_keep(uint64_t seed, int32_t site, int64_t row, int64_t col, float p);

int dmpnn_version(void);
/* Debug aid: a device buffer of 128 int64 that one workgroup of a kernel fills with shader-clock stamps at its phase boundaries
 * (NULL switches it off; never set in production): [0, 32) the whole-forward tile kernel / the per-step fused kernel, [32, 64) K0,
 * [64, 80) the head's row kernels, [80, 96) and [96, 112) its column kernels (scripts/probe_stamps*.py, scripts/probe_head_rows.py). */
int dmpnn_debug_timestamps(void* device_buf);
/* Debug aid (v14): on != 0 — after EVERY kernel launch of the library the whole LDS of every CU is filled with a NaN pattern (on the
 * legacy default stream), so that a kernel that reads LDS it never wrote shows it as a NaN instead of a leftover of the previous kernel
 * (LDS is not cleared between launches).  Also DMPNN_DEBUG_LDS_POISON=1 in the environment.  Never set in production. */
void dmpnn_debug_lds_poison(int on);
const char* dmpnn_last_error_string(void);
/* Number of kernels the last dmpnn_forward on this thread enqueued (diagnostics). */
int dmpnn_last_launch_count(void);

#ifdef __cplusplus
}
#endif
#endif /* DMPNN_H */
