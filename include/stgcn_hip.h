/*
 * stgcn_hip.h — C ABI of libstgcn_hip.so: the MI355X (gfx950) ST-GCN stem.
 *
 * The reference (zjtggssg/ST-GCN-AltFormer) is pure Python/PyTorch and has no FFI of
 * its own; the boundary it offers for this path is two nn.Modules.  Each entry point
 * below replaces the torch ops executed inside one of their forward() bodies, so that
 * a re-implementation of those modules (st-gcn-altformer_amd/model/{unit_agcn,net}.py,
 * bound with ctypes — see INTEGRATION.md) is a drop-in:
 *
 *   stgcn_agcn_attention / stgcn_agcn_forward   <- model/unit_agcn.py:73-93  (unit_agcn.forward)
 *   stgcn_tcn_*                                 <- model/net.py:47-57        (Unit2D.forward, dim=2)
 *   stgcn_stem_*                                <- model/AltFormer/ST_GCN_AltFormer.py:70-72
 *                                                  (tcn0(gcn0(x)) fused, intermediate kept on chip)
 *   stgcn_bn_fold                               <- eval-mode nn.BatchNorm2d at unit_agcn.py:54,60, net.py:40
 *   stgcn_st_attention_*                        <- model/ST_TR/gcn_attention.py:96-156 (gcn_unit_attention.forward)
 *   stgcn_vit_*                                 <- model/AltFormer/model_ST.py:18-88 (Mlp, Attention, Block; eval forward)
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer owned by the caller (e.g. the PyTorch caching
 *     allocator).  The library allocates nothing, frees nothing, keeps no global mutable
 *     state and never synchronises: all work is enqueued on `stream` (a hipStream_t
 *     passed as void*; NULL = the default stream).  Safe to call from several host
 *     threads / devices concurrently (the caller selects the device, as PyTorch does).
 *   - Streams.  Everything a call does - every kernel, memset and copy - is ordered on `stream` and on
 *     nothing else, and no call waits on the host: a call may be enqueued behind work that has not
 *     run yet, its inputs may be written by that work, and every entry point may be captured into a
 *     graph and replayed under new inputs (tests/test_stream_order_gpu.py; DESIGN.md section 4, "Streams").
 *   - Tensors are dense row-major fp32 unless stated: x is (N, C, T, V) exactly as
 *     unit_agcn.forward receives it.
 *   - Return value: 0 on success, a negative stgcn_status otherwise; the message for the
 *     calling thread is available from stgcn_last_error().  Nothing throws or exits.
 *   - `flags`: low 4 bits select the arithmetic of the temporal-conv contraction
 *     (stgcn_math); STGCN_OUT_BF16 stores the final activation as bf16.
 *   - Extents: an entry point is correct at every size it accepts, tensors past 2^31 elements
 *     included, or returns STGCN_ERR_UNSUPPORTED before anything is launched.  Two bounds hold
 *     wherever nothing else is said: at most 65535 clips a call where the clip rides on a grid
 *     axis (the graph conv, the stem, the temporal conv's inference and backward, the ST-TR
 *     unit, stgcn_patch_embed, the whole head), and fewer than 2^32 work-items a launch
 *     (workgroups times their threads), which bounds "any M / B / S" below: see each entry.
 *   - Alignment.  TENSOR OPERANDS - inputs, parameters, cotangents, results, a caller's `out` -
 *     need the alignment of their element only: 4 bytes for fp32, 2 bytes for bf16 (8 for the
 *     int64 labels / pred of stgcn_step_stats).  A dense view at any element offset is served in
 *     place: a batch slice x[1:], a parameter inside a flat buffer, a slice of a larger gradient.
 *     The exceptions are the operands an entry point lists by name ("16-byte aligned" in its
 *     comment): the ST-ViT ends (stgcn_vit_patch_embed: z, W; its backward: z, W, dx;
 *     stgcn_vit_pool: x, out; stgcn_vit_pool_classify: x, W; its backward: x, dx), head_weight of
 *     stgcn_altformer_head_forward, and m_proj, m_fc2, dy of stgcn_vit_block_backward_drop when a
 *     mask is given.  BLOBS AND WORKSPACES - everything sized by a *_bytes query or made by the
 *     library: prep, Wp, ws, the saved buffers - need 256 bytes, as the allocator gives them
 *     (they are read by LDS-DMA and hold the targets of fp64 atomics); save_stats of the graph
 *     conv's training pair keeps its 8.  An operand that misses its demand is refused with
 *     STGCN_ERR_ARG before anything is launched or written, the message names it, and the next
 *     correct call succeeds.  Checked on the host: 256 bytes for prep / ws of stgcn_stem_*, Wp / ws
 *     of stgcn_tcn_pack / _forward_packed / _forward and ws of the agcn, tcn and st_attention
 *     training and forward entry points; 16 bytes for the listed operands and the ws of their
 *     entry points.  DESIGN.md section 4 ("Operand alignment") has the table of accesses behind
 *     this.
 */
#ifndef STGCN_HIP_H
#define STGCN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STGCN_ABI_VERSION 11

typedef enum {
    STGCN_OK = 0,
    STGCN_ERR_ARG = -1,          /* null pointer / non-positive dimension / an operand off its alignment */
    STGCN_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels cover  */
    STGCN_ERR_WORKSPACE = -3,    /* caller workspace too small            */
    STGCN_ERR_HIP = -4           /* a HIP runtime call failed             */
} stgcn_status;

typedef enum {
    STGCN_MATH_F32 = 0,      /* v_mfma_f32_32x32x2_f32: exact fp32 fma chain (default)      */
    STGCN_MATH_BF16X3 = 1,   /* fp32 split into bf16 hi+lo, 3 bf16 MFMAs, fp32 accumulate   */
    STGCN_MATH_BF16 = 2,     /* operands rounded to bf16, fp32 accumulate                   */
    STGCN_MATH_F32_VALU = 3  /* plain fp32 VALU kernels (any shape; on-device cross-check)  */
} stgcn_math;

#define STGCN_MATH_MASK 0xFu
#define STGCN_OUT_BF16 0x10u
#define STGCN_RAW 0x20u /* stgcn_tcn_*: store scale-folded conv + shift WITHOUT the ReLU (pre-activation) */
/* Layout fusion with the callers either side of the stem (stgcn_stem_* entry points only):
 *   STGCN_IN_NTVC : x is (N,T,V,Cin), the layout the data loader delivers — replaces the permute + contiguous copy
 *                   at model/AltFormer/ST_GCN_AltFormer.py:62-68;
 *   STGCN_OUT_NTVC: out is (N,T,V,C), channels last — `rearrange 'b c f p -> (b f) p c'` (model_ST.py:152) and
 *                   `'b c f p -> (b p) f c'` (model_TS.py:161) then are views, not copies. */
#define STGCN_IN_NTVC 0x40u
#define STGCN_OUT_NTVC 0x80u
/* stgcn_patch_embed: rows ordered (clip, joint, frame) — model_TS.py:161 — instead of (clip, frame, joint) */
#define STGCN_EMBED_TS 0x100u
/* stgcn_*_forward_train / stgcn_*_backward_train: BatchNorm on its RUNNING statistics (module.eval() with autograd — frozen-
 * BatchNorm fine-tuning, saliency; the reference's nn.BatchNorm2d stays differentiable in eval mode, model/net.py:52,
 * model/unit_agcn.py:54,91).  Forward: normalises with running_mean / running_var, leaves both untouched, and saves them as
 * (mean, invstd).  Backward: mean and invstd are constants — dz = gamma*invstd*g, dgamma = sum g*xhat, dbeta = sum g. */
#define STGCN_BN_FROZEN 0x200u
/* stgcn_stem_* entry points, with STGCN_MATH_BF16X3: where the kernel covers the shape (V <= ~25 joints, C % 128 == 0, K = 9)
 * the fused stem's temporal conv runs as fp16 x fp16 plus two block-scaled e4m3 residual products
 * (v_mfma_scale_f32_16x16x128_f8f6f4) instead of three bf16 products: the same 1e-4 contract (measured 2-4e-5 of max|ref|,
 * tools/math_error_2term.py) at two thirds of the matrix-core cycles.  Everything else about the call is unchanged; shapes
 * outside the kernel run the three-bf16 kernels.  The flag must be the same in stgcn_stem_prep_bytes / _prepare /
 * _ws_bytes / _attention / _tail (the prep blob carries a third weight packing, the workspace a per-clip bound). */
#define STGCN_STEM_F16MX 0x400u
/* stgcn_tcn_forward[_packed] with STGCN_MATH_F32_VALU: the 1-D convolution runs along the JOINT axis (Unit2D(dim=3),
 * model/net.py:28-36: kernel (1,K), padding (0,pad), stride (1,stride)); y is (N,Cout,T,V_out), V_out = (V+2*pad-K)/stride+1.
 * Inference only; no reference model builds this variant (plain-FMA kernel). */
#define STGCN_CONV_ALONG_V 0x800u

int stgcn_version(void);
const char *stgcn_last_error(void);

/* ---- eval-mode BatchNorm folding -------------------------------------------------------
 * scale[c] = weight[c] / sqrt(running_var[c] + eps)
 * shift[c] = bias[c] + (conv_bias[c] - running_mean[c]) * scale[c]      (conv_bias may be NULL)
 */
int stgcn_bn_fold(const float *weight, const float *bias, const float *running_mean,
                  const float *running_var, const float *conv_bias, float eps, float *scale,
                  float *shift, int C, void *stream);

/* ---- adaptive graph convolution (unit_agcn) -------------------------------------------
 * A_eff (S,V,V) = self.A + self.PA (unit_agcn.py:75-76), any dense values.
 * Wa,Wb (S,inter_c,Cin), ba,bb (S,inter_c)  : conv_a / conv_b 1x1 weights and biases
 * Wd (S,Cout,Cin), bd (S,Cout)              : conv_d
 * Wdown (Cout,Cin), bdown (Cout)            : down[0]; pass NULL for both when Cin == Cout
 *                                             (the reference then adds x itself, :57-58)
 * bn_scale/bn_shift, down_scale/down_shift  : folded eval BatchNorm of self.bn / down[1]
 *
 * stgcn_agcn_attention: P[n,s,v,w] = softmax_v( sum_{c,t} a[c,t,v] b[c,t,w] / (inter_c*T) ) + A_eff[s,v,w]
 *                       (unit_agcn.py:81-85); P is (N,S,V,V).
 * stgcn_agcn_forward  : the whole forward; P_ws (N,S,V,V) is caller workspace and holds P on return;
 *                       y is (N,Cout,T,V).
 */
int stgcn_agcn_attention(const float *x, const float *A_eff, const float *Wa, const float *ba,
                         const float *Wb, const float *bb, float *P, int N, int Cin, int T, int V,
                         int inter_c, int subsets, void *stream);

int stgcn_agcn_forward(const float *x, const float *A_eff, const float *Wa, const float *ba,
                       const float *Wb, const float *bb, const float *Wd, const float *bd,
                       const float *Wdown, const float *bdown, const float *bn_scale,
                       const float *bn_shift, const float *down_scale, const float *down_shift,
                       float *P_ws, float *y, int N, int Cin, int Cout, int T, int V, int inter_c,
                       int subsets, void *stream);
/* Names, with template arguments, of the kernels that compute P and y for a shape ("attention_folded_kernel<4,16>",
 * "agcn_expand_mfma_kernel<1,16>", ...; "" when the call is refused) — for profilers and benchmarks that match kernel
 * names in rocprofv3 output.  extra: what the attention writes besides P — 0 nothing (stgcn_agcn_attention and the
 * forwards), 1 the fused stem's features, 2 its attention fragments, 3 the fragments of a wide frame's joint split.
 * has_down: Wdown is given.  (additive, ABI 11) */
const char *stgcn_agcn_attention_kernel_name(int N, int Cin, int T, int V, int inter_c, int subsets, int extra);
const char *stgcn_agcn_expand_kernel_name(int N, int Cin, int Cout, int T, int V, int subsets, int has_down);

/* ---- temporal conv block (Unit2D, dim=2) -----------------------------------------------
 * W (Cout,Cin,K) = conv.weight with the trailing 1 squeezed; pad = (K-1)/2; T_out = (T+2*pad-K)/stride+1.
 * scale/shift = folded BN (shift includes the conv bias).  y is (N,Cout,T_out,V), fp32 or bf16
 * (STGCN_OUT_BF16).
 *
 * The contraction reads W re-ordered into MFMA fragment order with `scale` multiplied in
 * ("packed").  Pack once per weight update with stgcn_tcn_pack into a buffer of
 * stgcn_tcn_packed_bytes() bytes, then call stgcn_tcn_forward_packed per batch; or call
 * stgcn_tcn_forward, which packs into `ws` (>= stgcn_tcn_packed_bytes) on every call.
 */
size_t stgcn_tcn_packed_bytes(int Cin, int Cout, int K, unsigned flags);
/* 1 when the matrix-core kernel of `flags` covers the shape, 0 when only STGCN_MATH_F32_VALU does */
int stgcn_tcn_supported(int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
/* Name of the kernel stgcn_tcn_forward[_packed] launches for the shape ("tcn_bf16_v6_kernel", "tcn_bf16_v4_kernel",
 * "tcn_mfma_bf16_kernel", "tcn_mfma_f32_kernel", "tcn_valu_kernel", "tcn_valu_joint_axis_kernel"; "" when the call is
 * refused) — for profilers and benchmarks that match kernel names in rocprofv3 output.  (ABI 11) */
const char *stgcn_tcn_kernel_name(int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
int stgcn_tcn_pack(const float *W, const float *scale, void *Wp, int Cin, int Cout, int K,
                   unsigned flags, void *stream);
int stgcn_tcn_forward_packed(const float *x, const void *Wp, const float *shift, void *y, int N,
                             int Cin, int Cout, int T, int V, int K, int stride, unsigned flags,
                             void *stream);
int stgcn_tcn_forward(const float *x, const float *W, const float *scale, const float *shift,
                      void *y, int N, int Cin, int Cout, int T, int V, int K, int stride, void *ws,
                      size_t ws_bytes, unsigned flags, void *stream);

/* ---- fused stem: tcn0(gcn0(x)) ----------------------------------------------------------
 * Same operands as the two calls above (the temporal conv has Cin = Cout = C, stride 1).
 * The (N,C,T,V) activation between the two modules is produced tile by tile in LDS and never
 * written to HBM.  `prep` holds the folded graph-conv weights and the packed temporal weights:
 * fill it with stgcn_stem_prepare (stgcn_stem_prep_bytes bytes) once per weight update.
 */
size_t stgcn_stem_prep_bytes(int Cin, int C, int K, int subsets, unsigned flags);
/* 1 when the fused kernel covers the shape (else run stgcn_agcn_forward + stgcn_tcn_forward) */
int stgcn_stem_supported(int Cin, int C, int T, int V, int K, int subsets, unsigned flags);
int stgcn_stem_prepare(const float *Wd, const float *bd, const float *Wdown, const float *bdown,
                       const float *bn_scale, const float *bn_shift, const float *down_scale,
                       const float *down_shift, const float *Wt, const float *t_scale, void *prep,
                       int Cin, int C, int K, int subsets, unsigned flags, void *stream);
/* Workspace of the fused stem (caller-provided, stgcn_stem_ws_bytes bytes): the attention matrices
 * P (N,S,V,V) at offset 0 (valid on return), then whatever the chosen kernel reads besides them. */
size_t stgcn_stem_ws_bytes(int N, int Cin, int C, int T, int V, int K, int subsets, unsigned flags);
/* Name of the kernel stgcn_stem_tail_prepared launches for the shape ("stem_f16mx_kernel", "stem_bf16_v6_kernel",
 * "stem_bf16_v4_kernel", "stem_mfma_bf16_kernel", "stem_mfma_f32_kernel"; "" when no fused kernel covers it) — for
 * profilers and benchmarks that match kernel names in rocprofv3 output. */
const char *stgcn_stem_kernel_name(int Cin, int C, int T, int V, int K, int subsets, unsigned flags);
/* stem_bf16_v6_kernel in bf16x3 on narrow frames (V <= 32) gives a clip's last tile of at most 128 pixels a half-size form and
 * then walks the tiles in contiguous runs balanced by cost (a full tile 2 units, a short one 1).  Two queries for tests and
 * tools: the 16-row blocks of its image the taps of that short tile read (0 when the shape has no short form), and the run
 * [*first, *end) of clip-major tile indices that workgroup wg of a launch on num_wg compute units walks over nclips clips
 * of tiles_per_clip tiles (short_last = 0: every tile costs the same). */
int stgcn_stem_short_tile_blocks(int C, int T, int V, int K);
int stgcn_stem_walk_run(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *first, int *end);
/* The tiles of that run in the ORDER the workgroup walks them (two store phases: a workgroup with bit 3 of its index set walks
 * the first short tile of its run first, then the rest in order).  *count = the number of tiles of the run; the first
 * min(cap, *count) of them are written to tiles (which may be NULL with cap = 0).  Additive: the ABI version stays. */
int stgcn_stem_walk_order(int wg, int num_wg, int nclips, int tiles_per_clip, int short_last, int *tiles, int cap, int *count);
/* 1 when one of the large-tile kernels serves the shape (stem_bf16_v4/_v6/_f16mx_kernel): the workspace then holds,
 * behind P, graph-conv features or attention fragments that stgcn_stem_attention writes for the kernel */
int stgcn_stem_features_used(int Cin, int C, int T, int V, int K, int subsets, unsigned flags);
/* The two halves of stgcn_stem_forward_prepared, separately launchable (e.g. to time them):
 * stgcn_stem_attention fills the workspace; stgcn_stem_tail_prepared launches only the fused
 * graph-conv + temporal-conv kernel on a filled workspace. */
int stgcn_stem_attention(const float *x, const float *A_eff, const float *Wa, const float *ba,
                         const float *Wb, const float *bb, void *ws, size_t ws_bytes, int N, int Cin,
                         int C, int T, int V, int inter_c, int subsets, int K, unsigned flags,
                         void *stream);
int stgcn_stem_tail_prepared(const float *x, const void *ws, size_t ws_bytes, const void *prep,
                             const float *t_shift, void *out, int N, int Cin, int C, int T, int V,
                             int subsets, int K, unsigned flags, void *stream);
int stgcn_stem_forward_prepared(const float *x, const float *A_eff, const float *Wa,
                                const float *ba, const float *Wb, const float *bb,
                                const void *prep, const float *t_shift, void *ws, size_t ws_bytes,
                                void *out, int N, int Cin, int C, int T, int V, int inter_c,
                                int subsets, int K, unsigned flags, void *stream);

/* ---- training-mode forward (batch-statistics BatchNorm) ------------------------------------------
 * Same math as the eval entry points, but every BatchNorm2d normalises with the statistics of the
 * batch over (N,T,V) and updates its running buffers in place exactly like torch (momentum, unbiased
 * variance); num_batches_tracked is the caller's to increment.  bn_* / dbn_* are the raw BatchNorm
 * tensors (weight, bias, running_mean, running_var), not folded scale/shift.  `ws` is caller workspace
 * of stgcn_*_train_ws_bytes bytes.
 *   stgcn_agcn_forward_train <- model/unit_agcn.py:73-93 with self.training (P_ws, y as in stgcn_agcn_forward)
 *   stgcn_tcn_forward_train  <- model/net.py:47-57 with self.training (dropout p = 0)
 */
/* materialise = 1: room for the two pre-BatchNorm branches (when save_zm/save_zd are wanted, or the shape is outside
 * the stem class); 0: the stem class (C_in=3, 3 subsets, down branch) derives the batch statistics from the moments of its
 * 12 per-pixel features and never writes the branches — scratch of a few hundred KB. */
size_t stgcn_agcn_train_ws_bytes(int N, int Cin, int Cout, int T, int V, int subsets, int materialise);
int stgcn_agcn_forward_train(const float *x, const float *A_eff, const float *Wa, const float *ba,
                             const float *Wb, const float *bb, const float *Wd, const float *bd,
                             const float *Wdown, const float *bdown, const float *bn_weight,
                             const float *bn_bias, float *bn_running_mean, float *bn_running_var,
                             const float *dbn_weight, const float *dbn_bias, float *dbn_running_mean,
                             float *dbn_running_var, float momentum, float eps, float *P_ws, void *ws,
                             size_t ws_bytes, float *y, float *save_zm, float *save_zd, float *save_stats,
                             int N, int Cin, int Cout, int T, int V, int inter_c, int subsets,
                             unsigned flags /* 0 or STGCN_BN_FROZEN (then size ws with materialise = 1) */, void *stream);
/* save_zm / save_zd (N,Cout,T,V): the two pre-BatchNorm branches (sum_s conv_d_s(x P_s), conv_down(x)) — asking for
 * them selects the materialising path; save_stats (STGCN_AGCN_SAVE_STATS_FLOATS(Cout) floats, 8-byte aligned): batch
 * mean, invstd of `bn`, then of the down BatchNorm (4*Cout), followed — on the moments path only — by the 63 feature
 * moments as doubles, which the stem-class backward reads back, and a validity mark in one of the two spare floats
 * behind them (ABI 8): the materialising path clears that block, and the moment-form backward answers NaN in every
 * gradient when it is handed statistics without the mark (a forward that saved the branches, followed by a backward
 * call with zm == NULL) instead of working from uninitialised moments.  All optional (NULL). */
#define STGCN_AGCN_SAVE_STATS_FLOATS(Cout) (4 * (Cout) + 128)
/* recompute: bit 0 = zm / zd are not supplied (the forward ran the moments path; the generic path rebuilds them in the
 * workspace, the stem-class path never needs them); bit 1 = size for the generic path — needed when an input gradient
 * is wanted (dx != NULL), with the identity residual, or for a shape outside the stem class (the call below picks the
 * path from its arguments; size for what you will ask).  0 for an invalid size. */
size_t stgcn_agcn_backward_ws_bytes(int N, int Cin, int Cout, int T, int V, int subsets, int recompute);
/* Gradients of every parameter of unit_agcn (model/unit_agcn.py:35-62) from dy (N,Cout,T,V) in training mode:
 * dWa/dWb (S,inter_c,Cin), dba/dbb (S,inter_c), dWd (S,Cout,Cin), dbd (S,Cout), dWdown (Cout,Cin), dbdown, the
 * two BatchNorms' dgamma/dbeta (main, then "dd" = down), dPA (S,V,V), and — optionally — dx (N,Cin,T,V), the gradient
 * of the input that the deeper TCN_GCN_unit layers need (model/ST_TR/ST_TR_new.py:355-372); NULL when x is data.
 * Identity residual (Cin == Cout, unit_agcn.py:57-58): pass NULL for Wdown, bdown, the down BatchNorm tensors, zd and
 * the four down-gradient outputs.  zm / zd: the branches the forward saved, or NULL.  y: the forward's output.
 * Two implementations:
 *   - the stem's shape class (Cin = 3, 3 subsets, Cout in {64,128,256}, down branch, no dx) with zm == zd == NULL and
 *     y != NULL — i.e. after a moments-path forward whose save_stats carries the feature moments: ONE pass over dy / y
 *     (fp32 MFMA), everything else from moments (csrc/agcn_backward.hip; no branch is rebuilt, no statistics pass);
 *   - a chain of strided batched fp32-MFMA GEMMs for everything else (V <= 64, inter_c <= Cout/4, N * subsets <= 65535: a
 *     batch entry per (clip, subset) pair; else STGCN_ERR_UNSUPPORTED before anything is launched); y is not read. */
int stgcn_agcn_backward_train(const float *x, const float *A_eff, const float *Wa, const float *ba,
                              const float *Wb, const float *bb, const float *Wd, const float *bd,
                              const float *Wdown, const float *bdown, const float *P, const float *zm,
                              const float *zd, const float *bn_weight, const float *bn_bias,
                              const float *dbn_weight, const float *dbn_bias, const float *save_stats,
                              const float *y, const float *dy, float *dWa, float *dba, float *dWb, float *dbb, float *dWd,
                              float *dbd, float *dWdown, float *dbdown, float *dgamma, float *dbeta,
                              float *ddgamma, float *ddbeta, float *dPA, float *dx, void *ws, size_t ws_bytes,
                              int N, int Cin, int Cout, int T, int V, int inter_c, int subsets,
                              unsigned flags /* 0 or STGCN_BN_FROZEN (generic path: size ws with recompute bit 1) */, void *stream);
size_t stgcn_tcn_train_ws_bytes(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
/* save_z (N,Cout,T_out,V), save_mean, save_invstd (Cout): optional outputs for the backward — the raw
 * convolution conv_t(x)+b and the batch statistics, torch's save_mean / save_invstd.  NULL: not kept. */
int stgcn_tcn_forward_train(const float *x, const float *W, const float *conv_bias,
                            const float *bn_weight, const float *bn_bias, float *bn_running_mean,
                            float *bn_running_var, float momentum, float eps, void *ws, size_t ws_bytes,
                            float *y, float *save_z, float *save_mean, float *save_invstd, int N, int Cin,
                            int Cout, int T, int V, int K, int stride, unsigned flags, void *stream);

/* ---- backward of the training-mode blocks ------------------------------
 * What autograd derives for y = relu(BatchNorm_batch(conv_t(x) + b)) (model/net.py:47-57 under
 * train_sttran.py:185-191) from dy (N,Cout,T_out,V):
 *   dW (Cout,Cin,K), dbias (Cout, NULL when the conv has no bias), dgamma / dbeta (Cout) of the
 *   BatchNorm, and dx (N,Cin,T,V; NULL when the input needs no gradient).
 * z, save_mean, save_invstd are the tensors stgcn_tcn_forward_train saved.  The weight gradient
 * runs on the bf16 matrix cores with the arithmetic of `flags` (BF16X3: fp32 contract) where the
 * shape allows (stride 1, Cout%128==0, Cin%32==0, K<=9), on plain fp32 FMAs otherwise; the input
 * gradient of a stride-1 block is the forward kernel on the flipped weights. */
size_t stgcn_tcn_backward_ws_bytes(int N, int Cin, int Cout, int T, int V, int K, int stride, unsigned flags);
int stgcn_tcn_backward_train(const float *x, const float *W, const float *z, const float *bn_weight,
                             const float *bn_bias, const float *save_mean, const float *save_invstd,
                             const float *dy, float *dx, float *dW, float *dbias, float *dgamma,
                             float *dbeta, void *ws, size_t ws_bytes, int N, int Cin, int Cout, int T,
                             int V, int K, int stride, unsigned flags, void *stream);

/* ---- first patch embedding of the transformer heads, on the stem's output -----------------------------
 * What the callers do next with z = tcn0(gcn0(x)):
 *   ST head: rearrange 'b c f p -> (b f) p c', Spatial_patch_to_embedding = nn.Linear(C, E), += Spatial_pos_embed
 *            (model/AltFormer/model_ST.py:101-103,152-155)                      -> out ((N*T), V, E)
 *   TS head: rearrange 'b c f p -> (b p) f c', temporal_patch_to_embedding = nn.Linear(C, E), += Temporal_pos_embed
 *            (model/AltFormer/model_TS.py:110-111,161-163; STGCN_EMBED_TS)      -> out ((N*V), T, E)
 * as ONE strided GEMM per clip: the rearrange is the addressing of the product, no copy of z is made.
 * z: (N,C,T,V), or (N,T,V,C) with STGCN_IN_NTVC (what stgcn_stem_* writes with STGCN_OUT_NTVC);
 * W (E,C) = Linear.weight, b (E) = Linear.bias, pos: (V,E) [ST] / (T,E) [TS] or NULL.  fp32 throughout (exact fp32
 * matrix-core arithmetic).  out fp32, dense. */
int stgcn_patch_embed(const float *z, const float *W, const float *b, const float *pos, float *out, int N, int C,
                      int E, int T, int V, unsigned flags, void *stream);

/* ---- data-parallel harness -------------------------------------------------------------------
 * Per-rank reductions that the ranks all-reduce once per step — the data-parallel form of the
 * reference's accuracy reduction get_acc (SHREC/ST_TS/train_sttran.py:105-109: np.argmax of the
 * logits on the host, compared with the labels, summed): stats[0] = n_local, stats[1] = sum probe,
 * stats[2] = sum probe^2, stats[3] = #{n : argmax_c logits[n][c] == labels[n]}, with
 * probe[n][c] = out[n][c][0][0] = element n*clip_stride + c*chan_stride of `out` (ABI 8: element strides instead of a
 * plane size, so the channels-last result of STGCN_OUT_NTVC — clip_stride = T*V*C, chan_stride = 1 — is probed in place;
 * a dense (N,C,T,V) tensor has clip_stride = C*T*V, chan_stride = T*V).
 * logits (n_logits, classes) fp32 and labels (n_logits) int64 are optional (NULL: stats[3] = 0);
 * pred (n_logits) int64, optional, receives the class indices.  argmax follows numpy: the lowest
 * index among equal maxima, a NaN is the maximum.  `out` may be NULL when only the count is wanted.
 * One launch, one workgroup. */
int stgcn_step_stats(const void *out, int out_is_bf16, float *stats, int N, int C, long clip_stride,
                     long chan_stride, float n_local, const float *logits, const long long *labels, long long *pred,
                     int n_logits, int classes, void *stream);

/* ---- ST-TR spatial self-attention unit (gcn_unit_attention, ABI 9) ---------------------------------------------------
 * model/ST_TR/gcn_attention.py:96-156 with spatial_transformer.py:82-156, in the configuration the reference's scripts
 * build (only_attention, data_normalization, skip_conn, bn_flag, drop_connect; no relative / adjacency / more_channels):
 *   xn = data_bn(x)   (BatchNorm1d over the Cin*V channels (c,v) of the (N, Cin*V, T) view: channel c*V + v)
 *   qkv = Wqkv . xn + bqkv per frame, Wqkv (2dk+Cout, Cin); q, k, v and the heads are contiguous channel blocks
 *   w = softmax over keys of (q_h * dkh^-0.5)^T k_h  (V x V per frame and head); training with drop-connect:
 *       w = w*m[key] / (sum_key w*m[key] + 1e-8), mask m (N*T, heads, V) floats of 0 / 1 (NULL: no drop-connect)
 *   o = heads of w . v_h^T concatenated (Cout channels);  z = Wout . o + bout (+ x when Cin == Cout), Wout (Cout, Cout)
 *   y = relu(BatchNorm2d(z))
 * x, y: (N,Cin,T,V) / (N,Cout,T,V).  dk = Cout/4 in the reference's configuration; covered: (dk/heads, Cout/heads) in
 * {(4,16), (8,32), (16,64)} — Cout in {128, 256, 512} with 8 heads — any Cin, V <= 64, N <= 65535 clips with
 * N*T < 2^26 frames and N*max(Cin,Cout) < 2^24 (its launches' 2^32 work-items: below 32768 clips at 512 channels), and
 * T*V columns a clip up to what the product kernel of the call's arithmetic tiles: T*V <= 65535*64 = 4,194,240 with
 * STGCN_MATH_F32, T*V <= 65535*128 = 8,388,480 with STGCN_MATH_BF16X3 (the backward's weight gradients are f32 GEMMs over T*V
 * and hold either), every operand of one clip below 2^31 elements.  Else STGCN_ERR_UNSUPPORTED.  Every entry point decides
 * this before its first launch: a refused call has written nothing - not y, not the workspace, not a saved tensor or a
 * gradient, and not the running statistics of either BatchNorm. */
int stgcn_st_attention_supported(int Cin, int Cout, int dk, int V, int heads);
/* workspace bytes of pass 0 = stgcn_st_attention_forward, 1 = _forward_train, 2 = _backward (0 for invalid sizes) */
size_t stgcn_st_attention_ws_bytes(int N, int Cin, int Cout, int dk, int T, int V, int heads, int pass);
/* Eval forward: both BatchNorms folded on their running statistics (stgcn_bn_fold; data_bn over Cin*V channels). */
int stgcn_st_attention_forward(const float *x, const float *dbn_scale, const float *dbn_shift, const float *Wqkv,
                               const float *bqkv, const float *Wout, const float *bout, const float *bn_scale,
                               const float *bn_shift, void *ws, size_t ws_bytes, float *y, int N, int Cin, int Cout,
                               int dk, int T, int V, int heads, void *stream);
/* Training forward: batch statistics for both BatchNorms (running buffers updated like torch, with one momentum / eps for
 * both), or with STGCN_BN_FROZEN the running statistics (nothing updated).  Saved for the backward: save_qkv
 * (N,2dk+Cout,T,V), save_o (N,Cout,T,V), save_z (N,Cout,T,V), save_rowstats (N*T*heads*V float4: row max, sum of
 * exponentials, drop-connect sum, 0), save_stats (2*Cin*V + 2*Cout floats: mean, invstd of data_bn, then of bn). */
int stgcn_st_attention_forward_train(const float *x, const float *dbn_weight, const float *dbn_bias, float *dbn_running_mean,
                                     float *dbn_running_var, const float *Wqkv, const float *bqkv, const float *Wout,
                                     const float *bout, const float *bn_weight, const float *bn_bias,
                                     float *bn_running_mean, float *bn_running_var, const float *mask, float momentum,
                                     float eps, void *ws, size_t ws_bytes, float *y, float *save_qkv, float *save_o,
                                     float *save_z, float *save_rowstats, float *save_stats, int N, int Cin, int Cout,
                                     int dk, int T, int V, int heads, unsigned flags, void *stream);
/* Backward from dy (N,Cout,T,V) with what the training forward saved (same flags and mask): the gradients of data_bn's
 * weight / bias (Cin*V), Wqkv / bqkv, Wout / bout, bn's weight / bias, and dx (N,Cin,T,V; NULL when x needs none). */
int stgcn_st_attention_backward(const float *x, const float *dbn_weight, const float *dbn_bias, const float *Wqkv,
                                const float *Wout, const float *bn_weight, const float *bn_bias, const float *mask,
                                const float *save_qkv, const float *save_o, const float *save_z, const float *save_rowstats,
                                const float *save_stats, const float *dy, float *dx, float *ddbn_weight, float *ddbn_bias,
                                float *dWqkv, float *dbqkv, float *dWout, float *dbout, float *dbn_weight_grad,
                                float *dbn_bias_grad, void *ws, size_t ws_bytes, int N, int Cin, int Cout, int dk, int T,
                                int V, int heads, unsigned flags, void *stream);
/* Arithmetic of the unit's matrix products (additive to ABI 11).  The low 4 bits of `flags` of stgcn_st_attention_forward_train,
 * stgcn_st_attention_backward and stgcn_st_attention_forward_math choose how the two 1x1 projections (qkv = Wqkv . xn,
 * z = Wout . o) and their two input gradients (Wout^T . dz, Wqkv^T . dqkv) are computed: STGCN_MATH_F32 (0, the default: the
 * fp32 matrix cores, what every caller got before) or STGCN_MATH_BF16X3 (both operands split into bf16 hi + lo, three
 * v_mfma_f32_16x16x32_bf16 products, fp32 sums; the skip connection is read in that kernel's epilogue).  The weight-gradient
 * products, the V x V attention and both BatchNorms are fp32 either way.  STGCN_MATH_BF16, STGCN_MATH_F32_VALU and unknown
 * values return STGCN_ERR_UNSUPPORTED.  The forward and the backward of one step must be called with the SAME flags, the
 * arithmetic bits like STGCN_BN_FROZEN.  stgcn_st_attention_ws_bytes holds for both arithmetics. */
int stgcn_st_attention_math_supported(int Cin, int Cout, int dk, int V, int heads, unsigned flags);
/* stgcn_st_attention_forward with the arithmetic in the low 4 bits of `flags` (0: exactly stgcn_st_attention_forward). */
int stgcn_st_attention_forward_math(const float *x, const float *dbn_scale, const float *dbn_shift, const float *Wqkv,
                                    const float *bqkv, const float *Wout, const float *bout, const float *bn_scale,
                                    const float *bn_shift, void *ws, size_t ws_bytes, float *y, int N, int Cin, int Cout,
                                    int dk, int T, int V, int heads, unsigned flags, void *stream);
/* The product of those projections on its own: C[n][m][j] = sum_k W[m][k] X[n][k][j] (+ bias[m]) (+ R[n][m][j]) for n < N,
 * m < M, j < TV.  W is (M,K) row-major, or (K,M) with w_transposed; X[n] (K,TV), C[n] and R[n] (M,TV) are dense with TV
 * contiguous; bias and R may be NULL, R may not be C.  The low 4 bits of `flags`: STGCN_MATH_F32 (the strided fp32 GEMM; R is
 * copied to C and the product accumulated onto it) or STGCN_MATH_BF16X3 (three-term split on the bf16 matrix cores; ragged M,
 * K and TV are staged as zeros, never loaded; no alignment demand on TV).  Covered: M, K, TV >= 1 with max(M,K)*TV < 2^31, M*K < 2^29,
 * TV <= 65535*64 and N <= 65535.  Bit-identical between runs.  `ws` may be NULL where the size query gives 0 (it does today). */
int stgcn_wx_product_supported(int M, int K, long long TV, unsigned flags);   /* 1, or 0: other arithmetic or outside the limits */
const char *stgcn_wx_product_kernel_name(int M, int K, long long TV, unsigned flags);   /* "" where unsupported */
size_t stgcn_wx_product_ws_bytes(int M, int K, unsigned flags);
int stgcn_wx_product(const float *W, const float *X, const float *bias, const float *R, float *C, void *ws, size_t ws_bytes,
                     int N, int M, int K, long long TV, int w_transposed, unsigned flags, void *stream);

/* ---- AltFormer heads: transformer block (Block of model/AltFormer/model_ST.py:18-88 = model_TS.py, ABI 10) -----------
 * Eval forward only (no dropout, no stochastic depth), tokens in rows, x (B, L, D) dense fp32:
 *   x1 = x  + proj(MHA(LN1(x)))          qkv = LN1(x) Wqkv^T (+ bqkv), packed (B, L, 3, heads, hd) as nn.Linear writes it;
 *   y  = x1 + fc2(GELU(fc1(LN2(x1))))    softmax over keys of scale * q k^T; GELU in its exact erf form.
 * Weights are nn.Linear.weight as stored: (out_features, in_features), in_features contiguous.
 * `flags`: low 4 bits STGCN_MATH_F32 (v_mfma_f32_32x32x2_f32) or STGCN_MATH_BF16X3 (hi + lo split of both operands, three
 * bf16 MFMAs, fp32 accumulate) for the linears; the attention itself always runs on the fp32 matrix cores.
 * STGCN_VIT_BF16 (below, opt-in) runs the whole block, attention included, on bf16 operands instead. */
#define STGCN_VIT_GELU 0x1000u    /* stgcn_vit_linear: exact GELU after the bias                                     */
#define STGCN_VIT_QKV_F32 0x2000u /* stgcn_vit_block_forward: the qkv linear in f32 whatever the low bits say (an error
                                   * in q or k is multiplied by the size of the scores before the exponential)        */
/* Tile form of the linears (additive to ABI 10: new flag bits and one query).  The linear kernel exists in three forms that
 * differ only in the tile of y a workgroup owns: 128 x 128, 64 x 64, and 32 rows x 64 columns.  Every form computes an
 * element of y with the same instructions in the same order, so results are bit-identical across forms; the smaller ones
 * spread a small call (one clip) over more workgroups.  stgcn_vit_linear and stgcn_vit_block_forward (all four linears)
 * honour the field; the training entry points (stgcn_vit_block_forward_train, stgcn_vit_block_backward,
 * stgcn_vit_linear_backward) always run 128 x 128 and answer STGCN_ERR_ARG to a non-zero field; the training pair with
 * dropout at the end of this header (stgcn_vit_block_forward_train_drop, stgcn_vit_block_backward_drop) honours it. */
#define STGCN_VIT_TILE_MASK 0x30000u
#define STGCN_VIT_TILE_AUTO 0x10000u /* the plan picks: the largest form that gives at least 256 tiles, else the smallest  */
#define STGCN_VIT_TILE_64 0x20000u   /* force 64 x 64                                                                  */
#define STGCN_VIT_TILE_32 0x30000u   /* force the 32-row form (32 x 64)                                                */
/* field 0: 128 x 128 */
/* The form `flags` gives a linear of this shape, as (BM << 16) | BN; 0 if stgcn_vit_linear does not cover it.  Pure host
 * function of its arguments (no device query).  stgcn_vit_block_forward walks inputs of more than 32768 tokens in slabs of
 * whole sequences and plans each slab's linears with M = the slab's tokens, so for such a call ask with a slab's M (and a
 * short last slab may get a smaller form than the others; the result does not depend on it). */
int stgcn_vit_linear_tile(int M, int K, int Nout, unsigned flags);
/* y (M, Nout) = act(LN?(x) W^T + bias) (+ residual).  x (M, K), W (Nout, K).  bias, residual may be NULL; LayerNorm over
 * the rows of x when ln_weight / ln_bias (K) are given (both or neither), biased variance, eps inside the root.
 * Covered: any M, any Nout, K % 32 == 0, with LayerNorm K <= 4096; f32 or bf16x3 (else STGCN_ERR_UNSUPPORTED); the tiles of
 * stgcn_vit_linear_tile times their workgroup's threads (64 a wave) stay below 2^32 work-items (the same for
 * stgcn_vit_linear_bf16).
 * y may alias residual, not x.  One launch: the row statistics are taken inside the workgroup that owns the rows. */
int stgcn_vit_linear_supported(int M, int K, int Nout, unsigned flags);
int stgcn_vit_linear(const float *x, const float *W, const float *bias, const float *ln_weight, const float *ln_bias,
                     float ln_eps, const float *residual, float *y, int M, int K, int Nout, unsigned flags,
                     void *stream);
/* out (B, L, heads*head_dim) = concatenated heads of softmax(scale * q k^T) v, qkv (B, L, 3, heads, head_dim).
 * The resident form: K and V of a (sequence, head) pair stay in LDS, a query's score row in registers.
 * Covered: head_dim in {32, 64}, 1 <= L <= 256, B and heads with B*heads*ceil(L/32) < 2^26 (a wave per 32 queries of a
 * pair: 2^32 work-items a launch; the split form: B*heads*ceil(L/32)^2 < 2^26) (else STGCN_ERR_UNSUPPORTED).  One launch.
 * stgcn_vit_attention_supported describes this form (and the length the training entry points cover), not the streaming one. */
int stgcn_vit_attention_supported(int L, int heads, int head_dim);
int stgcn_vit_attention(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale, void *stream);
/* The streaming form (additive to ABI 11): the same layouts and fp32-exact products, K and V streamed through LDS in tiles of
 * 64 keys under a running soft-max, 128 queries of a pair per workgroup.  Covered: head_dim in {32, 64},
 * 1 <= L <= STGCN_VIT_MAX_STREAM_L, any B and heads; it runs the streaming kernel at every covered length, the short ones
 * included.  Agrees with the resident form within rounding (another summation order), bit-identical from run to run.
 * One launch on the caller's stream - one per 2^24 / (heads * ceil(L/128)) sequences, the most a launch of 2^32 work-items
 * holds - no workspace, no allocation, no synchronisation.  (The streaming backward is one launch pair and refuses
 * B*heads*ceil(L/128) >= 2^24.) */
#define STGCN_VIT_MAX_STREAM_L 4096
int stgcn_vit_attention_stream_supported(int L, int heads, int head_dim);
int stgcn_vit_attention_stream(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale,
                               void *stream);
/* One block.  Covered: head_dim = D / heads in {32, 64}, L <= STGCN_VIT_MAX_STREAM_L (a slab of 32768 tokens holds whole
 * sequences), D and hidden multiples of 64, D <= 4096, any B (else STGCN_ERR_UNSUPPORTED): stgcn_vit_block_forward_supported
 * tells.  The attention launch is the resident form for L <= 256 and the streaming form above.
 * stgcn_vit_block_supported describes the resident form only (L <= 256): it is the coverage of the training entry points
 * below and answers 0 for longer sequences that stgcn_vit_block_forward runs.
 * bqkv may be NULL (qkv_bias=False); bproj, b1, b2 may be NULL too.  eps: both LayerNorms.
 * ws: stgcn_vit_block_ws_bytes(B, L, D, hidden) bytes (bounded: the input is walked in slabs of whole sequences).
 * y must not alias x.  Five launches per slab, no atomics: results are bit-identical from run to run. */
int stgcn_vit_block_supported(int L, int D, int heads, int hidden);
int stgcn_vit_block_forward_supported(int L, int D, int heads, int hidden);
size_t stgcn_vit_block_ws_bytes(int B, int L, int D, int hidden);
int stgcn_vit_block_forward(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv,
                            const float *bqkv, const float *Wproj, const float *bproj, const float *norm2_weight,
                            const float *norm2_bias, const float *W1, const float *b1, const float *W2, const float *b2,
                            float eps, float scale, void *ws, size_t ws_bytes, float *y, int B, int L, int D, int heads,
                            int hidden, unsigned flags, void *stream);

/* ---- ViT block in bf16 (additive to ABI 11: new symbols and one flag bit; inference only) ----------------------------------
 * STGCN_VIT_BF16 on stgcn_vit_block_forward runs the whole block with bf16 matrix operands: operands rounded to nearest-even
 * bf16, products accumulated in fp32 (v_mfma_f32_32x32x16_bf16), everything that is not a matrix operand fp32:
 *   qkv  : LN1(x) in fp32, rounded as the A operand; Wqkv rounded while staged; bias in fp32; the result STORED AS bf16;
 *   attn : scores = bf16 q . bf16 k in fp32, times `scale` in fp32; max, exp and row sum in fp32 (the sum adds the unrounded
 *          p = exp(s - max)); p rounded to bf16 as the operand of P V; O accumulated in fp32, divided by the sum, STORED AS bf16;
 *   proj : bf16 attention output x rounded Wproj + bias + the fp32 residual x -> x1 in fp32;
 *   fc1  : LN2(x1) in fp32, rounded; W1 rounded; bias and the exact erf GELU in fp32; the hidden tensor STORED AS bf16;
 *   fc2  : bf16 hidden x rounded W2 + bias + x1 -> y in fp32.
 * The low math bits are ignored, the STGCN_VIT_TILE_* field is honoured (same bits for every form); with STGCN_VIT_QKV_F32 the
 * call answers STGCN_ERR_ARG.  Covered: the resident form (stgcn_vit_block_forward_bf16_supported: head_dim 32 / 64, L <= 256,
 * D and hidden multiples of 64), STGCN_ERR_UNSUPPORTED elsewhere.  The workspace is stgcn_vit_block_ws_bytes' (the mode needs
 * less of it).  The training entry points (stgcn_vit_block_forward_train, stgcn_vit_block_backward,
 * stgcn_vit_linear_backward) answer STGCN_ERR_ARG to the bit.  Gate: 1e-2 of max|y| (the stem's bf16 gate). */
#define STGCN_VIT_BF16 0x40000u
int stgcn_vit_block_forward_bf16_supported(int L, int D, int heads, int hidden);
/* stgcn_vit_linear in the bf16 arithmetic above.  x is fp32, or bf16 storage with STGCN_VIT_X_BF16 (no LayerNorm then:
 * STGCN_ERR_UNSUPPORTED); y is fp32, or bf16 storage with STGCN_VIT_Y_BF16.  W, bias, residual and the LayerNorm vectors are
 * fp32.  `flags`: the two storage bits, STGCN_VIT_GELU and a STGCN_VIT_TILE_* field.  Covered: any M and Nout, K % 32 == 0,
 * with LayerNorm K <= 4096. */
#define STGCN_VIT_X_BF16 0x80000u
#define STGCN_VIT_Y_BF16 0x100000u
int stgcn_vit_linear_bf16_supported(int M, int K, int Nout, unsigned flags);
int stgcn_vit_linear_bf16(const void *x, const float *W, const float *bias, const float *ln_weight, const float *ln_bias,
                          float ln_eps, const float *residual, void *y, int M, int K, int Nout, unsigned flags, void *stream);
/* stgcn_vit_attention (the resident form) on bf16 qkv (B, L, 3, heads, head_dim) and bf16 out (B, L, heads*head_dim).
 * Covered: head_dim in {32, 64}, 1 <= L <= 256, any B and heads.  One launch, K and V of a pair in LDS as bf16. */
int stgcn_vit_attention_bf16_supported(int L, int heads, int head_dim);
int stgcn_vit_attention_bf16(const void *qkv, void *out, int B, int L, int heads, int head_dim, float scale, void *stream);

/* ---- ViT block: training (additive to ABI 10: new symbols and flag bits only) ------------------------------------------
 * The training forward is the eval forward's five launches with the tensors the backward reads written to the caller's
 * `saved` buffer: qkv (M,3D), the attention output (M,D), x1 (M,D), the fc1 output before and after the GELU (M,hidden
 * each); M = B*L.  scale1 / scale2 (B floats each, or NULL = 1) are stochastic depth's per-sequence factors (0 or
 * 1 / keep): x1 = x + scale1[b] * branch, y = x1 + scale2[b] * branch.  The backward takes the same two vectors.
 * No atomics anywhere: reductions over the tokens are partial slabs added in a fixed order, two runs are bit-identical.
 * Arithmetic: `flags` as in the forward select f32 / bf16x3 for the dgrads (which run the forward's linear kernel on
 * transposed weights) and STGCN_VIT_QKV_F32 keeps the qkv dgrad in f32; weight gradients, LayerNorm and attention
 * backward always run in fp32 (v_mfma_f32_32x32x2_f32 where they are products).  STGCN_VIT_TRAIN_BF16 (at the end of this
 * header, opt-in) moves the linears' products, weight gradients included, to bf16 operands, and
 * STGCN_VIT_TRAIN_ATTN_BF16 (there too, opt-in) the attention forward and backward of sequences of up to 256 tokens. */
#define STGCN_VIT_DGELU 0x4000u      /* stgcn_vit_linear_backward: dx is multiplied by GELU'(h_pre) (exact erf form)    */
#define STGCN_VIT_ACCUMULATE 0x8000u /* stgcn_vit_linear_backward: dx += instead of dx =                                 */
/* Backward of y = a W^T + b:  dx (M,K) = dy W [* GELU'(h_pre (M,K))] [+ dx],  dW (Nout,K) = dy^T a,  db (Nout) = column sums
 * of dy.  dx, dW, db may each be NULL (db only with dW); `a` is the linear's input as the forward saw it.
 * Covered: K % 32 == 0, Nout % 4 == 0, any M.  ws: stgcn_vit_linear_backward_ws_bytes (0 for uncovered shapes). */
int stgcn_vit_linear_backward_supported(int M, int K, int Nout, unsigned flags);
size_t stgcn_vit_linear_backward_ws_bytes(int M, int K, int Nout);
int stgcn_vit_linear_backward(const float *dy, const float *a, const float *W, const float *h_pre, float *dx, float *dW,
                              float *db, void *ws, size_t ws_bytes, int M, int K, int Nout, unsigned flags, void *stream);
/* dqkv (B,L,3,heads,head_dim) from the packed qkv, the forward's output `out` and its gradient dout (both (B,L,heads*head_dim));
 * S and P are recomputed on chip.  Same coverage as the resident forward (L <= 256).  One launch, no workspace. */
int stgcn_vit_attention_backward_supported(int L, int heads, int head_dim);
int stgcn_vit_attention_backward(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L, int heads,
                                 int head_dim, float scale, void *stream);
/* The same gradient (up to the summation order) for every 1 <= L <= STGCN_VIT_MAX_STREAM_L: two kernels that stream the other
 * side of each product through LDS under the forward's running soft-max, whose statistics they recompute (nothing but `out`
 * is needed from the forward).  It runs the streaming kernels at every covered length, the short ones included.
 * ws: stgcn_vit_attention_backward_stream_ws_bytes(B, L, heads) bytes, 16 per (sequence, head, query); 0 if uncovered. */
int stgcn_vit_attention_backward_stream_supported(int L, int heads, int head_dim);
size_t stgcn_vit_attention_backward_stream_ws_bytes(int B, int L, int heads);
int stgcn_vit_attention_backward_stream(const float *qkv, const float *out, const float *dout, float *dqkv, void *ws,
                                        size_t ws_bytes, int B, int L, int heads, int head_dim, float scale, void *stream);
/* LayerNorm backward over the rows of x (M,D), dn = gradient of the LayerNorm's output: dx = rstd (g - mean(g) - xhat
 * mean(g xhat)) (+ dres), g = dn * weight;  dweight = sum dn xhat,  dbias = sum dn.  D % 4 == 0, M < 2^26 rows (a wave per
 * row: 2^32 work-items a launch).  dx may alias dn or dres. */
size_t stgcn_vit_layernorm_backward_ws_bytes(int M, int D);
int stgcn_vit_layernorm_backward(const float *x, const float *dn, const float *weight, float eps, const float *dres, float *dx,
                                 float *dweight, float *dbias, void *ws, size_t ws_bytes, int M, int D, void *stream);
/* One block, training.  stgcn_vit_block_forward_train and stgcn_vit_block_backward cover what stgcn_vit_block_forward covers:
 * L <= 256 on the resident attention kernels, 256 < L <= STGCN_VIT_MAX_STREAM_L on the streaming ones (forward and backward).
 * These three queries describe the resident form only (= stgcn_vit_block_supported) and answer 0 for L > 256; the three
 * `_long` queries below cover both ranges and are the ones to size buffers with. */
int stgcn_vit_block_train_supported(int L, int D, int heads, int hidden);
size_t stgcn_vit_block_saved_bytes(int B, int L, int D, int hidden);
size_t stgcn_vit_block_backward_ws_bytes(int B, int L, int D, int hidden);
/* Both ranges.  At L <= 256 they answer what the three above answer.  Above: `saved` is the same layout (the streaming
 * backward recomputes its soft-max statistics, nothing new is saved); the workspace is the resident one plus the attention
 * statistics of one slab of sequences. */
int stgcn_vit_block_train_long_supported(int L, int D, int heads, int hidden);
size_t stgcn_vit_block_train_long_saved_bytes(int B, int L, int D, int hidden);
size_t stgcn_vit_block_train_long_ws_bytes(int B, int L, int D, int heads, int hidden);
int stgcn_vit_block_forward_train(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv,
                                  const float *bqkv, const float *Wproj, const float *bproj, const float *norm2_weight,
                                  const float *norm2_bias, const float *W1, const float *b1, const float *W2, const float *b2,
                                  const float *scale1, const float *scale2, float eps, float scale, void *saved,
                                  size_t saved_bytes, float *y, int B, int L, int D, int heads, int hidden, unsigned flags,
                                  void *stream);
/* dy (B,L,D) -> dx and the twelve parameter gradients (dbqkv may be NULL: qkv_bias=False), each written, not added to. */
int stgcn_vit_block_backward(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv,
                             const float *Wproj, const float *norm2_weight, const float *norm2_bias, const float *W1,
                             const float *W2, const float *scale1, const float *scale2, const void *saved, size_t saved_bytes,
                             const float *dy, float *dx, float *dnorm1_weight, float *dnorm1_bias, float *dWqkv, float *dbqkv,
                             float *dWproj, float *dbproj, float *dnorm2_weight, float *dnorm2_bias, float *dW1, float *db1,
                             float *dW2, float *db2, float eps, float scale, void *ws, size_t ws_bytes, int B, int L, int D,
                             int heads, int hidden, unsigned flags, void *stream);

/* ---- ViT block: training on bf16 matrix operands (additive to ABI 11: one flag bit and two queries; opt-in) -----------------
 * STGCN_VIT_TRAIN_BF16 is accepted by exactly stgcn_vit_block_forward_train, stgcn_vit_block_backward and
 * stgcn_vit_linear_backward.  With it every matrix product of a linear takes both operands rounded to nearest-even bf16 while
 * they are staged (no packed or cached weight format) and accumulates in fp32 (v_mfma_f32_32x32x16_bf16):
 *   forward proj, fc1, fc2 : r(A) r(W)^T, A = the attention output, LN2(x1), the GELU output as they are in fp32;
 *   every dgrad, qkv's too : r(dY) r(W), the forward kernel on the transposed weight; GELU' and the row factor stay in the fp32
 *                            epilogue, after the product;
 *   every wgrad, qkv's too : dW = r(s dY)^T r(A), the row factor s applied before the rounding; THE BIAS GRADIENT SUMS THE
 *                            UNROUNDED fp32 s dY.
 * The one exception is the qkv FORWARD linear: it runs in the arithmetic of the low math bits (bf16x3, or f32 where the low bits
 * or STGCN_VIT_QKV_F32 say so), because an error in q or k is multiplied by the size of the scores before the exponential.
 * Everything that is not a linear's matrix operand is fp32 and the kernel it is without the bit: both LayerNorms forward and
 * backward, the attention forward and backward (resident and streaming), bias adds, GELU and GELU', the stochastic-depth
 * factors, residuals, every stored tensor.  `saved` and the workspace keep layout and size: every *_bytes query above answers
 * for the mode too.  Results are bit-identical from run to run (no atomics, fixed summation order), as without the bit.
 * The low bits must be STGCN_MATH_F32 or STGCN_MATH_BF16X3 as ever (else STGCN_ERR_UNSUPPORTED); STGCN_VIT_BF16 and a
 * STGCN_VIT_TILE_* field keep their STGCN_ERR_ARG answers on the three entry points and are checked first.
 * stgcn_vit_block_forward and stgcn_vit_linear answer STGCN_ERR_ARG to the bit.
 * The training forward of this mode is NOT an inference mode's forward: STGCN_VIT_BF16 inference also rounds the qkv linear's
 * operands, the soft-max weights and the stored intermediates, this mode none of them; its y differs from the default
 * inference result by about 3e-4 of max|y|.  There is no inference twin.  Gate: 1e-2 of max|.| per tensor.
 * Coverage: stgcn_vit_block_train_bf16_supported = stgcn_vit_block_train_long_supported (streaming lengths included);
 * stgcn_vit_linear_backward_bf16_supported = stgcn_vit_linear_backward_supported with covered low bits. */
#define STGCN_VIT_TRAIN_BF16 0x200000u
int stgcn_vit_block_train_bf16_supported(int L, int D, int heads, int hidden);
int stgcn_vit_linear_backward_bf16_supported(int M, int K, int Nout);

/* ---- ViT block: training attention on bf16 matrix operands (additive to ABI 11: one flag bit, two entry points, two queries;
 * opt-in) ----
 * STGCN_VIT_TRAIN_ATTN_BF16 is accepted by exactly stgcn_vit_block_forward_train and stgcn_vit_block_backward, with every flag
 * combination that is legal without it (with or without STGCN_VIT_TRAIN_BF16, low bits f32 or bf16x3).  Where L <= 256 the
 * attention forward and backward of the call then run on v_mfma_f32_32x32x16_bf16 instead of the fp32 matrix cores; above,
 * the call runs the fp32 streaming kernels it runs without the bit, bit for bit.  With r = round to nearest-even bf16 and every
 * sum in fp32, per (sequence, head):
 *   s = scale * (qh kh^T + qh kl^T + ql kh^T), qh = r(q), ql = r(q - qh), kh and kl alike, of the unscaled fp32 q and k as they
 *       lie in the packed qkv (a rounded q or k is multiplied by the size of the scores: the score product takes three terms);
 *   m = max s, p = exp(s - m), l = sum p (of the unrounded p), keys past L score -inf;
 *   forward : out = (r(p) r(v)) / l, stored fp32;
 *   backward: P = p / l recomputed as above, dP = r(dO) r(v)^T, delta_i = sum_j P_ij dP_ij (NOT rowsum(dO * out): `out` is an
 *             argument and is not read), dS = P (dP - delta), dV = r(P)^T r(dO), dQ = scale r(dS) r(k), dK = scale r(dS)^T r(q),
 *             dqkv stored fp32, packed as qkv.
 * LayerNorm, GELU, residuals, row factors and the linears are what they are without the bit; `saved` and the workspace keep
 * layout and size, so every *_bytes query answers for the mode too.  Results are bit-identical from run to run.  Gate with
 * STGCN_VIT_TRAIN_BF16: 1e-2 of max|.| per tensor, as that mode alone.
 * stgcn_vit_block_forward, stgcn_vit_linear and stgcn_vit_linear_backward answer STGCN_ERR_ARG to the bit, after their older
 * flag refusals and before the pointers are looked at.
 * The value is 0x800000: 0x400000 stays unassigned (the host test of STGCN_VIT_TRAIN_BF16 uses it as its unknown bit).
 * stgcn_vit_attention_train_bf16 / stgcn_vit_attention_backward_bf16: the two kernels alone, arguments as stgcn_vit_attention /
 * stgcn_vit_attention_backward; covered (stgcn_vit_attention_train_bf16_supported): 1 <= L <= 256, head_dim 32 / 64.
 * stgcn_vit_block_train_attn_bf16_supported: 1 where a block call with the bit runs these kernels, 0 where the bit changes
 * nothing (256 < L) or the shape is not covered. */
#define STGCN_VIT_TRAIN_ATTN_BF16 (STGCN_VIT_TRAIN_BF16 << 2)
int stgcn_vit_attention_train_bf16_supported(int L, int heads, int head_dim);
int stgcn_vit_attention_train_bf16(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale,
                                   void *stream);
int stgcn_vit_attention_backward_bf16(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L,
                                      int heads, int head_dim, float scale, void *stream);
int stgcn_vit_block_train_attn_bf16_supported(int L, int D, int heads, int hidden);

/* ---- ViT block: the attention split over key tiles, for calls of a few clips (additive to ABI 11: one flag bit, two entry
 * points, two queries; opt-in) ----
 * The resident attention gives a (sequence, head) pair one workgroup, so one clip of 8 heads occupies 8 of the 256 CUs.
 * stgcn_vit_attention_split computes the same fp32 attention with a workgroup per (pair, tile of 32 queries) whose
 * NT = ceil(L / 32) waves each own one tile of 32 keys: per wave the scores of its keys, their maximum m_w, e = exp(s - m_w),
 * l_w = sum e and the unnormalised O_w = V_w^T e; then, through LDS and in ascending w,
 *   m = max m_w, f_w = exp(m_w - m), out = (sum f_w O_w) / (sum f_w l_w).
 * The same instructions as stgcn_vit_attention (v_mfma_f32_32x32x2_f32, exact fp32 products), no atomics, no workspace, one
 * launch; results are bit-identical from run to run and agree with the resident form within rounding (another summation
 * order).  Arguments, checks and coverage (stgcn_vit_attention_split_supported: 1 <= L <= 256, head_dim 32 / 64) are
 * stgcn_vit_attention's; the entry point runs the split kernel whatever B is.
 * STGCN_VIT_ATTN_SPLIT is accepted by stgcn_vit_block_forward only.  The block's attention launch then takes the split form
 * where it is the fp32 resident one (L <= 256, no STGCN_VIT_BF16), L > 32 (two key tiles or more) and the launch has fewer
 * than 192 (sequence, head) pairs (a measured constant; stgcn_vit_block_attention_form tells); everywhere else the bit is
 * legal and changes nothing (with STGCN_VIT_BF16, above 256 tokens, at L <= 32, from 192 pairs on).  Workspace sizes do not change.  stgcn_vit_block_forward_train,
 * stgcn_vit_block_backward, stgcn_vit_linear_backward and stgcn_vit_linear answer STGCN_ERR_ARG to the bit, after their older
 * flag refusals and before the pointers are looked at.
 * The value is 0x2000000: 0x400000 and 0x1000000 stay unassigned (host tests use them as unknown bits).
 * stgcn_vit_block_attention_form: the attention kernel stgcn_vit_block_forward runs for this call (of its first slab, which is
 * the whole call up to 32768 tokens): 0 uncovered or refused, 1 resident, 2 streaming, 3 resident bf16, 4 resident split.
 * A pure host function of its arguments. */
#define STGCN_VIT_ATTN_SPLIT (0x2000000u)
int stgcn_vit_attention_split_supported(int L, int heads, int head_dim);
int stgcn_vit_attention_split(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale, void *stream);
int stgcn_vit_block_attention_form(int B, int L, int D, int heads, int hidden, unsigned flags);

/* ---- The whole AltFormer head: stem output to logits in one call (additive to ABI 11: one flag bit, three structs, three
 * entry points, four queries; inference only) ----
 * model/AltFormer/model_ST.py (ST) and model_TS.py (TS) after the stem, eval forward:
 *   ST: first embedding (C -> E1, + pos1 per joint) -> depth1 blocks over the V joints of each of the N*T frames -> MEAN over the
 *       joints -> second embedding (E1 -> E2, + pos2 per frame) -> depth2 blocks over the T frames of each clip -> MAX over the
 *       frames -> LayerNorm(E2) -> Linear(E2 -> classes);
 *   TS: first embedding (+ pos1 per frame) -> depth1 blocks over the T frames of each of the N*V joints -> MAX over the frames ->
 *       second embedding (+ pos2 per joint) -> depth2 blocks over the V joints of each clip -> MEAN over the joints -> the same
 *       LayerNorm and Linear.
 * Two kernels of their own, both fp32, without atomics and with a fixed summation order (bit-identical from run to run):
 *   stgcn_vit_pool         : out (S, D) = the mean (sum / L) or, with STGCN_VIT_POOL_MAX, the maximum over the L tokens of the
 *                            dense x (S, L, D).  The maximum is a selection that starts from a token of the sequence: on finite
 *                            input it is the largest element bit for bit.  Covered: D % 4 == 0, any L, and S * ceil(D / 256) < 2^24
 *                            sequences (a launch holds fewer than 2^32 work-items).  x and out 16-byte aligned.  One launch, no
 *                            workspace.
 *   stgcn_vit_pool_classify: logits (N, classes) = LayerNorm(pool over L of x (N, L, D)) W^T + bias; the LayerNorm is affine with
 *                            the biased variance and ln_eps inside the root; W is (classes, D) as nn.Linear stores it, bias may
 *                            be NULL.  Covered: D % 64 == 0, D <= 4096, N < 2^22 clips, any L and classes >= 1.  One workgroup
 *                            of 1024 threads per clip, one launch, no workspace.
 * The embeddings are stgcn_patch_embed's strided fp32 GEMM (the second one with one frame of L2 "joints" per clip: the pooled
 * rows times embed2_weight^T, plus the bias, plus pos2 by row % L2).
 *
 * stgcn_altformer_head_forward covers the head only.  The stem keeps its own entry points and its prepared blob; the two
 * compose as  stgcn_stem_* with STGCN_OUT_NTVC  ->  this call with STGCN_IN_NTVC in head_flags  (z is then the stem's (N,T,V,C)
 * output, read in place; without the bit z is (N,C,T,V)).
 * The structs are HOST structs of DEVICE pointers (blocks1 / blocks2: host arrays of depth1 / depth2 entries); the library
 * copies nothing and keeps nothing after the call.  In a block's weights bqkv, bproj, b1, b2 may be NULL; pos1 and pos2 may be
 * NULL (no position table); everything else is required.
 * flags1 / flags2: the flag words of the two stages' blocks, exactly what stgcn_vit_block_forward takes (math bits,
 * STGCN_VIT_QKV_F32, the STGCN_VIT_TILE_* field, STGCN_VIT_ATTN_SPLIT, STGCN_VIT_BF16); a stage whose word that entry point
 * refuses (STGCN_ERR_ARG) or whose shape it does not cover (STGCN_ERR_UNSUPPORTED) makes the whole call answer that status.
 * head_flags: STGCN_EMBED_TS (off: the ST order and pooling, on: TS) and STGCN_IN_NTVC; any other bit: STGCN_ERR_ARG.
 * eps_blocks: the LayerNorms of every block; eps_head: the LayerNorm before the classifier (nn.LayerNorm's default 1e-5 in the
 * reference, not the blocks' 1e-6); scale1 / scale2: the attention scale of the two stages (head_dim ** -0.5 by default).
 * ws: stgcn_altformer_head_ws_bytes bytes (0 for a call the entry point would not run): the two activation buffers of each
 * stage, the pooled rows and one block workspace (bounded, stgcn_vit_block_ws_bytes'); short: STGCN_ERR_WORKSPACE.
 * Order of the answers: flags (STGCN_ERR_ARG), then pointers and dimensions (STGCN_ERR_ARG), then coverage
 * (STGCN_ERR_UNSUPPORTED), then the workspace; nothing is launched before all four passed.
 * Launches: 2 embeddings, 5 per block and slab, 1 pool, 1 pooled classifier; all on `stream`, no synchronisation. */
#define STGCN_VIT_POOL_MAX (0x4000000u)
typedef struct { const float *norm1_weight, *norm1_bias, *Wqkv, *bqkv, *Wproj, *bproj,
                             *norm2_weight, *norm2_bias, *W1, *b1, *W2, *b2; } stgcn_vit_block_weights;
typedef struct { int N, T, V, C, E1, E2, heads, hidden1, hidden2, depth1, depth2, classes; } stgcn_altformer_head_shape;
typedef struct {
    const float *embed1_weight, *embed1_bias, *pos1;          /* (E1,C) (E1) (V,E1) [ST] / (T,E1) [TS]; pos may be NULL */
    const stgcn_vit_block_weights *blocks1;                   /* host array, depth1 entries                           */
    const float *embed2_weight, *embed2_bias, *pos2;          /* (E2,E1) (E2) (T,E2) [ST] / (V,E2) [TS]               */
    const stgcn_vit_block_weights *blocks2;                   /* host array, depth2 entries                           */
    const float *head_norm_weight, *head_norm_bias, *head_weight, *head_bias;   /* (E2) (E2) (classes,E2) (classes)   */
} stgcn_altformer_head_weights;
int stgcn_vit_pool_supported(int S, int L, int D);
int stgcn_vit_pool(const float *x, float *out, int S, int L, int D, unsigned flags, void *stream);
int stgcn_vit_pool_classify_supported(int N, int L, int D, int classes);
int stgcn_vit_pool_classify(const float *x, const float *ln_weight, const float *ln_bias, float ln_eps, const float *W,
                            const float *bias, float *logits, int N, int L, int D, int classes, unsigned flags, void *stream);
int stgcn_altformer_head_supported(const stgcn_altformer_head_shape *shape, unsigned flags1, unsigned flags2,
                                   unsigned head_flags);
size_t stgcn_altformer_head_ws_bytes(const stgcn_altformer_head_shape *shape, unsigned flags1, unsigned flags2,
                                     unsigned head_flags);
int stgcn_altformer_head_forward(const float *z, const stgcn_altformer_head_weights *weights,
                                 const stgcn_altformer_head_shape *shape, float eps_blocks, float eps_head, float scale1,
                                 float scale2, void *ws, size_t ws_bytes, float *logits, unsigned flags1, unsigned flags2,
                                 unsigned head_flags, void *stream);

/* ---- The ST-ViT head: patch embedding with class token, class-token pooling (additive to ABI 11: one flag bit, one entry
 * point, three queries; inference - the backwards are further down, "training the two ends") ----
 * model/ST_Vit/trans.py (ViT) after the stem, eval forward: patch embedding -> class row -> + position table -> depth blocks
 * (stgcn_vit_block_forward: the same pre-norm block, qkv without bias, LayerNorm eps 1e-5) -> class token or mean over the
 * tokens -> LayerNorm -> Linear (stgcn_vit_pool_classify).
 *
 * stgcn_vit_patch_embed: z is the stem output, (N, C, T, V), or with STGCN_IN_NTVC (N, T, V, C) as the stem writes it with
 * STGCN_OUT_NTVC, read in place.  T % p1 == 0 and V % p2 == 0; h = T / p1, w = V / p2, n = h w patches per clip.  Patch (a, b)
 * of clip i is the vector of length K = p1 p2 C with element k = (f p2 + j) C + c equal to z[i][c][a p1 + f][b p2 + j] (f
 * slowest, then j, then c).  x is (N, n + 1, E):
 *     x[i][0]           = cls + pos[0]
 *     x[i][1 + a w + b] = patch(a, b) . W^T + bias + pos[1 + a w + b]
 * W (E, K) as nn.Linear stores it, bias (E) or NULL, cls (E), pos (n + 1, E) or NULL (with both NULL the patch rows are the
 * plain product).
 * In the (N, T, V, C) layout a patch is p1 runs of p2 C contiguous floats and the kernel stages its A operand straight from
 * them: no rearranged (N, n, K) copy exists.  (N, C, T, V) input is first written as (N, T, V, C) into the workspace by one
 * transposing pass (N C T V floats more).  Covered: (p2 C) % 32 == 0 (a K chunk of 32 never crosses a run), STGCN_MATH_F32 or
 * STGCN_MATH_BF16X3, a clip and the output below 2^31 elements, and every launch below 2^32 work-items (the transposing
 * pass: N ceil(T V / 32) ceil(C / 32) < 2^24 workgroups of 256 threads; the same holds for the backward's launches).
 * The contraction is cut over workgroups (few rows, long K); each part's sums go to a slab of the workspace and one kernel adds
 * the slabs in a fixed order with the bias and the position row and writes the class rows.  No atomics: bit-identical from run
 * to run.  The cut is a host function of (N n, K, E): stgcn_vit_patch_embed_cut returns (tile rows << 16) | parts, 0 if the
 * call is not covered; stgcn_vit_patch_embed_ws_bytes reads the same plan (0 if not covered).
 * Order of the answers: flags (STGCN_ERR_ARG for any bit outside the math bits and STGCN_IN_NTVC), then pointers and
 * dimensions (STGCN_ERR_ARG; z, W and ws 16-byte aligned), then coverage (STGCN_ERR_UNSUPPORTED), then the workspace
 * (STGCN_ERR_WORKSPACE); nothing is launched before all four passed.  2 launches (3 for (N, C, T, V) input) on `stream`, the
 * caller's buffers, no allocation, no synchronisation.
 *
 * STGCN_VIT_POOL_CLS on stgcn_vit_pool / stgcn_vit_pool_classify: the "pool" is token 0 of every sequence, bit for bit.
 * Together with STGCN_VIT_POOL_MAX: STGCN_ERR_ARG.  Without the bit both behave as before.  (The ViT's pool = 'mean' is the
 * plain mean: it includes the class token.) */
#define STGCN_VIT_POOL_CLS (0x8000000u)
int stgcn_vit_patch_embed_supported(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags);
size_t stgcn_vit_patch_embed_ws_bytes(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags);
int stgcn_vit_patch_embed_cut(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags);
int stgcn_vit_patch_embed(const float *z, const float *W, const float *bias, const float *cls, const float *pos, float *x, int N,
                          int C, int T, int V, int p1, int p2, int E, void *ws, size_t ws_bytes, unsigned flags, void *stream);

/* ---- ViT block: training with dropout (additive to ABI 11: two structs, two entry points, two queries) ----
 * The ST-ViT layers (model/ST_Vit/trans.py) are the block above with three live nn.Dropouts: behind the projection, behind
 * the GELU and behind the second MLP linear.  stgcn_vit_block_forward_train_drop / stgcn_vit_block_backward_drop take what
 * stgcn_vit_block_forward_train / stgcn_vit_block_backward take (the twelve parameters and the twelve gradients as structs of
 * device pointers; bqkv, bproj, b1, b2 and the gradient bqkv may be NULL as there) plus `masks`: three fp32 tensors of factors,
 * 0 or 1 / (1 - p), each optional (a NULL member, or masks == NULL, means 1):
 *   m_proj (B, L, D)   m_act (B, L, hidden)   m_fc2 (B, L, D)
 * With * elementwise and s1 / s2 the per-sequence factors scale1 / scale2:
 *   forward   a     = att Wproj^T + bproj            x1 = x + s1[b] (m_proj * a)
 *             h_pre = LN2(x1) W1^T + b1              h  = m_act * GELU(h_pre)          saved: h_pre unmasked, h masked
 *             y     = x1 + s2[b] (m_fc2 * (h W2^T + b2))
 *   backward  g2 = m_fc2 * dy     dW2 = (s2 g2)^T h     db2 = sum s2 g2     dh = (s2 g2 W2) * GELU'(h_pre) * m_act
 *             LN2's residual gradient is the UNMASKED dy
 *             g1 = m_proj * dx1   dWproj = (s1 g1)^T att   dbproj = sum s1 g1   datt = s1 g1 Wproj
 *             everything else as stgcn_vit_block_backward.
 * A mask is applied in fp32, in the epilogue of the linear that produces the masked tensor (after GELU / GELU', before the
 * row factor and the residual), so before any bf16 rounding of STGCN_VIT_TRAIN_BF16; g2 and g1 are each written once by a small
 * vector kernel into a workspace slab that is free at that point and read by a dgrad and a wgrad.  No atomics: two runs are
 * bit-identical.  m_proj, m_fc2, dy and ws must be 16-byte aligned when m_proj or m_fc2 is given.
 * `saved` keeps layout and size (stgcn_vit_block_train_long_saved_bytes); the workspace is
 * stgcn_vit_block_train_drop_ws_bytes (= stgcn_vit_block_train_long_ws_bytes); stgcn_vit_block_train_drop_supported =
 * stgcn_vit_block_train_long_supported.
 * Flags: as the older pair (f32 / bf16x3 low bits, STGCN_VIT_QKV_F32, STGCN_VIT_TRAIN_BF16, STGCN_VIT_TRAIN_ATTN_BF16;
 * STGCN_VIT_BF16 and STGCN_VIT_ATTN_SPLIT: STGCN_ERR_ARG before the pointers are looked at), with one difference: a
 * STGCN_VIT_TILE_* field is accepted and selects the tile form of every forward and dgrad linear of the call (the weight
 * gradients' form is not this field's: STGCN_VIT_WGRAD_SMALL, at the end of this header).  Results are bit-identical across the forms, as in inference.
 * With no mask and no tile field the pair runs what the older pair runs, bit for bit: both are one forward and one backward. */
typedef struct { const float *m_proj, *m_act, *m_fc2; } stgcn_vit_drop_masks;
typedef struct { float *norm1_weight, *norm1_bias, *Wqkv, *bqkv, *Wproj, *bproj,
                       *norm2_weight, *norm2_bias, *W1, *b1, *W2, *b2; } stgcn_vit_block_grads;
int stgcn_vit_block_train_drop_supported(int L, int D, int heads, int hidden);
size_t stgcn_vit_block_train_drop_ws_bytes(int B, int L, int D, int heads, int hidden);
int stgcn_vit_block_forward_train_drop(const float *x, const stgcn_vit_block_weights *weights, const float *scale1,
                                       const float *scale2, const stgcn_vit_drop_masks *masks, float eps, float scale,
                                       void *saved, size_t saved_bytes, float *y, int B, int L, int D, int heads, int hidden,
                                       unsigned flags, void *stream);
int stgcn_vit_block_backward_drop(const float *x, const stgcn_vit_block_weights *weights, const float *scale1,
                                  const float *scale2, const stgcn_vit_drop_masks *masks, const void *saved, size_t saved_bytes,
                                  const float *dy, float *dx, const stgcn_vit_block_grads *grads, float eps, float scale, void *ws,
                                  size_t ws_bytes, int B, int L, int D, int heads, int hidden, unsigned flags, void *stream);

/* ---- The ST-ViT head: training the two ends (additive to ABI 11: two entry points, five queries) ----
 * The backward of stgcn_vit_patch_embed and of stgcn_vit_pool_classify.  Their forwards in training are those two entry points
 * themselves, unchanged; both backwards recompute what they need from the forward's inputs, so nothing is saved.
 *
 * stgcn_vit_patch_embed_backward: z, W, the dimensions and the flags are the forward's (STGCN_IN_NTVC: z and dz are
 * (N, T, V, C), else (N, C, T, V)); dx (N, n + 1, E) is the gradient of the forward's x.  With dx_tokens the N n patch rows of dx
 * (row i (n + 1) + 1 + p for patch p of clip i; the class rows reach dcls and dpos only) and patches the rows of the forward:
 *     dW (E, K)       = dx_tokens^T . patches          dbias (E) = the column sums of dx_tokens
 *     dz (as z)       = dx_tokens . W, element k of patch (a, b) stored where the forward read it
 *     dpos (n + 1, E) = sum over the clips of dx[i]     dcls (E)  = sum over the clips of dx[i][0]
 * Each of the five outputs is optional (NULL: not wanted); what an output holds does not depend on which others were asked for.
 * dW: the fp32 weight-gradient kernel of the blocks (128 x 128 tiles of dW, chunks of 32 tokens, v_mfma_f32_32x32x2_f32, in
 * every math mode) with its A operand read in place from the (N, T, V, C) tensor; the tokens are cut into
 * stgcn_vit_patch_embed_backward_cut's splits (returns (tokens per split << 16) | splits; 0 if not covered, and for a split of
 * 32,768 tokens or more, which the word cannot hold and the call still runs), whose slabs are added in split order.  dz: the linears' tile kernel on the weight transposed once into the workspace, f32 or bf16x3 as the
 * math bits say, fp32 accumulate; every element of z belongs to exactly one patch, so dz is written whole - the caller
 * zero-fills nothing.  No (N, n, K) tensor exists at any point; (N, C, T, V) input costs one transposing pass of z (for dW) and
 * one of dz, through the workspace.  The sums over the clips run in clip order.  No atomics: two runs are bit-identical.
 * Covered: what stgcn_vit_patch_embed covers, E % 4 == 0 and E K < 2^31.  z, W, dx and ws 16-byte aligned; dz must not be z.
 * Order of the answers: flags, then pointers / dimensions / alignment (STGCN_ERR_ARG), then coverage (STGCN_ERR_UNSUPPORTED),
 * then the workspace (STGCN_ERR_WORKSPACE; stgcn_vit_patch_embed_backward_ws_bytes, 0 if not covered, sized for all outputs);
 * nothing is launched before all four passed.  At most 8 launches on `stream`, the caller's buffers, no allocation, no
 * synchronisation.
 *
 * stgcn_vit_pool_classify_backward: x, the LayerNorm, W and the flags are the forward's; dlogits (N, classes).
 *     p = x[:, 0] (STGCN_VIT_POOL_CLS) or the mean over the L tokens;  xhat = (p - mean(p)) rstd;  y = xhat ln_weight + ln_bias
 *     g = dlogits W       dW (classes, D) = dlogits^T y       dbias (classes) = the column sums of dlogits
 *     dln_weight = sum over the clips of g xhat                dln_bias = sum over the clips of g
 *     dp = rstd (g ln_weight - mean(g ln_weight) - xhat mean(g ln_weight xhat))
 *     dx (N, L, D): STGCN_VIT_POOL_CLS: row 0 of every clip = dp, rows 1 .. L - 1 written as zeros; mean: every row = dp / L
 * Each of the five outputs is optional (NULL: not wanted).  dx is written whole by the kernel: the caller zero-fills nothing.
 * fp32, one workgroup per clip recomputing the pooled row and its statistics, the sums over the clips in clip order, no
 * atomics.  STGCN_VIT_POOL_MAX: STGCN_ERR_UNSUPPORTED (with STGCN_VIT_POOL_CLS: STGCN_ERR_ARG, as in the forward).  Covered:
 * what the forward covers (D % 64 == 0, D <= 4096).  x, dx and ws 16-byte aligned; dx must not be x.  The answers come in the
 * order above; ws: stgcn_vit_pool_classify_backward_ws_bytes (3 N D floats; 0 if not covered).  At most 4 launches. */
int stgcn_vit_patch_embed_backward_supported(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags);
size_t stgcn_vit_patch_embed_backward_ws_bytes(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags);
int stgcn_vit_patch_embed_backward_cut(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags);
int stgcn_vit_patch_embed_backward(const float *z, const float *W, const float *dx, float *dW, float *dbias, float *dcls,
                                   float *dpos, float *dz, int N, int C, int T, int V, int p1, int p2, int E, void *ws,
                                   size_t ws_bytes, unsigned flags, void *stream);
int stgcn_vit_pool_classify_backward_supported(int N, int L, int D, int classes, unsigned flags);
size_t stgcn_vit_pool_classify_backward_ws_bytes(int N, int L, int D, int classes, unsigned flags);
int stgcn_vit_pool_classify_backward(const float *x, const float *ln_weight, const float *ln_bias, float ln_eps, const float *W,
                                     const float *dlogits, float *dx, float *dln_weight, float *dln_bias, float *dW, float *dbias,
                                     int N, int L, int D, int classes, void *ws, size_t ws_bytes, unsigned flags, void *stream);

/* ---- ViT block: small training calls (additive to ABI 11: one flag, five queries) ----
 * The weight-gradient kernels (fp32, and bf16 operands under STGCN_VIT_TRAIN_BF16) have two forms: a workgroup owns a
 * 128 x 128 tile of dW, or a 64 x 64 one (the same instruction, chunk of 32 tokens and staging; four times the workgroups per
 * split).  Without the flag below every weight gradient runs the 128 form with the tokens cut into uniform splits of at least
 * 256, as it always did.  STGCN_VIT_WGRAD_SMALL lets every weight gradient of the call pick per product (M tokens, dW (Nout, K)):
 *   - where that 128 launch already has 256 workgroups or more: the 128 form, in as many splits as that rule aims at, cut evenly;
 *   - else the 64 form in min(floor(256 / tiles64), chunks / 4) (at least 1) even splits, tiles64 = ceil(Nout / 64) ceil(K / 64),
 *     chunks = ceil(M / 32), where that gives no fewer workgroups than the 128 launch; where it would, the 128 form as above.
 * Splits are ranges of whole chunks of 32 tokens (the first chunks % splits of them one chunk longer), none empty, each at least
 * 4 chunks long in the 64 form.  The workgroup count never falls as M grows and is never below the unflagged launch's.  The
 * slabs are added in split order, no atomics: two runs are bit-identical.  Where a product has ONE split and the call does not
 * accumulate onto dW (every call of stgcn_vit_linear_backward; the first slab of sequences of a block call), the kernel stores
 * dW and db itself and the two summing launches are skipped.  Against the unflagged call the weight and bias gradients differ
 * in summation order only (a bias gradient also between the forms); dx and everything else is the same bits.
 * The flag is a bit of its own, not part of the STGCN_VIT_TILE_* field, which keeps selecting forward and dgrad forms only.
 * Read by stgcn_vit_block_backward_drop and stgcn_vit_linear_backward; accepted and ignored by
 * stgcn_vit_block_forward_train_drop (no weight gradient runs there); every other entry point that plans a block
 * (stgcn_vit_block_forward, stgcn_vit_block_forward_train, stgcn_vit_block_backward) answers STGCN_ERR_ARG naming it, before the
 * pointers are looked at.
 * Queries (pure host functions; `flags`: only STGCN_VIT_WGRAD_SMALL is read; 0 for an empty shape):
 *   stgcn_vit_wgrad_tile: 128 or 64;  stgcn_vit_wgrad_splits;  stgcn_vit_wgrad_writes_direct: 1 where the kernel stores dW
 *   itself in a call that does not accumulate (always 0 without the flag: such calls keep their summing launches).
 * Workspaces: more splits need more slab space, so the flagged calls have size queries of their own, which answer what the
 * older ones answer without the flag and at least that with it: stgcn_vit_block_train_small_ws_bytes (for
 * stgcn_vit_block_backward_drop) and stgcn_vit_linear_backward_small_ws_bytes.  Each entry point checks the workspace its own
 * flags need and answers STGCN_ERR_WORKSPACE before any launch. */
#define STGCN_VIT_WGRAD_SMALL (0x10000000u)
int stgcn_vit_wgrad_tile(int M, int K, int Nout, unsigned flags);
int stgcn_vit_wgrad_splits(int M, int K, int Nout, unsigned flags);
int stgcn_vit_wgrad_writes_direct(int M, int K, int Nout, unsigned flags);
size_t stgcn_vit_block_train_small_ws_bytes(int B, int L, int D, int heads, int hidden, unsigned flags);
size_t stgcn_vit_linear_backward_small_ws_bytes(int M, int K, int Nout, unsigned flags);

#ifdef __cplusplus
}
#endif
#endif /* STGCN_HIP_H */
