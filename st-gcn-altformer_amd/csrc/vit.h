// Launchers of the AltFormer heads' transformer-block kernels (vit_linear.hip, vit_attention*.hip, vit_backward.hip) and the
// coverage rules, shared by the entry points in vit_block.hip (inference) and vit_block_train.hip (training).
// All launchers enqueue on `st` and return a stgcn_status.
#pragma once

#include "common.h"

namespace stgcn {
namespace vit {

constexpr int kMaxL = 256;      // longest sequence the resident attention kernel keeps on chip (and the training kernels' limit)
constexpr int kMaxStreamL = STGCN_VIT_MAX_STREAM_L;   // longest sequence of the streaming attention kernel: a slab holds 8 of them
constexpr int kStreamKeys = 64;       // keys per LDS stage of the streaming kernel (vit_attention_stream.hip)
constexpr int kStreamQueries = 128;   // queries per workgroup there: four waves of 32

// ---- what the entry points cover (vit_block.hip, vit_block_train.hip) ----
// Long inputs are walked in slabs of whole sequences of about this many tokens (forward and backward alike).
constexpr int kSlabRows = 32768;
constexpr int kMaxLnDim = 4096;   // longest row a LayerNorm is fused over

inline bool math_ok(unsigned flags) {
    const unsigned m = flags & STGCN_MATH_MASK;
    return m == STGCN_MATH_F32 || m == STGCN_MATH_BF16X3;
}

inline bool linear_ok(int K, int Nout, bool ln) { return K % 32 == 0 && Nout >= 1 && (!ln || K <= kMaxLnDim); }

// ---- the linear's tile form, chosen here and nowhere else (launch_linear_ex and stgcn_vit_linear_tile read it) ----
// vit_linear.hip has three forms of one kernel: 128 x 128 (4 waves, 2 x 2 blocks of 32 x 32 each), 64 x 64 (4 waves, one
// block each) and 32 x 64 (2 waves, one block each).  All compute an element of Y with the same instructions in the same
// order, so the choice moves time, never a bit of the result.
struct LinearTile {
    int bm, bn;
};
constexpr LinearTile kLinearTiles[3] = {{128, 128}, {64, 64}, {32, 64}};   // largest first
// STGCN_VIT_TILE_AUTO takes the largest form that cuts the linear into at least this many tiles, the smallest if none does.
// A compile-time constant (the plan never asks the device): 256 is the CU count of the MI355X, one workgroup per CU.
// NOT MEASURED yet: tools/time_altformer.py --tiles sweep is the run that settles it (DESIGN section 14 "small calls").
constexpr int kLinearTileCut = 256;

inline long long linear_tiles(int M, int Nout, LinearTile t) {
    return (long long)ceil_div(M, t.bm) * ceil_div(Nout, t.bn);
}

// `flags`: only the STGCN_VIT_TILE_MASK field is read (0: 128 x 128, today's behaviour and what training always runs).
inline LinearTile linear_tile(int M, int K, int Nout, unsigned flags) {
    (void)K;   // every form walks all of K in one workgroup
    switch (flags & STGCN_VIT_TILE_MASK) {
        case STGCN_VIT_TILE_64: return kLinearTiles[1];
        case STGCN_VIT_TILE_32: return kLinearTiles[2];
        case STGCN_VIT_TILE_AUTO:
            for (const LinearTile t : kLinearTiles)
                if (linear_tiles(M, Nout, t) >= kLinearTileCut) return t;
            return kLinearTiles[2];
        default: return kLinearTiles[0];
    }
}

// The resident form: what the training entry points and stgcn_vit_block_supported cover.
inline bool block_ok(int L, int D, int heads, int hidden) {
    if (L < 1 || D < 1 || heads < 1 || hidden < 1 || D % heads != 0) return false;
    const int hd = D / heads;
    return (hd == 32 || hd == 64) && L <= kMaxL && D % 64 == 0 && hidden % 64 == 0 && D <= kMaxLnDim;
}

inline bool attention_stream_ok(int L, int heads, int hd) {
    return L >= 1 && L <= kMaxStreamL && heads >= 1 && (hd == 32 || hd == 64);
}

// ---- the inference block's attention launch, chosen here and nowhere else (stgcn_vit_block_forward and
// stgcn_vit_block_forward_supported read it) ----
// resident up to kMaxL, exactly as before the streaming kernel existed (bit-identical results); streaming above, up to
// kMaxStreamL: kSlabRows / kMaxStreamL = 8 whole sequences still fit a slab.  Everything else about the block is length-agnostic.
enum class BlockAttention { none, resident, stream };
inline BlockAttention plan_block_forward(int L, int D, int heads, int hidden) {
    if (block_ok(L, D, heads, hidden)) return BlockAttention::resident;
    if (L > kMaxL && L <= kMaxStreamL && block_ok(kMaxL, D, heads, hidden)) return BlockAttention::stream;
    return BlockAttention::none;
}

// ---- the training block's attention launches, chosen here and nowhere else (stgcn_vit_block_forward_train,
// stgcn_vit_block_backward and the stgcn_vit_block_train_long_* queries read it) ----
// One form for the forward and the backward of a block: resident (launch_attention_packed, launch_attention_backward) up to
// kMaxL, exactly as before the streaming backward existed; stream (launch_attention_stream,
// launch_attention_backward_stream) above.  Today the cut is the inference block's; it is a function of its own because
// it decides other kernels, and a measurement may move one cut without the other.
inline BlockAttention plan_block_train(int L, int D, int heads, int hidden) { return plan_block_forward(L, D, heads, hidden); }

inline int slab_seqs(int B, int L) {
    const int s = kSlabRows / L;
    return s < 1 ? 1 : (s > B ? B : s);
}

// Y (M, Nout) = act(LN?(X) W^T + bias) (+ R).  X (M, K), W (Nout, K), K % 32 == 0.  gamma / beta / eps: LayerNorm of X's
// rows applied while the A tile is staged (gamma == nullptr: none).  math: STGCN_MATH_F32 or STGCN_MATH_BF16X3, optionally
// with a STGCN_VIT_TILE_* field for linear_tile (every other bit must be clear).  launch_linear_ex also takes STGCN_MATH_BF16
// (both operands rounded to nearest-even bf16 while staged, fp32 in memory on both sides): the training mode
// STGCN_VIT_TRAIN_BF16 (vit_block_train.hip) is its only caller, the entry points' math_ok never lets it in from outside.
// Y may alias R (each element is read and written by one thread); it must not alias X.
int launch_linear(const float *X, const float *W, const float *bias, const float *R, const float *gamma, const float *beta,
                  float eps, float *Y, int M, int K, int Nout, bool gelu, unsigned math, hipStream_t st);

// What the training forward and the backward add to the linear (all optional, zero-initialised = the plain linear above):
//   pre      : the value before the activation, acc + bias, is also stored here (M, Nout)           [forward_train: h_pre]
//   dgelu    : the result is multiplied by GELU'(dgelu[row][col]), exact erf form                   [dgrad of fc2]
//   rowscale : then by rowscale[row / L] (stochastic depth: one factor per sequence), before R is added
//   kx       : X's rows are kx long (kx <= K, kx % 4 == 0) and read as zero from kx to K            [dgrad with Nout % 32 != 0]
struct LinearExtra {
    float *pre = nullptr;
    const float *dgelu = nullptr;
    const float *rowscale = nullptr;
    int L = 1;
    int kx = 0;
};
int launch_linear_ex(const float *X, const float *W, const float *bias, const float *R, const float *gamma, const float *beta,
                     float eps, float *Y, int M, int K, int Nout, bool gelu, unsigned math, const LinearExtra &ex,
                     hipStream_t st);

// out (B, L, H*hd) = softmax(scale * q k^T) v per (sequence, head) of the packed qkv (B, L, 3, H, hd); hd in {32, 64},
// L <= kMaxL: K and V of a pair resident in LDS, the whole score row in registers (vit_attention.hip).
int launch_attention_packed(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st);
// The same result up to the summation order for L <= kMaxStreamL: K and V streamed through LDS in tiles of kStreamKeys keys
// under a running soft-max, kStreamQueries queries of a pair per workgroup (vit_attention_stream.hip).
int launch_attention_stream(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st);

// ---- the bf16 mode of the inference block (STGCN_VIT_BF16; vit_block.hip) -------------------------------------------------
// Operands rounded to nearest-even bf16, fp32 accumulate; qkv, the attention output and the fc1 hidden live in the workspace
// as bf16 (each is read by one consumer, as a matrix-core operand only).  Inference, resident attention form only.
inline bool block_bf16_ok(int L, int D, int heads, int hidden) { return block_ok(L, D, heads, hidden); }

// The linear in the bf16 arithmetic (vit_linear.hip): X fp32 (rounded while staged, after the LayerNorm if any) or bf16
// storage (no LayerNorm then), Y fp32 or bf16 storage; W, bias, R, gamma, beta fp32.  `tile`: a STGCN_VIT_TILE_* field.
int launch_linear_bf16(const void *X, bool x_bf16, const float *W, const float *bias, const float *R, const float *gamma,
                       const float *beta, float eps, void *Y, bool y_bf16, int M, int K, int Nout, bool gelu, unsigned tile,
                       hipStream_t st);

// The resident attention on bf16 qkv / out (vit_attention_bf16.hip); L <= kMaxL, hd in {32, 64}.  Its LDS per workgroup:
// K as [keys][hd + 8] and V transposed as [hd][keys + 8], keys = L rounded up to 32, for the pairs a workgroup packs.
inline size_t attention_bf16_lds_bytes(int L, int hd) {
    const int nt = ceil_div(L, 32), g = nt >= 4 ? 1 : 4 / nt, rows = nt * 32;
    return (size_t)g * ((size_t)rows * (hd + 8) + (size_t)hd * (rows + 8)) * 2;
}
int launch_attention_bf16(const void *qkv, void *out, int B, int L, int H, int hd, float scale, hipStream_t st);

// ---- backward (vit_backward.hip) ----------------------------------------------------------------------------------------
// Wt (cols, rows_pad) = W (rows, cols)^T, the columns from `rows` to rows_pad zero-filled: the dgrad dX = dY W is the
// forward linear on the transposed weight, so it shares launch_linear's kernel, arithmetic modes and epilogues.
int launch_transpose_pad(const float *W, float *Wt, int rows, int cols, int rows_pad, hipStream_t st);

// Weight / bias gradient of Y = A W^T + b over the rows [0, M):  dW (Nout, K) = (s dY)^T A,  db (Nout) = column sums of s dY,
// s = rowscale[row / L] or 1.  The reduction over M is cut into wgrad_splits(M, K, Nout) row ranges; each writes one slab of
// `part` ((Nout * K) floats per split, then Nout floats per split for the bias) and launch_sum_parts adds them in split order.
// fp32 matrix cores (v_mfma_f32_32x32x2_f32), no atomics.  `accumulate`: add onto dW / db (sum in `tmp` first).
constexpr int kWgradChunk = 32;                       // tokens per LDS chunk of both wgrad kernels
int wgrad_rows_per_split(int M, int K, int Nout);   // a multiple of kWgradChunk
int wgrad_splits(int M, int K, int Nout);
size_t wgrad_part_floats(int M, int K, int Nout);   // floats of `part`, and of `tmp` = Nout * K + Nout
int launch_wgrad(const float *dY, const float *A, const float *rowscale, int L, float *dW, float *db, float *part, float *tmp,
                 int M, int K, int Nout, bool accumulate, hipStream_t st);
// partial slabs of n floats -> dst, or (accumulate) dst += their sum taken in `tmp`; slab order, no atomics
int reduce_parts(const float *part, int parts, size_t n, float *dst, float *tmp, bool accumulate, hipStream_t st);
// The same gradient in the STGCN_VIT_TRAIN_BF16 arithmetic (vit_wgrad_bf16.hip): dW = r(s dY)^T r(A) with r = round to
// nearest-even bf16 applied while the operands are staged (after the row factor), fp32 accumulate on
// v_mfma_f32_32x32x16_bf16; db sums the unrounded fp32 s dY.  Same splits, slabs, workspace and reduction as launch_wgrad.
int launch_wgrad_bf16(const float *dY, const float *A, const float *rowscale, int L, float *dW, float *db, float *part,
                      float *tmp, int M, int K, int Nout, bool accumulate, hipStream_t st);

// LayerNorm backward over the rows of x (M, D):  dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres),  g = dn * gamma; also
// writes a = LN(x) (the input of the linear behind the LayerNorm, for its wgrad; may be NULL) and the rows' (mean, rstd) to
// `stats` (M, 2), which launch_ln_param_grad reads for dgamma = sum dn xhat, dbeta = sum dn (two-stage, fixed order).
// dx may alias dres or dn (one wave owns a row and reads all of it before it writes).
int launch_ln_backward(const float *x, const float *dn, const float *gamma, const float *beta, float eps, const float *dres,
                       float *dx, float *a, float *stats, int M, int D, hipStream_t st);
int ln_param_splits(int M);
int launch_ln_param_grad(const float *x, const float *dn, const float *stats, float *dgamma, float *dbeta, float *part,
                         float *tmp, int M, int D, bool accumulate, hipStream_t st);   // part: splits * 2 D, tmp: D floats

// dqkv (B, L, 3, H, hd) from the packed qkv, the forward's output `out` and its gradient `dout` (both (B, L, H*hd)).
int launch_attention_backward(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L, int H, int hd,
                              float scale, hipStream_t st);

// The same gradient up to the summation order for L <= kMaxStreamL (vit_attention_bwd_stream.hip): a query kernel (soft-max
// statistics, dQ) and a key kernel (dK, dV) that stream the other side through LDS.  `stats`: attention_stats_floats(B, L, H)
// floats, (m, 1 / l, delta, 0) per (sequence, head, query), written by the first kernel and read by the second.
inline size_t attention_stats_floats(int B, int L, int H) { return (size_t)B * H * L * 4; }
int launch_attention_backward_stream(const float *qkv, const float *out, const float *dout, float *dqkv, float *stats, int B,
                                     int L, int H, int hd, float scale, hipStream_t st);

}  // namespace vit
}  // namespace stgcn
