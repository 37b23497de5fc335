// What the AltFormer heads' transformer block shares between its entry points (vit_block.hip: inference, vit_block_train.hip:
// training): the plan of a block call (plan_block: what every entry point and every query reads to learn whether the flags are
// legal, whether the shape is covered, and which kernels, arithmetic and storage the call runs), the forward's slab walker
// (block_forward), the launchers of the kernels (vit_linear.hip, vit_attention*.hip, vit_backward.hip, vit_wgrad_bf16.hip), and
// the plan and workspace of the whole head (plan_head, HeadStore: vit_head.hip), which hands each stage to plan_block.
// All launchers enqueue on `st` and return a stgcn_status.
#pragma once

#include "common.h"

namespace stgcn {
namespace vit {

constexpr int kMaxL = 256;      // longest sequence the resident attention kernels keep on chip
constexpr int kMaxStreamL = STGCN_VIT_MAX_STREAM_L;   // longest sequence of the streaming attention kernels: a slab holds 8 of them
constexpr int kStreamKeys = 64;       // keys per LDS stage of the streaming kernel (vit_attention_stream.hip)
constexpr int kStreamQueries = 128;   // queries per workgroup there: four waves of 32

// Long inputs are walked in slabs of whole sequences of about this many tokens (forward and backward alike): the
// intermediates of a slab (about 7 KB per token at D = 256) then stay within reach of the caches between the launches that
// write and read them, and the inference workspace does not grow with the batch.
constexpr int kSlabRows = 32768;
constexpr int kMaxLnDim = 4096;   // longest row a LayerNorm is fused over

inline int slab_seqs(int B, int L) {
    const int s = kSlabRows / L;
    return s < 1 ? 1 : (s > B ? B : s);
}

// ---- what the primitives cover ----
inline bool math_ok(unsigned flags) {
    const unsigned m = flags & STGCN_MATH_MASK;
    return m == STGCN_MATH_F32 || m == STGCN_MATH_BF16X3;
}

inline bool linear_ok(int K, int Nout, bool ln) { return K % 32 == 0 && Nout >= 1 && (!ln || K <= kMaxLnDim); }

// the resident attention kernels (forward, bf16 forward, backward, the training bf16 pair) and the streaming ones (forward, backward)
inline bool attention_resident_ok(int L, int heads, int hd) { return L >= 1 && L <= kMaxL && heads >= 1 && (hd == 32 || hd == 64); }
inline bool attention_stream_ok(int L, int heads, int hd) {
    return L >= 1 && L <= kMaxStreamL && heads >= 1 && (hd == 32 || hd == 64);
}

// ---- the linear's tile form, chosen here and nowhere else (launch_linear and stgcn_vit_linear_tile read it) ----
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

// `flags`: only the STGCN_VIT_TILE_MASK field is read (0: 128 x 128, what training always runs).
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

// ---- the plan of a block call, decided here and nowhere else ----
// A plain host function of (entry point, L, D, heads, hidden, flags).  The four entry points below and every stgcn_vit_block_*
// query read it; none of them looks at a flag bit or compares a length again.
// forward_train_drop / backward_drop: the training pair with per-element dropout masks (stgcn_vit_block_forward_train_drop,
// stgcn_vit_block_backward_drop).  They plan as forward_train / backward do, but for the one thing they add: a tile field.
enum class BlockEntry { forward, forward_train, backward, linear_backward, forward_train_drop, backward_drop };
constexpr const char *kBlockEntryName[] = {"stgcn_vit_block_forward", "stgcn_vit_block_forward_train", "stgcn_vit_block_backward",
                                           "stgcn_vit_linear_backward", "stgcn_vit_block_forward_train_drop",
                                           "stgcn_vit_block_backward_drop"};
inline bool block_entry_drop(BlockEntry e) { return e == BlockEntry::forward_train_drop || e == BlockEntry::backward_drop; }
// resident (launch_attention_packed, launch_attention_backward): K and V of a (sequence, head) on chip, up to kMaxL tokens;
// stream (launch_attention_stream, launch_attention_backward_stream): K and V in key tiles through LDS, above kMaxL and up to
// kMaxStreamL; resident_bf16 (launch_attention_bf16): the resident form on bf16 qkv / out, STGCN_VIT_BF16 only;
// resident_train_bf16 (launch_attention_train_bf16, launch_attention_backward_bf16): the resident form on fp32 qkv / out with
// bf16 matrix operands, the two training entries with STGCN_VIT_TRAIN_ATTN_BF16 up to kMaxL tokens; resident_split
// (launch_attention_split): the fp32 resident result with the keys of a (pair, query tile) split over the waves of a workgroup,
// stgcn_vit_block_forward with STGCN_VIT_ATTN_SPLIT at two key tiles or more.  In a plan it means "where the launch is small
// enough": block_attention below decides per launch between it and resident.
enum class BlockAttention { none, resident, stream, resident_bf16, resident_train_bf16, resident_split };

// The split form runs where a launch has fewer (sequence, head) pairs than this.  A compile-time constant, as kLinearTileCut
// (the plan never asks the device).  It started at 256, the CU count of the MI355X (from there on the resident kernel has a
// workgroup for every CU), and was MEASURED down to 192 by profiles/altformer_split_attention_times.json
// (tools/time_altformer.py --attention split --batches 1,2,4,8,16,24,32; the launch-alone rows, DESIGN section 14 "small
// calls"): at 8 to 128 pairs the split launch is never slower than the resident one by more than the spread (2.9 x faster at
// 8 pairs of L = 180, head_dim 64), at 192 pairs of that shape it is (0.80 x), so 192 is the largest measured count beneath
// which that never happens.
constexpr int kAttentionSplitPairs = 192;

struct BlockPlan {
    BlockEntry entry;
    // The flags are not legal for this entry point (STGCN_ERR_ARG, answered before the pointers are looked at): why, or nullptr.
    const char *refusal = nullptr;
    // L, D and hidden fit the layouts (what a size query without `heads` can tell); `resident`: L is a length of the resident
    // kernels, which is all that the older queries (stgcn_vit_block_supported, .._train_supported, .._saved_bytes,
    // .._backward_ws_bytes) cover.
    bool sized = false, resident = false;
    // The shape and the low math bits are covered (else STGCN_ERR_UNSUPPORTED, answered after the pointers).  For
    // linear_backward: the low math bits alone (its shape is the linear's own, L, D, heads and hidden are not read).
    bool covered = false;
    int max_len = 0;                 // the longest sequence this entry point takes with these flags
    BlockAttention attention = BlockAttention::none;
    // The arithmetic (a STGCN_MATH_* value) of each product of the four linears: the qkv forward, the three other forwards,
    // the qkv dgrad, the three other dgrads; and whether the weight gradients take bf16 operands (launch_wgrad_bf16).
    unsigned qkv_fwd = 0, lin_fwd = 0, qkv_dgrad = 0, lin_dgrad = 0;
    bool wgrad_bf16 = false;
    bool bf16_store = false;         // qkv, the attention output and the fc1 hidden are bf16 storage between the launches
    // the STGCN_VIT_TILE_* field the forward's linears get (and the dgrads of backward_drop); the older training pair: 0, 128 x 128 only
    unsigned tile = 0;
    // STGCN_VIT_WGRAD_SMALL (backward_drop, linear_backward): every weight gradient picks its form and cut per product
    // (plan_wgrad below); without it all of them run the 128 form on wgrad_rows_per_split's cut.
    bool wgrad_small = false;
};

inline BlockPlan plan_block(BlockEntry entry, int L, int D, int heads, int hidden, unsigned flags) {
    BlockPlan p;
    p.entry = entry;
    const unsigned low = flags & STGCN_MATH_MASK;
    const bool inference = entry == BlockEntry::forward, bf16 = inference && (flags & STGCN_VIT_BF16) != 0;
    if (inference) {
        if (flags & STGCN_VIT_TRAIN_BF16)
            p.refusal = "STGCN_VIT_TRAIN_BF16 is a training mode (stgcn_vit_block_forward_train, stgcn_vit_block_backward, "
                        "stgcn_vit_linear_backward only)";
        else if (bf16 && (flags & STGCN_VIT_QKV_F32))
            p.refusal = "STGCN_VIT_BF16 and STGCN_VIT_QKV_F32 exclude each other";
        else if (flags & STGCN_VIT_TRAIN_ATTN_BF16)
            p.refusal = "STGCN_VIT_TRAIN_ATTN_BF16 is a training mode (stgcn_vit_block_forward_train, stgcn_vit_block_backward only)";
        else if (flags & STGCN_VIT_WGRAD_SMALL)
            p.refusal = "STGCN_VIT_WGRAD_SMALL is a training option (stgcn_vit_block_backward_drop, stgcn_vit_linear_backward)";
    } else if (flags & STGCN_VIT_BF16) {
        p.refusal = "STGCN_VIT_BF16 is an inference mode (stgcn_vit_block_forward only)";
    } else if ((flags & STGCN_VIT_TILE_MASK) && !block_entry_drop(entry)) {
        p.refusal = "training runs the 128 x 128 linear only (STGCN_VIT_TILE_* set)";
    } else if ((flags & STGCN_VIT_WGRAD_SMALL) && !block_entry_drop(entry) && entry != BlockEntry::linear_backward) {
        p.refusal = "STGCN_VIT_WGRAD_SMALL is read by stgcn_vit_block_forward_train_drop, stgcn_vit_block_backward_drop and "
                    "stgcn_vit_linear_backward only";
    } else if (entry == BlockEntry::linear_backward && (flags & STGCN_VIT_TRAIN_ATTN_BF16)) {
        p.refusal = "STGCN_VIT_TRAIN_ATTN_BF16 is a mode of the block (stgcn_vit_block_forward_train, stgcn_vit_block_backward only)";
    } else if (flags & STGCN_VIT_ATTN_SPLIT) {
        p.refusal = "STGCN_VIT_ATTN_SPLIT is an inference option (stgcn_vit_block_forward only)";
    }
    // Arithmetic.  STGCN_VIT_QKV_F32 moves the qkv linear (and its dgrad) to f32: an error in q or k is multiplied by the size
    // of the scores before the exponential.  STGCN_VIT_BF16 (inference): every product on operands rounded to bf16, the three
    // intermediates that only feed matrix cores stored as bf16; the low bits are not read.  STGCN_VIT_TRAIN_BF16: bf16
    // operands for every product of a linear (fp32 in memory on both sides) but the qkv FORWARD, which stays what it is
    // without the bit, for the reason above.
    p.wgrad_bf16 = !inference && (flags & STGCN_VIT_TRAIN_BF16) != 0;
    p.wgrad_small = (entry == BlockEntry::backward_drop || entry == BlockEntry::linear_backward) && (flags & STGCN_VIT_WGRAD_SMALL) != 0;
    p.bf16_store = bf16;
    p.tile = inference || block_entry_drop(entry) ? flags & STGCN_VIT_TILE_MASK : 0;
    p.qkv_fwd = bf16 ? (unsigned)STGCN_MATH_BF16 : (flags & STGCN_VIT_QKV_F32) ? (unsigned)STGCN_MATH_F32 : low;
    p.lin_fwd = p.lin_dgrad = bf16 || p.wgrad_bf16 ? (unsigned)STGCN_MATH_BF16 : low;
    p.qkv_dgrad = p.wgrad_bf16 ? (unsigned)STGCN_MATH_BF16 : p.qkv_fwd;
    const bool low_ok = bf16 || math_ok(flags);
    if (entry == BlockEntry::linear_backward) {
        p.covered = low_ok;
        return p;
    }
    // Coverage.  Everything about the block but its attention is length-agnostic; kSlabRows / kMaxStreamL = 8 whole sequences
    // fit a slab.  The bf16 attention has a resident form only.
    p.max_len = bf16 ? kMaxL : kMaxStreamL;
    p.resident = L <= kMaxL;
    p.sized = L >= 1 && L <= p.max_len && D >= 1 && hidden >= 1 && D % 64 == 0 && hidden % 64 == 0;
    const bool heads_ok = heads >= 1 && D % heads == 0 && (D / heads == 32 || D / heads == 64) && D <= kMaxLnDim;
    // STGCN_VIT_TRAIN_ATTN_BF16 moves the resident attention of the two training entries to bf16 operands; the streaming
    // lengths run the fp32 kernels they run without it.
    const bool attn_bf16 = !inference && (flags & STGCN_VIT_TRAIN_ATTN_BF16) != 0;
    // STGCN_VIT_ATTN_SPLIT (inference) moves the fp32 resident attention to its split form where there are two key tiles or
    // more to split; the bf16 and the streaming attention have no such form and run as they do without the bit.
    const bool split = inference && (flags & STGCN_VIT_ATTN_SPLIT) != 0 && L > 32;
    if (p.sized && heads_ok)
        p.attention = bf16 ? BlockAttention::resident_bf16
                      : !p.resident ? BlockAttention::stream
                      : attn_bf16 ? BlockAttention::resident_train_bf16
                      : split ? BlockAttention::resident_split : BlockAttention::resident;
    p.covered = p.attention != BlockAttention::none && low_ok;
    return p;
}

// The attention kernel of one launch of a planned call: the plan's, but for the one thing a plan cannot know, the launch's
// sequence count.  block_forward and stgcn_vit_block_attention_form read this and nothing else.
inline BlockAttention block_attention(const BlockPlan &p, int sequences, int heads) {
    if (p.attention != BlockAttention::resident_split) return p.attention;
    return (long long)sequences * heads < kAttentionSplitPairs ? BlockAttention::resident_split : BlockAttention::resident;
}

// The two answers an entry point gives from the plan alone: before its pointer checks, and after them.
inline int block_refused(const BlockPlan &p) { return fail(STGCN_ERR_ARG, "%s: %s", kBlockEntryName[(int)p.entry], p.refusal); }
inline int block_unsupported(const BlockPlan &p, int L, int D, int heads, int hidden, unsigned flags) {
    if (p.bf16_store)
        return fail(STGCN_ERR_UNSUPPORTED, "%s: L = %d, D = %d, heads = %d, hidden = %d with STGCN_VIT_BF16 (covered: head_dim "
                    "32 / 64, L <= %d, D and hidden multiples of 64)", kBlockEntryName[(int)p.entry], L, D, heads, hidden, p.max_len);
    return fail(STGCN_ERR_UNSUPPORTED, "%s: L = %d, D = %d, heads = %d, hidden = %d, math %u (covered: head_dim 32 / 64, L <= %d, "
                "D and hidden multiples of 64, f32 / bf16x3)", kBlockEntryName[(int)p.entry], L, D, heads, hidden,
                flags & STGCN_MATH_MASK, p.max_len);
}

// The parameters of a block as the forward reads them (nn.Linear.weight as stored; a bias may be NULL).
struct BlockWeights {
    const float *norm1_weight, *norm1_bias, *Wqkv, *bqkv, *Wproj, *bproj, *norm2_weight, *norm2_bias, *W1, *b1, *W2, *b2;
    bool present() const { return norm1_weight && norm1_bias && Wqkv && Wproj && norm2_weight && norm2_bias && W1 && W2; }
};

// Where the forward's intermediates live: one slab's rows in the caller's workspace, reused by every slab (inference), or the
// whole batch's in `saved`, where the backward reads them (training: 9 D floats per token at hidden = 2 D, h_pre = the fc1
// output before the GELU included).  One carve for both, in this order; run on a NULL base it sizes the buffer.  The bf16
// pieces are at most as large as the fp32 ones, so the bf16 mode fits what stgcn_vit_block_ws_bytes sizes.
struct BlockStore {
    void *qkv, *att, *hid;      // fp32, or bf16 storage where the plan says so
    float *x1, *hpre;           // hpre: NULL in the workspace
    bool per_slab;
    size_t total;
    BlockStore(void *base, const BlockPlan &plan, int B, int L, int D, int hidden) : per_slab(plan.entry == BlockEntry::forward) {
        const size_t rows = (size_t)(per_slab ? slab_seqs(B, L) : B) * L, es = plan.bf16_store ? 2 : 4;
        Carve c(base);
        qkv = c.take<char>(rows * 3 * D * es);
        att = c.take<char>(rows * D * es);
        x1 = c.take<float>(rows * D);
        hpre = per_slab ? nullptr : c.take<float>(rows * hidden);
        hid = c.take<char>(rows * hidden * es);
        total = c.off;
    }
};

// Per-element dropout factors of a training call (0 or 1 / (1 - p), fp32; a NULL member = 1): behind the projection (B, L, D),
// behind the GELU (B, L, hidden), behind the second MLP linear (B, L, D).  stgcn_vit_drop_masks of the C ABI, member for member.
struct BlockDrop {
    const float *proj = nullptr, *act = nullptr, *fc2 = nullptr;
    bool any() const { return proj || act || fc2; }
};

// The forward of one block, the one loop that every forward entry point runs: five launches per slab of whole sequences,
//   qkv = LN1(x) Wqkv^T + b -> attention -> x1 = s1 (a Wproj^T + b) + x -> h = GELU(LN2(x1) W1^T + b1) -> y = s2 (h W2^T + b2) + x1
// (both LayerNorms inside the linear that consumes them), with the kernels, arithmetic and storage of `plan`, the
// intermediates in `store`, and stochastic depth's per-sequence factors scale1 / scale2 (B floats each, or NULL = 1).
// `drop` (the _drop training forward only): x1 = x + s1 (m_proj * a), h = m_act * GELU(h_pre), y = x1 + s2 (m_fc2 * (h W2^T + b2)),
// each mask walked per slab as scale1 / scale2 are.
int block_forward(const BlockPlan &plan, const float *x, const BlockWeights &w, const BlockStore &store, const float *scale1,
                  const float *scale2, float eps, float scale, float *y, int B, int L, int D, int heads, int hidden, hipStream_t st,
                  const BlockDrop &drop = BlockDrop{});

// What the training forward and the backward add to the linear (all optional, zero-initialised = the plain linear):
//   pre      : the value before the activation, acc + bias, is also stored here (M, Nout)           [forward_train: h_pre]
//   dgelu    : the result is multiplied by GELU'(dgelu[row][col]), exact erf form                   [dgrad of fc2]
//   mask     : then by mask[row][col], an (M, Nout) fp32 factor (dropout: 0 or 1 / (1 - p)), after GELU / GELU'    [_drop entries]
//   rowscale : then by rowscale[row / L] (stochastic depth: one factor per sequence), before R is added
//   kx       : X's rows are kx long (kx <= K, kx % 4 == 0) and read as zero from kx to K            [dgrad with Nout % 32 != 0]
struct LinearExtra {
    float *pre = nullptr;
    const float *dgelu = nullptr;
    const float *mask = nullptr;
    const float *rowscale = nullptr;
    int L = 1;
    int kx = 0;
};
// Y (M, Nout) = act(LN?(X) W^T + bias) (+ R).  X (M, K), W (Nout, K), K % 32 == 0.  gamma / beta / eps: LayerNorm of X's
// rows applied while the A tile is staged (gamma == nullptr: none).  The one host launcher of vit_linear.hip.  `mode`:
//   a STGCN_MATH_* value: F32, BF16X3, or BF16 (both operands rounded to nearest-even bf16 while staged, fp32 accumulate;
//     only the plan's two bf16 modes and stgcn_vit_linear_bf16 hand it in, the entry points' math_ok never lets it in from outside)
//   | a STGCN_VIT_TILE_* field for linear_tile
//   | STGCN_VIT_X_BF16, STGCN_VIT_Y_BF16 (BF16 arithmetic only): X (no LayerNorm then) / Y is bf16 storage, else fp32.
// W, bias, R, gamma, beta are fp32.  Y may alias R (each element is read and written by one thread); it must not alias X.
int launch_linear(const void *X, const float *W, const float *bias, const float *R, const float *gamma, const float *beta,
                  float eps, void *Y, int M, int K, int Nout, bool gelu, unsigned mode, hipStream_t st,
                  const LinearExtra &ex = LinearExtra{});

// out (B, L, H*hd) = softmax(scale * q k^T) v per (sequence, head) of the packed qkv (B, L, 3, H, hd); hd in {32, 64},
// L <= kMaxL: K and V of a pair resident in LDS, the whole score row in registers (vit_attention.hip).
int launch_attention_packed(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st);
// The same result up to the summation order for L <= kMaxStreamL: K and V streamed through LDS in tiles of kStreamKeys keys
// under a running soft-max, kStreamQueries queries of a pair per workgroup (vit_attention_stream.hip).
int launch_attention_stream(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st);
// The resident result up to the summation order for L <= kMaxL, for launches of few pairs: a workgroup per (pair, query tile of
// 32), a wave per key tile, the waves' partial soft-maxes merged through LDS in a fixed order (vit_attention_split.hip).
int launch_attention_split(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st);

// The resident attention on bf16 qkv / out (vit_attention_bf16.hip); L <= kMaxL, hd in {32, 64}.
int launch_attention_bf16(const void *qkv, void *out, int B, int L, int H, int hd, float scale, hipStream_t st);

// The resident attention for training on bf16 matrix operands (vit_attention_train_bf16.hip): fp32 qkv, out, dout and dqkv,
// L <= kMaxL, hd in {32, 64}.  Scores scale * (qh kh^T + qh kl^T + ql kh^T) of the split q and k, every other product on
// operands rounded once; the backward's delta is sum P dP of its own products and `out` is not read.
// (How the resident kernels pack pairs into workgroups and what LDS each takes: vit_attention_common.h.)
int launch_attention_train_bf16(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st);
int launch_attention_backward_bf16(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L, int H, int hd,
                                   float scale, hipStream_t st);

// ---- backward (vit_backward.hip) ----------------------------------------------------------------------------------------
// Wt (cols, rows_pad) = W (rows, cols)^T, the columns from `rows` to rows_pad zero-filled: the dgrad dX = dY W is the
// forward linear on the transposed weight, so it shares launch_linear's kernel, arithmetic modes and epilogues.
int launch_transpose_pad(const float *W, float *Wt, int rows, int cols, int rows_pad, hipStream_t st);

// out (n floats) = a * m elementwise, n % 4 == 0 and all three 16-byte aligned: a masked gradient made once for the dgrad and
// the wgrad that both read it (16-byte loads and stores, one owner per element).
int launch_mask_mul(const float *a, const float *m, float *out, size_t n, hipStream_t st);

// Weight / bias gradient of Y = A W^T + b over the rows [0, M):  dW (Nout, K) = (s dY)^T A,  db (Nout) = column sums of s dY,
// s = rowscale[row / L] or 1.  The reduction over M is cut into row ranges (plan_wgrad below); each writes one slab of
// `part` ((Nout * K) floats per split, then Nout floats per split for the bias) and launch_sum_parts adds them in split order.
// fp32 matrix cores (v_mfma_f32_32x32x2_f32), no atomics.  `accumulate`: add onto dW / db (sum in `tmp` first).
constexpr int kWgradChunk = 32;                       // tokens per LDS chunk of both wgrad kernels
int wgrad_rows_per_split(int M, int K, int Nout);   // a multiple of kWgradChunk

// ---- the form and the cut of one weight gradient, chosen here and nowhere else ----
// Both kernels have two forms: a workgroup owns a 128 x 128 tile of dW (2 x 2 accumulator blocks per wave) or a 64 x 64 one
// (one block per wave, four times the workgroups per split).  Split s covers the chunks [s cps + min(s, long_splits), ...),
// cps + 1 of them for the first long_splits splits and cps for the rest: ranges are multiples of the chunk, none is empty.
struct WgradPlan {
    int tile = 128;                       // 128 or 64
    int splits = 1, cps = 1, long_splits = 0;
    bool may_direct = false;              // STGCN_VIT_WGRAD_SMALL only: calls without it keep their launch_sum_parts
    long long workgroups(int K, int Nout) const { return (long long)ceil_div(Nout, tile) * ceil_div(K, tile) * splits; }
    // one split that does not accumulate: the kernel stores dW and db itself, no slab and no launch_sum_parts
    bool direct(bool accumulate) const { return may_direct && splits == 1 && !accumulate; }
    size_t part_floats(int K, int Nout) const { return (size_t)splits * ((size_t)Nout * K + Nout); }
};
// A launch of the 128 form on today's cut hands over to nothing smaller from this many workgroups on: one per CU of the
// MI355X, a compile-time constant as kLinearTileCut is (the plan never asks the device).
constexpr int kWgradHandOver = 256;
constexpr int kWgradSmallMinChunks = 4;   // a split of the small rule is at least this many chunks (128 tokens) long

inline WgradPlan wgrad_cut(int tile, int chunks, int splits) {   // `splits` ranges of whole chunks, as even as they come
    WgradPlan w;
    w.tile = tile, w.splits = splits, w.cps = chunks / splits, w.long_splits = chunks % splits;
    w.may_direct = true;
    return w;
}

// small == false: the 128 form on wgrad_rows_per_split's uniform cut, what every call ran before there was a choice.
// small == true (STGCN_VIT_WGRAD_SMALL), with u = the workgroups of that launch:
//   u >= kWgradHandOver: the 128 form in as many splits as that rule aims at, min(ceil(512 / tiles128), ceil(M / 256)), cut
//   evenly (the uniform cut rounds a split up to whole chunks and can so end a split or two short of its aim, 29 for 32
//   at 8,193 tokens of D = 512: a count that falls while M grows);
//   else the 64 form, in min(floor(kWgradHandOver / tiles64), chunks / kWgradSmallMinChunks) (at least one) even splits,
//   where that gives at least u workgroups; where it does not (tiles64 so many that two splits would pass the hand-over
//   count, while the 128 form's cut has grown past one split's worth), the 128 form as in the first case.
// The 64 form's target is the hand-over count, one workgroup per CU, not the 128 rule's two: a count that stepped DOWN where
// the rows grow into the 128 form would make a larger call the slower one.  With these pieces the workgroup count never
// falls as M grows and is never below u.  A split of the 64 form is at least 4 chunks long: it reads 2 x 128 x 64 floats
// (64 KB) of operands for a 16 KB slab that launch_sum_parts reads again, so slab traffic stays at half the operand
// traffic or less; at 2 chunks the two would be level.
inline WgradPlan plan_wgrad(int M, int K, int Nout, bool small) {
    const int rps = wgrad_rows_per_split(M, K, Nout);
    WgradPlan w;
    w.splits = ceil_div(M, rps), w.cps = rps / kWgradChunk;
    if (!small) return w;
    const long long u = w.workgroups(K, Nout);
    const int chunks = ceil_div(M, kWgradChunk), tiles128 = ceil_div(Nout, 128) * ceil_div(K, 128);
    const int aim = ceil_div(512, tiles128) < ceil_div(M, 256) ? ceil_div(512, tiles128) : ceil_div(M, 256);
    if (u >= kWgradHandOver) return wgrad_cut(128, chunks, aim);
    const long long tiles64 = (long long)ceil_div(Nout, 64) * ceil_div(K, 64);
    long long s = kWgradHandOver / tiles64;
    if (s > chunks / kWgradSmallMinChunks) s = chunks / kWgradSmallMinChunks;
    if (s < 1) s = 1;
    if (tiles64 <= kWgradHandOver && tiles64 * s >= u) return wgrad_cut(64, chunks, (int)s);
    return wgrad_cut(128, chunks, aim);
}
inline WgradPlan plan_wgrad(const BlockPlan &p, int M, int K, int Nout) { return plan_wgrad(M, K, Nout, p.wgrad_small); }

// `wp`: plan_wgrad's answer for this product; `part` holds wp.part_floats(K, Nout) floats (not touched where wp.direct()).
int launch_wgrad(const WgradPlan &wp, const float *dY, const float *A, const float *rowscale, int L, float *dW, float *db,
                 float *part, float *tmp, int M, int K, int Nout, bool accumulate, hipStream_t st);
// partial slabs of n floats -> dst, or (accumulate) dst += their sum taken in `tmp`; slab order, no atomics
int reduce_parts(const float *part, int parts, size_t n, float *dst, float *tmp, bool accumulate, hipStream_t st);
// The same gradient in the STGCN_VIT_TRAIN_BF16 arithmetic (vit_wgrad_bf16.hip): dW = r(s dY)^T r(A) with r = round to
// nearest-even bf16 applied while the operands are staged (after the row factor), fp32 accumulate on
// v_mfma_f32_32x32x16_bf16; db sums the unrounded fp32 s dY.  Same splits, slabs, workspace and reduction as launch_wgrad.
int launch_wgrad_bf16(const WgradPlan &wp, const float *dY, const float *A, const float *rowscale, int L, float *dW, float *db,
                      float *part, float *tmp, int M, int K, int Nout, bool accumulate, hipStream_t st);

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

// ---- the whole head (vit_head.hip) ------------------------------------------------------------------------------------------
// out (S, D) = the mean (sum / L) or the maximum over the L tokens of every sequence of the dense x (S, L, D), D % 4 == 0:
// a workgroup per (sequence, chunk of D), 16-byte loads along D, the token lanes of a workgroup joined through LDS in
// ascending order.  The maximum starts from a token of the sequence, never from zero.
// (the grid: one workgroup of 256 threads per sequence and 64 float4 columns where there are many sequences - launch_pool)
inline bool pool_ok(long long S, int L, int D) {
    return S >= 1 && S < (1ll << 31) && L >= 1 && D >= 4 && D % 4 == 0 && grid_fits(S * ceil_div(D / 4, 64), 256);
}
// `first` (STGCN_VIT_POOL_CLS): the "pool" is token 0 of every sequence - the selection over a sequence of one token, L apart.
int launch_pool(const float *x, float *out, long long S, int L, int D, bool max, hipStream_t st, bool first = false);
// logits (N, classes) = LayerNorm_D(pool_L(x (N, L, D))) W^T + bias, one workgroup per clip: the pooled row and its LayerNorm
// in LDS, a wave per class.  D % 64 == 0, D <= kMaxLnDim (the blocks' rule), any L and classes.  bias may be NULL.
inline bool pool_classify_ok(int N, int L, int D, int classes) {
    return N >= 1 && L >= 1 && classes >= 1 && D >= 64 && D % 64 == 0 && D <= kMaxLnDim && grid_fits(N, 1024);   // (kClsThreads)
}
int launch_pool_classify(const float *x, const float *gamma, const float *beta, float eps, const float *W, const float *bias,
                         float *logits, int N, int L, int D, int classes, bool max, hipStream_t st, bool first = false);

// ---- the ST-ViT head's patch embedding (vit_patch.hip) --------------------------------------------------------------------
// x (N, n + 1, E) from the stem output z cut into p1 x p2 patches: row 0 of a clip is cls + pos[0], row 1 + a w + b is
// patch (a, b) W^T + bias + pos[1 + a w + b] (include/stgcn_hip.h, "The ST-ViT head").  The product is vit_linear_kernel on
// PatchRows: M = N n rows, K = p1 p2 C, read in place from z as (N, T, V, C).  M is small (99 rows per clip) and K long (5120),
// so the contraction is cut into `splits` slabs of `cps` chunks of 32 over grid.y; the slabs' sums land in the workspace and
// one kernel adds them in slab order, with the bias and the position row, and writes the class rows.  No atomics.
// The plan, decided here and nowhere else (stgcn_vit_patch_embed, .._supported, .._ws_bytes and .._cut read it):
//   tile  : the largest form whose tiles, each cut into as many slabs as kPatchMinChunks allows, still make kLinearTileCut
//           workgroups (a large tile reads each operand element less often, the cut supplies the workgroups), else 32 x 64;
//   splits: as many as bring tiles x splits to kLinearTileCut, while a slab keeps kPatchMinChunks chunks.
// MEASURED against three other rules at 1 to 64 clips of the reference shape (profiles/stvit_patch_cut_ab.txt: the tile by
// STGCN_VIT_TILE_AUTO's rule first and the cut second, and both rules aiming at 512 workgroups with slabs of 4 chunks): in
// bf16x3 this one is the fastest or within 5 % of it at every count but 4 clips (0.049 against 0.044 ms) and 8 clips (0.063
// against 0.057 ms), and 1.2 - 1.8 x faster than the tile-first rule from 2 to 64 clips.
constexpr int kPatchMinChunks = 8;
struct PatchPlan {
    const char *refusal = nullptr;   // a flag bit this entry point does not know (STGCN_ERR_ARG)
    bool shaped = false;             // positive dimensions, T % p1 == 0, V % p2 == 0 (else STGCN_ERR_ARG)
    bool covered = false;            // (p2 C) % 32 == 0, f32 / bf16x3, sizes within the index types (else STGCN_ERR_UNSUPPORTED)
    bool transpose = false;          // z is (N, C, T, V): one pass writes it as (N, T, V, C) into the workspace first
    unsigned math = 0;
    int n = 0, w = 0, K = 0, M = 0;
    LinearTile tile{0, 0};
    int splits = 0, cps = 0;
};

inline PatchPlan plan_patch(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    PatchPlan p;
    if (flags & ~(unsigned)(STGCN_MATH_MASK | STGCN_IN_NTVC)) p.refusal = "only the math bits and STGCN_IN_NTVC are read";
    p.shaped = N >= 1 && C >= 1 && T >= 1 && V >= 1 && p1 >= 1 && p2 >= 1 && E >= 1 && T % p1 == 0 && V % p2 == 0;
    if (!p.shaped) return p;
    p.transpose = (flags & STGCN_IN_NTVC) == 0;
    p.math = flags & STGCN_MATH_MASK;
    p.w = V / p2;
    p.n = (T / p1) * p.w;
    const long long K = (long long)p1 * p2 * C, M = (long long)N * p.n, clip = (long long)T * V * C, lim = 1ll << 31;
    if (!math_ok(flags) || ((long long)p2 * C) % 32 != 0 || clip >= lim || (M + N) * E >= lim) return p;
    p.K = (int)K;
    p.M = (int)M;
    const int chunks = p.K / 32;
    const long long most = chunks / kPatchMinChunks > 0 ? chunks / kPatchMinChunks : 1;
    p.tile = kLinearTiles[2];
    for (const LinearTile t : kLinearTiles)
        if (linear_tiles(p.M, E, t) * most >= kLinearTileCut) {
            p.tile = t;
            break;
        }
    const long long tiles = linear_tiles(p.M, E, p.tile);
    long long want = (kLinearTileCut + tiles - 1) / tiles;
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.cps = ceil_div(chunks, (int)want);
    p.splits = ceil_div(chunks, p.cps);
    p.covered = true;
    return p;
}

// The workspace of a patch embedding, one carve: the transposed copy of z where it arrives as (N, C, T, V), and the slabs.
// Nothing of the size of the rearranged patches (N n K floats) exists for (N, T, V, C) input.
struct PatchStore {
    float *zt, *part;
    size_t total;
    PatchStore(void *base, const PatchPlan &p, int N, int C, int T, int V, int E) {
        Carve c(base);
        zt = p.transpose ? c.take<float>((size_t)N * C * T * V) : nullptr;
        part = c.take<float>((size_t)p.splits * p.M * E);
        total = c.off;
    }
};
int launch_patch_embed_vit(const PatchPlan &p, const PatchStore &store, const float *z, const float *W, const float *bias,
                           const float *cls, const float *pos, float *x, int N, int C, int T, int V, int p1, int p2, int E,
                           hipStream_t st);
// zt (N, P, C) = z (N, C, P)^T per clip: the pass that brings (N, C, T, V) input to the layout the patches are read from
// (P = T V), and, with C and P exchanged, the one that takes the patches' gradient back (vit_patch.hip).
int launch_patch_transpose(const float *z, float *zt, int N, int C, int P, hipStream_t st);

// ---- the backward of that embedding (vit_patch_backward.hip) ---------------------------------------------------------------
// From dx (N, n + 1, E), the gradient of the embedding's output; each output optional:
//   dW (E, K)   = dx_tokens^T patches      vit_wgrad_kernel on PatchWgradRows: the A operand read in place from z, the dY rows
//   dbias (E)   = column sums of dx_tokens   skipping the class rows; token splits into slabs, launch_sum_parts adds them
//   dz          = dx_tokens W              vit_linear_kernel on PatchGradRows: the weight transposed once into the workspace,
//                                          the epilogue stores into z's (N, T, V, C) layout, every element written once
//   dpos (n + 1, E), dcls (E)              sums over the clips in clip order, one thread per element
// dx_tokens: the N n patch rows of dx.  No (N, n, K) tensor exists; (N, C, T, V) input is transposed into the workspace for
// the wgrad and dz is transposed back from it, mirroring the forward.  The plan, decided here and nowhere else
// (stgcn_vit_patch_embed_backward, .._supported, .._ws_bytes and .._cut read it): the forward's coverage plus E % 4 == 0 (the
// dgrad reads dx's rows with 16-byte loads); the wgrad's token splits by wgrad_rows_per_split, the blocks' rule; the dgrad's
// tile by STGCN_VIT_TILE_AUTO's rule (the forms agree bit for bit).
struct PatchBackwardPlan {
    const char *refusal = nullptr;   // a flag bit this entry point does not know (STGCN_ERR_ARG)
    bool shaped = false;             // as PatchPlan
    bool covered = false;
    bool transpose = false;          // z and dz are (N, C, T, V)
    unsigned math = 0;               // of the dgrad; the wgrad is fp32 matrix cores always
    int n = 0, w = 0, K = 0, M = 0;
    int Epad = 0;                    // E rounded up to the linear's chunk: the dgrad's contraction length
    int rps = 0, splits = 0;         // the wgrad's tokens per split and splits
    LinearTile tile{0, 0};           // the dgrad's
};

inline PatchBackwardPlan plan_patch_backward(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    PatchBackwardPlan b;
    const PatchPlan f = plan_patch(N, C, T, V, p1, p2, E, flags);
    b.refusal = f.refusal, b.shaped = f.shaped, b.transpose = f.transpose, b.math = f.math;
    b.n = f.n, b.w = f.w, b.K = f.K, b.M = f.M;
    if (!f.shaped || !f.covered || E % 4 != 0 || (long long)E * f.K >= (1ll << 31)) return b;
    b.Epad = ceil_div(E, 32) * 32;
    b.rps = wgrad_rows_per_split(b.M, b.K, E);
    b.splits = ceil_div(b.M, b.rps);
    b.tile = linear_tile(b.M, b.Epad, b.K, STGCN_VIT_TILE_AUTO);
    b.covered = true;
    return b;
}

// The workspace of the backward, one carve, sized for all outputs: for (N, C, T, V) input one buffer of z's size, which holds
// the transposed copy of z while the wgrad reads it and then the gradient before it is transposed back (the launches follow
// each other on one stream: the dgrad, which writes it whole, starts after the wgrad has finished); the transposed weight; the
// wgrad's slabs (dW's, then dbias').
struct PatchBackwardStore {
    float *zt, *dzt, *Wt, *part;
    size_t total;
    PatchBackwardStore(void *base, const PatchBackwardPlan &p, int N, int C, int T, int V, int E) {
        Carve c(base);
        zt = dzt = p.transpose ? c.take<float>((size_t)N * C * T * V) : nullptr;
        Wt = c.take<float>((size_t)p.K * p.Epad);
        part = c.take<float>((size_t)p.splits * ((size_t)E * p.K + E));
        total = c.off;
    }
};
int launch_patch_embed_backward(const PatchBackwardPlan &p, const PatchBackwardStore &store, const float *z, const float *W,
                                const float *dx, float *dW, float *dbias, float *dcls, float *dpos, float *dz, int N, int C, int T,
                                int V, int p1, int p2, int E, hipStream_t st);

// ---- the backward of the pooled classifier (vit_head.hip) -------------------------------------------------------------------
// logits = LN(pooled) W^T + bias with pooled = x[:, 0] (`first`) or the mean over the L tokens.  Two launches and two ordered
// sums: a workgroup per clip recomputes the pooled row and its statistics, takes g = dlogits[n] W, the LayerNorm backward of
// it, writes dx of the clip whole (first: the pooled gradient in row 0 and zeros below; mean: the pooled gradient / L in every
// row) and the clip's parts of dln_weight and dln_bias and its normalised row; a second kernel owns one element of dW each and
// adds dlogits[n][c] * normalised[n][d] over the clips in clip order, as the sums of the parts and of dbias are.
struct ClassifyBackwardStore {
    float *normed, *gpart, *bpart;   // (N, D) each: LN(pooled) rows, the clips' dln_weight / dln_bias parts
    size_t total;
    ClassifyBackwardStore(void *base, int N, int D) {
        Carve c(base);
        normed = c.take<float>((size_t)N * D);
        gpart = c.take<float>((size_t)N * D);
        bpart = c.take<float>((size_t)N * D);
        total = c.off;
    }
};
int launch_pool_classify_backward(const ClassifyBackwardStore &store, const float *x, const float *gamma, const float *beta,
                                  float eps, const float *W, const float *dlogits, float *dx, float *dgamma, float *dbeta,
                                  float *dW, float *dbias, int N, int L, int D, int classes, bool first, hipStream_t st);

// The plan of a whole-head call, decided here and nowhere else: stgcn_altformer_head_supported, .._ws_bytes and .._forward read
// it and none of them looks at a flag bit or compares a length again.  The two stages' blocks are plan_block's, unrestated.
//   ST (STGCN_EMBED_TS off): N*T sequences of V joints at E1 -> mean over the joints -> N sequences of T frames at E2 -> max
//   TS (STGCN_EMBED_TS on) : N*V sequences of T frames at E1 -> max over the frames  -> N sequences of V joints at E2 -> mean
struct HeadPlan {
    const char *refusal = nullptr;   // head_flags carries a bit this entry point does not know (STGCN_ERR_ARG)
    bool shaped = false;             // every dimension is positive (else STGCN_ERR_ARG: nothing below is meaningful)
    bool covered = false;            // both stages' plans are legal and covered, and so is the glue
    unsigned embed_flags = 0;        // what launch_patch_embed gets for the first embedding
    bool pool1_max = false, pool2_max = false;
    int B1 = 0, L1 = 0, L2 = 0;      // sequences and tokens per sequence of stage 1; tokens per sequence of stage 2 (N sequences)
    BlockPlan stage1, stage2;
};

inline HeadPlan plan_head(const stgcn_altformer_head_shape &s, unsigned flags1, unsigned flags2, unsigned head_flags) {
    HeadPlan p;
    if (head_flags & ~(unsigned)(STGCN_EMBED_TS | STGCN_IN_NTVC)) p.refusal = "head_flags: only STGCN_EMBED_TS and STGCN_IN_NTVC are read";
    p.shaped = s.N >= 1 && s.T >= 1 && s.V >= 1 && s.C >= 1 && s.E1 >= 1 && s.E2 >= 1 && s.heads >= 1 && s.hidden1 >= 1 &&
               s.hidden2 >= 1 && s.depth1 >= 1 && s.depth2 >= 1 && s.classes >= 1;
    const bool ts = (head_flags & STGCN_EMBED_TS) != 0;
    p.embed_flags = head_flags & (STGCN_EMBED_TS | STGCN_IN_NTVC);
    p.pool1_max = ts;
    p.pool2_max = !ts;
    p.L1 = ts ? s.T : s.V;
    p.L2 = ts ? s.V : s.T;
    p.stage1 = plan_block(BlockEntry::forward, p.L1, s.E1, s.heads, s.hidden1, flags1);
    p.stage2 = plan_block(BlockEntry::forward, p.L2, s.E2, s.heads, s.hidden2, flags2);
    if (!p.shaped) return p;
    const long long B1 = (long long)s.N * p.L2;
    // 65535 clips: the embeddings put the clip on a grid axis (stgcn_patch_embed's own limit)
    const bool glue = s.N <= 65535 && pool_ok(B1, p.L1, s.E1) && pool_classify_ok(s.N, p.L2, s.E2, s.classes);
    p.B1 = glue ? (int)B1 : 0;
    p.covered = glue && !p.stage1.refusal && !p.stage2.refusal && p.stage1.covered && p.stage2.covered;
    return p;
}

// The workspace of a whole-head call, one carve: the two activation buffers of each stage (block_forward's y must not alias
// its x), the pooled rows between the stages, and one block workspace, the larger stage's.  Run on a NULL base it sizes the
// buffer; `block_bytes` is the one term that does not grow with the batch beyond a slab.
struct HeadStore {
    float *a1, *b1, *pooled, *a2, *b2;
    void *block;
    size_t block_bytes, total;
    HeadStore(void *base, const HeadPlan &p, const stgcn_altformer_head_shape &s) {
        const size_t rows1 = (size_t)p.B1 * p.L1, rows2 = (size_t)s.N * p.L2;
        const size_t w1 = BlockStore(nullptr, p.stage1, p.B1, p.L1, s.E1, s.hidden1).total;
        const size_t w2 = BlockStore(nullptr, p.stage2, s.N, p.L2, s.E2, s.hidden2).total;
        block_bytes = w1 > w2 ? w1 : w2;
        Carve c(base);
        a1 = c.take<float>(rows1 * s.E1);
        b1 = c.take<float>(rows1 * s.E1);
        pooled = c.take<float>((size_t)p.B1 * s.E1);
        a2 = c.take<float>(rows2 * s.E2);
        b2 = c.take<float>(rows2 * s.E2);
        block = c.take<char>(block_bytes);
        total = c.off;
    }
};

}  // namespace vit
}  // namespace stgcn
