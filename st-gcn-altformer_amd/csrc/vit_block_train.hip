// C entry points for training the AltFormer heads' transformer block (include/stgcn_hip.h, "ViT block: training"):
// the three backward pieces on their own (linear, attention, LayerNorm), the training forward of one Block, which is the
// eval forward's five launches writing what the backward reads into the caller's `saved` buffer, and the backward.
//
// Backward of one slab of whole sequences (M tokens), in this order, every temporary in the caller's workspace:
//   dhid = (s2 dy) W2 * GELU'(h_pre)            dW2, db2   = (s2 dy)^T hid
//   dn   = dhid W1                              LN2 backward: dx1 = dy + ...,  a = LN2(x1),  dnorm2
//                                               dW1, db1   = dhid^T a
//   datt = (s1 dx1) Wproj                       dWproj, dbproj = (s1 dx1)^T att
//   dqkv = attention backward(qkv, att, datt)     resident up to 256 tokens (fp32, or on bf16 operands with
//                                               STGCN_VIT_TRAIN_ATTN_BF16), streaming above
//   dn   = dqkv Wqkv                            LN1 backward: dx = dx1 + ...,  a = LN1(x),   dnorm1
//                                               dWqkv, dbqkv = dqkv^T a
// The dgrads are the forward linear kernel on weights transposed once per call; the weight gradients run on the fp32
// matrix cores, or on bf16 operands with STGCN_VIT_TRAIN_BF16.  Which arithmetic each product takes and which attention form
// runs is vit.h's plan_block; LayerNorm, the soft-max, bias, GELU / GELU', row factors, residuals, bias gradients and every
// stored tensor are fp32 in every mode (the attention's products too, unless STGCN_VIT_TRAIN_ATTN_BF16 moves the resident
// form to bf16 operands), so `saved` and the workspace have one layout.  Parameter gradients of the second and
// later slabs are added onto the first slab's in slab order, so the result does not depend on anything but the shapes.
//
// Two pairs of entry points run the one forward_train and the one backward below: stgcn_vit_block_forward_train /
// stgcn_vit_block_backward, and the _drop pair of the ST-ViT layers, which adds three per-element dropout masks (BlockDrop:
// behind the projection, behind the GELU, behind fc2) and takes a tile field for its forward and dgrad linears.  A mask is
// one more factor in the epilogue of the linear that makes the masked tensor (LinearExtra::mask, fp32, after GELU / GELU',
// before the row factor, the residual and any later bf16 rounding); the two masked gradients that a dgrad AND a wgrad read,
// g2 = m_fc2 * dy and g1 = m_proj * dx1, are each made once by launch_mask_mul into a slab that is free then (datt during the
// MLP branch, dn between LN2's parameter gradient and the qkv dgrad).  Every mask pointer is advanced per slab by the
// slab's first row, as x and dy are.
#include "vit.h"

namespace stgcn {
namespace vit {
namespace {

size_t max2(size_t a, size_t b) { return a > b ? a : b; }

// The slab space of one weight gradient.  `small` (the plan's wgrad_small): what plan_wgrad's cut needs and never less than the
// default cut's, so that a workspace sized for a flagged call also serves the same call without the flag.
size_t wgrad_part(int M, int K, int Nout, bool small) {
    const size_t p = plan_wgrad(M, K, Nout, false).part_floats(K, Nout);
    return small ? max2(p, plan_wgrad(M, K, Nout, true).part_floats(K, Nout)) : p;
}

// the backward's temporaries: one slab of gradients, the four transposed weights, the partial sums of one reduction
struct BackwardWs {
    float *dhid, *dn, *dx1, *datt, *dqkv, *a, *stats, *wt_qkv, *wt_proj, *wt_fc1, *wt_fc2, *part, *tmp;
    size_t total;
    // `small`: the plan's wgrad_small, which sizes `part` for plan_wgrad's cut (never less than the default cut's)
    BackwardWs(void *base, int B, int L, int D, int hidden, bool small = false) {
        const int M = slab_seqs(B, L) * L;
        const size_t rows = (size_t)M;
        Carve c(base);
        dhid = c.take<float>(rows * hidden);
        dn = c.take<float>(rows * D);
        dx1 = c.take<float>(rows * D);
        datt = c.take<float>(rows * D);
        dqkv = c.take<float>(rows * 3 * D);
        a = c.take<float>(rows * D);
        stats = c.take<float>(rows * 2);
        wt_qkv = c.take<float>((size_t)3 * D * D);
        wt_proj = c.take<float>((size_t)D * D);
        wt_fc1 = c.take<float>((size_t)D * hidden);
        wt_fc2 = c.take<float>((size_t)D * hidden);
        // (a shorter last slab needs no more under the small rule: its split count does not fall as the rows grow)
        size_t p = wgrad_part(M, D, 3 * D, small);
        p = max2(p, wgrad_part(M, D, D, small));
        p = max2(p, wgrad_part(M, D, hidden, small));
        p = max2(p, wgrad_part(M, hidden, D, small));
        p = max2(p, (size_t)ln_param_splits(M) * 2 * D);
        part = c.take<float>(p);
        tmp = c.take<float>(max2((size_t)3 * D * D, (size_t)D * hidden) + max2((size_t)3 * D, (size_t)hidden));
        total = c.off;
    }
};

// the whole workspace of stgcn_vit_block_backward: the streaming attention backward's statistics of one slab behind BackwardWs
struct TrainWs {
    BackwardWs w;
    float *att_stats = nullptr;
    size_t total;
    TrainWs(void *base, const BlockPlan &plan, int B, int L, int D, int heads, int hidden) : w(base, B, L, D, hidden, plan.wgrad_small) {
        Carve c(base);
        c.off = w.total;
        if (plan.attention == BlockAttention::stream) att_stats = c.take<float>(attention_stats_floats(slab_seqs(B, L), L, heads));
        total = c.off;
    }
};

struct LinearBwdWs {
    float *wt, *part, *tmp;
    int nout_pad;
    size_t total;
    LinearBwdWs(void *base, int M, int K, int Nout, bool small = false) {
        nout_pad = ceil_div(Nout, 32) * 32;
        Carve c(base);
        wt = c.take<float>((size_t)K * nout_pad);
        part = c.take<float>(wgrad_part(M, K, Nout, small));
        tmp = c.take<float>((size_t)Nout * K + Nout);
        total = c.off;
    }
};

struct LnBwdWs {
    float *stats, *part, *tmp;
    size_t total;
    LnBwdWs(void *base, int M, int D) {
        Carve c(base);
        stats = c.take<float>((size_t)M * 2);
        part = c.take<float>((size_t)ln_param_splits(M) * 2 * D);
        tmp = c.take<float>((size_t)D);
        total = c.off;
    }
};

// the weight gradient in the arithmetic, form and cut of the plan
int wgrad(const BlockPlan &plan, const float *dY, const float *A, const float *rowscale, int L, float *dW, float *db, float *part,
          float *tmp, int M, int K, int Nout, bool accumulate, hipStream_t st) {
    const WgradPlan wp = plan_wgrad(plan, M, K, Nout);
    return plan.wgrad_bf16 ? launch_wgrad_bf16(wp, dY, A, rowscale, L, dW, db, part, tmp, M, K, Nout, accumulate, st)
                           : launch_wgrad(wp, dY, A, rowscale, L, dW, db, part, tmp, M, K, Nout, accumulate, st);
}

bool linear_bwd_ok(int M, int K, int Nout) { return M >= 1 && K >= 1 && Nout >= 1 && K % 32 == 0 && Nout % 4 == 0; }

// the twelve parameter gradients of a block (bqkv may be NULL: qkv_bias=False)
struct BlockGrads {
    float *norm1_weight, *norm1_bias, *Wqkv, *bqkv, *Wproj, *bproj, *norm2_weight, *norm2_bias, *W1, *b1, *W2, *b2;
    bool present() const {
        return norm1_weight && norm1_bias && Wqkv && Wproj && bproj && norm2_weight && norm2_bias && W1 && b1 && W2 && b2;
    }
};

BlockWeights block_weights(const stgcn_vit_block_weights &b) {
    return BlockWeights{b.norm1_weight, b.norm1_bias, b.Wqkv, b.bqkv, b.Wproj, b.bproj, b.norm2_weight, b.norm2_bias, b.W1, b.b1, b.W2, b.b2};
}

BlockDrop block_drop(const stgcn_vit_drop_masks *m) {
    BlockDrop d;
    if (m != nullptr) d.proj = m->m_proj, d.act = m->m_act, d.fc2 = m->m_fc2;
    return d;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The training forward of both pairs: `entry` is forward_train (no masks, no tile field) or forward_train_drop.
int forward_train(BlockEntry entry, const float *x, const BlockWeights &w, const float *scale1, const float *scale2,
                  const BlockDrop &drop, float eps, float scale, void *saved, size_t saved_bytes, float *y, int B, int L, int D,
                  int heads, int hidden, unsigned flags, void *stream) {
    const BlockPlan plan = plan_block(entry, L, D, heads, hidden, flags);
    const char *name = kBlockEntryName[(int)entry];
    if (plan.refusal) return block_refused(plan);
    if (!x || !w.present() || !y || !saved) return fail(STGCN_ERR_ARG, "%s: null pointer", name);
    if (B < 1) return fail(STGCN_ERR_ARG, "%s: B = %d", name, B);
    if (y == x) return fail(STGCN_ERR_ARG, "%s: y must not alias x", name);
    if (!plan.covered) return block_unsupported(plan, L, D, heads, hidden, flags);
    const BlockStore sv(saved, plan, B, L, D, hidden);
    if (saved_bytes < sv.total) return fail(STGCN_ERR_WORKSPACE, "%s: saved buffer %zu < %zu bytes", name, saved_bytes, sv.total);
    return block_forward(plan, x, w, sv, scale1, scale2, eps, scale, y, B, L, D, heads, hidden, static_cast<hipStream_t>(stream), drop);
}

// The backward of both pairs (the order of the header comment).  With masks, per slab: g2 = m_fc2 * dy is made once into the
// datt slab, which nothing holds during the MLP branch, and read by the fc2 dgrad and wgrad; m_act rides in that dgrad's
// epilogue, behind GELU'; LN2's residual gradient stays the unmasked dy; g1 = m_proj * dx1 is made once into the dn slab,
// which is free between LN2's parameter gradient and the qkv dgrad, and read by the proj dgrad and wgrad, while dx1 itself
// stays LN1's residual gradient.  A mask that is NULL costs no launch and no read.
int backward(BlockEntry entry, const float *x, const BlockWeights &wt, const float *scale1, const float *scale2, const BlockDrop &drop,
             const void *saved, size_t saved_bytes, const float *dy, float *dx, const BlockGrads &g, float eps, float scale, void *ws,
             size_t ws_bytes, int B, int L, int D, int heads, int hidden, unsigned flags, void *stream) {
    const BlockPlan plan = plan_block(entry, L, D, heads, hidden, flags);
    const char *name = kBlockEntryName[(int)entry];
    if (plan.refusal) return block_refused(plan);
    if (!x || !wt.present() || !saved || !dy || !dx || !g.present() || !ws) return fail(STGCN_ERR_ARG, "%s: null pointer", name);
    if (B < 1) return fail(STGCN_ERR_ARG, "%s: B = %d", name, B);
    if (dx == dy || dx == x) return fail(STGCN_ERR_ARG, "%s: dx must not alias dy or x", name);
    if ((drop.fc2 != nullptr || drop.proj != nullptr) && !(aligned16(drop.fc2) && aligned16(drop.proj) && aligned16(dy) && aligned16(ws)))
        return fail(STGCN_ERR_ARG, "%s: with m_proj or m_fc2, both masks, dy and ws must be 16-byte aligned", name);
    if (!plan.covered) return block_unsupported(plan, L, D, heads, hidden, flags);
    const BlockStore sv(const_cast<void *>(saved), plan, B, L, D, hidden);
    if (saved_bytes < sv.total) return fail(STGCN_ERR_WORKSPACE, "%s: saved buffer %zu < %zu bytes", name, saved_bytes, sv.total);
    const TrainWs tw(ws, plan, B, L, D, heads, hidden);
    if (ws_bytes < tw.total) return fail(STGCN_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", name, ws_bytes, tw.total);
    const BackwardWs &w = tw.w;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned math = plan.lin_dgrad | plan.tile, math_qkv = plan.qkv_dgrad | plan.tile;
    int rc;
    if ((rc = launch_transpose_pad(wt.Wqkv, w.wt_qkv, 3 * D, D, 3 * D, st))) return rc;
    if ((rc = launch_transpose_pad(wt.Wproj, w.wt_proj, D, D, D, st))) return rc;
    if ((rc = launch_transpose_pad(wt.W1, w.wt_fc1, hidden, D, hidden, st))) return rc;
    if ((rc = launch_transpose_pad(wt.W2, w.wt_fc2, D, hidden, D, st))) return rc;
    const int per = slab_seqs(B, L);
    for (int b0 = 0; b0 < B; b0 += per) {
        const int nb = B - b0 < per ? B - b0 : per;
        const int M = nb * L;
        const size_t r0 = (size_t)b0 * L;
        const bool acc = b0 > 0;
        const float *xs = x + r0 * D, *dys = dy + r0 * D;
        const float *qkv = (const float *)sv.qkv + r0 * 3 * D, *att = (const float *)sv.att + r0 * D, *x1 = sv.x1 + r0 * D;
        const float *hpre = sv.hpre + r0 * hidden, *hid = (const float *)sv.hid + r0 * hidden;
        const float *s1 = scale1 != nullptr ? scale1 + b0 : nullptr, *s2 = scale2 != nullptr ? scale2 + b0 : nullptr;
        // the masks cover the whole batch, as x and dy do: this slab's first row is r0
        const float *mproj = drop.proj != nullptr ? drop.proj + r0 * D : nullptr, *mfc2 = drop.fc2 != nullptr ? drop.fc2 + r0 * D : nullptr;
        LinearExtra e2, e1;
        e2.dgelu = hpre;
        e2.mask = drop.act != nullptr ? drop.act + r0 * hidden : nullptr;
        e2.rowscale = s2;
        e1.rowscale = s1;
        e1.L = e2.L = L;
        // MLP branch
        const float *g2 = dys;
        if (mfc2 != nullptr) {
            if ((rc = launch_mask_mul(dys, mfc2, w.datt, (size_t)M * D, st))) return rc;
            g2 = w.datt;
        }
        if ((rc = launch_linear(g2, w.wt_fc2, nullptr, nullptr, nullptr, nullptr, 0.f, w.dhid, M, D, hidden, false, math, st, e2)))
            return rc;
        if ((rc = wgrad(plan, g2, hid, s2, L, g.W2, g.b2, w.part, w.tmp, M, hidden, D, acc, st))) return rc;
        if ((rc = launch_linear(w.dhid, w.wt_fc1, nullptr, nullptr, nullptr, nullptr, 0.f, w.dn, M, hidden, D, false, math, st)))
            return rc;
        if ((rc = launch_ln_backward(x1, w.dn, wt.norm2_weight, wt.norm2_bias, eps, dys, w.dx1, w.a, w.stats, M, D, st))) return rc;
        if ((rc = launch_ln_param_grad(x1, w.dn, w.stats, g.norm2_weight, g.norm2_bias, w.part, w.tmp, M, D, acc, st))) return rc;
        if ((rc = wgrad(plan, w.dhid, w.a, nullptr, L, g.W1, g.b1, w.part, w.tmp, M, D, hidden, acc, st))) return rc;
        // attention branch
        const float *g1 = w.dx1;
        if (mproj != nullptr) {
            if ((rc = launch_mask_mul(w.dx1, mproj, w.dn, (size_t)M * D, st))) return rc;
            g1 = w.dn;
        }
        if ((rc = launch_linear(g1, w.wt_proj, nullptr, nullptr, nullptr, nullptr, 0.f, w.datt, M, D, D, false, math, st, e1)))
            return rc;
        if ((rc = wgrad(plan, g1, att, s1, L, g.Wproj, g.bproj, w.part, w.tmp, M, D, D, acc, st))) return rc;
        switch (plan.attention) {
            case BlockAttention::stream:
                rc = launch_attention_backward_stream(qkv, att, w.datt, w.dqkv, tw.att_stats, nb, L, heads, D / heads, scale, st);
                break;
            case BlockAttention::resident_train_bf16:
                rc = launch_attention_backward_bf16(qkv, att, w.datt, w.dqkv, nb, L, heads, D / heads, scale, st);
                break;
            default: rc = launch_attention_backward(qkv, att, w.datt, w.dqkv, nb, L, heads, D / heads, scale, st); break;
        }
        if (rc) return rc;
        if ((rc = launch_linear(w.dqkv, w.wt_qkv, nullptr, nullptr, nullptr, nullptr, 0.f, w.dn, M, 3 * D, D, false, math_qkv, st)))
            return rc;
        if ((rc = launch_ln_backward(xs, w.dn, wt.norm1_weight, wt.norm1_bias, eps, w.dx1, dx + r0 * D, w.a, w.stats, M, D, st))) return rc;
        if ((rc = launch_ln_param_grad(xs, w.dn, w.stats, g.norm1_weight, g.norm1_bias, w.part, w.tmp, M, D, acc, st))) return rc;
        if ((rc = wgrad(plan, w.dqkv, w.a, nullptr, L, g.Wqkv, g.bqkv, w.part, w.tmp, M, D, 3 * D, acc, st))) return rc;
    }
    return STGCN_OK;
}

}  // namespace
}  // namespace vit
}  // namespace stgcn

using namespace stgcn;
using namespace stgcn::vit;

extern "C" {

int stgcn_vit_linear_backward_supported(int M, int K, int Nout, unsigned flags) {
    return linear_bwd_ok(M, K, Nout) && math_ok(flags) ? 1 : 0;
}

int stgcn_vit_linear_backward_bf16_supported(int M, int K, int Nout) { return linear_bwd_ok(M, K, Nout) ? 1 : 0; }

size_t stgcn_vit_linear_backward_ws_bytes(int M, int K, int Nout) {
    if (!linear_bwd_ok(M, K, Nout)) return 0;
    return LinearBwdWs(nullptr, M, K, Nout).total;
}

size_t stgcn_vit_linear_backward_small_ws_bytes(int M, int K, int Nout, unsigned flags) {
    if (!linear_bwd_ok(M, K, Nout)) return 0;
    return LinearBwdWs(nullptr, M, K, Nout, (flags & STGCN_VIT_WGRAD_SMALL) != 0).total;
}

// The three queries of plan_wgrad: `flags`: only STGCN_VIT_WGRAD_SMALL is read.  0 for an empty shape.
int stgcn_vit_wgrad_tile(int M, int K, int Nout, unsigned flags) {
    return M >= 1 && K >= 1 && Nout >= 1 ? plan_wgrad(M, K, Nout, (flags & STGCN_VIT_WGRAD_SMALL) != 0).tile : 0;
}

int stgcn_vit_wgrad_splits(int M, int K, int Nout, unsigned flags) {
    return M >= 1 && K >= 1 && Nout >= 1 ? plan_wgrad(M, K, Nout, (flags & STGCN_VIT_WGRAD_SMALL) != 0).splits : 0;
}

int stgcn_vit_wgrad_writes_direct(int M, int K, int Nout, unsigned flags) {
    return M >= 1 && K >= 1 && Nout >= 1 && plan_wgrad(M, K, Nout, (flags & STGCN_VIT_WGRAD_SMALL) != 0).direct(false) ? 1 : 0;
}

int stgcn_vit_linear_backward(const float *dy, const float *a, const float *W, const float *h_pre, float *dx, float *dW,
                              float *db, void *ws, size_t ws_bytes, int M, int K, int Nout, unsigned flags, void *stream) {
    const BlockPlan plan = plan_block(BlockEntry::linear_backward, 0, 0, 0, 0, flags);   // the flags' part of it: no block shape here
    if (plan.refusal) return block_refused(plan);
    if (!dy || !ws || M < 1 || K < 1 || Nout < 1) return fail(STGCN_ERR_ARG, "stgcn_vit_linear_backward: null pointer or empty shape");
    if ((dx != nullptr && !W) || (dW != nullptr && !a) || (db != nullptr && !dW))
        return fail(STGCN_ERR_ARG, "stgcn_vit_linear_backward: dx needs W, dW needs a, db goes with dW");
    if (((flags & STGCN_VIT_DGELU) != 0) != (h_pre != nullptr))
        return fail(STGCN_ERR_ARG, "stgcn_vit_linear_backward: h_pre and STGCN_VIT_DGELU go together");
    if (dx == dy) return fail(STGCN_ERR_ARG, "stgcn_vit_linear_backward: dx must not alias dy");
    if (!linear_bwd_ok(M, K, Nout) || !plan.covered)
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_linear_backward: K = %d, Nout = %d, math %u (covered: K %% 32 == 0, Nout %% 4 == 0, "
                    "f32 / bf16x3)", K, Nout, flags & STGCN_MATH_MASK);
    const LinearBwdWs w(ws, M, K, Nout, plan.wgrad_small);
    if (ws_bytes < w.total) return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_linear_backward: workspace %zu < %zu bytes", ws_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    if (dx != nullptr) {
        if ((rc = launch_transpose_pad(W, w.wt, Nout, K, w.nout_pad, st))) return rc;
        LinearExtra ex;
        ex.dgelu = h_pre;
        ex.kx = Nout;
        const float *R = (flags & STGCN_VIT_ACCUMULATE) ? dx : nullptr;
        if ((rc = launch_linear(dy, w.wt, nullptr, R, nullptr, nullptr, 0.f, dx, M, w.nout_pad, K, false, plan.lin_dgrad, st, ex)))
            return rc;
    }
    if (dW != nullptr && (rc = wgrad(plan, dy, a, nullptr, 1, dW, db, w.part, w.tmp, M, K, Nout, false, st))) return rc;
    return STGCN_OK;
}

int stgcn_vit_attention_backward_supported(int L, int heads, int head_dim) {
    return attention_resident_ok(L, heads, head_dim) ? 1 : 0;
}

int stgcn_vit_attention_backward(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L, int heads,
                                 int head_dim, float scale, void *stream) {
    if (!qkv || !out || !dout || !dqkv || B < 1 || L < 1 || heads < 1)
        return fail(STGCN_ERR_ARG, "stgcn_vit_attention_backward: null pointer or empty shape");
    if (!stgcn_vit_attention_backward_supported(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_backward: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)",
                    L, head_dim, kMaxL);
    return launch_attention_backward(qkv, out, dout, dqkv, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

int stgcn_vit_attention_backward_stream_supported(int L, int heads, int head_dim) {
    return attention_stream_ok(L, heads, head_dim) ? 1 : 0;
}

size_t stgcn_vit_attention_backward_stream_ws_bytes(int B, int L, int heads) {
    if (B < 1 || heads < 1 || L < 1 || L > kMaxStreamL) return 0;
    Carve c(nullptr);
    c.take<float>(attention_stats_floats(B, L, heads));
    return c.off;
}

int stgcn_vit_attention_backward_stream(const float *qkv, const float *out, const float *dout, float *dqkv, void *ws,
                                        size_t ws_bytes, int B, int L, int heads, int head_dim, float scale, void *stream) {
    if (!qkv || !out || !dout || !dqkv || !ws || B < 1 || L < 1 || heads < 1)
        return fail(STGCN_ERR_ARG, "stgcn_vit_attention_backward_stream: null pointer or empty shape");
    if (!attention_stream_ok(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_backward_stream: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)",
                    L, head_dim, kMaxStreamL);
    const size_t need = stgcn_vit_attention_backward_stream_ws_bytes(B, L, heads);
    if (ws_bytes < need) return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_attention_backward_stream: workspace %zu < %zu bytes", ws_bytes, need);
    return launch_attention_backward_stream(qkv, out, dout, dqkv, static_cast<float *>(ws), B, L, heads, head_dim, scale,
                                            static_cast<hipStream_t>(stream));
}

int stgcn_vit_attention_train_bf16_supported(int L, int heads, int head_dim) {
    return attention_resident_ok(L, heads, head_dim) ? 1 : 0;
}

int stgcn_vit_attention_train_bf16(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale, void *stream) {
    REQUIRE_PTR(qkv); REQUIRE_PTR(out);
    REQUIRE_POS(B); REQUIRE_POS(L); REQUIRE_POS(heads);
    if (!stgcn_vit_attention_train_bf16_supported(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_train_bf16: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)",
                    L, head_dim, kMaxL);
    return launch_attention_train_bf16(qkv, out, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

int stgcn_vit_attention_backward_bf16(const float *qkv, const float *out, const float *dout, float *dqkv, int B, int L, int heads,
                                      int head_dim, float scale, void *stream) {
    REQUIRE_PTR(qkv); REQUIRE_PTR(out); REQUIRE_PTR(dout); REQUIRE_PTR(dqkv);
    REQUIRE_POS(B); REQUIRE_POS(L); REQUIRE_POS(heads);
    if (!stgcn_vit_attention_train_bf16_supported(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_backward_bf16: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)",
                    L, head_dim, kMaxL);
    return launch_attention_backward_bf16(qkv, out, dout, dqkv, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

size_t stgcn_vit_layernorm_backward_ws_bytes(int M, int D) {
    if (M < 1 || D < 1 || D % 4 != 0) return 0;
    return LnBwdWs(nullptr, M, D).total;
}

int stgcn_vit_layernorm_backward(const float *x, const float *dn, const float *weight, float eps, const float *dres, float *dx,
                                 float *dweight, float *dbias, void *ws, size_t ws_bytes, int M, int D, void *stream) {
    if (!x || !dn || !weight || !dx || !dweight || !dbias || !ws || M < 1 || D < 1)
        return fail(STGCN_ERR_ARG, "stgcn_vit_layernorm_backward: null pointer or empty shape");
    if (D % 4 != 0) return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_layernorm_backward: D = %d (covered: D %% 4 == 0)", D);
    const LnBwdWs w(ws, M, D);
    if (ws_bytes < w.total) return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_layernorm_backward: workspace %zu < %zu bytes", ws_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    if ((rc = launch_ln_backward(x, dn, weight, nullptr, eps, dres, dx, nullptr, w.stats, M, D, st))) return rc;
    return launch_ln_param_grad(x, dn, w.stats, dweight, dbias, w.part, w.tmp, M, D, false, st);
}

// The size queries without `heads` ask the plan with none: they read what L, D and hidden alone decide.  The _long queries
// answer what the older, resident-only ones answer at L <= 256, and go on where those answer 0.
int stgcn_vit_block_train_supported(int L, int D, int heads, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::forward_train, L, D, heads, hidden, 0);
    return p.covered && p.resident ? 1 : 0;
}

size_t stgcn_vit_block_saved_bytes(int B, int L, int D, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::forward_train, L, D, 0, hidden, 0);
    return B >= 1 && p.sized && p.resident ? BlockStore(nullptr, p, B, L, D, hidden).total : 0;
}

size_t stgcn_vit_block_backward_ws_bytes(int B, int L, int D, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::backward, L, D, 0, hidden, 0);
    return B >= 1 && p.sized && p.resident ? BackwardWs(nullptr, B, L, D, hidden).total : 0;
}

int stgcn_vit_block_train_long_supported(int L, int D, int heads, int hidden) {
    return plan_block(BlockEntry::forward_train, L, D, heads, hidden, 0).covered ? 1 : 0;
}

int stgcn_vit_block_train_bf16_supported(int L, int D, int heads, int hidden) {
    return plan_block(BlockEntry::forward_train, L, D, heads, hidden, STGCN_VIT_TRAIN_BF16).covered ? 1 : 0;
}

int stgcn_vit_block_train_attn_bf16_supported(int L, int D, int heads, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::forward_train, L, D, heads, hidden, STGCN_VIT_TRAIN_ATTN_BF16);
    return p.covered && p.attention == BlockAttention::resident_train_bf16 ? 1 : 0;
}

size_t stgcn_vit_block_train_long_saved_bytes(int B, int L, int D, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::forward_train, L, D, 0, hidden, 0);
    return B >= 1 && p.sized ? BlockStore(nullptr, p, B, L, D, hidden).total : 0;
}

size_t stgcn_vit_block_train_long_ws_bytes(int B, int L, int D, int heads, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::backward, L, D, heads, hidden, 0);
    return B >= 1 && p.covered ? TrainWs(nullptr, p, B, L, D, heads, hidden).total : 0;
}

int stgcn_vit_block_forward_train(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv,
                                  const float *bqkv, const float *Wproj, const float *bproj, const float *norm2_weight,
                                  const float *norm2_bias, const float *W1, const float *b1, const float *W2, const float *b2,
                                  const float *scale1, const float *scale2, float eps, float scale, void *saved,
                                  size_t saved_bytes, float *y, int B, int L, int D, int heads, int hidden, unsigned flags,
                                  void *stream) {
    const BlockWeights w{norm1_weight, norm1_bias, Wqkv, bqkv, Wproj, bproj, norm2_weight, norm2_bias, W1, b1, W2, b2};
    return forward_train(BlockEntry::forward_train, x, w, scale1, scale2, BlockDrop{}, eps, scale, saved, saved_bytes, y, B, L, D,
                         heads, hidden, flags, stream);
}

int stgcn_vit_block_backward(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv,
                             const float *Wproj, const float *norm2_weight, const float *norm2_bias, const float *W1,
                             const float *W2, const float *scale1, const float *scale2, const void *saved, size_t saved_bytes,
                             const float *dy, float *dx, float *dnorm1_weight, float *dnorm1_bias, float *dWqkv, float *dbqkv,
                             float *dWproj, float *dbproj, float *dnorm2_weight, float *dnorm2_bias, float *dW1, float *db1,
                             float *dW2, float *db2, float eps, float scale, void *ws, size_t ws_bytes, int B, int L, int D,
                             int heads, int hidden, unsigned flags, void *stream) {
    const BlockWeights w{norm1_weight, norm1_bias, Wqkv, nullptr, Wproj, nullptr, norm2_weight, norm2_bias, W1, nullptr, W2, nullptr};
    const BlockGrads g{dnorm1_weight, dnorm1_bias, dWqkv, dbqkv, dWproj, dbproj, dnorm2_weight, dnorm2_bias, dW1, db1, dW2, db2};
    return backward(BlockEntry::backward, x, w, scale1, scale2, BlockDrop{}, saved, saved_bytes, dy, dx, g, eps, scale, ws, ws_bytes,
                    B, L, D, heads, hidden, flags, stream);
}

// ---- the pair with per-element dropout (include/stgcn_hip.h, "ViT block: training with dropout") ---------------------------
// The same forward_train and backward as above under the two _drop entries of the plan, which differ in one thing: a
// STGCN_VIT_TILE_* field is legal and reaches every forward and dgrad linear.  The masks ride in the linears' epilogues
// (LinearExtra::mask) and, in the backward, in two launch_mask_mul passes; with no mask and no tile field nothing else runs
// than what the older pair runs.
int stgcn_vit_block_train_drop_supported(int L, int D, int heads, int hidden) {
    return plan_block(BlockEntry::forward_train_drop, L, D, heads, hidden, 0).covered ? 1 : 0;
}

size_t stgcn_vit_block_train_drop_ws_bytes(int B, int L, int D, int heads, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::backward_drop, L, D, heads, hidden, 0);
    return B >= 1 && p.covered ? TrainWs(nullptr, p, B, L, D, heads, hidden).total : 0;
}

size_t stgcn_vit_block_train_small_ws_bytes(int B, int L, int D, int heads, int hidden, unsigned flags) {
    const BlockPlan p = plan_block(BlockEntry::backward_drop, L, D, heads, hidden, flags & STGCN_VIT_WGRAD_SMALL);
    return B >= 1 && p.covered ? TrainWs(nullptr, p, B, L, D, heads, hidden).total : 0;
}

int stgcn_vit_block_forward_train_drop(const float *x, const stgcn_vit_block_weights *weights, const float *scale1,
                                       const float *scale2, const stgcn_vit_drop_masks *masks, float eps, float scale,
                                       void *saved, size_t saved_bytes, float *y, int B, int L, int D, int heads, int hidden,
                                       unsigned flags, void *stream) {
    const BlockWeights w = weights != nullptr ? block_weights(*weights) : BlockWeights{};
    return forward_train(BlockEntry::forward_train_drop, x, w, scale1, scale2, block_drop(masks), eps, scale, saved, saved_bytes, y,
                         B, L, D, heads, hidden, flags, stream);
}

int stgcn_vit_block_backward_drop(const float *x, const stgcn_vit_block_weights *weights, const float *scale1,
                                  const float *scale2, const stgcn_vit_drop_masks *masks, const void *saved, size_t saved_bytes,
                                  const float *dy, float *dx, const stgcn_vit_block_grads *grads, float eps, float scale, void *ws,
                                  size_t ws_bytes, int B, int L, int D, int heads, int hidden, unsigned flags, void *stream) {
    const BlockWeights w = weights != nullptr ? block_weights(*weights) : BlockWeights{};
    const BlockGrads g = grads != nullptr ? BlockGrads{grads->norm1_weight, grads->norm1_bias, grads->Wqkv, grads->bqkv, grads->Wproj,
                                                       grads->bproj, grads->norm2_weight, grads->norm2_bias, grads->W1, grads->b1,
                                                       grads->W2, grads->b2}
                                          : BlockGrads{};
    return backward(BlockEntry::backward_drop, x, w, scale1, scale2, block_drop(masks), saved, saved_bytes, dy, dx, g, eps, scale, ws,
                    ws_bytes, B, L, D, heads, hidden, flags, stream);
}

}  // extern "C"
