// C entry points of the AltFormer heads' transformer block (include/stgcn_hip.h, "ViT block"): the linear and the attention
// (resident, split and streaming form, and their bf16 forms) on their own, and the eval forward of one Block.  What a block call runs -
// attention form, arithmetic per linear, bf16 or fp32 intermediates, tile field - is vit.h's plan_block; block_forward below
// is the one loop that runs it, for the eval forward here (intermediates in a per-slab workspace) and for the training
// forward in vit_block_train.hip (intermediates kept for the backward).
#include "vit.h"

namespace stgcn {
namespace vit {

int block_forward(const BlockPlan &plan, const float *x, const BlockWeights &w, const BlockStore &store, const float *scale1,
                  const float *scale2, float eps, float scale, float *y, int B, int L, int D, int heads, int hidden, hipStream_t st,
                  const BlockDrop &drop) {
    const size_t es = plan.bf16_store ? 2 : 4;   // bytes per element of qkv, att and hid
    const unsigned tile = plan.tile, xb = plan.bf16_store ? STGCN_VIT_X_BF16 : 0, yb = plan.bf16_store ? STGCN_VIT_Y_BF16 : 0;
    const int per = slab_seqs(B, L), hd = D / heads;
    for (int b0 = 0; b0 < B; b0 += per) {
        const int nb = B - b0 < per ? B - b0 : per;
        const int M = nb * L;
        const size_t r0 = (size_t)b0 * L, s0 = store.per_slab ? 0 : r0;   // first row of the slab in x / y, and in the store
        const float *xs = x + r0 * D;
        char *qkv = (char *)store.qkv + s0 * 3 * D * es, *att = (char *)store.att + s0 * D * es, *hid = (char *)store.hid + s0 * hidden * es;
        float *x1 = store.x1 + s0 * D;
        LinearExtra e1, eh, e2;
        e1.rowscale = scale1 != nullptr ? scale1 + b0 : nullptr;
        e2.rowscale = scale2 != nullptr ? scale2 + b0 : nullptr;
        e1.L = e2.L = L;
        eh.pre = store.hpre != nullptr ? store.hpre + s0 * hidden : nullptr;
        e1.mask = drop.proj != nullptr ? drop.proj + r0 * D : nullptr;        // the masks cover the whole batch: first row r0
        eh.mask = drop.act != nullptr ? drop.act + r0 * hidden : nullptr;
        e2.mask = drop.fc2 != nullptr ? drop.fc2 + r0 * D : nullptr;
        int rc;
        if ((rc = launch_linear(xs, w.Wqkv, w.bqkv, nullptr, w.norm1_weight, w.norm1_bias, eps, qkv, M, D, 3 * D, false,
                                plan.qkv_fwd | tile | yb, st)))
            return rc;
        switch (block_attention(plan, nb, heads)) {
            case BlockAttention::resident: rc = launch_attention_packed((float *)qkv, (float *)att, nb, L, heads, hd, scale, st); break;
            case BlockAttention::resident_split: rc = launch_attention_split((float *)qkv, (float *)att, nb, L, heads, hd, scale, st); break;
            case BlockAttention::stream: rc = launch_attention_stream((float *)qkv, (float *)att, nb, L, heads, hd, scale, st); break;
            case BlockAttention::resident_bf16: rc = launch_attention_bf16(qkv, att, nb, L, heads, hd, scale, st); break;
            case BlockAttention::resident_train_bf16:
                rc = launch_attention_train_bf16((float *)qkv, (float *)att, nb, L, heads, hd, scale, st);
                break;
            case BlockAttention::none: rc = fail(STGCN_ERR_UNSUPPORTED, "vit block: no attention form planned"); break;
        }
        if (rc) return rc;
        if ((rc = launch_linear(att, w.Wproj, w.bproj, xs, nullptr, nullptr, 0.f, x1, M, D, D, false, plan.lin_fwd | tile | xb, st, e1)))
            return rc;
        if ((rc = launch_linear(x1, w.W1, w.b1, nullptr, w.norm2_weight, w.norm2_bias, eps, hid, M, D, hidden, true,
                                plan.lin_fwd | tile | yb, st, eh)))
            return rc;
        if ((rc = launch_linear(hid, w.W2, w.b2, x1, nullptr, nullptr, 0.f, y + r0 * D, M, hidden, D, false, plan.lin_fwd | tile | xb,
                                st, e2)))
            return rc;
    }
    return STGCN_OK;
}

}  // namespace vit
}  // namespace stgcn

using namespace stgcn;
using namespace stgcn::vit;

extern "C" {

int stgcn_vit_linear_supported(int M, int K, int Nout, unsigned flags) {
    return M >= 1 && K >= 1 && math_ok(flags) && linear_ok(K, Nout, false) ? 1 : 0;
}

int stgcn_vit_linear_tile(int M, int K, int Nout, unsigned flags) {
    if (!stgcn_vit_linear_supported(M, K, Nout, flags)) return 0;
    const LinearTile t = linear_tile(M, K, Nout, flags);
    return (t.bm << 16) | t.bn;
}

int stgcn_vit_linear(const float *x, const float *W, const float *bias, const float *ln_weight, const float *ln_bias,
                     float ln_eps, const float *residual, float *y, int M, int K, int Nout, unsigned flags,
                     void *stream) {
    if (flags & STGCN_VIT_TRAIN_BF16)
        return fail(STGCN_ERR_ARG, "stgcn_vit_linear: STGCN_VIT_TRAIN_BF16 is a training mode (stgcn_vit_block_forward_train, "
                    "stgcn_vit_block_backward, stgcn_vit_linear_backward only)");
    if (flags & STGCN_VIT_TRAIN_ATTN_BF16)
        return fail(STGCN_ERR_ARG, "stgcn_vit_linear: STGCN_VIT_TRAIN_ATTN_BF16 is a training mode of the block "
                    "(stgcn_vit_block_forward_train, stgcn_vit_block_backward only)");
    if (flags & STGCN_VIT_ATTN_SPLIT)
        return fail(STGCN_ERR_ARG, "stgcn_vit_linear: STGCN_VIT_ATTN_SPLIT is an option of the block's attention "
                    "(stgcn_vit_block_forward only)");
    if (!x || !W || !y || M < 1 || K < 1 || Nout < 1) return fail(STGCN_ERR_ARG, "stgcn_vit_linear: null pointer or empty shape");
    if ((ln_weight == nullptr) != (ln_bias == nullptr)) return fail(STGCN_ERR_ARG, "stgcn_vit_linear: ln_weight and ln_bias go together");
    if (y == x) return fail(STGCN_ERR_ARG, "stgcn_vit_linear: y must not alias x");
    const bool ln = ln_weight != nullptr;
    if (!math_ok(flags) || !linear_ok(K, Nout, ln))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_linear: K = %d, Nout = %d, math %u (covered: K %% 32 == 0, f32 / bf16x3)", K,
                    Nout, flags & STGCN_MATH_MASK);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return launch_linear(x, W, bias, residual, ln_weight, ln_bias, ln_eps, y, M, K, Nout, (flags & STGCN_VIT_GELU) != 0,
                         flags & (STGCN_MATH_MASK | STGCN_VIT_TILE_MASK), st);
}

int stgcn_vit_attention_supported(int L, int heads, int head_dim) {
    return attention_resident_ok(L, heads, head_dim) ? 1 : 0;
}

int stgcn_vit_attention(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale, void *stream) {
    if (!qkv || !out || B < 1 || L < 1 || heads < 1) return fail(STGCN_ERR_ARG, "stgcn_vit_attention: null pointer or empty shape");
    if (!stgcn_vit_attention_supported(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)", L,
                    head_dim, kMaxL);
    return launch_attention_packed(qkv, out, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

int stgcn_vit_attention_stream_supported(int L, int heads, int head_dim) {
    return attention_stream_ok(L, heads, head_dim) ? 1 : 0;
}

int stgcn_vit_attention_stream(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale, void *stream) {
    REQUIRE_PTR(qkv); REQUIRE_PTR(out);
    REQUIRE_POS(B); REQUIRE_POS(L); REQUIRE_POS(heads);
    if (!attention_stream_ok(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_stream: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)",
                    L, head_dim, kMaxStreamL);
    return launch_attention_stream(qkv, out, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

int stgcn_vit_attention_split_supported(int L, int heads, int head_dim) {
    return attention_resident_ok(L, heads, head_dim) ? 1 : 0;
}

int stgcn_vit_attention_split(const float *qkv, float *out, int B, int L, int heads, int head_dim, float scale, void *stream) {
    if (!qkv || !out || B < 1 || L < 1 || heads < 1) return fail(STGCN_ERR_ARG, "stgcn_vit_attention_split: null pointer or empty shape");
    if (!stgcn_vit_attention_split_supported(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_split: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)", L,
                    head_dim, kMaxL);
    return launch_attention_split(qkv, out, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

int stgcn_vit_linear_bf16_supported(int M, int K, int Nout, unsigned flags) {
    (void)flags;   // storage bits, GELU and the tile field do not change the coverage (the query has no LayerNorm argument)
    return M >= 1 && K >= 1 && linear_ok(K, Nout, false) ? 1 : 0;
}

int stgcn_vit_linear_bf16(const void *x, const float *W, const float *bias, const float *ln_weight, const float *ln_bias,
                          float ln_eps, const float *residual, void *y, int M, int K, int Nout, unsigned flags, void *stream) {
    if (!x || !W || !y || M < 1 || K < 1 || Nout < 1) return fail(STGCN_ERR_ARG, "stgcn_vit_linear_bf16: null pointer or empty shape");
    if ((ln_weight == nullptr) != (ln_bias == nullptr))
        return fail(STGCN_ERR_ARG, "stgcn_vit_linear_bf16: ln_weight and ln_bias go together");
    if (y == x) return fail(STGCN_ERR_ARG, "stgcn_vit_linear_bf16: y must not alias x");
    const bool ln = ln_weight != nullptr;
    if (ln && (flags & STGCN_VIT_X_BF16)) return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_linear_bf16: LayerNorm needs fp32 x (STGCN_VIT_X_BF16 set)");
    if (!linear_ok(K, Nout, ln))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_linear_bf16: K = %d, Nout = %d (covered: K %% 32 == 0)", K, Nout);
    return launch_linear(x, W, bias, residual, ln_weight, ln_bias, ln_eps, y, M, K, Nout, (flags & STGCN_VIT_GELU) != 0,
                         STGCN_MATH_BF16 | (flags & (STGCN_VIT_TILE_MASK | STGCN_VIT_X_BF16 | STGCN_VIT_Y_BF16)),
                         static_cast<hipStream_t>(stream));
}

int stgcn_vit_attention_bf16_supported(int L, int heads, int head_dim) {
    return attention_resident_ok(L, heads, head_dim) ? 1 : 0;
}

int stgcn_vit_attention_bf16(const void *qkv, void *out, int B, int L, int heads, int head_dim, float scale, void *stream) {
    REQUIRE_PTR(qkv); REQUIRE_PTR(out);
    REQUIRE_POS(B); REQUIRE_POS(L); REQUIRE_POS(heads);
    if (!stgcn_vit_attention_bf16_supported(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_bf16: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)", L,
                    head_dim, kMaxL);
    return launch_attention_bf16(qkv, out, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

int stgcn_vit_block_forward_bf16_supported(int L, int D, int heads, int hidden) {
    return plan_block(BlockEntry::forward, L, D, heads, hidden, STGCN_VIT_BF16).covered ? 1 : 0;
}

int stgcn_vit_block_supported(int L, int D, int heads, int hidden) {
    const BlockPlan p = plan_block(BlockEntry::forward, L, D, heads, hidden, 0);
    return p.covered && p.resident ? 1 : 0;
}

int stgcn_vit_block_forward_supported(int L, int D, int heads, int hidden) {
    return plan_block(BlockEntry::forward, L, D, heads, hidden, 0).covered ? 1 : 0;
}

int stgcn_vit_block_attention_form(int B, int L, int D, int heads, int hidden, unsigned flags) {
    const BlockPlan plan = plan_block(BlockEntry::forward, L, D, heads, hidden, flags);
    if (B < 1 || plan.refusal || !plan.covered) return 0;
    switch (block_attention(plan, slab_seqs(B, L), heads)) {   // the call's first slab (all of it up to kSlabRows tokens)
        case BlockAttention::resident: return 1;
        case BlockAttention::stream: return 2;
        case BlockAttention::resident_bf16: return 3;
        case BlockAttention::resident_split: return 4;
        default: return 0;
    }
}

size_t stgcn_vit_block_ws_bytes(int B, int L, int D, int hidden) {
    if (B < 1 || L < 1 || D < 1 || hidden < 1) return 0;
    return BlockStore(nullptr, plan_block(BlockEntry::forward, L, D, 0, hidden, 0), B, L, D, hidden).total;   // the fp32 layout
}

int stgcn_vit_block_forward(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv,
                            const float *bqkv, const float *Wproj, const float *bproj, const float *norm2_weight,
                            const float *norm2_bias, const float *W1, const float *b1, const float *W2, const float *b2,
                            float eps, float scale, void *ws, size_t ws_bytes, float *y, int B, int L, int D, int heads,
                            int hidden, unsigned flags, void *stream) {
    const BlockPlan plan = plan_block(BlockEntry::forward, L, D, heads, hidden, flags);
    if (plan.refusal) return block_refused(plan);
    const BlockWeights w{norm1_weight, norm1_bias, Wqkv, bqkv, Wproj, bproj, norm2_weight, norm2_bias, W1, b1, W2, b2};
    if (!x || !w.present() || !y || !ws) return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: null pointer");
    if (B < 1) return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: B = %d", B);
    if (y == x) return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: y must not alias x");
    if (!plan.covered) return block_unsupported(plan, L, D, heads, hidden, flags);
    const BlockStore store(ws, plan, B, L, D, hidden);
    if (ws_bytes < store.total)
        return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_block_forward: workspace %zu < %zu bytes", ws_bytes, store.total);
    return block_forward(plan, x, w, store, nullptr, nullptr, eps, scale, y, B, L, D, heads, hidden, static_cast<hipStream_t>(stream));
}

}  // extern "C"
