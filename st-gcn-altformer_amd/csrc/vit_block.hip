// C entry points of the AltFormer heads' transformer block (include/stgcn_hip.h, "ViT block", ABI 10): the linear and the
// attention (resident and streaming form, and their bf16 forms) on their own, and the eval forward of one Block = five
// launches on one stream from a caller workspace (STGCN_VIT_BF16: the same five on bf16 operands, block_forward_bf16):
//   qkv = LN1(x) Wqkv^T + b -> attention -> x1 = a Wproj^T + b + x -> h = GELU(LN2(x1) W1^T + b1) -> y = h W2^T + b2 + x1
// (both LayerNorms inside the linear that consumes them).  A STGCN_VIT_TILE_* field in `flags` goes to the four linears.
// Long inputs are walked in slabs of whole sequences (kSlabRows tokens): the four intermediates of a slab (about 7 KB per
// token at D = 256) then stay within reach of the caches between the launches that write and read them, and the
// workspace does not grow with the batch.
#include "vit.h"

namespace stgcn {
namespace vit {
namespace {

struct BlockWs {
    float *qkv, *att, *x1, *hid;
    size_t total;
    BlockWs(void *base, int B, int L, int D, int hidden) {
        const size_t rows = (size_t)slab_seqs(B, L) * L;
        Carve c(base);
        qkv = c.take<float>(rows * 3 * D);
        att = c.take<float>(rows * D);
        x1 = c.take<float>(rows * D);
        hid = c.take<float>(rows * hidden);
        total = c.off;
    }
};

// The bf16 mode's plan: the same four pieces in the same order, the three that only feed matrix cores as bf16.  Every piece
// is at most as large as BlockWs's, so the plan fits what stgcn_vit_block_ws_bytes sizes.
struct BlockWsBf16 {
    unsigned short *qkv, *att, *hid;
    float *x1;
    size_t total;
    BlockWsBf16(void *base, int B, int L, int D, int hidden) {
        const size_t rows = (size_t)slab_seqs(B, L) * L;
        Carve c(base);
        qkv = c.take<unsigned short>(rows * 3 * D);
        att = c.take<unsigned short>(rows * D);
        x1 = c.take<float>(rows * D);
        hid = c.take<unsigned short>(rows * hidden);
        total = c.off;
    }
};

int block_forward_bf16(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv, const float *bqkv,
                       const float *Wproj, const float *bproj, const float *norm2_weight, const float *norm2_bias,
                       const float *W1, const float *b1, const float *W2, const float *b2, float eps, float scale, void *ws,
                       size_t ws_bytes, float *y, int B, int L, int D, int heads, int hidden, unsigned tile, hipStream_t st) {
    const BlockWsBf16 w(ws, B, L, D, hidden);
    if (ws_bytes < w.total) return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_block_forward: workspace %zu < %zu bytes", ws_bytes, w.total);
    const int per = slab_seqs(B, L);
    for (int b0 = 0; b0 < B; b0 += per) {
        const int nb = B - b0 < per ? B - b0 : per;
        const int M = nb * L;
        const float *xs = x + (size_t)b0 * L * D;
        float *ys = y + (size_t)b0 * L * D;
        int rc;
        if ((rc = launch_linear_bf16(xs, false, Wqkv, bqkv, nullptr, norm1_weight, norm1_bias, eps, w.qkv, true, M, D, 3 * D, false,
                                     tile, st)))
            return rc;
        if ((rc = launch_attention_bf16(w.qkv, w.att, nb, L, heads, D / heads, scale, st))) return rc;
        if ((rc = launch_linear_bf16(w.att, true, Wproj, bproj, xs, nullptr, nullptr, 0.f, w.x1, false, M, D, D, false, tile, st)))
            return rc;
        if ((rc = launch_linear_bf16(w.x1, false, W1, b1, nullptr, norm2_weight, norm2_bias, eps, w.hid, true, M, D, hidden, true,
                                     tile, st)))
            return rc;
        if ((rc = launch_linear_bf16(w.hid, true, W2, b2, w.x1, nullptr, nullptr, 0.f, ys, false, M, hidden, D, false, tile, st)))
            return rc;
    }
    return STGCN_OK;
}

}  // namespace
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
    return L >= 1 && L <= kMaxL && heads >= 1 && (head_dim == 32 || head_dim == 64) ? 1 : 0;
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
    const bool ln = ln_weight != nullptr, xb = (flags & STGCN_VIT_X_BF16) != 0, yb = (flags & STGCN_VIT_Y_BF16) != 0;
    if (ln && xb) return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_linear_bf16: LayerNorm needs fp32 x (STGCN_VIT_X_BF16 set)");
    if (!linear_ok(K, Nout, ln))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_linear_bf16: K = %d, Nout = %d (covered: K %% 32 == 0)", K, Nout);
    return launch_linear_bf16(x, xb, W, bias, residual, ln_weight, ln_bias, ln_eps, y, yb, M, K, Nout, (flags & STGCN_VIT_GELU) != 0,
                              flags & STGCN_VIT_TILE_MASK, static_cast<hipStream_t>(stream));
}

int stgcn_vit_attention_bf16_supported(int L, int heads, int head_dim) {
    return L >= 1 && L <= kMaxL && heads >= 1 && (head_dim == 32 || head_dim == 64) ? 1 : 0;
}

int stgcn_vit_attention_bf16(const void *qkv, void *out, int B, int L, int heads, int head_dim, float scale, void *stream) {
    REQUIRE_PTR(qkv); REQUIRE_PTR(out);
    REQUIRE_POS(B); REQUIRE_POS(L); REQUIRE_POS(heads);
    if (!stgcn_vit_attention_bf16_supported(L, heads, head_dim))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_attention_bf16: L = %d, head_dim = %d (covered: L <= %d, head_dim 32 / 64)", L,
                    head_dim, kMaxL);
    return launch_attention_bf16(qkv, out, B, L, heads, head_dim, scale, static_cast<hipStream_t>(stream));
}

int stgcn_vit_block_forward_bf16_supported(int L, int D, int heads, int hidden) { return block_bf16_ok(L, D, heads, hidden) ? 1 : 0; }

int stgcn_vit_block_supported(int L, int D, int heads, int hidden) { return block_ok(L, D, heads, hidden) ? 1 : 0; }

int stgcn_vit_block_forward_supported(int L, int D, int heads, int hidden) {
    return plan_block_forward(L, D, heads, hidden) != BlockAttention::none ? 1 : 0;
}

size_t stgcn_vit_block_ws_bytes(int B, int L, int D, int hidden) {
    if (B < 1 || L < 1 || D < 1 || hidden < 1) return 0;
    return BlockWs(nullptr, B, L, D, hidden).total;
}

int stgcn_vit_block_forward(const float *x, const float *norm1_weight, const float *norm1_bias, const float *Wqkv,
                            const float *bqkv, const float *Wproj, const float *bproj, const float *norm2_weight,
                            const float *norm2_bias, const float *W1, const float *b1, const float *W2, const float *b2,
                            float eps, float scale, void *ws, size_t ws_bytes, float *y, int B, int L, int D, int heads,
                            int hidden, unsigned flags, void *stream) {
    if (flags & STGCN_VIT_TRAIN_BF16)
        return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: STGCN_VIT_TRAIN_BF16 is a training mode (stgcn_vit_block_forward_train, "
                    "stgcn_vit_block_backward, stgcn_vit_linear_backward only)");
    if ((flags & STGCN_VIT_BF16) && (flags & STGCN_VIT_QKV_F32))
        return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: STGCN_VIT_BF16 and STGCN_VIT_QKV_F32 exclude each other");
    if (!x || !norm1_weight || !norm1_bias || !Wqkv || !Wproj || !norm2_weight || !norm2_bias || !W1 || !W2 || !y || !ws)
        return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: null pointer");
    if (B < 1) return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: B = %d", B);
    if (y == x) return fail(STGCN_ERR_ARG, "stgcn_vit_block_forward: y must not alias x");
    if (flags & STGCN_VIT_BF16) {
        if (!block_bf16_ok(L, D, heads, hidden))
            return fail(STGCN_ERR_UNSUPPORTED,
                        "stgcn_vit_block_forward: L = %d, D = %d, heads = %d, hidden = %d with STGCN_VIT_BF16 (covered: head_dim "
                        "32 / 64, L <= %d, D and hidden multiples of 64)", L, D, heads, hidden, kMaxL);
        return block_forward_bf16(x, norm1_weight, norm1_bias, Wqkv, bqkv, Wproj, bproj, norm2_weight, norm2_bias, W1, b1, W2, b2,
                                  eps, scale, ws, ws_bytes, y, B, L, D, heads, hidden, flags & STGCN_VIT_TILE_MASK,
                                  static_cast<hipStream_t>(stream));
    }
    const BlockAttention attention = plan_block_forward(L, D, heads, hidden);
    if (attention == BlockAttention::none || !math_ok(flags))
        return fail(STGCN_ERR_UNSUPPORTED,
                    "stgcn_vit_block_forward: L = %d, D = %d, heads = %d, hidden = %d, math %u (covered: head_dim 32 / 64, "
                    "L <= %d, D and hidden multiples of 64, f32 / bf16x3)", L, D, heads, hidden, flags & STGCN_MATH_MASK,
                    kMaxStreamL);
    const BlockWs w(ws, B, L, D, hidden);
    if (ws_bytes < w.total) return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_block_forward: workspace %zu < %zu bytes", ws_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *qkv = w.qkv, *att = w.att, *x1 = w.x1, *hid = w.hid;
    const unsigned tile = flags & STGCN_VIT_TILE_MASK;   // the plan (vit.h) reads it per linear
    const unsigned math = (flags & STGCN_MATH_MASK) | tile;
    const unsigned math_qkv = (flags & STGCN_VIT_QKV_F32) ? (unsigned)STGCN_MATH_F32 | tile : math;
    const int per = slab_seqs(B, L);
    for (int b0 = 0; b0 < B; b0 += per) {
        const int nb = B - b0 < per ? B - b0 : per;
        const int M = nb * L;
        const float *xs = x + (size_t)b0 * L * D;
        float *ys = y + (size_t)b0 * L * D;
        int rc;
        if ((rc = launch_linear(xs, Wqkv, bqkv, nullptr, norm1_weight, norm1_bias, eps, qkv, M, D, 3 * D, false, math_qkv, st)))
            return rc;
        if ((rc = attention == BlockAttention::stream ? launch_attention_stream(qkv, att, nb, L, heads, D / heads, scale, st)
                                                      : launch_attention_packed(qkv, att, nb, L, heads, D / heads, scale, st)))
            return rc;
        if ((rc = launch_linear(att, Wproj, bproj, xs, nullptr, nullptr, 0.f, x1, M, D, D, false, math, st))) return rc;
        if ((rc = launch_linear(x1, W1, b1, nullptr, norm2_weight, norm2_bias, eps, hid, M, D, hidden, true, math, st)))
            return rc;
        if ((rc = launch_linear(hid, W2, b2, x1, nullptr, nullptr, 0.f, ys, M, hidden, D, false, math, st))) return rc;
    }
    return STGCN_OK;
}

}  // extern "C"
