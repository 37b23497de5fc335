// The backward of the ST-ViT head's patch embedding (include/stgcn_hip.h, "The ST-ViT head: training the two ends"; vit.h's
// plan_patch_backward decides splits, tile and workspace, this file launches what it says).  From dx (N, n + 1, E):
//   vit_wgrad_kernel<PatchWgradRows>   : dW slabs = dx_tokens^T patches, the patches read in place from the (N, T, V, C) stem
//                                        output, the class rows of dx skipped; dbias' slabs ride in the first K tile
//   launch_sum_parts                   : the token splits' slabs added in split order
//   transpose_pad + vit_linear_kernel<PatchGradRows> : dz = dx_tokens W, stored straight into the (N, T, V, C) layout
//   vit_patch_posgrad_kernel           : dpos[t] = sum over the clips of dx[i][t], dcls = the same sum of row 0
//   vit_patch_transpose_kernel         : (N, C, T, V) input only: z into the workspace before the wgrad, dz out of the same
//                                        buffer after the dgrad
// Every output is optional.  What an output holds does not depend on which others were asked for: the launches are
// independent and each runs as it does in the all-outputs call.  fp32 in memory, the wgrad on fp32 matrix cores, the dgrad
// f32 or bf16x3, fp32 accumulate, no atomics: bit-identical from run to run.  No (N, n, K) tensor exists.
#include "vit_wgrad_kernel.h"

namespace stgcn {
namespace vit {
namespace {

using namespace linear_kernel;
using namespace wgrad_kernel;

// One thread per element (t, e) of the position table's gradient: the clips in ascending order.  `count`: (n + 1) E, or E
// when only dcls is wanted (row 0 alone).
__global__ __launch_bounds__(256) void vit_patch_posgrad_kernel(const float *__restrict__ dx, float *__restrict__ dpos,
                                                                float *__restrict__ dcls, int N, size_t clip, int E, int count) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    float a = 0.f;
    for (int i = 0; i < N; ++i) a += dx[(size_t)i * clip + idx];
    if (dpos != nullptr) dpos[idx] = a;
    if (dcls != nullptr && idx < E) dcls[idx] = a;
}

PatchRows patch_rows(const PatchBackwardPlan &p, int C, int T, int V, int p1, int p2) {
    PatchRows rows;
    rows.n = p.n, rows.w = p.w, rows.run = p2 * C, rows.frame = V * C, rows.patch_rows = p1 * V * C, rows.clip = T * V * C;
    rows.cps = 0;
    return rows;
}

template <int MATH, class F>
int launch_dgrad_form(const PatchBackwardPlan &p, const PatchGradRows &rows, const float *dx, const float *Wt, float *dz, int E,
                      hipStream_t st) {
    const int tiles_n = ceil_div(p.K, F::BN);
    const long long tiles = (long long)tiles_n * ceil_div(p.M, F::BM);
    if (!grid_fits(tiles, F::THREADS)) return fail(STGCN_ERR_UNSUPPORTED, "vit patch embed backward: %lld tiles", tiles);
    LinearExtra ex;
    ex.kx = E;   // dx's rows are E long; the transposed weight's are padded to Epad with zeros
    vit_linear_kernel<MATH, F, false, false, PatchGradRows><<<dim3((unsigned)tiles), dim3(F::THREADS), 0, st>>>(
        dx, Wt, nullptr, nullptr, nullptr, nullptr, 0.f, dz, p.M, p.Epad, p.K, tiles_n, 0, ex, rows);
    STGCN_LAUNCH_CHECK("vit_linear_kernel (patches' gradient)");
    return STGCN_OK;
}

template <int MATH>
int launch_dgrad_math(const PatchBackwardPlan &p, const PatchGradRows &rows, const float *dx, const float *Wt, float *dz, int E,
                      hipStream_t st) {
    if (p.tile.bm == Form128::BM) return launch_dgrad_form<MATH, Form128>(p, rows, dx, Wt, dz, E, st);
    if (p.tile.bm == Form64::BM) return launch_dgrad_form<MATH, Form64>(p, rows, dx, Wt, dz, E, st);
    return launch_dgrad_form<MATH, Form32>(p, rows, dx, Wt, dz, E, st);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_patch_embed_backward(const PatchBackwardPlan &p, const PatchBackwardStore &store, const float *z, const float *W,
                                const float *dx, float *dW, float *dbias, float *dcls, float *dpos, float *dz, int N, int C, int T,
                                int V, int p1, int p2, int E, hipStream_t st) {
    int rc;
    const PatchRows rows = patch_rows(p, C, T, V, p1, p2);
    if (dW != nullptr || dbias != nullptr) {
        if (p.transpose && dW != nullptr) {
            if ((rc = launch_patch_transpose(z, store.zt, N, C, T * V, st))) return rc;
            z = store.zt;
        }
        // dbias alone: the workgroups of the first K tile, which sum dx's columns exactly as they do beside the others
        const int tiles_n = ceil_div(E, WT), tiles_k = dW != nullptr ? ceil_div(p.K, WT) : 1;
        const long long blocks = (long long)tiles_n * tiles_k * p.splits;
        if (!grid_fits(blocks, 256)) return fail(STGCN_ERR_UNSUPPORTED, "vit patch embed backward: %lld wgrad workgroups", blocks);
        float *bpart = dbias != nullptr ? store.part + (size_t)p.splits * E * p.K : nullptr;
        PatchWgradRows pol;
        pol.rows = rows;
        vit_wgrad_kernel<PatchWgradRows><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(dx, z, nullptr, 1, store.part, bpart, p.M, p.K,
                                                                                      E, tiles_n, tiles_k, p.rps / WC, 0, pol);
        STGCN_LAUNCH_CHECK("vit_wgrad_kernel (patches)");
        if (dW != nullptr && (rc = launch_sum_parts(store.part, dW, p.splits, (size_t)E * p.K, st))) return rc;
        if (dbias != nullptr && (rc = launch_sum_parts(bpart, dbias, p.splits, (size_t)E, st))) return rc;
    }
    if (dz != nullptr) {
        if ((rc = launch_transpose_pad(W, store.Wt, E, p.K, p.Epad, st))) return rc;
        PatchGradRows grad;
        grad.to = rows;
        float *out = p.transpose ? store.dzt : dz;
        if (p.math == STGCN_MATH_F32) rc = launch_dgrad_math<STGCN_MATH_F32>(p, grad, dx, store.Wt, out, E, st);
        else rc = launch_dgrad_math<STGCN_MATH_BF16X3>(p, grad, dx, store.Wt, out, E, st);
        if (rc) return rc;
        // (N, P, C) -> (N, C, P): the forward's pass with the two extents exchanged
        if (p.transpose && (rc = launch_patch_transpose(store.dzt, dz, N, T * V, C, st))) return rc;
    }
    if (dpos != nullptr || dcls != nullptr) {
        const int count = dpos != nullptr ? (p.n + 1) * E : E;
        vit_patch_posgrad_kernel<<<dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, st>>>(dx, dpos, dcls, N, (size_t)(p.n + 1) * E,
                                                                                           E, count);
        STGCN_LAUNCH_CHECK("vit_patch_posgrad_kernel");
    }
    return STGCN_OK;
}

}  // namespace vit
}  // namespace stgcn

using namespace stgcn;
using namespace stgcn::vit;

extern "C" {

int stgcn_vit_patch_embed_backward_supported(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    const PatchBackwardPlan p = plan_patch_backward(N, C, T, V, p1, p2, E, flags);
    return !p.refusal && p.shaped && p.covered ? 1 : 0;
}

size_t stgcn_vit_patch_embed_backward_ws_bytes(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    const PatchBackwardPlan p = plan_patch_backward(N, C, T, V, p1, p2, E, flags);
    return !p.refusal && p.shaped && p.covered ? PatchBackwardStore(nullptr, p, N, C, T, V, E).total : 0;
}

int stgcn_vit_patch_embed_backward_cut(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    const PatchBackwardPlan p = plan_patch_backward(N, C, T, V, p1, p2, E, flags);
    return !p.refusal && p.shaped && p.covered && p.rps < 32768 && p.splits < 65536 ? (p.rps << 16) | p.splits : 0;
}

int stgcn_vit_patch_embed_backward(const float *z, const float *W, const float *dx, float *dW, float *dbias, float *dcls,
                                   float *dpos, float *dz, int N, int C, int T, int V, int p1, int p2, int E, void *ws,
                                   size_t ws_bytes, unsigned flags, void *stream) {
    const PatchBackwardPlan p = plan_patch_backward(N, C, T, V, p1, p2, E, flags);
    if (p.refusal) return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed_backward: %s (got 0x%x)", p.refusal, flags);
    REQUIRE_PTR(z); REQUIRE_PTR(W); REQUIRE_PTR(dx); REQUIRE_PTR(ws);
    REQUIRE_POS(N); REQUIRE_POS(C); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(p1); REQUIRE_POS(p2); REQUIRE_POS(E);
    if (!p.shaped)
        return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed_backward: T = %d, V = %d are not whole patches of %d x %d", T, V, p1, p2);
    if (!aligned16(z) || !aligned16(W) || !aligned16(dx) || !aligned16(ws))
        return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed_backward: z, W, dx and ws must be 16-byte aligned");
    if (dz == z) return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed_backward: dz must not alias z");
    if (!p.covered)
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_patch_embed_backward: C = %d, p2 = %d, E = %d, math %u (covered: (p2 C) %% 32 "
                    "== 0, E %% 4 == 0, f32 / bf16x3, a clip, the output and the weight below 2^31 elements)", C, p2, E,
                    flags & STGCN_MATH_MASK);
    const PatchBackwardStore store(ws, p, N, C, T, V, E);
    if (ws_bytes < store.total)
        return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_patch_embed_backward: workspace %zu < %zu bytes", ws_bytes, store.total);
    return launch_patch_embed_backward(p, store, z, W, dx, dW, dbias, dcls, dpos, dz, N, C, T, V, p1, p2, E,
                                       static_cast<hipStream_t>(stream));
}

}  // extern "C"
