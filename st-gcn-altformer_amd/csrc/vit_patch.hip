// The front of the ST-ViT head (include/stgcn_hip.h, "The ST-ViT head"): the patch embedding of the stem output with the class
// row and the position table, x (N, n + 1, E).  The product is the linears' tile kernel (vit_linear_kernel.h) on PatchRows: a
// patch is read from the (N, T, V, C) stem output as its p1 runs of p2 C floats, so the rearranged (N, n, K) tensor never
// exists; the contraction (K = 5120 in the reference, against 99 rows per clip) is cut over grid.y into slabs whose sums one
// kernel adds in slab order.  vit.h's plan_patch decides tile and cut; this file launches what it says.
//   vit_patch_transpose_kernel : (N, C, T, V) -> (N, T, V, C), only for input that arrives channels-first
//   vit_linear_kernel<PatchRows>: slab s of the workspace = patches[:, chunks of s] W[:, chunks of s]^T
//   vit_patch_sum_kernel       : x[i][1 + p] = ((slab 0 + slab 1 + ...) + bias) + pos[1 + p],  x[i][0] = cls + pos[0]
// fp32 in memory on every side, f32 or bf16x3 products, fp32 accumulate, no atomics: bit-identical from run to run.
#include "vit_linear_kernel.h"

namespace stgcn {
namespace vit {
namespace {

using namespace linear_kernel;

// zt (N, P, C) = z (N, C, P)^T per clip, P = T V: 32 x 32 tiles through LDS (33 floats a row: no bank conflicts either way),
// a workgroup of 256 threads per tile, the tiles of all clips on grid.x.
__global__ __launch_bounds__(256) void vit_patch_transpose_kernel(const float *__restrict__ z, float *__restrict__ zt, int C, int P,
                                                                  int tiles_p, int tiles_c) {
    __shared__ float tile[32][33];
    const int per = tiles_p * tiles_c, clip = (int)blockIdx.x / per, t = (int)blockIdx.x % per;
    const int p0 = (t % tiles_p) * 32, c0 = (t / tiles_p) * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float *zc = z + (size_t)clip * C * P;
    float *ztc = zt + (size_t)clip * C * P;
#pragma unroll
    for (int r = ty; r < 32; r += 8)
        if (c0 + r < C && p0 + tx < P) tile[r][tx] = zc[(size_t)(c0 + r) * P + p0 + tx];
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8)
        if (p0 + r < P && c0 + tx < C) ztc[(size_t)(p0 + r) * C + c0 + tx] = tile[tx][r];
}

// One thread per element of x (N, n + 1, E).  part: `splits` slabs of (N n, E), added in slab order.
__global__ __launch_bounds__(256) void vit_patch_sum_kernel(const float *__restrict__ part, int splits, size_t slab,
                                                            const float *__restrict__ bias, const float *__restrict__ cls,
                                                            const float *__restrict__ pos, float *__restrict__ x, int n, int E,
                                                            size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t row = idx / E;
    const int e = (int)(idx - row * E), i = (int)(row / (n + 1)), t = (int)(row - (size_t)i * (n + 1));
    float v;
    if (t == 0) {
        v = cls[e];
    } else {
        const size_t src = ((size_t)i * n + (t - 1)) * E + e;
        v = part[src];
        for (int s = 1; s < splits; ++s) v += part[(size_t)s * slab + src];
        if (bias != nullptr) v += bias[e];
    }
    if (pos != nullptr) v += pos[(size_t)t * E + e];
    x[idx] = v;
}

template <int MATH, class F>
int launch_patch_form(const PatchPlan &p, const float *z, const float *W, float *part, int C, int V, int T, int p1, int p2, int E,
                      hipStream_t st) {
    const int tiles_n = ceil_div(E, F::BN);
    const long long tiles = (long long)tiles_n * ceil_div(p.M, F::BM);
    if (!grid_fits(tiles, F::THREADS) || p.splits > 65535) return fail(STGCN_ERR_UNSUPPORTED, "vit patch embed: %lld tiles x %d slabs", tiles, p.splits);
    PatchRows rows;
    rows.n = p.n, rows.w = p.w, rows.run = p2 * C, rows.frame = V * C, rows.patch_rows = p1 * V * C, rows.clip = T * V * C;
    rows.cps = p.cps;
    vit_linear_kernel<MATH, F, false, false, PatchRows><<<dim3((unsigned)tiles, (unsigned)p.splits), dim3(F::THREADS), 0, st>>>(
        z, W, nullptr, nullptr, nullptr, nullptr, 0.f, part, p.M, p.K, E, tiles_n, 0, LinearExtra{}, rows);
    STGCN_LAUNCH_CHECK("vit_linear_kernel (patches)");
    return STGCN_OK;
}

template <int MATH>
int launch_patch_math(const PatchPlan &p, const float *z, const float *W, float *part, int C, int V, int T, int p1, int p2, int E,
                      hipStream_t st) {
    if (p.tile.bm == Form128::BM) return launch_patch_form<MATH, Form128>(p, z, W, part, C, V, T, p1, p2, E, st);
    if (p.tile.bm == Form64::BM) return launch_patch_form<MATH, Form64>(p, z, W, part, C, V, T, p1, p2, E, st);
    return launch_patch_form<MATH, Form32>(p, z, W, part, C, V, T, p1, p2, E, st);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_patch_transpose(const float *z, float *zt, int N, int C, int P, hipStream_t st) {
    const int tiles_p = ceil_div(P, 32), tiles_c = ceil_div(C, 32);
    const long long blocks = (long long)N * tiles_p * tiles_c;
    if (!grid_fits(blocks, 256)) return fail(STGCN_ERR_UNSUPPORTED, "vit patch embed: %lld transpose tiles", blocks);
    vit_patch_transpose_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(z, zt, C, P, tiles_p, tiles_c);
    STGCN_LAUNCH_CHECK("vit_patch_transpose_kernel");
    return STGCN_OK;
}

int launch_patch_embed_vit(const PatchPlan &p, const PatchStore &store, const float *z, const float *W, const float *bias,
                           const float *cls, const float *pos, float *x, int N, int C, int T, int V, int p1, int p2, int E,
                           hipStream_t st) {
    int rc;
    if (p.transpose) {
        if ((rc = launch_patch_transpose(z, store.zt, N, C, T * V, st))) return rc;
        z = store.zt;
    }
    if (p.math == STGCN_MATH_F32) rc = launch_patch_math<STGCN_MATH_F32>(p, z, W, store.part, C, V, T, p1, p2, E, st);
    else rc = launch_patch_math<STGCN_MATH_BF16X3>(p, z, W, store.part, C, V, T, p1, p2, E, st);
    if (rc) return rc;
    const size_t total = (size_t)N * (p.n + 1) * E, slab = (size_t)p.M * E;
    vit_patch_sum_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(store.part, p.splits, slab, bias, cls, pos, x,
                                                                                     p.n, E, total);
    STGCN_LAUNCH_CHECK("vit_patch_sum_kernel");
    return STGCN_OK;
}

}  // namespace vit
}  // namespace stgcn

using namespace stgcn;
using namespace stgcn::vit;

extern "C" {

int stgcn_vit_patch_embed_supported(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    const PatchPlan p = plan_patch(N, C, T, V, p1, p2, E, flags);
    return !p.refusal && p.shaped && p.covered ? 1 : 0;
}

size_t stgcn_vit_patch_embed_ws_bytes(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    const PatchPlan p = plan_patch(N, C, T, V, p1, p2, E, flags);
    return !p.refusal && p.shaped && p.covered ? PatchStore(nullptr, p, N, C, T, V, E).total : 0;
}

int stgcn_vit_patch_embed_cut(int N, int C, int T, int V, int p1, int p2, int E, unsigned flags) {
    const PatchPlan p = plan_patch(N, C, T, V, p1, p2, E, flags);
    return !p.refusal && p.shaped && p.covered ? (p.tile.bm << 16) | p.splits : 0;
}

int stgcn_vit_patch_embed(const float *z, const float *W, const float *bias, const float *cls, const float *pos, float *x, int N,
                          int C, int T, int V, int p1, int p2, int E, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    const PatchPlan p = plan_patch(N, C, T, V, p1, p2, E, flags);
    if (p.refusal) return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed: %s (got 0x%x)", p.refusal, flags);
    REQUIRE_PTR(z); REQUIRE_PTR(W); REQUIRE_PTR(cls); REQUIRE_PTR(x); REQUIRE_PTR(ws);
    REQUIRE_POS(N); REQUIRE_POS(C); REQUIRE_POS(T); REQUIRE_POS(V); REQUIRE_POS(p1); REQUIRE_POS(p2); REQUIRE_POS(E);
    if (!p.shaped)
        return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed: T = %d, V = %d are not whole patches of %d x %d", T, V, p1, p2);
    if (!aligned16(z) || !aligned16(W) || !aligned16(ws))
        return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed: z, W and ws must be 16-byte aligned");
    if (x == z) return fail(STGCN_ERR_ARG, "stgcn_vit_patch_embed: x must not alias z");
    if (!p.covered)
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_patch_embed: C = %d, p2 = %d, math %u (covered: (p2 C) %% 32 == 0, f32 / bf16x3, "
                    "a clip and the output below 2^31 elements)", C, p2, flags & STGCN_MATH_MASK);
    const PatchStore store(ws, p, N, C, T, V, E);
    if (ws_bytes < store.total)
        return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_patch_embed: workspace %zu < %zu bytes", ws_bytes, store.total);
    return launch_patch_embed_vit(p, store, z, W, bias, cls, pos, x, N, C, T, V, p1, p2, E, static_cast<hipStream_t>(stream));
}

}  // extern "C"
