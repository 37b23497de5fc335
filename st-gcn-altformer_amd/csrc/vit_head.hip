// The whole AltFormer head from the stem output to the logits (include/stgcn_hip.h, "The whole AltFormer head"): the two
// kernels the head needs beside its blocks - the pooling over the tokens of a sequence between the stages, and the pooled
// classifier (pooling, LayerNorm, Linear) at the end - and the entry point that runs embeddings, blocks and both under one
// plan (vit.h: plan_head) on one workspace (HeadStore).  The blocks are block_forward's, the embeddings launch_patch_embed's.
// Both kernels are fp32, deterministic (no atomics, a fixed summation order), allocate nothing and never synchronise.
#include "vit.h"

namespace stgcn {
namespace vit {
namespace {

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
__device__ __forceinline__ float4 max4(float4 a, float4 b) {
    return float4{max_nan(a.x, b.x), max_nan(a.y, b.y), max_nan(a.z, b.z), max_nan(a.w, b.w)};
}

// The pooled float4 column `c4` of one sequence (`xs` = its first token, D4 = D / 4 columns per token) as token lane `ty` of
// `TY` sees it: the tokens ty, ty + TY, ... in that order.  MAX: the accumulator starts from a token of the sequence (lane
// ty's first one, or the last token for a lane that has none: a token counted twice does not move a maximum); mean: from zero,
// and a lane without tokens adds nothing.
template <bool MAX>
__device__ __forceinline__ float4 pool_lane(const float4 *__restrict__ xs, int L, int D4, int c4, int ty, int TY) {
    float4 acc = MAX ? xs[(size_t)(ty < L ? ty : L - 1) * D4 + c4] : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int l = ty; l < L; l += TY) {
        const float4 v = xs[(size_t)l * D4 + c4];
        acc = MAX ? max4(acc, v) : add4(acc, v);
    }
    return acc;
}

// out (S, D) from x (S, L, D).  Workgroup (256 threads) = (sequence, chunk of CX float4 columns): CX lanes along D (16 bytes
// each, CX * 16 contiguous bytes per token), 256 / CX token lanes, joined through LDS in ascending lane order.  CX = 64 reads
// whole 1 KB rows; CX = 16 cuts D four times finer for calls of few sequences (launch_pool picks).
// L: the tokens pooled, the first L of every sequence; Ls: the tokens a sequence has (L, or L = 1 for the class token).
template <int CX, bool MAX>
__global__ __launch_bounds__(256) void vit_pool_kernel(const float *__restrict__ x, float *__restrict__ out, int L, int Ls, int D4,
                                                       int chunks) {
    constexpr int TY = 256 / CX;
    __shared__ float4 part[TY][CX];
    const int s = blockIdx.x / chunks, c4 = (blockIdx.x % chunks) * CX + (threadIdx.x % CX), ty = threadIdx.x / CX;
    const bool live = c4 < D4;                       // the last chunk of a D that is no multiple of 4 CX
    const float4 *xs = reinterpret_cast<const float4 *>(x) + (size_t)s * Ls * D4;
    if (live) part[ty][threadIdx.x % CX] = pool_lane<MAX>(xs, L, D4, c4, ty, TY);
    __syncthreads();
    if (ty == 0 && live) {
        float4 acc = part[0][threadIdx.x];
#pragma unroll
        for (int j = 1; j < TY; ++j) acc = MAX ? max4(acc, part[j][threadIdx.x]) : add4(acc, part[j][threadIdx.x]);
        if (!MAX) {
            const float n = (float)L;
            acc = float4{acc.x / n, acc.y / n, acc.z / n, acc.w / n};
        }
        reinterpret_cast<float4 *>(out)[(size_t)s * D4 + c4] = acc;
    }
}

constexpr int kClsThreads = 1024, kClsWaves = kClsThreads / kWave;

// The sum of `v` over the workgroup, the same value in every thread: lanes by shuffles, the waves' sums through `red` and
// added in ascending wave order.  Two barriers; `red` may be reused after it returns.
__device__ __forceinline__ float block_sum(float v, float *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                                  // the previous use of `red` is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < kClsWaves; ++w) s += red[w];
    return s;
}

// logits[n] = LayerNorm(pool_L(x[n])) W^T + bias.  One workgroup (1024 threads) per clip, three phases:
//   pool   : as vit_pool_kernel, min(D / 4, 1024) lanes along D and the rest of the workgroup as token lanes, D walked in
//            passes of 1024 columns where it is longer; the pooled row lands in LDS;
//   norm   : mean and biased variance of the row in two passes over LDS, then the affine LayerNorm in place;
//   linear : a wave per class, 16-byte loads along the class's row of W, the lanes' sums joined by shuffles.
template <bool MAX>
__global__ __launch_bounds__(kClsThreads) void vit_pool_classify_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                                         const float *__restrict__ beta, float eps,
                                                                         const float *__restrict__ W, const float *__restrict__ bias,
                                                                         float *__restrict__ logits, int L, int Ls, int D,
                                                                         int classes) {
    __shared__ float4 part[kClsThreads];
    __shared__ float4 row4[kMaxLnDim / 4];
    __shared__ float red[kClsWaves];
    float *row = reinterpret_cast<float *>(row4);
    const int n = blockIdx.x, tid = threadIdx.x, D4 = D / 4;
    const float4 *xs = reinterpret_cast<const float4 *>(x) + (size_t)n * Ls * D4;   // L, Ls: as in vit_pool_kernel
    const int CX = D4 < kClsThreads ? D4 : kClsThreads, TY = kClsThreads / CX;   // D % 64 == 0: CX is a multiple of 16
    const int cx = tid % CX, ty = tid / CX;
    for (int c0 = 0; c0 < D4; c0 += CX) {            // one pass unless D = 4096 (CX = 1024 = D4 then: no tail)
        if (ty < TY) part[ty * CX + cx] = pool_lane<MAX>(xs, L, D4, c0 + cx, ty, TY);
        __syncthreads();
        if (ty == 0) {
            float4 acc = part[cx];
            for (int j = 1; j < TY; ++j) acc = MAX ? max4(acc, part[j * CX + cx]) : add4(acc, part[j * CX + cx]);
            if (!MAX) {
                const float len = (float)L;
                acc = float4{acc.x / len, acc.y / len, acc.z / len, acc.w / len};
            }
            row4[c0 + cx] = acc;
        }
        __syncthreads();
    }
    float s = 0.f;
    for (int d = tid; d < D; d += kClsThreads) s += row[d];
    const float mean = block_sum(s, red) / (float)D;
    float q = 0.f;
    for (int d = tid; d < D; d += kClsThreads) {
        const float c = row[d] - mean;
        q = fmaf(c, c, q);
    }
    const float rstd = 1.f / sqrtf(block_sum(q, red) / (float)D + eps);
    for (int d = tid; d < D; d += kClsThreads) row[d] = (row[d] - mean) * rstd * gamma[d] + beta[d];
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int c = wave; c < classes; c += kClsWaves) {
        const float4 *w4 = reinterpret_cast<const float4 *>(W) + (size_t)c * D4;
        float a = 0.f;
        for (int j = lane; j < D4; j += 64) {
            const float4 w = w4[j], r = row4[j];
            a = fmaf(w.x, r.x, a);
            a = fmaf(w.y, r.y, a);
            a = fmaf(w.z, r.z, a);
            a = fmaf(w.w, r.w, a);
        }
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        if (lane == 0) logits[(size_t)n * classes + c] = a + (bias != nullptr ? bias[c] : 0.f);
    }
}

// The backward of vit_pool_classify_kernel for one clip per workgroup (vit.h, "the backward of the pooled classifier"):
//   pool, norm : the forward's phases again (the pooled row, its mean and rstd), xhat kept in LDS;
//   g          : g[d] = sum_c dlogits[n][c] W[c][d], a thread per d, the classes in ascending order;
//   LayerNorm  : dp = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat)), the two means by block_sum;
//   parts      : normed[n] = xhat gamma + beta (dW's operand), gpart[n] = g xhat, bpart[n] = g;
//   dx         : the clip's L rows, all of them: FIRST: dp in row 0 and zeros below, else dp / L in every row.
template <bool FIRST>
__global__ __launch_bounds__(kClsThreads) void vit_pool_classify_bwd_kernel(
    const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
    const float *__restrict__ W, const float *__restrict__ dlogits, float *__restrict__ dx, float *__restrict__ normed,
    float *__restrict__ gpart, float *__restrict__ bpart, int L, int D, int classes) {
    __shared__ float4 part[kClsThreads];
    __shared__ float4 row4[kMaxLnDim / 4];
    __shared__ float4 grad4[kMaxLnDim / 4];
    __shared__ float red[kClsWaves];
    float *row = reinterpret_cast<float *>(row4), *grad = reinterpret_cast<float *>(grad4);
    const int n = blockIdx.x, tid = threadIdx.x, D4 = D / 4;
    const int Lp = FIRST ? 1 : L;                                                    // the tokens pooled
    const float4 *xs = reinterpret_cast<const float4 *>(x) + (size_t)n * L * D4;
    const int CX = D4 < kClsThreads ? D4 : kClsThreads, TY = kClsThreads / CX;
    const int cx = tid % CX, ty = tid / CX;
    for (int c0 = 0; c0 < D4; c0 += CX) {
        if (ty < TY) part[ty * CX + cx] = pool_lane<FIRST>(xs, Lp, D4, c0 + cx, ty, TY);   // FIRST: the selection over one token
        __syncthreads();
        if (ty == 0) {
            float4 acc = part[cx];
            for (int j = 1; j < TY; ++j) acc = FIRST ? max4(acc, part[j * CX + cx]) : add4(acc, part[j * CX + cx]);
            if (!FIRST) {
                const float len = (float)L;
                acc = float4{acc.x / len, acc.y / len, acc.z / len, acc.w / len};
            }
            row4[c0 + cx] = acc;
        }
        __syncthreads();
    }
    float s = 0.f;
    for (int d = tid; d < D; d += kClsThreads) s += row[d];
    const float mean = block_sum(s, red) / (float)D;
    float q = 0.f;
    for (int d = tid; d < D; d += kClsThreads) {
        const float c = row[d] - mean;
        q = fmaf(c, c, q);
    }
    const float rstd = 1.f / sqrtf(block_sum(q, red) / (float)D + eps);
    const float *dl = dlogits + (size_t)n * classes;
    float s1 = 0.f, s2 = 0.f;
    for (int d = tid; d < D; d += kClsThreads) {      // a thread owns its d from here to the store of dp
        const float xh = (row[d] - mean) * rstd;
        float g = 0.f;
        for (int c = 0; c < classes; ++c) g = fmaf(dl[c], W[(size_t)c * D + d], g);
        const float gw = g * gamma[d];
        s1 += gw;
        s2 = fmaf(gw, xh, s2);
        row[d] = xh;
        grad[d] = gw;
        const size_t o = (size_t)n * D + d;
        if (normed != nullptr) normed[o] = xh * gamma[d] + beta[d];
        if (gpart != nullptr) gpart[o] = g * xh;
        if (bpart != nullptr) bpart[o] = g;
    }
    const float m1 = block_sum(s1, red) / (float)D, m2 = block_sum(s2, red) / (float)D;
    if (dx == nullptr) return;
    for (int d = tid; d < D; d += kClsThreads) {
        const float dp = rstd * (grad[d] - m1 - row[d] * m2);
        grad[d] = FIRST ? dp : dp / (float)L;
    }
    __syncthreads();
    float4 *dxs = reinterpret_cast<float4 *>(dx) + (size_t)n * L * D4;
    const float4 zero = float4{0.f, 0.f, 0.f, 0.f};
    for (int e = tid; e < L * D4; e += kClsThreads) dxs[e] = FIRST && e >= D4 ? zero : grad4[e % D4];
}

// One thread per element of dW (classes, D), then of dbias (classes): the clips in ascending order.
__global__ __launch_bounds__(256) void vit_classify_wgrad_kernel(const float *__restrict__ dlogits, const float *__restrict__ normed,
                                                                  float *__restrict__ dW, float *__restrict__ dbias, int N, int D,
                                                                  int classes) {
    const int idx = blockIdx.x * 256 + threadIdx.x, nw = dW != nullptr ? classes * D : 0;
    if (idx < nw) {
        const int c = idx / D, d = idx - c * D;
        float a = 0.f;
        for (int n = 0; n < N; ++n) a = fmaf(dlogits[(size_t)n * classes + c], normed[(size_t)n * D + d], a);
        dW[idx] = a;
    } else if (idx - nw < classes && dbias != nullptr) {
        const int c = idx - nw;
        float a = 0.f;
        for (int n = 0; n < N; ++n) a += dlogits[(size_t)n * classes + c];
        dbias[c] = a;
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool pool_flags_clash(unsigned flags) { return (flags & STGCN_VIT_POOL_MAX) && (flags & STGCN_VIT_POOL_CLS); }

}  // namespace

int launch_pool(const float *x, float *out, long long S, int L, int D, bool max, hipStream_t st, bool first) {
    const int Ls = L;
    if (first) L = 1, max = true;   // the selection over one token: that token, bit for bit
    // Whole 1 KB rows per workgroup where that still gives every CU some workgroups; a quarter of that per workgroup below
    // (one clip of TS: 22 sequences of 180 tokens at D = 256 are 22 workgroups of the wide form and 88 of the narrow one).
    const int D4 = D / 4;
    const bool wide = S * ceil_div(D4, 64) >= 1024;
    const int chunks = ceil_div(D4, wide ? 64 : 16);
    if (!grid_fits(S * chunks, 256)) return fail(STGCN_ERR_UNSUPPORTED, "vit pool: %lld sequences of %d columns exceed the grid", S, D);
    const dim3 grid((unsigned)(S * chunks));
    if (wide) {
        if (max) hipLaunchKernelGGL((vit_pool_kernel<64, true>), grid, dim3(256), 0, st, x, out, L, Ls, D4, chunks);
        else hipLaunchKernelGGL((vit_pool_kernel<64, false>), grid, dim3(256), 0, st, x, out, L, Ls, D4, chunks);
    } else {
        if (max) hipLaunchKernelGGL((vit_pool_kernel<16, true>), grid, dim3(256), 0, st, x, out, L, Ls, D4, chunks);
        else hipLaunchKernelGGL((vit_pool_kernel<16, false>), grid, dim3(256), 0, st, x, out, L, Ls, D4, chunks);
    }
    STGCN_LAUNCH_CHECK("vit_pool_kernel");
    return STGCN_OK;
}

int launch_pool_classify(const float *x, const float *gamma, const float *beta, float eps, const float *W, const float *bias,
                         float *logits, int N, int L, int D, int classes, bool max, hipStream_t st, bool first) {
    const int Ls = L;
    if (first) L = 1, max = true;
    if (max)
        hipLaunchKernelGGL((vit_pool_classify_kernel<true>), dim3(N), dim3(kClsThreads), 0, st, x, gamma, beta, eps, W, bias,
                           logits, L, Ls, D, classes);
    else
        hipLaunchKernelGGL((vit_pool_classify_kernel<false>), dim3(N), dim3(kClsThreads), 0, st, x, gamma, beta, eps, W, bias,
                           logits, L, Ls, D, classes);
    STGCN_LAUNCH_CHECK("vit_pool_classify_kernel");
    return STGCN_OK;
}

int launch_pool_classify_backward(const ClassifyBackwardStore &store, const float *x, const float *gamma, const float *beta,
                                  float eps, const float *W, const float *dlogits, float *dx, float *dgamma, float *dbeta,
                                  float *dW, float *dbias, int N, int L, int D, int classes, bool first, hipStream_t st) {
    int rc;
    if (dx != nullptr || dgamma != nullptr || dbeta != nullptr || dW != nullptr) {
        float *normed = dW != nullptr ? store.normed : nullptr, *gpart = dgamma != nullptr ? store.gpart : nullptr;
        float *bpart = dbeta != nullptr ? store.bpart : nullptr;
        if (first)
            hipLaunchKernelGGL((vit_pool_classify_bwd_kernel<true>), dim3(N), dim3(kClsThreads), 0, st, x, gamma, beta, eps, W,
                               dlogits, dx, normed, gpart, bpart, L, D, classes);
        else
            hipLaunchKernelGGL((vit_pool_classify_bwd_kernel<false>), dim3(N), dim3(kClsThreads), 0, st, x, gamma, beta, eps, W,
                               dlogits, dx, normed, gpart, bpart, L, D, classes);
        STGCN_LAUNCH_CHECK("vit_pool_classify_bwd_kernel");
    }
    if (dgamma != nullptr && (rc = launch_sum_parts(store.gpart, dgamma, N, (size_t)D, st))) return rc;
    if (dbeta != nullptr && (rc = launch_sum_parts(store.bpart, dbeta, N, (size_t)D, st))) return rc;
    if (dW != nullptr || dbias != nullptr) {
        const long long total = (dW != nullptr ? (long long)classes * D : 0) + classes;
        vit_classify_wgrad_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(dlogits, store.normed, dW, dbias, N, D,
                                                                                              classes);
        STGCN_LAUNCH_CHECK("vit_classify_wgrad_kernel");
    }
    return STGCN_OK;
}

namespace {

// `depth` blocks from `cur` to wherever the last one writes, between the buffers `cur` and `other`; returns that buffer in *out.
int run_stage(const BlockPlan &plan, const stgcn_vit_block_weights *blocks, int depth, const BlockStore &store, float eps,
              float scale, float *cur, float *other, float **out, int B, int L, int D, int heads, int hidden, hipStream_t st) {
    for (int i = 0; i < depth; ++i) {
        const stgcn_vit_block_weights &b = blocks[i];
        const BlockWeights w{b.norm1_weight, b.norm1_bias, b.Wqkv, b.bqkv, b.Wproj, b.bproj, b.norm2_weight, b.norm2_bias, b.W1, b.b1,
                             b.W2, b.b2};
        const int rc = block_forward(plan, cur, w, store, nullptr, nullptr, eps, scale, other, B, L, D, heads, hidden, st);
        if (rc) return rc;
        float *t = cur;
        cur = other;
        other = t;
    }
    *out = cur;
    return STGCN_OK;
}

bool blocks_present(const stgcn_vit_block_weights *blocks, int depth) {
    if (blocks == nullptr) return false;
    for (int i = 0; i < depth; ++i) {
        const stgcn_vit_block_weights &b = blocks[i];
        if (!BlockWeights{b.norm1_weight, b.norm1_bias, b.Wqkv, b.bqkv, b.Wproj, b.bproj, b.norm2_weight, b.norm2_bias, b.W1, b.b1,
                          b.W2, b.b2}.present())
            return false;
    }
    return true;
}

}  // namespace
}  // namespace vit
}  // namespace stgcn

using namespace stgcn;
using namespace stgcn::vit;

extern "C" {

int stgcn_vit_pool_supported(int S, int L, int D) { return pool_ok(S, L, D) ? 1 : 0; }

int stgcn_vit_pool(const float *x, float *out, int S, int L, int D, unsigned flags, void *stream) {
    if (flags & ~(unsigned)(STGCN_VIT_POOL_MAX | STGCN_VIT_POOL_CLS)) return fail(STGCN_ERR_ARG, "stgcn_vit_pool: unknown flag bits 0x%x", flags);
    if (pool_flags_clash(flags)) return fail(STGCN_ERR_ARG, "stgcn_vit_pool: STGCN_VIT_POOL_MAX and STGCN_VIT_POOL_CLS exclude each other");
    REQUIRE_PTR(x); REQUIRE_PTR(out);
    REQUIRE_POS(S); REQUIRE_POS(L); REQUIRE_POS(D);
    if (!aligned16(x) || !aligned16(out)) return fail(STGCN_ERR_ARG, "stgcn_vit_pool: x and out must be 16-byte aligned");
    if (!pool_ok(S, L, D)) return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_pool: D = %d (covered: D %% 4 == 0)", D);
    return launch_pool(x, out, S, L, D, (flags & STGCN_VIT_POOL_MAX) != 0, static_cast<hipStream_t>(stream),
                       (flags & STGCN_VIT_POOL_CLS) != 0);
}

int stgcn_vit_pool_classify_supported(int N, int L, int D, int classes) { return pool_classify_ok(N, L, D, classes) ? 1 : 0; }

int stgcn_vit_pool_classify(const float *x, const float *ln_weight, const float *ln_bias, float ln_eps, const float *W,
                            const float *bias, float *logits, int N, int L, int D, int classes, unsigned flags, void *stream) {
    if (flags & ~(unsigned)(STGCN_VIT_POOL_MAX | STGCN_VIT_POOL_CLS))
        return fail(STGCN_ERR_ARG, "stgcn_vit_pool_classify: unknown flag bits 0x%x", flags);
    if (pool_flags_clash(flags))
        return fail(STGCN_ERR_ARG, "stgcn_vit_pool_classify: STGCN_VIT_POOL_MAX and STGCN_VIT_POOL_CLS exclude each other");
    REQUIRE_PTR(x); REQUIRE_PTR(ln_weight); REQUIRE_PTR(ln_bias); REQUIRE_PTR(W); REQUIRE_PTR(logits);
    REQUIRE_POS(N); REQUIRE_POS(L); REQUIRE_POS(D); REQUIRE_POS(classes);
    if (!aligned16(x) || !aligned16(W)) return fail(STGCN_ERR_ARG, "stgcn_vit_pool_classify: x and W must be 16-byte aligned");
    if (!pool_classify_ok(N, L, D, classes))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_pool_classify: N = %d, D = %d (covered: D %% 64 == 0, D <= %d, N < 2^22 clips)",
                    N, D, kMaxLnDim);
    return launch_pool_classify(x, ln_weight, ln_bias, ln_eps, W, bias, logits, N, L, D, classes, (flags & STGCN_VIT_POOL_MAX) != 0,
                                static_cast<hipStream_t>(stream), (flags & STGCN_VIT_POOL_CLS) != 0);
}

static bool classify_backward_ok(int N, int L, int D, int classes, unsigned flags) {
    return !(flags & ~(unsigned)(STGCN_VIT_POOL_MAX | STGCN_VIT_POOL_CLS)) && !(flags & STGCN_VIT_POOL_MAX) &&
           pool_classify_ok(N, L, D, classes) && (long long)classes * D + classes < (1ll << 31) && (long long)L * D < (1ll << 31);
}

int stgcn_vit_pool_classify_backward_supported(int N, int L, int D, int classes, unsigned flags) {
    return classify_backward_ok(N, L, D, classes, flags) ? 1 : 0;
}

size_t stgcn_vit_pool_classify_backward_ws_bytes(int N, int L, int D, int classes, unsigned flags) {
    return classify_backward_ok(N, L, D, classes, flags) ? ClassifyBackwardStore(nullptr, N, D).total : 0;
}

int stgcn_vit_pool_classify_backward(const float *x, const float *ln_weight, const float *ln_bias, float ln_eps, const float *W,
                                     const float *dlogits, float *dx, float *dln_weight, float *dln_bias, float *dW, float *dbias,
                                     int N, int L, int D, int classes, void *ws, size_t ws_bytes, unsigned flags, void *stream) {
    if (flags & ~(unsigned)(STGCN_VIT_POOL_MAX | STGCN_VIT_POOL_CLS))
        return fail(STGCN_ERR_ARG, "stgcn_vit_pool_classify_backward: unknown flag bits 0x%x", flags);
    if (pool_flags_clash(flags))
        return fail(STGCN_ERR_ARG, "stgcn_vit_pool_classify_backward: STGCN_VIT_POOL_MAX and STGCN_VIT_POOL_CLS exclude each other");
    REQUIRE_PTR(x); REQUIRE_PTR(ln_weight); REQUIRE_PTR(ln_bias); REQUIRE_PTR(W); REQUIRE_PTR(dlogits); REQUIRE_PTR(ws);
    REQUIRE_POS(N); REQUIRE_POS(L); REQUIRE_POS(D); REQUIRE_POS(classes);
    if (!aligned16(x) || !aligned16(ws) || (dx != nullptr && !aligned16(dx)))
        return fail(STGCN_ERR_ARG, "stgcn_vit_pool_classify_backward: x, dx and ws must be 16-byte aligned");
    if (dx == x) return fail(STGCN_ERR_ARG, "stgcn_vit_pool_classify_backward: dx must not alias x");
    if (flags & STGCN_VIT_POOL_MAX)
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_pool_classify_backward: STGCN_VIT_POOL_MAX has no backward (covered: the "
                    "class token and the mean)");
    if (!classify_backward_ok(N, L, D, classes, flags))
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_vit_pool_classify_backward: D = %d, classes = %d (covered: D %% 64 == 0, D <= %d, "
                    "dW and a clip of dx below 2^31 elements)", D, classes, kMaxLnDim);
    const ClassifyBackwardStore store(ws, N, D);
    if (ws_bytes < store.total)
        return fail(STGCN_ERR_WORKSPACE, "stgcn_vit_pool_classify_backward: workspace %zu < %zu bytes", ws_bytes, store.total);
    return launch_pool_classify_backward(store, x, ln_weight, ln_bias, ln_eps, W, dlogits, dx, dln_weight, dln_bias, dW, dbias, N, L,
                                         D, classes, (flags & STGCN_VIT_POOL_CLS) != 0, static_cast<hipStream_t>(stream));
}

int stgcn_altformer_head_supported(const stgcn_altformer_head_shape *shape, unsigned flags1, unsigned flags2, unsigned head_flags) {
    if (shape == nullptr) return 0;
    const HeadPlan p = plan_head(*shape, flags1, flags2, head_flags);
    return !p.refusal && p.covered ? 1 : 0;
}

size_t stgcn_altformer_head_ws_bytes(const stgcn_altformer_head_shape *shape, unsigned flags1, unsigned flags2,
                                     unsigned head_flags) {
    if (shape == nullptr) return 0;
    const HeadPlan p = plan_head(*shape, flags1, flags2, head_flags);
    return !p.refusal && p.covered ? HeadStore(nullptr, p, *shape).total : 0;
}

int stgcn_altformer_head_forward(const float *z, const stgcn_altformer_head_weights *weights,
                                 const stgcn_altformer_head_shape *shape, float eps_blocks, float eps_head, float scale1,
                                 float scale2, void *ws, size_t ws_bytes, float *logits, unsigned flags1, unsigned flags2,
                                 unsigned head_flags, void *stream) {
    REQUIRE_PTR(shape);
    const stgcn_altformer_head_shape &s = *shape;
    const HeadPlan p = plan_head(s, flags1, flags2, head_flags);
    if (p.refusal) return fail(STGCN_ERR_ARG, "stgcn_altformer_head_forward: %s (got 0x%x)", p.refusal, head_flags);
    if (p.stage1.refusal) return block_refused(p.stage1);
    if (p.stage2.refusal) return block_refused(p.stage2);
    REQUIRE_PTR(z); REQUIRE_PTR(weights); REQUIRE_PTR(ws); REQUIRE_PTR(logits);
    if (!p.shaped) return fail(STGCN_ERR_ARG, "stgcn_altformer_head_forward: every field of the shape must be positive");
    const stgcn_altformer_head_weights &w = *weights;
    if (!w.embed1_weight || !w.embed1_bias || !w.embed2_weight || !w.embed2_bias || !w.head_norm_weight || !w.head_norm_bias ||
        !w.head_weight || !blocks_present(w.blocks1, s.depth1) || !blocks_present(w.blocks2, s.depth2))
        return fail(STGCN_ERR_ARG, "stgcn_altformer_head_forward: null pointer among the weights");
    if (!aligned16(ws) || !aligned16(w.head_weight))
        return fail(STGCN_ERR_ARG, "stgcn_altformer_head_forward: ws and head_weight must be 16-byte aligned");
    if (!p.stage1.covered) return block_unsupported(p.stage1, p.L1, s.E1, s.heads, s.hidden1, flags1);
    if (!p.stage2.covered) return block_unsupported(p.stage2, p.L2, s.E2, s.heads, s.hidden2, flags2);
    if (!p.covered)
        return fail(STGCN_ERR_UNSUPPORTED, "stgcn_altformer_head_forward: N = %d, E1 = %d, E2 = %d (covered: N <= 65535 clips, "
                    "fewer than 2^31 stage-1 sequences, E1 %% 4 == 0, E2 %% 64 == 0, E2 <= %d)", s.N, s.E1, s.E2, kMaxLnDim);
    const HeadStore store(ws, p, s);
    if (ws_bytes < store.total)
        return fail(STGCN_ERR_WORKSPACE, "stgcn_altformer_head_forward: workspace %zu < %zu bytes", ws_bytes, store.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    float *y1 = nullptr, *y2 = nullptr;
    if ((rc = launch_patch_embed(z, w.embed1_weight, w.embed1_bias, w.pos1, store.a1, s.N, s.C, s.E1, s.T, s.V, p.embed_flags, st)))
        return rc;
    const BlockStore bs1(store.block, p.stage1, p.B1, p.L1, s.E1, s.hidden1);
    if ((rc = run_stage(p.stage1, w.blocks1, s.depth1, bs1, eps_blocks, scale1, store.a1, store.b1, &y1, p.B1, p.L1, s.E1, s.heads,
                        s.hidden1, st)))
        return rc;
    if ((rc = launch_pool(y1, store.pooled, p.B1, p.L1, s.E1, p.pool1_max, st))) return rc;
    // the second embedding: per clip one "frame" of L2 rows, channels last, the position table indexed by the row
    if ((rc = launch_patch_embed(store.pooled, w.embed2_weight, w.embed2_bias, w.pos2, store.a2, s.N, s.E1, s.E2, 1, p.L2,
                                 STGCN_IN_NTVC, st)))
        return rc;
    const BlockStore bs2(store.block, p.stage2, s.N, p.L2, s.E2, s.hidden2);
    if ((rc = run_stage(p.stage2, w.blocks2, s.depth2, bs2, eps_blocks, scale2, store.a2, store.b2, &y2, s.N, p.L2, s.E2, s.heads,
                        s.hidden2, st)))
        return rc;
    return launch_pool_classify(y2, w.head_norm_weight, w.head_norm_bias, eps_head, w.head_weight, w.head_bias, logits, s.N, p.L2,
                                s.E2, s.classes, p.pool2_max, st);
}

}  // extern "C"
