// The fp32 weight-gradient kernel of a token-major linear (vit_backward.hip describes the tiling), in a header because two
// translation units launch it: vit_backward.hip on dense rows (every linear of the blocks) and vit_patch_backward.hip on the
// ST-ViT head's patch embedding, whose A operand is the stem output read in place and whose dY rows skip the class rows.
// What differs between the two is where a token's row of each operand lies: the `Rows` policy below.  Everything else -
// staging, LDS layout, fragments, MFMA order, the bias column sums, the slabs - is one piece of code.
#pragma once

#include "vit_linear_kernel.h"

namespace stgcn {
namespace vit {
namespace wgrad_kernel {

using bf16k::f32x16;
using linear_kernel::PatchRows;

constexpr int WT = 128, WC = kWgradChunk, WLD = 160;   // tile edge, tokens per chunk, LDS row stride (floats)

__device__ __forceinline__ float4 load_row4(const float *p, int c, int width, bool vec) {
    if (c >= width) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) return *reinterpret_cast<const float4 *>(p + c);
    float4 v;
    v.x = p[c];
    v.y = c + 1 < width ? p[c + 1] : 0.f;
    v.z = c + 2 < width ? p[c + 2] : 0.f;
    v.w = c + 3 < width ? p[c + 3] : 0.f;
    return v;
}

// DenseWgradRows: dY is (M, Nout) and A is (M, K), both row-major; token m is row m of both.
struct DenseWgradRows {
    static constexpr bool kPatch = false;
};
// PatchWgradRows: token m = i n + p is patch p of clip i.  Its A row is that patch of the (N, T, V, C) stem output, read in
// place (PatchRows::row_base / col: p1 runs of p2 C floats; a thread's four columns never cross a run, (p2 C) % 4 == 0), and
// its dY row is row i (n + 1) + 1 + p of the (N, n + 1, Nout) gradient of the embedding's output: the class rows are skipped.
struct PatchWgradRows {
    static constexpr bool kPatch = true;
    PatchRows rows;
    __device__ __forceinline__ size_t dy_row(int m) const { return (size_t)m + m / rows.n + 1; }
};

template <class R>
__global__ __launch_bounds__(256) void vit_wgrad_kernel(const float *__restrict__ dY, const float *__restrict__ A,
                                                       const float *__restrict__ rowscale, int L, float *__restrict__ part,
                                                       float *__restrict__ bpart, int M, int K, int Nout, int tiles_n,
                                                       int tiles_k, int rows_per_split, const R pol) {
    __shared__ __attribute__((aligned(16))) float ld[WC * WLD], la[WC * WLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
    const int tile = (int)blockIdx.x % (tiles_n * tiles_k), split = (int)blockIdx.x / (tiles_n * tiles_k);
    const int n0 = (tile / tiles_k) * WT, k0 = (tile % tiles_k) * WT;
    const int r_lo = split * rows_per_split, r_hi = min(M, r_lo + rows_per_split);
    const int sr = tid >> 5, sc = (tid & 31) * 4;       // staging: rows sr + 8 i of the chunk, floats sc .. sc + 3 of the tile
    const bool vec_n = (Nout & 3) == 0;
    const bool with_bias = bpart != nullptr && k0 == 0;
    int acol = 0;                                       // PatchWgradRows: where the thread's four columns lie inside a patch
    if constexpr (R::kPatch) acol = k0 + sc < K ? pol.rows.col(k0 + sc) : 0;

    float4 gd[4], ga[4];
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto gload = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + sr + 8 * i;
            if (row < r_hi) {
                size_t drow = (size_t)row;
                if constexpr (R::kPatch) drow = pol.dy_row(row);
                float4 d = load_row4(dY + drow * Nout, n0 + sc, Nout, vec_n);
                if (rowscale != nullptr) {
                    const float s = rowscale[row / L];
                    d.x *= s, d.y *= s, d.z *= s, d.w *= s;
                }
                gd[i] = d;
                if constexpr (R::kPatch)
                    ga[i] = k0 + sc < K ? *reinterpret_cast<const float4 *>(A + pol.rows.row_base(row) + acol)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
                else
                    ga[i] = load_row4(A + (size_t)row * K, k0 + sc, K, true);
            } else {
                gd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                ga[i] = gd[i];
            }
        }
    };
    auto sstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4 *>(&ld[(sr + 8 * i) * WLD + sc]) = gd[i];
            *reinterpret_cast<float4 *>(&la[(sr + 8 * i) * WLD + sc]) = ga[i];
            bsum.x += gd[i].x, bsum.y += gd[i].y, bsum.z += gd[i].z, bsum.w += gd[i].w;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;

    if (r_lo < r_hi) {
        gload(r_lo);
        sstore();
    }
    __syncthreads();
    for (int r0 = r_lo; r0 < r_hi; r0 += WC) {
        const bool more = r0 + WC < r_hi;
        if (more) gload(r0 + WC);
#pragma unroll
        for (int s = 0; s < WC / 2; ++s) {
            const float *dp = &ld[(2 * s + half) * WLD + wm * 64 + l31], *ap = &la[(2 * s + half) * WLD + wn * 64 + l31];
            const float d0 = dp[0], d1 = dp[32], a0 = ap[0], a1 = ap[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, a0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(d0, a1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, a0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(d1, a1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            sstore();
            __syncthreads();
        }
    }

    // lane holds column k = l31 of each 32 x 32 block, rows (= output features n) 8 (i / 4) + 4 half + i % 4
    float *out = part + (size_t)split * Nout * K;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int col = k0 + wn * 64 + n * 32 + l31;
        if (col >= K) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = n0 + wm * 64 + m * 32 + 8 * (i >> 2) + 4 * half + (i & 3);
                if (row < Nout) out[(size_t)row * K + col] = acc[m][n][i];
            }
    }
    if (with_bias) {   // (uniform over the workgroup) the 8 staging rows of a column, added in the order 0 .. 7
        *reinterpret_cast<float4 *>(&ld[sr * WLD + sc]) = bsum;
        __syncthreads();
        if (tid < WT && n0 + tid < Nout) {
            float t = ld[tid];
#pragma unroll
            for (int r = 1; r < 8; ++r) t += ld[r * WLD + tid];
            bpart[(size_t)split * Nout + n0 + tid] = t;
        }
    }
}

}  // namespace wgrad_kernel
}  // namespace vit
}  // namespace stgcn
