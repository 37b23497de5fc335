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

constexpr int WT = 128, WC = kWgradChunk;   // the large form's tile edge, tokens per chunk
// The LDS row stride (floats) of a form of tile edge T: 160 for the 128 form, as it always was, and 64, no padding, for the
// 64 form.  Neither the fragment reads nor the staging stores depend on it (the bank rule is the one of the bf16 kernel's
// header: 32 banks of 4 bytes for ds_read_b32 and every ds_write, conflicts only inside a lane group):
//   reads : ds_read_b32 in two groups of 32 lanes; a group reads the 32 CONSECUTIVE floats row * stride + c + l31 of one
//           chunk row (`half` picks the row and is constant in a group), 32 different banks whatever the stride;
//   writes: ds_write_b128 in groups of eight consecutive lanes; T / 4 = 32 or 16 threads stage a row, a multiple of eight, so
//           a group writes 128 contiguous bytes of one row: the 32 banks once each, for every stride that is a multiple of 4.
// So the narrower image is dense: 2 x 32 x 64 floats = 16 KB against the 128 form's 40 KB.
template <int T>
constexpr int wld() { return T == 128 ? 160 : T; }

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

// `T`: the edge of the workgroup's tile of dW, 128 (each of the 4 waves holds 2 x 2 accumulator blocks of 32 x 32) or 64 (one
// block each; four times the workgroups per split, for calls whose token count cannot supply them: plan_wgrad in vit.h).
// Split `s` covers the chunks [s cps + min(s, long_splits), ...) of cps (+ 1 for the first long_splits splits) chunks:
// long_splits = 0 is the uniform cut of wgrad_rows_per_split.
template <class R, int T = WT>
__global__ __launch_bounds__(256) void vit_wgrad_kernel(const float *__restrict__ dY, const float *__restrict__ A,
                                                       const float *__restrict__ rowscale, int L, float *__restrict__ part,
                                                       float *__restrict__ bpart, int M, int K, int Nout, int tiles_n,
                                                       int tiles_k, int cps, int long_splits, const R pol) {
    static_assert(T == 128 || T == 64, "two forms");
    constexpr int WLD = wld<T>(), NB = T / 64;          // LDS row stride; 32 x 32 blocks per wave and dimension
    constexpr int TPR = T / 4, RS = 256 / TPR, NI = WC / RS;   // staging: threads per chunk row, rows per pass, passes
    __shared__ __attribute__((aligned(16))) float ld[WC * WLD], la[WC * WLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
    const int tile = (int)blockIdx.x % (tiles_n * tiles_k), split = (int)blockIdx.x / (tiles_n * tiles_k);
    const int n0 = (tile / tiles_k) * T, k0 = (tile % tiles_k) * T;
    const int r_lo = (split * cps + min(split, long_splits)) * WC;
    const int r_hi = min(M, r_lo + (cps + (split < long_splits ? 1 : 0)) * WC);
    const int sr = tid / TPR, sc = (tid % TPR) * 4;     // staging: rows sr + RS i of the chunk, floats sc .. sc + 3 of the tile
    const bool vec_n = (Nout & 3) == 0;
    const bool with_bias = bpart != nullptr && k0 == 0;
    int acol = 0;                                       // PatchWgradRows: where the thread's four columns lie inside a patch
    if constexpr (R::kPatch) acol = k0 + sc < K ? pol.rows.col(k0 + sc) : 0;

    float4 gd[NI], ga[NI];
    float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
    auto gload = [&](int r0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int row = r0 + sr + RS * i;
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
        for (int i = 0; i < NI; ++i) {
            *reinterpret_cast<float4 *>(&ld[(sr + RS * i) * WLD + sc]) = gd[i];
            *reinterpret_cast<float4 *>(&la[(sr + RS * i) * WLD + sc]) = ga[i];
            bsum.x += gd[i].x, bsum.y += gd[i].y, bsum.z += gd[i].z, bsum.w += gd[i].w;
        }
    };

    f32x16 acc[NB][NB];
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n)
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
            const float *dp = &ld[(2 * s + half) * WLD + wm * (T / 2) + l31], *ap = &la[(2 * s + half) * WLD + wn * (T / 2) + l31];
            float d[NB], a[NB];
#pragma unroll
            for (int m = 0; m < NB; ++m) d[m] = dp[32 * m], a[m] = ap[32 * m];
#pragma unroll
            for (int m = 0; m < NB; ++m)
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(d[m], a[n], acc[m][n], 0, 0, 0);
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
    for (int n = 0; n < NB; ++n) {
        const int col = k0 + wn * (T / 2) + n * 32 + l31;
        if (col >= K) continue;
#pragma unroll
        for (int m = 0; m < NB; ++m)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = n0 + wm * (T / 2) + m * 32 + 8 * (i >> 2) + 4 * half + (i & 3);
                if (row < Nout) out[(size_t)row * K + col] = acc[m][n][i];
            }
    }
    if (with_bias) {   // (uniform over the workgroup) the RS staging rows of a column, added in the order 0 .. RS - 1
        *reinterpret_cast<float4 *>(&ld[sr * WLD + sc]) = bsum;
        __syncthreads();
        if (tid < T && n0 + tid < Nout) {
            float t = ld[tid];
#pragma unroll
            for (int r = 1; r < RS; ++r) t += ld[r * WLD + tid];
            bpart[(size_t)split * Nout + n0 + tid] = t;
        }
    }
}

}  // namespace wgrad_kernel
}  // namespace vit
}  // namespace stgcn
