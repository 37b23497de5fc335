// The tile kernel of the token-major linear (vit_linear.hip describes the tiling, the arithmetics and the tile forms), in a
// header because three translation units launch it: vit_linear.hip on dense rows (every linear of the blocks),
// vit_patch.hip on the patches of the ST-ViT head's embedding, which it reads straight from the stem output, and
// vit_patch_backward.hip for that embedding's input gradient, which it stores straight into the stem output's layout.  What
// differs between them is where a row of the A operand lies, which part of the contraction a workgroup walks and where an
// element of Y is stored: the `Rows` policy below.  Everything else - staging, LDS layout, fragments, MFMA order, epilogue - is one piece of code.
#pragma once

#include "bf16_common.h"
#include "vit.h"

namespace stgcn {
namespace vit {
namespace linear_kernel {

using bf16k::bf16_hi_to_f32;
using bf16k::bf16_lo_to_f32;
using bf16k::f32x16;
using bf16k::FragB;
using bf16k::pack_bf16x2;


constexpr int KC = 32;
constexpr int LDF = KC + 4;  // fp32 tile row stride, floats
constexpr int LDH = KC + 8;  // bf16 tile row stride, elements (80 bytes)

__device__ __forceinline__ void split4(const float4 v, uint2 &hi, uint2 &lo) {
    hi.x = pack_bf16x2(v.x, v.y);
    hi.y = pack_bf16x2(v.z, v.w);
    lo.x = pack_bf16x2(v.x - bf16_lo_to_f32(hi.x), v.y - bf16_hi_to_f32(hi.x));
    lo.y = pack_bf16x2(v.z - bf16_lo_to_f32(hi.y), v.w - bf16_hi_to_f32(hi.y));
}

// A workgroup of WAVES waves, two of them side by side along Nout, each owning WM x WN blocks of 32 x 32.
template <int WAVES_, int WM_, int WN_>
struct Form {
    static constexpr int WAVES = WAVES_, WM = WM_, WN = WN_;
    static constexpr int THREADS = 64 * WAVES;
    static constexpr int BM = (WAVES / 2) * WM * 32, BN = 2 * WN * 32;
    static constexpr int RS = THREADS / 8;            // rows staged per pass: 8 threads, one float4 each, per 32-float row
    static constexpr int PA = BM / RS, PB = BN / RS;  // passes over the A and the B tile
    static constexpr int PMAX = PA > PB ? PA : PB;
    static_assert(WAVES % 2 == 0 && BM % RS == 0 && BN % RS == 0 && WM == WN, "tile form");
};
using Form128 = Form<4, 2, 2>;   // 128 x 128
using Form64 = Form<4, 1, 1>;    //  64 x  64
using Form32 = Form<2, 1, 1>;    //  32 x  64

template <int MATH, int BM, int BN>
struct Tiles;
template <int BM, int BN>
struct Tiles<STGCN_MATH_F32, BM, BN> {
    float a[BM * LDF];
    float b[BN * LDF];
};
template <int BM, int BN>
struct Tiles<STGCN_MATH_BF16X3, BM, BN> {
    unsigned short ah[BM * LDH], al[BM * LDH];
    unsigned short bh[BN * LDH], bl[BN * LDH];
};

template <int BM, int BN>
struct Tiles<STGCN_MATH_BF16, BM, BN> {
    unsigned short ah[BM * LDH];
    unsigned short bh[BN * LDH];
};

// Where the rows of the A operand lie, and which part of the contraction and of Y a workgroup owns.
// DenseRows: X is (M, kx) row-major, every workgroup walks all of K and writes Y as given (grid.y = 1).
struct DenseRows {
    static constexpr bool kPatch = false, kPatchStore = false;
};
// PatchRows: row r = (clip i, patch a, b) of the (N, T, V, C) tensor X cut into p1 x p2 patches (n = h w of them per clip, w
// along V); column k = (f p2 + j) C + c is X[i][a p1 + f][b p2 + j][c], so a patch is p1 runs of `run` = p2 C contiguous floats,
// `frame` = V C apart, and a chunk of KC columns never crosses a run (run % KC == 0, the coverage rule).  The contraction is
// cut over grid.y: workgroup y walks the chunks [y cps, (y + 1) cps) and writes its sums to slab y of Y (M Nout floats each),
// which the caller adds up in slab order.  No LayerNorm, X fp32.
struct PatchRows {
    static constexpr bool kPatch = true, kPatchStore = false;
    int n, w, run, frame, patch_rows, clip;   // patch_rows = p1 V C (one row of patches), clip = T V C
    int cps;                                   // chunks per slab
    __device__ __forceinline__ size_t row_base(int row) const {
        const int i = row / n, p = row - i * n, a = p / w, b = p - a * w;
        return (size_t)i * clip + (size_t)a * patch_rows + (size_t)b * run;
    }
    __device__ __forceinline__ int col(int k) const {
        const int f = k / run;
        return f * frame + (k - f * run);
    }
};

// PatchGradRows: the input gradient of that embedding, dz = dx_tokens W, as this linear on the transposed weight.  Row
// m = i n + p of the A operand is row i (n + 1) + 1 + p of the (N, n + 1, kx) gradient X (the class rows are skipped), every
// workgroup walks all of K, and element (m, col) of Y is stored where column `col` of patch m lies in the (N, T, V, C) tensor
// (`to`): 32 consecutive columns lie inside one run, so a half-wave's store stays 128 contiguous bytes, and every element of
// that tensor belongs to exactly one (m, col), so the launch writes it whole.  No LayerNorm, fp32 on both sides, and none of
// the epilogue's optional operands (bias, R, LinearExtra's pointers), which are indexed as a dense Y.
struct PatchGradRows {
    static constexpr bool kPatch = false, kPatchStore = true;
    PatchRows to;
    __device__ __forceinline__ size_t src_row(int m) const { return (size_t)m + m / to.n + 1; }
};

// XB / YB (bf16 arithmetic only): X / Y point at bf16 storage, not fp32.
template <int MATH, class F, bool XB = false, bool YB = false, class A = DenseRows>
__global__ __launch_bounds__(F::THREADS) void vit_linear_kernel(const void *__restrict__ Xv, const float *__restrict__ W,
                                                        const float *__restrict__ bias, const float *R,
                                                        const float *__restrict__ gamma, const float *__restrict__ beta,
                                                        float eps, void *Yv, int M, int K, int Nout, int tiles_n,
                                                        int gelu, const LinearExtra ex, const A rows) {
    static_assert(MATH == STGCN_MATH_BF16 || (!XB && !YB), "bf16 storage goes with the bf16 arithmetic");
    static_assert(!A::kPatch || !XB, "patches are read from fp32");
    static_assert(!A::kPatchStore || (!XB && !YB), "the patches' gradient is fp32 on both sides");
    constexpr int BM = F::BM, BN = F::BN, RS = F::RS, PA = F::PA, PB = F::PB, WM = F::WM, WN = F::WN;
    const float *__restrict__ X = static_cast<const float *>(Xv);                      // !XB
    const unsigned short *__restrict__ Xh = static_cast<const unsigned short *>(Xv);   // XB
    float *Y = static_cast<float *>(Yv);
    __shared__ __attribute__((aligned(16))) Tiles<MATH, BM, BN> lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = ((int)blockIdx.x % tiles_n) * BN, m0 = ((int)blockIdx.x / tiles_n) * BM;
    const int lr = tid >> 3, lc = (tid & 7) * 4;   // staging: rows lr + RS i, floats lc .. lc + 3 of the chunk
    const int l31 = lane & 31, half = lane >> 5;

    // LayerNorm statistics of the tile's BM rows, workgroup-local: the 8 threads that stage a row read it once (K is the
    // whole row; it is about to be read again for the A tiles, so this pass mostly primes the cache), sum x - c and
    // (x - c)^2 with c = the row's first element (no cancellation for rows with a large offset), and combine with three
    // exchanges in a fixed order.  Every workgroup of a row slab repeats this; it replaces a pre-pass and its buffer.
    const bool ln = !XB && !A::kPatch && !A::kPatchStore && gamma != nullptr;   // (a LayerNorm of bf16 rows is refused at the entry point)
    float mean[PA], rstd[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int row = m0 + lr + RS * i;
        float s = 0.f, q = 0.f, c = 0.f;
        if (ln && row < M) {
            const float4 *p = reinterpret_cast<const float4 *>(X + (size_t)row * K);
            c = X[(size_t)row * K];
            for (int j = tid & 7; j < (K >> 2); j += 8) {
                const float4 v = p[j];
                const float a = v.x - c, b = v.y - c, d = v.z - c, e = v.w - c;
                s += (a + b) + (d + e);
                q += (a * a + b * b) + (d * d + e * e);
            }
        }
#pragma unroll
        for (int o = 1; o <= 4; o <<= 1) {
            s += __shfl_xor(s, o, 64);
            q += __shfl_xor(q, o, 64);
        }
        const float ms = s / (float)K;
        mean[i] = c + ms;
        rstd[i] = 1.0f / sqrtf(fmaxf(q / (float)K - ms * ms, 0.f) + eps);
    }

    const int kx = ex.kx > 0 ? ex.kx : K;   // X's row length: K, or (backward) a length that is no multiple of KC, zero-padded
    float4 xa[XB ? 1 : PA], wb[PB];
    size_t xrow[A::kPatch ? PA : 1];   // PatchRows: where each staged row's patch starts
    if constexpr (A::kPatch) {
#pragma unroll
        for (int i = 0; i < PA; ++i) xrow[i] = rows.row_base(m0 + lr + RS * i < M ? m0 + lr + RS * i : 0);
        Y += (size_t)blockIdx.y * M * Nout;
    }
    uint2 xh[XB ? PA : 1];   // XB: four bf16 of the row, as stored
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < F::PMAX; ++i) {
            const int row = m0 + lr + RS * i, n = n0 + lr + RS * i;
            if constexpr (XB) {
                if (i < PA)
                    xh[i] = row < M ? *reinterpret_cast<const uint2 *>(Xh + (size_t)row * K + k0 + lc) : make_uint2(0u, 0u);
            } else if constexpr (A::kPatch) {
                if (i < PA)
                    xa[i] = row < M ? *reinterpret_cast<const float4 *>(X + xrow[i] + rows.col(k0) + lc)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
            } else if constexpr (A::kPatchStore) {
                if (i < PA)
                    xa[i] = row < M && k0 + lc < kx ? *reinterpret_cast<const float4 *>(X + rows.src_row(row) * kx + k0 + lc)
                                                    : make_float4(0.f, 0.f, 0.f, 0.f);
            } else if (i < PA)
                xa[i] = row < M && k0 + lc < kx ? *reinterpret_cast<const float4 *>(X + (size_t)row * kx + k0 + lc)
                                                : make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < PB)
                wb[i] = n < Nout ? *reinterpret_cast<const float4 *>(W + (size_t)n * K + k0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto sstore = [&](int k0) {
        float4 g = make_float4(1.f, 1.f, 1.f, 1.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ln) {
            g = *reinterpret_cast<const float4 *>(gamma + k0 + lc);
            b = *reinterpret_cast<const float4 *>(beta + k0 + lc);
        }
#pragma unroll
        for (int i = 0; i < F::PMAX; ++i) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!XB && i < PA) {
                v = xa[XB ? 0 : i];
                if (ln) {
                    v.x = (v.x - mean[i]) * rstd[i] * g.x + b.x;
                    v.y = (v.y - mean[i]) * rstd[i] * g.y + b.y;
                    v.z = (v.z - mean[i]) * rstd[i] * g.z + b.z;
                    v.w = (v.w - mean[i]) * rstd[i] * g.w + b.w;
                }
            }
            const int r = lr + RS * i;
            if constexpr (MATH == STGCN_MATH_F32) {
                if (i < PA) *reinterpret_cast<float4 *>(&lds.a[r * LDF + lc]) = v;
                if (i < PB) *reinterpret_cast<float4 *>(&lds.b[r * LDF + lc]) = wb[i];
            } else if constexpr (MATH == STGCN_MATH_BF16) {
                if (i < PA)
                    *reinterpret_cast<uint2 *>(&lds.ah[r * LDH + lc]) =
                        XB ? xh[XB ? i : 0] : make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                if (i < PB)
                    *reinterpret_cast<uint2 *>(&lds.bh[r * LDH + lc]) =
                        make_uint2(pack_bf16x2(wb[i].x, wb[i].y), pack_bf16x2(wb[i].z, wb[i].w));
            } else {
                uint2 hi, lo;
                if (i < PA) {
                    split4(v, hi, lo);
                    *reinterpret_cast<uint2 *>(&lds.ah[r * LDH + lc]) = hi;
                    *reinterpret_cast<uint2 *>(&lds.al[r * LDH + lc]) = lo;
                }
                if (i < PB) {
                    split4(wb[i], hi, lo);
                    *reinterpret_cast<uint2 *>(&lds.bh[r * LDH + lc]) = hi;
                    *reinterpret_cast<uint2 *>(&lds.bl[r * LDH + lc]) = lo;
                }
            }
        }
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;

    int c0 = 0, chunks = K / KC;   // this workgroup's chunks [c0, chunks)
    if constexpr (A::kPatch) {
        c0 = (int)blockIdx.y * rows.cps;
        chunks = c0 + rows.cps < chunks ? c0 + rows.cps : chunks;
    }
    gload(c0 * KC);
    sstore(c0 * KC);
    __syncthreads();
    for (int c = c0; c < chunks; ++c) {
        const bool more = c + 1 < chunks;
        if (more) gload((c + 1) * KC);
        if constexpr (MATH == STGCN_MATH_F32) {
            float a[WM][16], b[WN][16];
#pragma unroll
            for (int m = 0; m < WM; ++m) {   // WM == WN: one loop reads both operands' fragments
                const float4 *ap = reinterpret_cast<const float4 *>(&lds.a[(wm * (32 * WM) + m * 32 + l31) * LDF + half * 16]);
                const float4 *bp = reinterpret_cast<const float4 *>(&lds.b[(wn * (32 * WN) + m * 32 + l31) * LDF + half * 16]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 va = ap[j], vb = bp[j];
                    a[m][4 * j] = va.x, a[m][4 * j + 1] = va.y, a[m][4 * j + 2] = va.z, a[m][4 * j + 3] = va.w;
                    b[m][4 * j] = vb.x, b[m][4 * j + 1] = vb.y, b[m][4 * j + 2] = vb.z, b[m][4 * j + 3] = vb.w;
                }
            }
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int m = 0; m < WM; ++m)
#pragma unroll
                    for (int n = 0; n < WN; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m][s], b[n][s], acc[m][n], 0, 0, 0);
        } else if constexpr (MATH == STGCN_MATH_BF16) {
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                FragB<1, WM> fa;
                FragB<1, WN> fb;
#pragma unroll
                for (int m = 0; m < WM; ++m) {   // WM == WN: one loop reads both operands' fragments
                    fa.hi[m] = *reinterpret_cast<const uint4 *>(&lds.ah[(wm * (32 * WM) + m * 32 + l31) * LDH + ks * 16 + half * 8]);
                    fb.hi[m] = *reinterpret_cast<const uint4 *>(&lds.bh[(wn * (32 * WN) + m * 32 + l31) * LDH + ks * 16 + half * 8]);
                }
                bf16k::mfma_kstep_bf16<1, WM, WN>(acc, fa, fb);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                FragB<3, WM> fa;
                FragB<3, WN> fb;
#pragma unroll
                for (int m = 0; m < WM; ++m) {   // WM == WN: one loop reads both operands' fragments
                    const int ao = (wm * (32 * WM) + m * 32 + l31) * LDH + ks * 16 + half * 8;
                    const int bo = (wn * (32 * WN) + m * 32 + l31) * LDH + ks * 16 + half * 8;
                    fa.hi[m] = *reinterpret_cast<const uint4 *>(&lds.ah[ao]);
                    fa.lo[m] = *reinterpret_cast<const uint4 *>(&lds.al[ao]);
                    fb.hi[m] = *reinterpret_cast<const uint4 *>(&lds.bh[bo]);
                    fb.lo[m] = *reinterpret_cast<const uint4 *>(&lds.bl[bo]);
                }
                bf16k::mfma_kstep_bf16<3, WM, WN>(acc, fa, fb);
            }
        }
        __syncthreads();
        if (more) {
            sstore((c + 1) * KC);
            __syncthreads();
        }
    }

    // epilogue: lane holds column n = l31 of each 32 x 32 block, rows 8 (i / 4) + 4 half + i % 4
    constexpr float kRsqrt2 = 0.70710678118654752440f;
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int col = n0 + wn * (32 * WN) + n * 32 + l31;
        if (col >= Nout) continue;
        const float bv = bias != nullptr ? bias[col] : 0.f;
#pragma unroll
        for (int m = 0; m < WM; ++m) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = m0 + wm * (32 * WM) + m * 32 + 8 * (i >> 2) + 4 * half + (i & 3);
                if (row >= M) continue;
                float v = acc[m][n][i] + bv;
                if constexpr (A::kPatchStore) {
                    Y[rows.to.row_base(row) + rows.to.col(col)] = v;
                    continue;
                }
                const size_t idx = (size_t)row * Nout + col;
                if (ex.pre != nullptr) ex.pre[idx] = v;
                if (gelu) {
                    // bf16 arithmetic: the erfc form, accurate RELATIVE to the result in the negative tail too (1 + erff cancels
                    // there: GELU(-4) = -1.3e-4 comes out with 1e-3 relative error), because a bf16 store rounds relative to
                    // the value; the other arithmetics keep the form their results were pinned with
                    if constexpr (MATH == STGCN_MATH_BF16) v = 0.5f * v * erfcf(-v * kRsqrt2);
                    else v = 0.5f * v * (1.0f + erff(v * kRsqrt2));
                }
                if (ex.dgelu != nullptr) {   // d GELU / dh = Phi(h) + h phi(h)
                    const float h = ex.dgelu[idx];
                    v *= 0.5f * (1.0f + erff(h * kRsqrt2)) + h * 0.39894228040143267794f * __expf(-0.5f * h * h);
                }
                if (ex.mask != nullptr) v *= ex.mask[idx];
                if (ex.rowscale != nullptr) v *= ex.rowscale[row / ex.L];
                if (R != nullptr) v += R[idx];
                if constexpr (YB) bf16k::store_out<true>(Yv, idx, v);
                else Y[idx] = v;
            }
        }
    }
}

}  // namespace linear_kernel
}  // namespace vit
}  // namespace stgcn
