// Weights times channel-first activations on the bf16 matrix cores, in the three-term split arithmetic (STGCN_MATH_BF16X3):
//
//   C[n][m][j] = sum_k W[m][k] . X[n][k][j]  (+ bias[m])  (+ R[n][m][j]),     n < N, m < M, j < TV
//
// W (M, K) row-major, or (K, M) with `wt` (the input gradient through the weights); X[n] (K, TV), C[n] and R[n] (M, TV) dense
// with TV contiguous.  The products of ST-TR's attention unit (st_attention.hip: qkv, out and their two input gradients).
// Every fp32 operand is split once, where it is staged, into wh = bf16(w), wl = bf16(w - wh) (bf16_common.h's split8), and
//   C = sum  wh.xl + wl.xh + wh.xh     on v_mfma_f32_16x16x32_bf16, fp32 accumulators, no wl.xl,
// in bf16_common.h's product order.  One k-step of that instruction is the K chunk (32).
//
// Tile: 32*MB rows x 128 columns of one clip per workgroup of 4 waves (2 x 2: a wave owns 16*MB rows x 64 columns = MB x 4
// accumulator blocks), MB = 4 (128 rows) or 2 (64 rows, for M whose last 128-row tile would be less than half full: 192, 131).
//
// Staging is where the transposition happens: the memory-contiguous index of X is the column j, the fragment-contiguous
// index of the MFMA is k.  A staging unit is (row, 8 consecutive k): 8 dword loads (for X coalesced along j across the
// lanes, for W along m when it is given as (K, M); a W given as (M, K) with 16-byte aligned rows takes its 8 k as two 16-byte
// loads instead, any other as dwords along k), one split8, one 16-byte LDS write of the hi and one of the lo image.  Both
// images are [row][32 k] bf16 (64 bytes a row) with the four 16-byte pieces of a row XORed by (row >> 2) & 3, so that the 16
// lanes of an LDS pass (16 consecutive rows, one piece) cover all 64 banks in the staging writes and the fragment reads alike.
// Dword loads and stores of X, R and C carry no alignment demand, so rows of TV*4 bytes that are no multiple of 16 (TV = 75,
// 110) take the same path as aligned ones.  Everything outside the operands - k >= K, j >= TV, m >= M - is staged as zeros by predicate and
// never loaded; tail outputs are not stored.
//
// The global loads of chunk c+1 are issued before the MFMAs of chunk c and land in registers; one LDS buffer, two barriers a
// chunk; latency is hidden by the other workgroups of the CU (32 KiB of LDS each).  Fixed summation order, no atomics.
#include "bf16_common.h"

namespace stgcn {

namespace {

using namespace bf16k;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kBN = 128;    // columns of a tile
constexpr int kKC = 32;     // contraction chunk: one k-step
constexpr int kRowB = 64;   // bytes of an image row (32 bf16)

// byte offset of piece g (8 k) of row r
__device__ __forceinline__ int img_off(int r, int g) { return r * kRowB + ((g ^ ((r >> 2) & 3)) << 4); }

template <int MB>
__global__ __launch_bounds__(256) void wx_bf16x3_kernel(const float *__restrict__ W, const float *__restrict__ X,
                                                        const float *__restrict__ bias, const float *__restrict__ R,
                                                        float *__restrict__ C, int M, int K, long long TV, int wt) {
    constexpr int BM = 32 * MB;
    constexpr int WU = BM * 4 / 256;     // staging units of W per thread
    constexpr int XU = kBN * 4 / 256;    // ... and of X
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * (BM + kBN) * kRowB];
    unsigned char *Wh = lds, *Wl = Wh + BM * kRowB, *Xh = Wl + BM * kRowB, *Xl = Xh + kBN * kRowB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * BM;
    const long long j0 = (long long)blockIdx.y * kBN;
    const size_t n = blockIdx.z;
    const float *Xn = X + n * (size_t)K * (size_t)TV;

    // this thread's staging units: (row, piece), with the byte offset of the unit's first element inside a K chunk and whether
    // its row exists at all (m < M, j < TV).  Offsets are 32-bit against a chunk base that is uniform over the workgroup.
    int wrow[WU], wg[WU], xrow[XU], xg[XU];
    unsigned woff[WU], xoff[XU];
    bool wok[WU], xok[XU];
    const unsigned wstride = wt == 1 ? 4u * (unsigned)M : 4u;      // bytes between two k of a row of W
    const unsigned xstride = 4u * (unsigned)TV;
#pragma unroll
    for (int i = 0; i < WU; ++i) {
        const int u = tid + 256 * i;
        if (wt == 1) { wrow[i] = u % BM; wg[i] = u / BM; }  // W as (K, M): lanes along m
        else { wrow[i] = u >> 2; wg[i] = u & 3; }           // W as (M, K): lanes along k
        const int m = m0 + wrow[i];
        wok[i] = m < M;
        woff[i] = wt == 1 ? 4u * ((unsigned)(8 * wg[i]) * (unsigned)M + (unsigned)m) : 4u * ((unsigned)m * (unsigned)K + 8u * wg[i]);
    }
#pragma unroll
    for (int i = 0; i < XU; ++i) {
        const int u = tid + 256 * i;
        xrow[i] = u & (kBN - 1);
        xg[i] = u >> 7;
        const long long j = j0 + xrow[i];
        xok[i] = j < TV;
        xoff[i] = 4u * ((unsigned)(8 * xg[i]) * (unsigned)TV + (unsigned)j);
    }

    float wr[WU][8], xr[XU][8];
    // FULL: every k of the chunk is below K (no predicate on k); else the K tail, staged as zeros
    auto load_chunk = [&](int k0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const char *Wc = reinterpret_cast<const char *>(W) + (size_t)k0 * wstride;
        const char *Xc = reinterpret_cast<const char *>(Xn) + (size_t)k0 * xstride;
#pragma unroll
        for (int i = 0; i < WU; ++i) {
            if (FULL && wt == 2) {                 // W as (M, K) with 16-byte aligned rows: the unit's 8 k as two wide loads
                float4 lo4 = make_float4(0.f, 0.f, 0.f, 0.f), hi4 = lo4;
                if (wok[i]) {
                    lo4 = *reinterpret_cast<const float4 *>(Wc + woff[i]);
                    hi4 = *reinterpret_cast<const float4 *>(Wc + woff[i] + 16u);
                }
                wr[i][0] = lo4.x; wr[i][1] = lo4.y; wr[i][2] = lo4.z; wr[i][3] = lo4.w;
                wr[i][4] = hi4.x; wr[i][5] = hi4.y; wr[i][6] = hi4.z; wr[i][7] = hi4.w;
                continue;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = 0.f;
                if (wok[i] && (FULL || k0 + 8 * wg[i] + e < K)) v = *reinterpret_cast<const float *>(Wc + (woff[i] + e * wstride));
                wr[i][e] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < XU; ++i) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = 0.f;
                if (xok[i] && (FULL || k0 + 8 * xg[i] + e < K)) v = *reinterpret_cast<const float *>(Xc + (xoff[i] + e * xstride));
                xr[i][e] = v;
            }
        }
    };
    auto load = [&](int k0) {
        if (k0 + kKC <= K) load_chunk(k0, std::true_type{});
        else load_chunk(k0, std::false_type{});
    };

    f32x4 acc[MB][4];
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;     // fragment row inside a block, and its piece of the k-step

    load(0);
    for (int k0 = 0; k0 < K; k0 += kKC) {
#pragma unroll
        for (int i = 0; i < WU; ++i) {
            uint4 hi, lo;
            split8(wr[i], hi, lo);
            const int off = img_off(wrow[i], wg[i]);
            *reinterpret_cast<uint4 *>(Wh + off) = hi;
            *reinterpret_cast<uint4 *>(Wl + off) = lo;
        }
#pragma unroll
        for (int i = 0; i < XU; ++i) {
            uint4 hi, lo;
            split8(xr[i], hi, lo);
            const int off = img_off(xrow[i], xg[i]);
            *reinterpret_cast<uint4 *>(Xh + off) = hi;
            *reinterpret_cast<uint4 *>(Xl + off) = lo;
        }
        __syncthreads();
        if (k0 + kKC < K) load(k0 + kKC);     // in flight under the MFMAs

        FragB<3, MB> a;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int off = img_off(wm * 16 * MB + mb * 16 + fr, fg);
            a.hi[mb] = *reinterpret_cast<const uint4 *>(Wh + off);
            a.lo[mb] = *reinterpret_cast<const uint4 *>(Wl + off);
        }
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int off = img_off(wn * 64 + nb * 16 + fr, fg);
            const bf16x8 bh = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(Xh + off));
            const bf16x8 bl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(Xl + off));
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const bf16x8 ah = __builtin_bit_cast(bf16x8, a.hi[mb]);
                const bf16x8 al = __builtin_bit_cast(bf16x8, a.lo[mb]);
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc[mb][nb], 0, 0, 0);
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc[mb][nb], 0, 0, 0);
                acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[mb][nb], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // epilogue: block (mb, nb) holds column j = lane & 15 and rows 4 * (lane >> 4) + r in register r
    const size_t cn = n * (size_t)M * (size_t)TV;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm * 16 * MB + mb * 16 + 4 * fg + r;
            if (m >= M) continue;
            const float bv = bias ? bias[m] : 0.f;
            const size_t rowo = cn + (size_t)m * (size_t)TV;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const long long j = j0 + wn * 64 + nb * 16 + fr;
                if (j >= TV) continue;
                float v = acc[mb][nb][r] + bv;
                if (R) v += R[rowo + (size_t)j];
                C[rowo + (size_t)j] = v;
            }
        }
    }
}

}  // namespace

int wx_bf16x3_tile_rows(int M) { return (M + 63) / 64 * 64 < (M + 127) / 128 * 128 ? 64 : 128; }

const char *wx_bf16x3_kernel_name(int M) {
    return wx_bf16x3_tile_rows(M) == 64 ? "wx_bf16x3_kernel<64x128>" : "wx_bf16x3_kernel<128x128>";
}

// the kernel's offsets inside W and inside 32 rows of X are 32-bit; column tiles and clips ride on 16-bit grid axes
bool wx_bf16x3_covers(int M, int K, long long TV, int N) {
    return M >= 1 && K >= 1 && TV >= 1 && (TV + kBN - 1) / kBN <= 65535 && (long long)(M + 128) * (K + 32) < (1LL << 29) && N >= 1 &&
           N <= 65535;
}

int launch_wx_bf16x3(const float *W, const float *X, const float *bias, const float *R, float *C, int N, int M, int K,
                     long long TV, bool w_transposed, hipStream_t st) {
    if (!wx_bf16x3_covers(M, K, TV, N))
        return fail(STGCN_ERR_UNSUPPORTED, "wx_bf16x3: M=%d K=%d TV=%lld N=%d exceed the grid", M, K, TV, N);
    const int BM = wx_bf16x3_tile_rows(M);
    const dim3 grid((unsigned)ceil_div(M, BM), (unsigned)((TV + kBN - 1) / kBN), (unsigned)N);   // row tiles of one X tile run together
    // W's form for the staging loads: 1 = (K, M); 2 = (M, K) whose rows are 16-byte aligned (wide loads); 0 = (M, K), dword loads
    const int wt = w_transposed ? 1 : ((K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0) ? 2 : 0;
    if (BM == 64) hipLaunchKernelGGL(wx_bf16x3_kernel<2>, grid, dim3(256), 0, st, W, X, bias, R, C, M, K, TV, wt);
    else hipLaunchKernelGGL(wx_bf16x3_kernel<4>, grid, dim3(256), 0, st, W, X, bias, R, C, M, K, TV, wt);
    STGCN_LAUNCH_CHECK("wx_bf16x3_kernel");
    return STGCN_OK;
}

}  // namespace stgcn
