// Weight / bias gradient of a linear on the bf16 matrix cores (vit.h, launch_wgrad_bf16; the STGCN_VIT_TRAIN_BF16 mode):
//     dW (Nout, K) = r(s dY)^T r(A),   db (Nout) = column sums of the UNROUNDED fp32 s dY,
// r = round to nearest-even bf16, products accumulated in fp32 (v_mfma_f32_32x32x16_bf16).  Everything around the operand
// path is vit_backward.hip's fp32 kernel: a workgroup of 4 waves owns a 128 x 128 tile of dW for one range of tokens
// (wgrad_rows_per_split), writes one partial slab, the slabs are added in range order (reduce_parts), the bias gradient rides
// in the workgroups of the first K tile, one owner per element, no atomics, two runs bit-identical.
//
// Operand path.  The contraction index of dW = dY^T A is the token, the slow index of both operands in memory, and a
// 32x32x16 fragment is eight consecutive TOKENS of one feature per lane (row / column l31, k = 8 half + j).  So both operands
// are transposed on the way to LDS, in registers: of a chunk of 32 tokens x 128 features a thread gathers the eight tokens
// 8 q .. 8 q + 7 (q = tid / 64, wave-uniform) of the feature pair 2 p, 2 p + 1 (p = tid % 64) with eight 8-byte loads (a wave
// reads 512 contiguous bytes of each of its eight rows), rounds them and writes, per feature, the eight bf16 as one 16-byte
// store: exactly the fragment a lane reads back.  The image is feature-major, [128 features][32 tokens] bf16 on a row stride
// of 40 elements (80 bytes), the bf16 linear's image with "feature" in the place of its row and "token" in the place of k:
//   reads : ds_read_b128 of lane l31 at row * 80 + 32 ks + 16 half bytes.  Banks are (a / 4) % 64, in 16-byte slots
//           (5 row) % 16 + const; the instruction's lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and + 32) hold
//           sixteen rows whose 5 row % 16 are all different, so no two lanes of a group share a slot: conflict-free.
//   writes: ds_write_b128 goes in groups of eight consecutive lanes, banks (a / 4) % 32.  Lane p writes rows 2 p + g;
//           with g = 0 for all, lanes p and p + 4 are 8 rows = 640 bytes = 160 dwords = 0 (mod 32) apart: 2-way.  So lanes
//           with bit 2 of p set write their odd feature first (g = e ^ (p >> 2 & 1) in pass e): a group's dword offsets are
//           8 j (j = 0 .. 3) and 20 + 8 j (mod 32), eight disjoint runs of four banks: conflict-free.
// The next chunk's sixteen global loads per thread are issued before the current chunk's MFMAs and stored after them.
// Tokens past the range and features past K / Nout are zero-filled (K % 32 == 0 and Nout % 4 == 0, so a pair is whole).
//
// The 64 form (template parameter T = 64: a 64 x 64 tile of dW, one accumulator block per wave, four times the workgroups per
// split; plan_wgrad in vit.h says where it runs).  Of a chunk of 32 tokens x 64 features a thread gathers the eight tokens
// 8 q .. 8 q + 7 of ONE feature p = tid % 64 with eight 4-byte loads (a wave reads 256 contiguous bytes of each of its eight
// rows) and writes them as one 16-byte store.  The image is [64 features][32 tokens] on the same 80-byte rows:
//   reads : unchanged.  A ds_read_b128 still covers 32 consecutive rows (wm * 32 + l31) at one token offset, so its lane
//           groups hold the same sixteen rows with sixteen different (5 row) % 16: conflict-free.
//   writes: lane p now writes row p, not rows 2 p + g.  A group of eight consecutive lanes p = 8 g + j writes at the dword
//           offsets 20 j + const (mod 32) = 0, 20, 8, 28, 16, 4, 24, 12 for j = 0 .. 7, eight disjoint runs of four banks:
//           conflict-free as it stands.  The 128 form's 2-way conflict came from lanes four apart being 160 dwords apart;
//           here they are 80 apart (16 mod 32), so the 64 form has no swap.
#include "bf16_common.h"
#include "vit.h"

namespace stgcn {
namespace vit {

using bf16k::bf16x8;
using bf16k::f32x16;
using bf16k::round8;

namespace {

constexpr int WC = 32, WLH = WC + 8;   // tokens per chunk, LDS row stride (bf16 elements)
static_assert(WC == kWgradChunk, "wgrad_rows_per_split cuts ranges in multiples of the chunk");

// component-wise, so that the choice is four v_cndmask and not an indexed private array
__device__ __forceinline__ uint4 pick(bool second, const uint4 a, const uint4 b) {
    return make_uint4(second ? b.x : a.x, second ? b.y : a.y, second ? b.z : a.z, second ? b.w : a.w);
}

template <int T>
__global__ __launch_bounds__(256) void vit_wgrad_bf16_kernel(const float *__restrict__ dY, const float *__restrict__ A,
                                                            const float *__restrict__ rowscale, int L, float *__restrict__ part,
                                                            float *__restrict__ bpart, int M, int K, int Nout, int tiles_n,
                                                            int tiles_k, int cps, int long_splits) {
    static_assert(T == 128 || T == 64, "two forms");
    constexpr int NB = T / 64, FP = T / 64;   // 32 x 32 blocks per wave and dimension; features a thread stages per operand
    __shared__ __attribute__((aligned(16))) unsigned short ld[T * WLH], la[T * WLH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
    const int tile = (int)blockIdx.x % (tiles_n * tiles_k), split = (int)blockIdx.x / (tiles_n * tiles_k);
    const int n0 = (tile / tiles_k) * T, k0 = (tile % tiles_k) * T;
    // split s: the chunks [s cps + min(s, long_splits), ...), one more than cps for the first long_splits splits
    const int r_lo = (split * cps + min(split, long_splits)) * WC;
    const int r_hi = min(M, r_lo + (cps + (split < long_splits ? 1 : 0)) * WC);
    const int sq = wave * 8, sf = lane * FP;           // staging: tokens sq .. sq + 7 of the chunk, features sf (, sf + 1) of the tile
    const bool swap = FP == 2 && ((lane >> 2) & 1) != 0;   // which feature of the pair goes to LDS first (see the header)
    const bool with_bias = bpart != nullptr && k0 == 0;

    float bsum[FP] = {};
    // Loads without a branch around them (a branch per load makes the compiler wait for each before it issues the next):
    // the row is clamped into the range and the feature pair into the matrix, what was clamped is zeroed after the load.
    const bool in_n = n0 + sf < Nout, in_k = k0 + sf < K;
    const float *dcol = dY + (in_n ? n0 + sf : 0), *acol = A + (in_k ? k0 + sf : 0);
    const int seq_last = rowscale != nullptr && r_hi > 0 ? (r_hi - 1) / L : 0;
    float gd[8][FP], ga[8][FP];   // [token] x the feature (pair)
    float gs[8];           // the tokens' row factors
    auto gload = [&](int r0) {
        const int row0 = r0 + sq;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = min(row0 + i, r_hi - 1);
            if constexpr (FP == 2) {
                const float2 d = *reinterpret_cast<const float2 *>(dcol + (size_t)row * Nout);
                const float2 a = *reinterpret_cast<const float2 *>(acol + (size_t)row * K);
                gd[i][0] = d.x, gd[i][1] = d.y, ga[i][0] = a.x, ga[i][1] = a.y;
            } else {
                gd[i][0] = dcol[(size_t)row * Nout];
                ga[i][0] = acol[(size_t)row * K];
            }
        }
        if (rowscale != nullptr) {   // (uniform) applied in sstore: nothing here waits for a load
            int seq = row0 / L, pos = row0 - seq * L;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                gs[i] = rowscale[min(seq, seq_last)];
                if (++pos == L) pos = 0, ++seq;
            }
        }
    };
    auto sstore = [&](int r0) {
        float fd[FP][8], fa[FP][8];   // [feature of the pair][token]
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool in_r = r0 + sq + i < r_hi;
            const float s = rowscale != nullptr ? gs[i] : 1.f;
#pragma unroll
            for (int f = 0; f < FP; ++f) {
                fd[f][i] = in_r && in_n ? gd[i][f] * s : 0.f;
                fa[f][i] = in_r && in_k ? ga[i][f] : 0.f;
            }
        }
        if constexpr (FP == 2) {
            const uint4 d0 = round8(fd[0]), d1 = round8(fd[1]), a0 = round8(fa[0]), a1 = round8(fa[1]);   // eight tokens of one feature
            const int first = (sf + (swap ? 1 : 0)) * WLH + sq, second = (sf + (swap ? 0 : 1)) * WLH + sq;
            *reinterpret_cast<uint4 *>(&ld[first]) = pick(swap, d0, d1);
            *reinterpret_cast<uint4 *>(&la[first]) = pick(swap, a0, a1);
            *reinterpret_cast<uint4 *>(&ld[second]) = pick(swap, d1, d0);
            *reinterpret_cast<uint4 *>(&la[second]) = pick(swap, a1, a0);
        } else {
            *reinterpret_cast<uint4 *>(&ld[sf * WLH + sq]) = round8(fd[0]);
            *reinterpret_cast<uint4 *>(&la[sf * WLH + sq]) = round8(fa[0]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)   // the unrounded values, in token order
#pragma unroll
            for (int f = 0; f < FP; ++f) bsum[f] += fd[f][i];
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
        sstore(r_lo);
    }
    __syncthreads();
    for (int r0 = r_lo; r0 < r_hi; r0 += WC) {
        const bool more = r0 + WC < r_hi;
        if (more) gload(r0 + WC);
#pragma unroll
        for (int ks = 0; ks < WC / 16; ++ks) {
            bf16x8 fd[NB], fa[NB];
#pragma unroll
            for (int m = 0; m < NB; ++m) {
                fd[m] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(&ld[(wm * (T / 2) + m * 32 + l31) * WLH + ks * 16 + half * 8]));
                fa[m] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(&la[(wn * (T / 2) + m * 32 + l31) * WLH + ks * 16 + half * 8]));
            }
#pragma unroll
            for (int m = 0; m < NB; ++m)
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fd[m], fa[n], acc[m][n], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            sstore(r0 + WC);
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
    if (with_bias) {   // (uniform over the workgroup) the four token octets of a column, added in the order 0 .. 3
        float *red = reinterpret_cast<float *>(ld);   // 4 x T floats; every wave is past its last fragment read (the loop's barrier)
#pragma unroll
        for (int f = 0; f < FP; ++f) red[wave * T + sf + f] = bsum[f];
        __syncthreads();
        if (tid < T && n0 + tid < Nout) {
            float t = red[tid];
#pragma unroll
            for (int r = 1; r < 4; ++r) t += red[r * T + tid];
            bpart[(size_t)split * Nout + n0 + tid] = t;
        }
    }
}

}  // namespace

int launch_wgrad_bf16(const WgradPlan &wp, const float *dY, const float *A, const float *rowscale, int L, float *dW, float *db,
                      float *part, float *tmp, int M, int K, int Nout, bool accumulate, hipStream_t st) {
    const bool direct = wp.direct(accumulate);   // the slab is dW itself: launch_wgrad
    const int tiles_n = ceil_div(Nout, wp.tile), tiles_k = ceil_div(K, wp.tile);
    float *slab = direct ? dW : part;
    float *bpart = db == nullptr ? nullptr : direct ? db : part + (size_t)wp.splits * Nout * K;
    const dim3 grid((unsigned)(tiles_n * tiles_k * wp.splits));
    if (wp.tile == 64)
        vit_wgrad_bf16_kernel<64><<<grid, dim3(256), 0, st>>>(dY, A, rowscale, L, slab, bpart, M, K, Nout, tiles_n, tiles_k, wp.cps,
                                                              wp.long_splits);
    else
        vit_wgrad_bf16_kernel<128><<<grid, dim3(256), 0, st>>>(dY, A, rowscale, L, slab, bpart, M, K, Nout, tiles_n, tiles_k, wp.cps,
                                                               wp.long_splits);
    STGCN_LAUNCH_CHECK("vit_wgrad_bf16_kernel");
    if (direct) return STGCN_OK;
    int rc;
    if ((rc = reduce_parts(part, wp.splits, (size_t)Nout * K, dW, tmp, accumulate, st))) return rc;
    if (db != nullptr && (rc = reduce_parts(bpart, wp.splits, (size_t)Nout, db, tmp, accumulate, st))) return rc;
    return STGCN_OK;
}

}  // namespace vit
}  // namespace stgcn
