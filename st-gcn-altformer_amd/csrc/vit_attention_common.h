// What the attention kernels of the AltFormer heads' blocks are built from (vit_attention.hip, vit_attention_bf16.hip,
// vit_attention_train_bf16.hip, the attention backward of vit_backward.hip: the RESIDENT family; vit_attention_stream.hip,
// vit_attention_bwd_stream.hip: the STREAMING one).  All of them map
//     qkv (B, L, 3, H, hd) exactly as the qkv nn.Linear writes it  <->  out (B, L, H*hd) ready for proj
// with no q / k / v permute copies, no L x L matrix in memory and no atomics: every output element has one owner and a fixed
// summation order, so results are bit-identical run to run.  The layout they share, described here and nowhere else:
//
//   work     A (sequence, head) PAIR is cut into tiles of 32 rows, a wave per tile.  Resident (L <= kMaxL = 256): the pair's
//            NT = ceil(L / 32) waves are one workgroup next to K and V of the pair in LDS (NT*32 rows, the rows past L
//            zero-filled, never read from memory); short sequences pack attention_pairs(NT) pairs into a workgroup so that it
//            has at least four waves.  Streaming: four waves own 128 rows and the other side passes through two LDS stages.
//            Split (vit_attention_split.hip, L <= kMaxL, few pairs): a workgroup per (pair, query tile), its NT waves one key
//            tile each, operands from global memory, the partial soft-maxes merged through LDS.
//   S^T = K Q^T  per key tile of 32: A = K rows from LDS, B = the wave's 32 query rows in registers.  The accumulator puts
//            query j in lanes j and j + 32, and register i of lane half h holds key 8 (i / 4) + 4 h + i % 4 of the tile
//            (ACC_KEY).  So a query's whole score row (resident: up to 8 x 16 registers) lives in two lanes, and the
//            soft-max is a two-pass one over registers in a fixed order (max, then exp and sum) with one exchange with
//            lane ^ 32 per pass; the streaming kernels keep a running form of it.  Keys past L score -inf.
//   O^T = V^T P^T  the score accumulators are already a B operand, so P never leaves the registers and nothing is transposed
//            through LDS.  fp32 (v_mfma_f32_32x32x2_f32): register i of the two lane halves is the two k values of one MFMA,
//            A = V^T read from LDS with lane = channel.  bf16 (v_mfma_f32_32x32x16_bf16): registers 0-7 (8-15) of a lane,
//            rounded and packed in pairs (pack8), are the B operand over the first (second) 16 keys of the tile in the
//            accumulator's key order; the A operand needs the same eight keys of one channel as 16 contiguous bytes, so that
//            side is staged TRANSPOSED and permuted (scatter8 at perm16):
//                T[channel][16 g + 8 h + j] = X[16 g + 8 (j / 4) + 4 h + j % 4][channel],    g = group of 16 keys.
//            The backward kernels use both products the same way with other operands (dQ^T = K^T dS^T, dV^T = dO^T P, ..).
//   LDS      fp32 tiles are rows of hd + 1 floats where a fragment is read along a row per lane (the 32 rows of a fragment
//            sit in 32 banks), hd floats where lane = channel.  bf16 row tiles have hd + 8 elements per row (80 / 144 bytes),
//            transposed ones keys + 8 (16 bytes more than a multiple of 64): 16-byte fragment reads without bank conflicts.
//            The *_lds_bytes functions below are these layouts' sizes; the kernels and their launcher read the same ones.
//
// Shared here: the packing rule, the LDS sizes and the launcher of the resident family (host); the accumulator index, the
// staging loops' index decomposition and zero-fill rule, the output stores and the bf16 operand helpers (device).  NOT shared,
// because as functions they moved the register allocation of some instantiation (profiles/vit_attention_shared_resources.txt
// holds the kernels to "no count may rise"): the wave / pair / tile preamble, the soft-max passes, the fp32 score and output
// product steps, the B fragment loads, the output stores of vit_attention_bwd_bf16_kernel, and one body for the two bf16
// forwards.  vit_attention_bwd_kernel (vit_backward.hip) keeps its staging loops and stores as well: with stage_slot and
// store_rows its registers held, but dq and dk moved in the last bit at NT = 3 and 4, hd = 32 (fp contraction is on in that
// file and chose other fusions; tests/test_vit_attention_digests_gpu.py).  Those stay written out in the kernels, in the
// same words wherever they appear.
// Every device piece is __forceinline__ and takes the fp contraction of the file that includes it: a file that switches
// contraction off (vit_attention_train_bf16.hip) does so ABOVE this include.
#pragma once

#include "bf16_common.h"
#include "vit.h"

namespace stgcn {
namespace vit {

using bf16k::bf16x8;
using bf16k::f32x16;
using bf16k::pack_bf16x2;
using bf16k::round8;
using bf16k::split8;

// ---- host: packing, LDS sizes, the resident family's launcher -----------------------------------------------------------------
constexpr int attention_tiles(int L) { return (L + 31) / 32; }
// (sequence, head) pairs per workgroup of a resident kernel: 4 waves for L <= 64, NT (= 3, 4 .. 8) above
constexpr int attention_pairs(int nt) { return nt >= 4 ? 1 : 4 / nt; }

constexpr int kPadF32 = 1, kPad16 = 8;    // what a row of an fp32 / bf16 tile has beyond its data (in elements)
constexpr size_t row_tile16(int nt, int hd) { return (size_t)nt * 32 * (hd + kPad16); }     // elements of [keys][hd + 8]
constexpr size_t col_tile16(int nt, int hd) { return (size_t)hd * (nt * 32 + kPad16); }     // elements of [hd][keys + 8]
// forward: K [rows][hd + 1], V [rows][hd]
constexpr size_t attention_f32_lds_bytes(int nt, int hd) { return (size_t)attention_pairs(nt) * nt * 32 * (2 * hd + kPadF32) * 4; }
// split forward (vit_attention_split.hip): K and V come from global memory, LDS holds the merge only: per wave (= key tile) a
// partial [32][hd + 4] and (max, sum) per query.  70 KiB at L = 256, hd = 64
constexpr int kPadSplit = 4;
constexpr int attention_split_wave_floats(int hd) { return 32 * (hd + kPadSplit) + 2 * 32; }
constexpr size_t attention_split_lds_bytes(int nt, int hd) { return (size_t)nt * attention_split_wave_floats(hd) * 4; }
// backward: two tiles [rows][hd + 1] and (max, 1 / sum, delta, -) per row.  134 KiB at L = 256, hd = 64
constexpr size_t attention_bwd_f32_lds_bytes(int nt, int hd) {
    return (size_t)attention_pairs(nt) * nt * 32 * (2 * (hd + kPadF32) + 4) * 4;
}
// bf16 forwards: `k_tiles` row tiles of K (1: K as stored; 2: K hi and K lo) and V^T.  52 KiB at L = 180, hd = 64, one chain
constexpr size_t attention_bf16_lds_bytes(int nt, int hd, int k_tiles) {
    return (size_t)attention_pairs(nt) * (k_tiles * row_tile16(nt, hd) + col_tile16(nt, hd)) * 2;
}
// bf16 backward: three row tiles, `transposed` transposed ones and 16 bytes of statistics per row.  With two transposed tiles
// hd = 64 at L > 224 is 178 KiB, more than the 160 there are: that one instantiation (SPLIT) makes do with one.
constexpr size_t attention_bwd_bf16_bytes(int nt, int hd, int transposed) {
    return (size_t)attention_pairs(nt) * ((3 * row_tile16(nt, hd) + transposed * col_tile16(nt, hd)) * 2 + (size_t)nt * 32 * 16);
}
constexpr bool attention_bwd_bf16_split(int nt, int hd) { return attention_bwd_bf16_bytes(nt, hd, 2) > (size_t)kLdsBytes; }
constexpr size_t attention_bwd_bf16_lds_bytes(int nt, int hd) {
    return attention_bwd_bf16_bytes(nt, hd, attention_bwd_bf16_split(nt, hd) ? 1 : 2);
}

// The one launcher of the resident kernels.  F names a kernel form:
//   F::what, F::kernel_name     the prefix of its messages, the kernel's name in a launch error
//   F::lds_bytes(nt, hd)        its LDS per workgroup
//   F::kernel<HD, NT>()         the __global__ function; its arguments are (ptrs..., pairs, L, H, scale, G)
template <class F, int HD, int NT, class... P>
int launch_resident_one(int B, int L, int H, float scale, hipStream_t st, P... ptrs) {
    constexpr int G = attention_pairs(NT);
    const long long pairs = (long long)B * H;
    if (pairs > 0x7fffffffLL || !grid_fits((pairs + G - 1) / G, 64 * G * NT)) return fail(STGCN_ERR_UNSUPPORTED, "%s: %lld (sequence, head) pairs", F::what, pairs);
    constexpr size_t bytes = F::lds_bytes(NT, HD);
    if (bytes > (size_t)kLdsBytes) return fail(STGCN_ERR_UNSUPPORTED, "%s: %zu bytes of LDS", F::what, bytes);
    auto kern = F::template kernel<HD, NT>();
    if (bytes > 64 * 1024) STGCN_HIP_CHECK(allow_lds(kern, bytes));
    kern<<<dim3((unsigned)((pairs + G - 1) / G)), dim3(64 * G * NT), bytes, st>>>(ptrs..., (int)pairs, L, H, scale, G);
    STGCN_LAUNCH_CHECK(F::kernel_name);
    return STGCN_OK;
}

template <class F, int HD, class... P>
int launch_resident_hd(int B, int L, int H, float scale, hipStream_t st, P... ptrs) {
    switch (attention_tiles(L)) {
        case 1: return launch_resident_one<F, HD, 1>(B, L, H, scale, st, ptrs...);
        case 2: return launch_resident_one<F, HD, 2>(B, L, H, scale, st, ptrs...);
        case 3: return launch_resident_one<F, HD, 3>(B, L, H, scale, st, ptrs...);
        case 4: return launch_resident_one<F, HD, 4>(B, L, H, scale, st, ptrs...);
        case 5: return launch_resident_one<F, HD, 5>(B, L, H, scale, st, ptrs...);
        case 6: return launch_resident_one<F, HD, 6>(B, L, H, scale, st, ptrs...);
        case 7: return launch_resident_one<F, HD, 7>(B, L, H, scale, st, ptrs...);
        case 8: return launch_resident_one<F, HD, 8>(B, L, H, scale, st, ptrs...);
    }
    return fail(STGCN_ERR_UNSUPPORTED, "%s: L = %d (covered: 1 .. %d)", F::what, L, kMaxL);
}

template <class F, class... P>
int launch_resident(int B, int L, int H, int hd, float scale, hipStream_t st, P... ptrs) {
    if (hd == 32) return launch_resident_hd<F, 32>(B, L, H, scale, st, ptrs...);
    if (hd == 64) return launch_resident_hd<F, 64>(B, L, H, scale, st, ptrs...);
    return fail(STGCN_ERR_UNSUPPORTED, "%s: head_dim = %d (covered: 32, 64)", F::what, hd);
}

// ---- device: the accumulator layout ---------------------------------------------------------------------------------------------
// The key (or query) that accumulator register i of lane half `half` holds in a tile whose first key is `first`.  A macro, not
// a function: behind a function boundary, even a __forceinline__ one, the compiler allocates the registers of the fp32 kernels
// differently (up to 30 VGPRs either way), and this header is not to move code generation.
#define ACC_KEY(first, i, half) ((first) + 8 * ((i) >> 2) + 4 * (half) + ((i) & 3))

// ---- device: staging --------------------------------------------------------------------------------------------------------
// Element e of a resident staging loop (e = tid, tid + blockDim.x, .. < G * ROWS * (HD / VEC)): VEC channels from d0 of row j of
// the workgroup's pair g.  `live`: the row exists (its pair is not past the end, j < L); everything else is staged as zeros
// and never read from memory.  A live row is token `tok` of (B * L) and its channels start at column `col` of (H * hd).
struct StageSlot {
    int g, j, d0;
    bool live;
    size_t tok, col;
};
template <int HD, int ROWS, int VEC>
__device__ __forceinline__ StageSlot stage_slot(int e, int G, int pairs, int L, int H) {
    StageSlot s;
    s.d0 = e % (HD / VEC) * VEC, s.j = (e / (HD / VEC)) % ROWS, s.g = e / ((HD / VEC) * ROWS);
    const int p = blockIdx.x * G + s.g;
    s.live = p < pairs && s.j < L;
    s.tok = (size_t)(p / H) * L + s.j, s.col = (size_t)(p % H) * HD + s.d0;
    return s;
}

// ---- device: output stores ----------------------------------------------------------------------------------------------------
// The lane's 16 accumulator registers are four runs of four channels, 8 channels apart: op = the row's channel 4 * half of
// the 32 the accumulator covers.
__device__ __forceinline__ void store_rows(float *op, const f32x16 &o) {
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<float4 *>(op + 8 * r) = make_float4(o[4 * r], o[4 * r + 1], o[4 * r + 2], o[4 * r + 3]);
}
__device__ __forceinline__ void store_rows(float *op, const f32x16 &o, float f) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4 *>(op + 8 * r) = make_float4(o[4 * r] * f, o[4 * r + 1] * f, o[4 * r + 2] * f, o[4 * r + 3] * f);
}
__device__ __forceinline__ void store_rows(unsigned short *op, const f32x16 &o, float f) {   // bf16, 8 bytes per store
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<uint2 *>(op + 8 * r) = make_uint2(pack_bf16x2(o[4 * r] * f, o[4 * r + 1] * f), pack_bf16x2(o[4 * r + 2] * f, o[4 * r + 3] * f));
}

// ---- device: bf16 operands ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load8(const float *p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
__device__ __forceinline__ void zero8(float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
}
// token j of its tile -> its place in a transposed tile: slot 8 h + j' of its group of 16
__device__ __forceinline__ int perm16(int j) {
    const int o = j & 15;
    return (j & ~15) + (((o >> 2) & 1) << 3) + ((o >> 3) << 2) + (o & 3);
}
// eight channels d0 .. d0 + 7 of one token (already bf16) into a transposed tile (t = its row d0) at column `pos`
__device__ __forceinline__ void scatter8(unsigned short *t, int stride, int pos, uint4 v) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        t[(size_t)(2 * c) * stride + pos] = (unsigned short)(w[c] & 0xffffu);
        t[(size_t)(2 * c + 1) * stride + pos] = (unsigned short)(w[c] >> 16);
    }
}
__device__ __forceinline__ uint4 lds16B(const unsigned short *p) { return *reinterpret_cast<const uint4 *>(p); }
__device__ __forceinline__ f32x16 mfma(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// The three chains of a score k-step on split operands, in one order wherever a score is computed: kl * qh, kh * ql, kh * qh.
// a_is_k: A = K (forward, the backward's phase (a)); else A = Q (phase (b)).
__device__ __forceinline__ f32x16 score_step(uint4 ah, uint4 al, uint4 bh, uint4 bl, f32x16 c, bool a_is_k) {
    if (a_is_k) {
        c = mfma(al, bh, c);
        c = mfma(ah, bl, c);
    } else {
        c = mfma(ah, bl, c);
        c = mfma(al, bh, c);
    }
    return mfma(ah, bh, c);
}
// a 16-register accumulator half -> B operand: registers 8 gk .. 8 gk + 7, rounded and packed in pairs
__device__ __forceinline__ uint4 pack8(const float (&e)[16], int gk) {
    return make_uint4(pack_bf16x2(e[8 * gk], e[8 * gk + 1]), pack_bf16x2(e[8 * gk + 2], e[8 * gk + 3]),
                      pack_bf16x2(e[8 * gk + 4], e[8 * gk + 5]), pack_bf16x2(e[8 * gk + 6], e[8 * gk + 7]));
}

}  // namespace vit
}  // namespace stgcn
