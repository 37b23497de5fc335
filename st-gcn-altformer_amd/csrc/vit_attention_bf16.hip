// Multi-head attention of the AltFormer heads' blocks on bf16 operands (the STGCN_VIT_BF16 mode of stgcn_vit_block_forward):
//     qkv (B, L, 3, H, hd) bf16 as the bf16 qkv linear stores it  ->  out (B, L, H*hd) bf16 ready for proj.
// The resident form of vit_attention.hip (L <= 256) on v_mfma_f32_32x32x16_bf16: a (sequence, head) pair gets
// NT = ceil(L / 32) waves, one per tile of 32 queries, and its K and V (NT*32 keys, the keys past L zero-filled, never read
// from memory) in LDS as bf16; short sequences pack several pairs into a workgroup exactly as there (L <= 32: one wave per
// pair, four pairs per workgroup).  Products are bf16 x bf16 (exact in fp32), every sum is fp32.
//
//   S^T = K Q^T per key tile: A = K rows from LDS (row stride hd + 8 elements = 80 / 144 bytes: the 16-byte fragment reads
//         of the 32 rows are bank-conflict free), B = the wave's 32 query rows read from memory as they are (lane = query,
//         8 consecutive channels per k-step and lane half), hd / 16 MFMAs per tile.  `scale` multiplies the fp32 score: q is
//         not rounded a second time.  The accumulator layout is the fp32 kernel's: query j in lanes j and j + 32, register i
//         of lane half h = key 8 (i / 4) + 4 h + i % 4 of the tile, so a query's score row (up to 256 keys = 8 x 16
//         registers) lives in two lanes and the soft-max is a two-pass one (max, then exp and sum) over registers in a
//         fixed order plus one exchange with lane ^ 32.  Keys past L get -inf.
//   P     : p = exp(s - max), unnormalised, rounded to bf16 as it is packed; the row sum adds the UNROUNDED fp32 p.
//   O^T = V^T P^T: registers 0-7 (8-15) of a lane are eight keys of one query, i.e. packed in pairs they are the B operand
//         of one MFMA over the first (second) 16 keys of the tile - in the accumulator's key order, not in memory order:
//         slot j of lane half h is key 8 (j / 4) + 4 h + j % 4 of the group of 16.  The A operand needs the same eight keys
//         of one channel as 16 contiguous bytes, so V is staged TRANSPOSED and permuted:
//             Vt[channel][16 g + 8 h + j] = V[16 g + 8 (j / 4) + 4 h + j % 4][channel],    g = group of 16 keys,
//         row stride NT*32 + 8 elements (16 bytes more than a multiple of 64: conflict-free 16-byte reads, lane = channel).
//         P never leaves the registers.  O is divided by the row sum in fp32 and stored as bf16, 8 bytes per store.
// LDS per workgroup: G pairs x (NT*32 (hd + 8) + hd (NT*32 + 8)) x 2 bytes: 52 KiB at L = 180, hd = 64 (the fp32 kernel: 99).
// No atomics; every output element has one owner and a fixed summation order, so results are bit-identical run to run.
#include "bf16_common.h"
#include "vit.h"

namespace stgcn {
namespace vit {

using bf16k::bf16x8;
using bf16k::f32x16;
using bf16k::pack_bf16x2;

namespace {

template <int HD, int NT>
__global__ __launch_bounds__(512) void vit_attention_bf16_kernel(const unsigned short *__restrict__ qkv,
                                                                unsigned short *__restrict__ out, int pairs, int L, int H,
                                                                float scale, int G) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds16[];
    constexpr int ROWS = NT * 32, KS = HD + 8, VS = ROWS + 8, KST = HD / 16;
    unsigned short *Ks = lds16;                          // [G][ROWS][KS]
    unsigned short *Vt = lds16 + (size_t)G * ROWS * KS;  // [G][HD][VS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD;    // elements per token of qkv

    // stage K and V of the workgroup's pairs: 8 channels (16 bytes) of one key per thread and step, keys past L and pairs
    // past the end zero-filled
    const int nvec = G * ROWS * (HD / 8);
    for (int e = tid; e < nvec; e += blockDim.x) {
        const int d8 = e % (HD / 8), j = (e / (HD / 8)) % ROWS, g = e / ((HD / 8) * ROWS);
        const int p = blockIdx.x * G + g;
        uint4 k = make_uint4(0u, 0u, 0u, 0u), v = k;
        if (p < pairs && j < L) {
            const unsigned short *base = qkv + ((size_t)(p / H) * L + j) * tok + (size_t)(p % H) * HD + d8 * 8;
            k = *reinterpret_cast<const uint4 *>(base + (size_t)H * HD);
            v = *reinterpret_cast<const uint4 *>(base + (size_t)2 * H * HD);
        }
        *reinterpret_cast<uint4 *>(Ks + ((size_t)g * ROWS + j) * KS + d8 * 8) = k;
        const int o = j & 15;                 // key j of its group of 16 -> slot 8 h + j' (see the header)
        const int pos = (j & ~15) + (((o >> 2) & 1) << 3) + ((o >> 3) << 2) + (o & 3);
        unsigned short *vd = Vt + ((size_t)g * HD + d8 * 8) * VS + pos;
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            vd[(2 * c) * VS] = (unsigned short)(w[c] & 0xffffu);
            vd[(2 * c + 1) * VS] = (unsigned short)(w[c] >> 16);
        }
    }
    __syncthreads();

    const int g = wave / NT, qt = wave % NT;
    const int p = blockIdx.x * G + g;
    if (p >= pairs) return;                   // wave-uniform
    const int b = p / H, h = p % H;
    const int qi = qt * 32 + l31;
    if (qt * 32 >= L) return;                 // wave-uniform: a query tile past the sequence (cannot happen with NT = ceil(L/32))

    // the wave's queries as B operand: lane holds Q[qi][16 s + 8 half .. + 7] for k-step s
    uint4 qf[KST];
#pragma unroll
    for (int s = 0; s < KST; ++s) qf[s] = make_uint4(0u, 0u, 0u, 0u);
    if (qi < L) {
        const unsigned short *qp = qkv + ((size_t)b * L + qi) * tok + (size_t)h * HD + half * 8;
#pragma unroll
        for (int s = 0; s < KST; ++s) qf[s] = *reinterpret_cast<const uint4 *>(qp + 16 * s);
    }

    const unsigned short *Kg = Ks + (size_t)g * ROWS * KS, *Vg = Vt + (size_t)g * HD * VS;
    f32x16 sc[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
        const unsigned short *kp = Kg + (size_t)(kt * 32 + l31) * KS + half * 8;
#pragma unroll
        for (int s = 0; s < KST; ++s)
            sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(kp + 16 * s)),
                                                             __builtin_bit_cast(bf16x8, qf[s]), sc[kt], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sc[kt][i] *= scale;
            if (kt == NT - 1 && kt * 32 + 8 * (i >> 2) + 4 * half + (i & 3) >= L) sc[kt][i] = -INFINITY;   // only the last tile is partial
            mx = fmaxf(mx, sc[kt][i]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // key 0 is always valid: mx is finite
    float sum = 0.f;
    uint4 pk[NT][2];                          // P^T as B operands: [key tile][group of 16 keys]
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        unsigned w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float e0 = __expf(sc[kt][2 * i] - mx), e1 = __expf(sc[kt][2 * i + 1] - mx);   // exp(-inf) = 0: masked keys
            sum += e0;
            sum += e1;
            w[i] = pack_bf16x2(e0, e1);
        }
        pk[kt][0] = make_uint4(w[0], w[1], w[2], w[3]);
        pk[kt][1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt) {
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
        const unsigned short *vp = Vg + (size_t)(dt * 32 + l31) * VS + half * 8;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int gk = 0; gk < 2; ++gk)
                o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(vp + kt * 32 + gk * 16)),
                    __builtin_bit_cast(bf16x8, pk[kt][gk]), o, 0, 0, 0);
        if (qi < L) {
            unsigned short *op = out + ((size_t)b * L + qi) * ((size_t)H * HD) + (size_t)h * HD + dt * 32 + 4 * half;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<uint2 *>(op + 8 * r) = make_uint2(pack_bf16x2(o[4 * r] * inv, o[4 * r + 1] * inv),
                                                                    pack_bf16x2(o[4 * r + 2] * inv, o[4 * r + 3] * inv));
        }
    }
}

template <int HD, int NT>
int launch_one(const unsigned short *qkv, unsigned short *out, int B, int L, int H, float scale, hipStream_t st) {
    const int G = NT >= 4 ? 1 : 4 / NT;       // the fp32 kernel's packing: 4 waves for L <= 64, NT (= 3, 4 .. 8) above
    const long long pairs = (long long)B * H;
    if (pairs > 0x7fffffffLL) return fail(STGCN_ERR_UNSUPPORTED, "vit attention (bf16): %lld (sequence, head) pairs", pairs);
    const size_t bytes = attention_bf16_lds_bytes(L, HD);
    if (bytes > (size_t)kLdsBytes) return fail(STGCN_ERR_UNSUPPORTED, "vit attention (bf16): %zu bytes of LDS", bytes);
    auto kern = vit_attention_bf16_kernel<HD, NT>;
    if (bytes > 64 * 1024) STGCN_HIP_CHECK(allow_lds(kern, bytes));
    kern<<<dim3((unsigned)((pairs + G - 1) / G)), dim3(64 * G * NT), bytes, st>>>(qkv, out, (int)pairs, L, H, scale, G);
    STGCN_LAUNCH_CHECK("vit_attention_bf16_kernel");
    return STGCN_OK;
}

template <int HD>
int launch_hd(const unsigned short *qkv, unsigned short *out, int B, int L, int H, float scale, hipStream_t st) {
    switch (ceil_div(L, 32)) {
        case 1: return launch_one<HD, 1>(qkv, out, B, L, H, scale, st);
        case 2: return launch_one<HD, 2>(qkv, out, B, L, H, scale, st);
        case 3: return launch_one<HD, 3>(qkv, out, B, L, H, scale, st);
        case 4: return launch_one<HD, 4>(qkv, out, B, L, H, scale, st);
        case 5: return launch_one<HD, 5>(qkv, out, B, L, H, scale, st);
        case 6: return launch_one<HD, 6>(qkv, out, B, L, H, scale, st);
        case 7: return launch_one<HD, 7>(qkv, out, B, L, H, scale, st);
        case 8: return launch_one<HD, 8>(qkv, out, B, L, H, scale, st);
    }
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention (bf16): L = %d (covered: 1 .. %d)", L, kMaxL);
}

}  // namespace

int launch_attention_bf16(const void *qkv, void *out, int B, int L, int H, int hd, float scale, hipStream_t st) {
    const unsigned short *q = static_cast<const unsigned short *>(qkv);
    unsigned short *o = static_cast<unsigned short *>(out);
    if (hd == 32) return launch_hd<32>(q, o, B, L, H, scale, st);
    if (hd == 64) return launch_hd<64>(q, o, B, L, H, scale, st);
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention (bf16): head_dim = %d (covered: 32, 64)", hd);
}

}  // namespace vit
}  // namespace stgcn
