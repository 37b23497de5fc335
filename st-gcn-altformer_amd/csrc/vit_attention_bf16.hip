// Multi-head attention of the AltFormer heads' blocks on bf16 operands (the STGCN_VIT_BF16 mode of stgcn_vit_block_forward):
//     qkv (B, L, 3, H, hd) bf16 as the bf16 qkv linear stores it  ->  out (B, L, H*hd) bf16 ready for proj.
// The resident form (L <= 256) on v_mfma_f32_32x32x16_bf16, in the layout that vit_attention_common.h describes.  Specific
// to this file: operands go to the matrix cores as they are stored, K as a row tile and V as a transposed one; one score
// chain, hd / 16 MFMAs per key tile; `scale` multiplies the fp32 score (q is not rounded a second time); only the last key
// tile is masked; p = exp(s - max), unnormalised, is rounded to bf16 as it is packed and the row sum adds the UNROUNDED fp32 p;
// O is divided by the row sum in fp32 and stored as bf16, 8 bytes per store.  Products are bf16 x bf16 (exact in fp32), every
// sum is fp32.  LDS: 52 KiB at L = 180, hd = 64 (the fp32 kernel: 99).
#include "vit_attention_common.h"

namespace stgcn {
namespace vit {

namespace {

template <int HD, int NT>
__global__ __launch_bounds__(512) void vit_attention_bf16_kernel(const unsigned short *__restrict__ qkv,
                                                                unsigned short *__restrict__ out, int pairs, int L, int H,
                                                                float scale, int G) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds16[];
    constexpr int ROWS = NT * 32, KS = HD + kPad16, VS = ROWS + kPad16, KST = HD / 16;
    unsigned short *Ks = lds16;                          // [G][ROWS][KS]
    unsigned short *Vt = lds16 + (size_t)G * ROWS * KS;  // [G][HD][VS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD;    // elements per token of qkv

    // stage K and V of the workgroup's pairs: 8 channels (16 bytes) of one key per thread and step, keys past L and pairs
    // past the end zero-filled
    const int nvec = G * ROWS * (HD / 8);
    for (int e = tid; e < nvec; e += blockDim.x) {
        const StageSlot s = stage_slot<HD, ROWS, 8>(e, G, pairs, L, H);
        uint4 k = make_uint4(0u, 0u, 0u, 0u), v = k;
        if (s.live) {
            const unsigned short *base = qkv + s.tok * tok + s.col;
            k = *reinterpret_cast<const uint4 *>(base + (size_t)H * HD);
            v = *reinterpret_cast<const uint4 *>(base + (size_t)2 * H * HD);
        }
        *reinterpret_cast<uint4 *>(Ks + ((size_t)s.g * ROWS + s.j) * KS + s.d0) = k;
        scatter8(Vt + ((size_t)s.g * HD + s.d0) * VS, VS, perm16(s.j), v);
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
            if (kt == NT - 1 && ACC_KEY(kt * 32, i, half) >= L) sc[kt][i] = -INFINITY;   // only the last tile is partial
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
        if (qi < L) store_rows(out + ((size_t)b * L + qi) * ((size_t)H * HD) + (size_t)h * HD + dt * 32 + 4 * half, o, inv);
    }
}

struct ForwardBf16 {
    static constexpr const char *what = "vit attention (bf16)", *kernel_name = "vit_attention_bf16_kernel";
    static constexpr size_t lds_bytes(int nt, int hd) { return attention_bf16_lds_bytes(nt, hd, 1); }
    template <int HD, int NT>
    static auto kernel() { return vit_attention_bf16_kernel<HD, NT>; }
};

}  // namespace

int launch_attention_bf16(const void *qkv, void *out, int B, int L, int H, int hd, float scale, hipStream_t st) {
    return launch_resident<ForwardBf16>(B, L, H, hd, scale, st, static_cast<const unsigned short *>(qkv),
                                        static_cast<unsigned short *>(out));
}

}  // namespace vit
}  // namespace stgcn
