// Multi-head attention over the packed qkv of the AltFormer heads' blocks (model/AltFormer/model_ST.py:48-66):
//     qkv (B, L, 3, H, hd) exactly as the qkv nn.Linear writes it  ->  out (B, L, H*hd) ready for proj.
// No q / k / v permute copies and no L x L matrix in memory.  One kernel for every covered length (L <= 256):
// a (sequence, head) pair gets NT = ceil(L / 32) waves, one per tile of 32 queries, and its K and V (NT*32 rows, the rows
// past L zero-filled, never read from memory) in LDS; short sequences pack several pairs into a workgroup (L <= 32: one
// wave per pair, four pairs per workgroup).  Everything runs on v_mfma_f32_32x32x2_f32, i.e. exact fp32 products:
//
//   S^T = K Q^T per key tile: A = K rows from LDS (row stride hd + 1 floats: the 32 rows of a fragment sit in 32 banks),
//         B = the wave's 32 query rows, pre-scaled, held in registers.  The accumulator layout puts query j in lane
//         j (and j + 32) and 16 keys of the tile in its 16 registers, so the whole score row of a query (up to 256 keys =
//         8 x 16 registers) lives in two lanes: the soft-max is a plain two-pass one (max, then exp and sum) over
//         registers in a fixed order plus one exchange with lane ^ 32.  Keys past L get -inf.
//   O^T = V^T P^T: the accumulator registers of S^T are already a B operand (register i of lanes 0-31 / 32-63 holds keys
//         a and a + 4 of the same query, the two k values of one MFMA), and A = V^T is read from LDS with lane = channel,
//         so there is no transpose through LDS and P never leaves the registers.  O is divided by the row sum on store.
// No atomics; every output element has one owner and a fixed summation order, so results are bit-identical run to run.
#include "bf16_common.h"
#include "vit.h"

namespace stgcn {
namespace vit {

using bf16k::f32x16;

namespace {

template <int HD, int NT>
__global__ __launch_bounds__(512) void vit_attention_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                           int pairs, int L, int H, float scale, int G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ROWS = NT * 32, KS = HD + 1, HH = HD / 2;
    float *Ks = lds;                          // [G][ROWS][KS]
    float *Vs = lds + (size_t)G * ROWS * KS;  // [G][ROWS][HD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD;    // floats per token of qkv

    // stage K and V of the workgroup's pairs: float4 per thread, rows past L and pairs past the end zero-filled
    const int nvec = G * ROWS * (HD / 4);
    for (int e = tid; e < nvec; e += blockDim.x) {
        const int d4 = e % (HD / 4), j = (e / (HD / 4)) % ROWS, g = e / ((HD / 4) * ROWS);
        const int p = blockIdx.x * G + g;
        float4 k = make_float4(0.f, 0.f, 0.f, 0.f), v = k;
        if (p < pairs && j < L) {
            const float *base = qkv + ((size_t)(p / H) * L + j) * tok + (size_t)(p % H) * HD + d4 * 4;
            k = *reinterpret_cast<const float4 *>(base + (size_t)H * HD);
            v = *reinterpret_cast<const float4 *>(base + (size_t)2 * H * HD);
        }
        float *kd = Ks + ((size_t)g * ROWS + j) * KS + d4 * 4;
        kd[0] = k.x, kd[1] = k.y, kd[2] = k.z, kd[3] = k.w;
        *reinterpret_cast<float4 *>(Vs + ((size_t)g * ROWS + j) * HD + d4 * 4) = v;
    }
    __syncthreads();

    const int g = wave / NT, qt = wave % NT;
    const int p = blockIdx.x * G + g;
    if (p >= pairs) return;                   // wave-uniform
    const int b = p / H, h = p % H;
    const int qi = qt * 32 + l31;
    if (qt * 32 >= L) return;                 // wave-uniform: a query tile past the sequence (cannot happen with NT = ceil(L/32))

    // the wave's queries as B operand: lane holds Q[qi][half*HH + s], s = 0 .. HH-1
    float qf[HH];
    if (qi < L) {
        const float4 *qp = reinterpret_cast<const float4 *>(qkv + ((size_t)b * L + qi) * tok + (size_t)h * HD + half * HH);
#pragma unroll
        for (int s = 0; s < HH / 4; ++s) {
            const float4 v = qp[s];
            qf[4 * s] = v.x * scale, qf[4 * s + 1] = v.y * scale, qf[4 * s + 2] = v.z * scale, qf[4 * s + 3] = v.w * scale;
        }
    } else {
#pragma unroll
        for (int s = 0; s < HH; ++s) qf[s] = 0.f;
    }

    const float *Kg = Ks + (size_t)g * ROWS * KS, *Vg = Vs + (size_t)g * ROWS * HD;
    f32x16 sc[NT];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
        const float *kp = Kg + (size_t)(kt * 32 + l31) * KS + half * HH;
#pragma unroll
        for (int s = 0; s < HH; ++s) sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[s], qf[s], sc[kt], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = kt * 32 + 8 * (i >> 2) + 4 * half + (i & 3);
            if (key >= L) sc[kt][i] = -INFINITY;
            mx = fmaxf(mx, sc[kt][i]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // key 0 is always valid: mx is finite
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float e = __expf(sc[kt][i] - mx);   // exp(-inf) = 0 for the masked keys
            sc[kt][i] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;

#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt) {
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kt * 32 + 8 * (i >> 2) + 4 * half + (i & 3);
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(Vg[(size_t)key * HD + dt * 32 + l31], sc[kt][i], o, 0, 0, 0);
            }
        if (qi < L) {
            float *op = out + ((size_t)b * L + qi) * ((size_t)H * HD) + (size_t)h * HD + dt * 32 + 4 * half;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<float4 *>(op + 8 * r) =
                    make_float4(o[4 * r] * inv, o[4 * r + 1] * inv, o[4 * r + 2] * inv, o[4 * r + 3] * inv);
        }
    }
}

template <int HD, int NT>
int launch_one(const float *qkv, float *out, int B, int L, int H, float scale, hipStream_t st) {
    const int G = NT >= 4 ? 1 : 4 / NT;       // waves per workgroup: 4 for L <= 64, NT (= 3, 4 .. 8) above
    const long long pairs = (long long)B * H;
    if (pairs > 0x7fffffffLL) return fail(STGCN_ERR_UNSUPPORTED, "vit attention: %lld (sequence, head) pairs", pairs);
    const size_t bytes = (size_t)G * NT * 32 * (2 * HD + 1) * sizeof(float);
    if (bytes > (size_t)kLdsBytes) return fail(STGCN_ERR_UNSUPPORTED, "vit attention: %zu bytes of LDS", bytes);
    auto kern = vit_attention_kernel<HD, NT>;
    if (bytes > 64 * 1024) STGCN_HIP_CHECK(allow_lds(kern, bytes));
    kern<<<dim3((unsigned)((pairs + G - 1) / G)), dim3(64 * G * NT), bytes, st>>>(qkv, out, (int)pairs, L, H, scale, G);
    STGCN_LAUNCH_CHECK("vit_attention_kernel");
    return STGCN_OK;
}

template <int HD>
int launch_hd(const float *qkv, float *out, int B, int L, int H, float scale, hipStream_t st) {
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
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention: L = %d (covered: 1 .. %d)", L, kMaxL);
}

}  // namespace

int launch_attention_packed(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st) {
    if (hd == 32) return launch_hd<32>(qkv, out, B, L, H, scale, st);
    if (hd == 64) return launch_hd<64>(qkv, out, B, L, H, scale, st);
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention: head_dim = %d (covered: 32, 64)", hd);
}

}  // namespace vit
}  // namespace stgcn
