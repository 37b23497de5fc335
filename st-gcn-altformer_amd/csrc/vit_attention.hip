// Multi-head attention over the packed qkv of the AltFormer heads' blocks (model/AltFormer/model_ST.py:48-66), fp32, the
// resident form (L <= 256): one kernel for every covered length, in the layout that vit_attention_common.h describes.
// Specific to this file: everything runs on v_mfma_f32_32x32x2_f32, i.e. exact fp32 products; the wave's query rows are
// pre-scaled in registers; K is staged as [rows][hd + 1] (read along a row per lane), V as [rows][hd] (lane = channel); keys
// past L are masked in every tile; O is divided by the row sum on store.
#include "vit_attention_common.h"

namespace stgcn {
namespace vit {

namespace {

template <int HD, int NT>
__global__ __launch_bounds__(512) void vit_attention_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                           int pairs, int L, int H, float scale, int G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ROWS = NT * 32, KS = HD + kPadF32, HH = HD / 2;
    float *Ks = lds;                          // [G][ROWS][KS]
    float *Vs = lds + (size_t)G * ROWS * KS;  // [G][ROWS][HD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD;    // floats per token of qkv

    // stage K and V of the workgroup's pairs: float4 per thread, rows past L and pairs past the end zero-filled
    const int nvec = G * ROWS * (HD / 4);
    for (int e = tid; e < nvec; e += blockDim.x) {
        const StageSlot s = stage_slot<HD, ROWS, 4>(e, G, pairs, L, H);
        float4 k = make_float4(0.f, 0.f, 0.f, 0.f), v = k;
        if (s.live) {
            const float *base = qkv + s.tok * tok + s.col;
            k = *reinterpret_cast<const float4 *>(base + (size_t)H * HD);
            v = *reinterpret_cast<const float4 *>(base + (size_t)2 * H * HD);
        }
        float *kd = Ks + ((size_t)s.g * ROWS + s.j) * KS + s.d0;
        kd[0] = k.x, kd[1] = k.y, kd[2] = k.z, kd[3] = k.w;
        *reinterpret_cast<float4 *>(Vs + ((size_t)s.g * ROWS + s.j) * HD + s.d0) = v;
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
            const int key = ACC_KEY(kt * 32, i, half);
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
                const int key = ACC_KEY(kt * 32, i, half);
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(Vg[(size_t)key * HD + dt * 32 + l31], sc[kt][i], o, 0, 0, 0);
            }
        if (qi < L) store_rows(out + ((size_t)b * L + qi) * ((size_t)H * HD) + (size_t)h * HD + dt * 32 + 4 * half, o, inv);
    }
}

struct Forward {
    static constexpr const char *what = "vit attention", *kernel_name = "vit_attention_kernel";
    static constexpr size_t lds_bytes(int nt, int hd) { return attention_f32_lds_bytes(nt, hd); }
    template <int HD, int NT>
    static auto kernel() { return vit_attention_kernel<HD, NT>; }
};

}  // namespace

int launch_attention_packed(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st) {
    return launch_resident<Forward>(B, L, H, hd, scale, st, qkv, out);
}

}  // namespace vit
}  // namespace stgcn
