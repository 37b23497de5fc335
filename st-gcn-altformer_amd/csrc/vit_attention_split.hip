// Multi-head attention over the packed qkv of the AltFormer heads' blocks, fp32, the SPLIT form of the resident kernel for calls
// of a few clips (STGCN_VIT_ATTN_SPLIT, stgcn_vit_attention_split): vit_attention.hip gives a (sequence, head) pair one
// workgroup whose waves each walk every key tile, so one clip of 8 heads is 8 workgroups with a chain of 2 NT hd/2 .. MFMAs per
// wave.  Here a workgroup is one (pair, query tile of 32) and its NT waves split the KEYS: wave w owns key tile w.
//   per wave   the accumulator layout of vit_attention_common.h: S^T = K_w Q^T on v_mfma_f32_32x32x2_f32 (exact fp32
//              products, the queries pre-scaled in registers), keys past L score -inf, m_w = the tile's maximum (one exchange
//              with lane ^ 32), e = exp(s - m_w), l_w = sum e, O_w = V_w^T e left unnormalised.  A wave reads its 32 keys
//              once, so both A operands come straight from global memory in the form the MFMA takes them: a K row is hd / 2
//              contiguous floats per lane (float4 loads), V is lane = channel (128 contiguous bytes per key and lane half).
//              Nothing is staged; rows past L are zeros and never read from memory.
//   merge      through LDS, in a fixed order: every wave writes (m_w, l_w) per query and its 32 x hd partial, one barrier, then
//              m = max_w m_w, f_w = exp(m_w - m), out = (sum_w f_w O_w) / (sum_w f_w l_w), both sums in ascending w, the
//              elements spread over all 64 NT threads, float4 stores.  No atomics, no workspace, one owner per element: results
//              are bit-identical run to run.  At NT = 1 the merge is the identity (f = 1).
//   LDS        attention_split_lds_bytes: per wave 32 rows of hd + 4 floats (float4 rows whose 16-byte writes of 32 lanes fall
//              into distinct banks) and 2 floats of statistics per query; 70 KiB at NT = 8, hd = 64.
#include "vit_attention_common.h"

namespace stgcn {
namespace vit {

namespace {

template <int HD, int NT>
__global__ __launch_bounds__(64 * NT) void vit_attention_split_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                                      int L, int H, float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int HH = HD / 2, PS = HD + kPadSplit, WAVE = attention_split_wave_floats(HD);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int p = blockIdx.x / NT, qt = blockIdx.x % NT;     // the grid is exactly pairs * NT workgroups
    const int b = p / H, h = p % H;
    const size_t tok = (size_t)3 * H * HD;                   // floats per token of qkv
    const float *base = qkv + (size_t)b * L * tok + (size_t)h * HD;   // q of the pair's token 0; k and v are H * HD, 2 H * HD on
    const int qi = qt * 32 + l31, ki = wave * 32 + l31;

    // B operand: lane holds Q[qi][half*HH + s] pre-scaled; A operand: K[ki][half*HH + s].  Rows past L are zeros.
    float qf[HH], kf[HH];
    if (qi < L) {
        const float4 *qp = reinterpret_cast<const float4 *>(base + (size_t)qi * tok + half * HH);
#pragma unroll
        for (int s = 0; s < HH / 4; ++s) {
            const float4 v = qp[s];
            qf[4 * s] = v.x * scale, qf[4 * s + 1] = v.y * scale, qf[4 * s + 2] = v.z * scale, qf[4 * s + 3] = v.w * scale;
        }
    } else {
#pragma unroll
        for (int s = 0; s < HH; ++s) qf[s] = 0.f;
    }
    if (ki < L) {
        const float4 *kp = reinterpret_cast<const float4 *>(base + (size_t)ki * tok + (size_t)H * HD + half * HH);
#pragma unroll
        for (int s = 0; s < HH / 4; ++s) {
            const float4 v = kp[s];
            kf[4 * s] = v.x, kf[4 * s + 1] = v.y, kf[4 * s + 2] = v.z, kf[4 * s + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < HH; ++s) kf[s] = 0.f;
    }
    // A operand of the output product, lane = channel: V[key of register i][dt*32 + l31], issued before the scores need anything
    float vf[HD / 32][16];
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = ACC_KEY(wave * 32, i, half);
            vf[dt][i] = key < L ? base[(size_t)key * tok + (size_t)2 * H * HD + dt * 32 + l31] : 0.f;
        }

    f32x16 sc;
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[i] = 0.f;
#pragma unroll
    for (int s = 0; s < HH; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[s], qf[s], sc, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int key = ACC_KEY(wave * 32, i, half);
        if (key >= L) sc[i] = -INFINITY;
        mx = fmaxf(mx, sc[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // the tile's first key is below L (NT = ceil(L / 32)): mx is finite
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float e = __expf(sc[i] - mx);   // exp(-inf) = 0 for the masked keys
        sc[i] = e;
        sum += e;
    }
    sum += __shfl_xor(sum, 32, 64);

    // the wave's part of the merge: its unnormalised 32 x HD partial (rows of PS floats) and (m_w, l_w) per query behind it
    float *part = lds + (size_t)wave * WAVE, *stat = part + 32 * PS;
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt) {
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[dt][i], sc[i], o, 0, 0, 0);
        store_rows(part + l31 * PS + dt * 32 + 4 * half, o);
    }
    if (half == 0) stat[2 * l31] = mx, stat[2 * l31 + 1] = sum;
    __syncthreads();

    // merge: float4 e of the tile's 32 x HD outputs = query e / (HD / 4), channels 4 (e % (HD / 4)) ..; ascending w
    constexpr int C4 = HD / 4;
    for (int e = tid; e < 32 * C4; e += 64 * NT) {
        const int q = e / C4, c = e % C4 * 4;
        if (qt * 32 + q >= L) continue;       // rows past L are never stored
        float m = -INFINITY;
#pragma unroll
        for (int w = 0; w < NT; ++w) m = fmaxf(m, lds[(size_t)w * WAVE + 32 * PS + 2 * q]);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float den = 0.f;
#pragma unroll
        for (int w = 0; w < NT; ++w) {
            const float *pw = lds + (size_t)w * WAVE;
            const float f = __expf(pw[32 * PS + 2 * q] - m);
            const float4 o = *reinterpret_cast<const float4 *>(pw + q * PS + c);
            den += f * pw[32 * PS + 2 * q + 1];
            acc.x += f * o.x, acc.y += f * o.y, acc.z += f * o.z, acc.w += f * o.w;
        }
        const float inv = 1.0f / den;
        *reinterpret_cast<float4 *>(out + ((size_t)b * L + qt * 32 + q) * ((size_t)H * HD) + (size_t)h * HD + c) =
            make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
}

template <int HD, int NT>
int launch_split_one(const float *qkv, float *out, int B, int L, int H, float scale, hipStream_t st) {
    const long long groups = (long long)B * H * NT;
    if (!grid_fits(groups, 64 * NT)) return fail(STGCN_ERR_UNSUPPORTED, "vit attention split: %lld workgroups", groups);
    constexpr size_t bytes = attention_split_lds_bytes(NT, HD);
    static_assert(bytes <= (size_t)kLdsBytes, "the merge buffers fit the LDS");
    auto kern = vit_attention_split_kernel<HD, NT>;
    if (bytes > 64 * 1024) STGCN_HIP_CHECK(allow_lds(kern, bytes));
    kern<<<dim3((unsigned)groups), dim3(64 * NT), bytes, st>>>(qkv, out, L, H, scale);
    STGCN_LAUNCH_CHECK("vit_attention_split_kernel");
    return STGCN_OK;
}

template <int HD>
int launch_split_hd(const float *qkv, float *out, int B, int L, int H, float scale, hipStream_t st) {
    switch (attention_tiles(L)) {
        case 1: return launch_split_one<HD, 1>(qkv, out, B, L, H, scale, st);
        case 2: return launch_split_one<HD, 2>(qkv, out, B, L, H, scale, st);
        case 3: return launch_split_one<HD, 3>(qkv, out, B, L, H, scale, st);
        case 4: return launch_split_one<HD, 4>(qkv, out, B, L, H, scale, st);
        case 5: return launch_split_one<HD, 5>(qkv, out, B, L, H, scale, st);
        case 6: return launch_split_one<HD, 6>(qkv, out, B, L, H, scale, st);
        case 7: return launch_split_one<HD, 7>(qkv, out, B, L, H, scale, st);
        case 8: return launch_split_one<HD, 8>(qkv, out, B, L, H, scale, st);
    }
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention split: L = %d (covered: 1 .. %d)", L, kMaxL);
}

}  // namespace

int launch_attention_split(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st) {
    if (hd == 32) return launch_split_hd<32>(qkv, out, B, L, H, scale, st);
    if (hd == 64) return launch_split_hd<64>(qkv, out, B, L, H, scale, st);
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention split: head_dim = %d (covered: 32, 64)", hd);
}

}  // namespace vit
}  // namespace stgcn
