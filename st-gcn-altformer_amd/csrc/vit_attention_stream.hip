// The same attention as vit_attention.hip for sequences it cannot keep on chip (256 < L <= kMaxStreamL, and every shorter
// length on request):  qkv (B, L, 3, H, hd) as the qkv nn.Linear writes it  ->  out (B, L, H*hd).  Built from
// vit_attention_common.h, which describes the operand layout; specific to this file:
// K and V are streamed through LDS in tiles of kStreamKeys = 64 keys and the soft-max is a running one, so neither the
// LDS nor the registers grow with L.  A workgroup of four waves owns kStreamQueries = 128 queries of one (sequence, head)
// pair (a wave 32 of them, its query rows pre-scaled in registers for the whole kernel) and walks all key tiles:
//
//   staging   two LDS stages of [64][hd + 1] K rows and [64][hd] V rows (hd = 64: 33,024 B each).  The global loads of tile
//             t + 1 are issued into registers before the products of tile t and written to the other stage behind them:
//             one barrier per tile.  Rows past L are zero-filled, never read from memory.
//   soft-max  query j lives in lanes j and j + 32.  Per tile: the tile's maximum (one lane ^ 32 exchange), m' = max(m, that),
//             alpha = exp(m - m'), the output accumulators (query = lane: a per-lane scalar) and the running sum times alpha,
//             p = exp(s - m') added.  Every tile holds at least one valid key (only the last is short, and
//             ceil(L / 64) leaves it one), so m' is finite and the first tile's alpha is exp(-inf) = 0, never exp(-inf + inf).
//             The two lanes' partial sums meet once, after the last tile; O / l on store.
#include "vit_attention_common.h"

namespace stgcn {
namespace vit {

namespace {

constexpr int kStreamThreads = 64 * (kStreamQueries / 32);

template <int HD>
__global__ __launch_bounds__(kStreamThreads) void vit_attention_stream_kernel(const float *__restrict__ qkv,
                                                                              float *__restrict__ out, int L, int H,
                                                                              float scale, int nqb) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int KT = kStreamKeys, KS = HD + kPadF32, HH = HD / 2;
    constexpr int STAGE = KT * KS + KT * HD;               // floats of one stage: K rows, then V rows
    constexpr int NV = KT * (HD / 4) / kStreamThreads;     // float4 of K (and of V) a thread moves per tile
    static_assert(KT * (HD / 4) % kStreamThreads == 0 && (KT * KS) % 4 == 0 && STAGE % 4 == 0, "staging split / alignment");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD;                 // floats per token of qkv
    const int p = blockIdx.x / nqb, qb = blockIdx.x % nqb; // (sequence, head) pair, block of kStreamQueries queries
    const int b = p / H, h = p % H;
    const float *kv = qkv + (size_t)b * L * tok + (size_t)h * HD + (size_t)H * HD;   // K of token 0; V is H * HD further

    float4 kr[NV], vr[NV];
    auto fetch = [&](int t) {                               // tile t: global -> registers
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * kStreamThreads, d4 = e % (HD / 4), key = t * KT + e / (HD / 4);
            kr[i] = vr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (key < L) {
                const float *src = kv + (size_t)key * tok + d4 * 4;
                kr[i] = *reinterpret_cast<const float4 *>(src);
                vr[i] = *reinterpret_cast<const float4 *>(src + (size_t)H * HD);
            }
        }
    };
    auto stage = [&](float *dst) {                          // registers -> one LDS stage
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * kStreamThreads, d4 = e % (HD / 4), j = e / (HD / 4);
            float *kd = dst + j * KS + d4 * 4;
            kd[0] = kr[i].x, kd[1] = kr[i].y, kd[2] = kr[i].z, kd[3] = kr[i].w;
            *reinterpret_cast<float4 *>(dst + KT * KS + j * HD + d4 * 4) = vr[i];
        }
    };

    const int q0 = qb * kStreamQueries + wave * 32;        // the wave's query tile
    const bool active = q0 < L;                            // wave-uniform; an idle wave still stages and meets the barriers
    const int qi = q0 + l31;

    // the wave's queries as B operand: lane holds Q[qi][half*HH + s], s = 0 .. HH-1
    float qf[HH];
#pragma unroll
    for (int s = 0; s < HH; ++s) qf[s] = 0.f;
    if (qi < L) {
        const float4 *qp = reinterpret_cast<const float4 *>(qkv + ((size_t)b * L + qi) * tok + (size_t)h * HD + half * HH);
#pragma unroll
        for (int s = 0; s < HH / 4; ++s) {
            const float4 v = qp[s];
            qf[4 * s] = v.x * scale, qf[4 * s + 1] = v.y * scale, qf[4 * s + 2] = v.z * scale, qf[4 * s + 3] = v.w * scale;
        }
    }

    f32x16 o[HD / 32];
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
    float m = -INFINITY, l = 0.f;                           // running maximum (both lanes of a query) and this lane's part of the sum

    const int nt = (L + KT - 1) / KT;
    fetch(0);
    stage(lds);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const float *Kb = lds + (t & 1) * STAGE, *Vb = Kb + KT * KS;
        if (t + 1 < nt) fetch(t + 1);                       // in flight under the products below
        if (active) {
            f32x16 sc[KT / 32];
            float tmax = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < KT / 32; ++kt) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
                const float *kp = Kb + (kt * 32 + l31) * KS + half * HH;
#pragma unroll
                for (int s = 0; s < HH; ++s) sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[s], qf[s], sc[kt], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = ACC_KEY(t * KT + kt * 32, i, half);
                    if (key >= L) sc[kt][i] = -INFINITY;
                    tmax = fmaxf(tmax, sc[kt][i]);
                }
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));   // the tile's first key is valid: finite
            const float mn = fmaxf(m, tmax);
            const float alpha = __expf(m - mn);             // first tile: exp(-inf) = 0 on accumulators that are 0
            m = mn;
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < KT / 32; ++kt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float e = __expf(sc[kt][i] - mn); // exp(-inf) = 0 for the masked keys
                    sc[kt][i] = e;
                    psum += e;
                }
            l = l * alpha + psum;
#pragma unroll
            for (int dt = 0; dt < HD / 32; ++dt) {
#pragma unroll
                for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
#pragma unroll
                for (int kt = 0; kt < KT / 32; ++kt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int key = ACC_KEY(kt * 32, i, half);
                        o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vb[key * HD + dt * 32 + l31], sc[kt][i], o[dt], 0, 0, 0);
                    }
            }
        }
        if (t + 1 < nt) stage(lds + ((t + 1) & 1) * STAGE); // the stage tile t - 1 was read from: everyone is past the last barrier
        __syncthreads();
    }

    if (!active || qi >= L) return;
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
        store_rows(out + ((size_t)b * L + qi) * ((size_t)H * HD) + (size_t)h * HD + dt * 32 + 4 * half, o[dt], inv);
}

template <int HD>
int launch_hd(const float *qkv, float *out, int B, int L, int H, float scale, hipStream_t st) {
    const int nqb = ceil_div(L, kStreamQueries);
    const long long per_seq = (long long)H * nqb;          // workgroups of one sequence
    if (!grid_fits(per_seq, kStreamThreads)) return fail(STGCN_ERR_UNSUPPORTED, "vit attention (stream): %lld workgroups a sequence", per_seq);
    const size_t bytes = (size_t)2 * kStreamKeys * (2 * HD + kPadF32) * sizeof(float);
    auto kern = vit_attention_stream_kernel<HD>;
    if (bytes > 64 * 1024) STGCN_HIP_CHECK(allow_lds(kern, bytes));
    // sequences are independent: as many of them a launch as its 2^32 work-items hold (grid_fits), the pointers moved on
    const long long seqs = 0xffffffffLL / kStreamThreads / per_seq;
    for (long long b0 = 0; b0 < B; b0 += seqs) {
        const long long nb = B - b0 < seqs ? B - b0 : seqs;
        kern<<<dim3((unsigned)(nb * per_seq)), dim3(kStreamThreads), bytes, st>>>(qkv + (size_t)b0 * L * 3 * H * HD,
                                                                                  out + (size_t)b0 * L * H * HD, L, H, scale, nqb);
        STGCN_LAUNCH_CHECK("vit_attention_stream_kernel");
    }
    return STGCN_OK;
}

}  // namespace

int launch_attention_stream(const float *qkv, float *out, int B, int L, int H, int hd, float scale, hipStream_t st) {
    if (L < 1 || L > kMaxStreamL) return fail(STGCN_ERR_UNSUPPORTED, "vit attention (stream): L = %d (covered: 1 .. %d)", L, kMaxStreamL);
    if (hd == 32) return launch_hd<32>(qkv, out, B, L, H, scale, st);
    if (hd == 64) return launch_hd<64>(qkv, out, B, L, H, scale, st);
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention (stream): head_dim = %d (covered: 32, 64)", hd);
}

}  // namespace vit
}  // namespace stgcn
