// The attention backward of vit_backward.hip for sequences it cannot keep on chip (256 < L <= kMaxStreamL, and every shorter
// length on request):  dqkv (B, L, 3, H, hd) from the packed qkv, the forward's `out` and its gradient `dout`.
// Neither the LDS nor the registers grow with L: the other side of every product is streamed through two LDS stages of 64
// rows, as vit_attention_stream.hip streams K and V.  Two kernels, one after the other on the stream, share `stats`:
// (m, 1 / l, delta, 0) per (sequence, head, query), B * H * L * 4 floats, written by the first and read by the second.
//
//   query kernel   a workgroup of four waves owns kStreamQueries = 128 queries of one (sequence, head) pair, a wave 32 of
//                  them: scale * Q and dO rows in registers, delta = rowsum(dO * O) from `out`.  It walks the key tiles twice.
//                  Pass 1 (K only): the running maximum m and sum l of the streaming forward, recomputed, not saved by it.
//                  Pass 2 (K and V): S^T = K Q^T, P = exp(S - m) / l, dP^T = V dO^T, dS = P (dP - delta), dQ^T += K^T dS^T.
//                  It writes scale * dQ and the statistics.  The two passes are one loop of 2 ceil(L / 64) tiles, so the first
//                  tile of pass 2 is loaded under the last products of pass 1.
//   key kernel     a workgroup of four waves owns 128 keys of the pair, a wave 32 of them: K and V rows in registers.  It
//                  streams tiles of 64 queries (scale * Q, dO and their statistics): S = Q K^T (the same products in the same
//                  order as the query kernel, and the same m and 1 / l: P is bit-identical between the two), dP = dO V^T,
//                  dS, dV^T += dO^T P, dK^T += (scale Q)^T dS.  It writes dK and dV.
//
// That is eight L x L x hd products against the resident kernel's seven: the extra one is pass 1.
// Built from vit_attention_common.h, which describes the operand layouts (those of the resident backward): the score
// accumulators are the B operand of the products behind them.  Every staged row has the HD + 1 stride (it is read both
// along a row per lane and across rows).  Staging as in the forward: the loads of tile t + 1 go into registers before the
// products of tile t and into the other stage behind them, one barrier per tile; rows past L are zero-filled, never read.
// Keys past L are masked to -inf before the exponent (P = 0).  Query rows past L reach the key kernel as zeros with
// m = 0, 1 / l = 0, delta = 0, so they add exp(0) * 0 = 0 to dK / dV (never exp(-inf + inf)).  Idle waves of a short last
// block still stage and meet the barriers.
// fp32 throughout (v_mfma_f32_32x32x2_f32).
#include "vit_attention_common.h"

namespace stgcn {
namespace vit {

namespace {

constexpr int kBwdThreads = 64 * (kStreamQueries / 32);   // four waves: 128 queries, or 128 keys, per workgroup
constexpr int kBwdRows = kStreamKeys;                     // rows of a stage, in both kernels

// one LDS row (HD + 1 stride) <- a float4
__device__ __forceinline__ void put_row4(float *d, const float4 v) { d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w; }

template <int HD>
__global__ __launch_bounds__(kBwdThreads) void vit_attention_bwd_stream_q_kernel(const float *__restrict__ qkv,
                                                                                 const float *__restrict__ out,
                                                                                 const float *__restrict__ dout,
                                                                                 float *__restrict__ dqkv,
                                                                                 float *__restrict__ stats, int L, int H,
                                                                                 float scale, int nqb) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int KT = kBwdRows, KS = HD + kPadF32, HH = HD / 2;
    constexpr int STAGE = 2 * KT * KS;                     // floats of one stage: K rows, then V rows
    constexpr int NV = KT * (HD / 4) / kBwdThreads;        // float4 of K (and of V) a thread moves per tile
    static_assert(KT * (HD / 4) % kBwdThreads == 0, "staging split");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD, otok = (size_t)H * HD;
    const int p = blockIdx.x / nqb, qb = blockIdx.x % nqb; // (sequence, head) pair, block of kStreamQueries queries
    const int b = p / H, h = p % H;
    const float *kv = qkv + (size_t)b * L * tok + (size_t)h * HD + (size_t)H * HD;   // K of token 0; V is H * HD further

    float4 kr[NV], vr[NV];
    auto fetch = [&](int t, bool with_v) {                  // tile t: global -> registers
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * kBwdThreads, d4 = e % (HD / 4), key = t * KT + e / (HD / 4);
            kr[i] = vr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (key < L) {
                const float *src = kv + (size_t)key * tok + d4 * 4;
                kr[i] = *reinterpret_cast<const float4 *>(src);
                if (with_v) vr[i] = *reinterpret_cast<const float4 *>(src + (size_t)H * HD);
            }
        }
    };
    auto stage = [&](float *dst, bool with_v) {             // registers -> one LDS stage
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * kBwdThreads, d4 = e % (HD / 4), j = e / (HD / 4);
            put_row4(dst + j * KS + d4 * 4, kr[i]);
            if (with_v) put_row4(dst + KT * KS + j * KS + d4 * 4, vr[i]);
        }
    };

    const int q0 = qb * kStreamQueries + wave * 32;        // the wave's query tile
    const bool active = q0 < L;                            // wave-uniform; an idle wave still stages and meets the barriers
    const int qi = q0 + l31;

    // the wave's scale * Q and dO rows as B operands: lane holds row qi, columns half*HH + s
    float qf[HH], df[HH];
    float delta = 0.f;
#pragma unroll
    for (int s = 0; s < HH; ++s) qf[s] = 0.f, df[s] = 0.f;
    if (qi < L) {
        const float4 *qp = reinterpret_cast<const float4 *>(qkv + ((size_t)b * L + qi) * tok + (size_t)h * HD + half * HH);
        const float4 *dp = reinterpret_cast<const float4 *>(dout + ((size_t)b * L + qi) * otok + (size_t)h * HD + half * HH);
        const float4 *op = reinterpret_cast<const float4 *>(out + ((size_t)b * L + qi) * otok + (size_t)h * HD + half * HH);
#pragma unroll
        for (int s = 0; s < HH / 4; ++s) {
            const float4 v = qp[s], d = dp[s], o = op[s];
            qf[4 * s] = v.x * scale, qf[4 * s + 1] = v.y * scale, qf[4 * s + 2] = v.z * scale, qf[4 * s + 3] = v.w * scale;
            df[4 * s] = d.x, df[4 * s + 1] = d.y, df[4 * s + 2] = d.z, df[4 * s + 3] = d.w;
            delta += (d.x * o.x + d.y * o.y) + (d.z * o.z + d.w * o.w);
        }
    }
    delta += __shfl_xor(delta, 32, 64);

    f32x16 dq[HD / 32];
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dq[dt][i] = 0.f;
    float m = -INFINITY, l = 0.f, inv = 0.f;                // running maximum, this lane's part of the sum; 1 / sum after pass 1

    const int nt = (L + KT - 1) / KT;
    fetch(0, false);
    stage(lds, false);
    __syncthreads();
    for (int it = 0; it < 2 * nt; ++it) {                   // pass 1: it < nt, pass 2 behind it, tile it % nt
        const int t = it < nt ? it : it - nt;
        const int tn = it + 1 < nt ? it + 1 : it + 1 - nt;  // the next step's tile, K and V from pass 2 on
        const bool more = it + 1 < 2 * nt, next_v = it + 1 >= nt;
        const float *Kb = lds + (it & 1) * STAGE, *Vb = Kb + KT * KS;
        if (more) fetch(tn, next_v);                        // in flight under the products below
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
            if (it < nt) {
                // the forward's running soft-max: every tile holds a valid key, so the new maximum is finite
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
                const float mn = fmaxf(m, tmax);
                float psum = 0.f;
#pragma unroll
                for (int kt = 0; kt < KT / 32; ++kt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) psum += __expf(sc[kt][i] - mn);
                l = l * __expf(m - mn) + psum;              // first tile: exp(-inf) = 0 on a sum that is 0
                m = mn;
                if (it == nt - 1) {
                    l += __shfl_xor(l, 32, 64);
                    inv = 1.0f / l;
                }
            } else {
                // dP^T = V dO^T per key tile, dS^T = P^T (dP^T - delta) in place of S^T
#pragma unroll
                for (int kt = 0; kt < KT / 32; ++kt) {
                    f32x16 dp;
#pragma unroll
                    for (int i = 0; i < 16; ++i) dp[i] = 0.f;
                    const float *vp = Vb + (kt * 32 + l31) * KS + half * HH;
#pragma unroll
                    for (int s = 0; s < HH; ++s) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[s], df[s], dp, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 16; ++i) sc[kt][i] = __expf(sc[kt][i] - m) * inv * (dp[i] - delta);   // masked: 0
                }
                // dQ^T += K^T dS^T
#pragma unroll
                for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                    for (int kt = 0; kt < KT / 32; ++kt)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int key = ACC_KEY(kt * 32, i, half);
                            dq[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kb[key * KS + dt * 32 + l31], sc[kt][i], dq[dt], 0, 0, 0);
                        }
            }
        }
        if (more) stage(lds + ((it + 1) & 1) * STAGE, next_v);   // the stage step it - 1 read: everyone is past the last barrier
        __syncthreads();
    }

    if (!active || qi >= L) return;
    if (half == 0) *reinterpret_cast<float4 *>(stats + ((size_t)p * L + qi) * 4) = make_float4(m, inv, delta, 0.f);
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
        store_rows(dqkv + ((size_t)b * L + qi) * tok + (size_t)h * HD + dt * 32 + 4 * half, dq[dt], scale);
}

template <int HD>
__global__ __launch_bounds__(kBwdThreads) void vit_attention_bwd_stream_k_kernel(const float *__restrict__ qkv,
                                                                                 const float *__restrict__ dout,
                                                                                 const float *__restrict__ stats,
                                                                                 float *__restrict__ dqkv, int L, int H,
                                                                                 float scale, int nkb) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int QT = kBwdRows, KS = HD + kPadF32, HH = HD / 2;
    constexpr int STAGE = 2 * QT * KS + QT * 4;            // floats of one stage: scale * Q rows, dO rows, (m, 1 / l, delta, -)
    constexpr int NV = QT * (HD / 4) / kBwdThreads;        // float4 of Q (and of dO) a thread moves per tile
    static_assert(QT * (HD / 4) % kBwdThreads == 0 && (2 * QT * KS) % 4 == 0 && STAGE % 4 == 0 && QT <= kBwdThreads,
                  "staging split / alignment");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const size_t tok = (size_t)3 * H * HD, otok = (size_t)H * HD;
    const int p = blockIdx.x / nkb, kb = blockIdx.x % nkb; // (sequence, head) pair, block of 128 keys
    const int b = p / H, h = p % H;
    const float *qg = qkv + (size_t)b * L * tok + (size_t)h * HD;        // Q of token 0
    const float *dg = dout + (size_t)b * L * otok + (size_t)h * HD;      // dO of token 0
    const float *sg = stats + (size_t)p * L * 4;

    float4 qr[NV], dr[NV], sr;
    auto fetch = [&](int t) {                               // query tile t: global -> registers; rows past L are zeros
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * kBwdThreads, d4 = e % (HD / 4), q = t * QT + e / (HD / 4);
            qr[i] = dr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < L) {
                qr[i] = *reinterpret_cast<const float4 *>(qg + (size_t)q * tok + d4 * 4);
                dr[i] = *reinterpret_cast<const float4 *>(dg + (size_t)q * otok + d4 * 4);
            }
        }
        sr = make_float4(0.f, 0.f, 0.f, 0.f);               // m = 0, 1 / l = 0, delta = 0: the row adds exp(0) * 0
        if (tid < QT && t * QT + tid < L) sr = *reinterpret_cast<const float4 *>(sg + (size_t)(t * QT + tid) * 4);
    };
    auto stage = [&](float *dst) {                          // registers -> one LDS stage
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = tid + i * kBwdThreads, d4 = e % (HD / 4), j = e / (HD / 4);
            put_row4(dst + j * KS + d4 * 4, make_float4(qr[i].x * scale, qr[i].y * scale, qr[i].z * scale, qr[i].w * scale));
            put_row4(dst + QT * KS + j * KS + d4 * 4, dr[i]);
        }
        if (tid < QT) *reinterpret_cast<float4 *>(dst + 2 * QT * KS + tid * 4) = sr;
    };

    const int k0 = kb * kStreamQueries + wave * 32;        // the wave's key tile
    const bool active = k0 < L;                            // wave-uniform; an idle wave still stages and meets the barriers
    const int ki = k0 + l31;

    // the wave's K and V rows as B operands: lane holds row ki, columns half*HH + s
    float kf[HH], vf[HH];
#pragma unroll
    for (int s = 0; s < HH; ++s) kf[s] = 0.f, vf[s] = 0.f;
    if (ki < L) {
        const float *base = qg + (size_t)ki * tok + half * HH;
        const float4 *kp = reinterpret_cast<const float4 *>(base + (size_t)H * HD);
        const float4 *vp = reinterpret_cast<const float4 *>(base + (size_t)2 * H * HD);
#pragma unroll
        for (int s = 0; s < HH / 4; ++s) {
            const float4 k = kp[s], v = vp[s];
            kf[4 * s] = k.x, kf[4 * s + 1] = k.y, kf[4 * s + 2] = k.z, kf[4 * s + 3] = k.w;
            vf[4 * s] = v.x, vf[4 * s + 1] = v.y, vf[4 * s + 2] = v.z, vf[4 * s + 3] = v.w;
        }
    }
    f32x16 dk[HD / 32], dv[HD / 32];
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) dk[dt][i] = 0.f, dv[dt][i] = 0.f;

    const int nt = (L + QT - 1) / QT;
    fetch(0);
    stage(lds);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
        const float *Qb = lds + (t & 1) * STAGE, *Ob = Qb + QT * KS, *Sb = Qb + 2 * QT * KS;
        if (t + 1 < nt) fetch(t + 1);                       // in flight under the products below
        if (active) {
#pragma unroll
            for (int qt = 0; qt < QT / 32; ++qt) {
                f32x16 s, dp;
#pragma unroll
                for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
                const float *qp = Qb + (qt * 32 + l31) * KS + half * HH, *op = Ob + (qt * 32 + l31) * KS + half * HH;
#pragma unroll
                for (int c = 0; c < HH; ++c) {
                    s = __builtin_amdgcn_mfma_f32_32x32x2f32(qp[c], kf[c], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x2f32(op[c], vf[c], dp, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int q = ACC_KEY(qt * 32, i, half);
                    const float4 st = *reinterpret_cast<const float4 *>(&Sb[q * 4]);   // (max, 1 / sum, delta, -); 1 / sum = 0 past L
                    const float pr = ki < L ? __expf(s[i] - st.x) * st.y : 0.f;
                    s[i] = pr;
                    dp[i] = pr * (dp[i] - st.z);
                }
#pragma unroll
                for (int dt = 0; dt < HD / 32; ++dt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int q = ACC_KEY(qt * 32, i, half);
                        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ob[q * KS + dt * 32 + l31], s[i], dv[dt], 0, 0, 0);
                        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qb[q * KS + dt * 32 + l31], dp[i], dk[dt], 0, 0, 0);
                    }
            }
        }
        if (t + 1 < nt) stage(lds + ((t + 1) & 1) * STAGE); // the stage tile t - 1 was read from: everyone is past the last barrier
        __syncthreads();
    }

    if (!active || ki >= L) return;
    float *base = dqkv + ((size_t)b * L + ki) * tok + (size_t)h * HD + 4 * half;
#pragma unroll
    for (int dt = 0; dt < HD / 32; ++dt) {
        store_rows(base + (size_t)H * HD + dt * 32, dk[dt]);
        store_rows(base + (size_t)2 * H * HD + dt * 32, dv[dt]);
    }
}

template <int HD>
int launch_hd(const float *qkv, const float *out, const float *dout, float *dqkv, float *stats, int B, int L, int H,
              float scale, hipStream_t st) {
    const int nb = ceil_div(L, kStreamQueries);            // blocks of 128 queries, and of 128 keys, per pair
    const long long blocks = (long long)B * H * nb;
    if (!grid_fits(blocks, kBwdThreads)) return fail(STGCN_ERR_UNSUPPORTED, "vit attention backward (stream): %lld workgroups", blocks);
    const size_t qbytes = (size_t)2 * 2 * kBwdRows * (HD + kPadF32) * sizeof(float);
    const size_t kbytes = qbytes + (size_t)2 * kBwdRows * 4 * sizeof(float);
    auto qkern = vit_attention_bwd_stream_q_kernel<HD>;
    auto kkern = vit_attention_bwd_stream_k_kernel<HD>;
    if (qbytes > 64 * 1024) STGCN_HIP_CHECK(allow_lds(qkern, qbytes));
    if (kbytes > 64 * 1024) STGCN_HIP_CHECK(allow_lds(kkern, kbytes));
    qkern<<<dim3((unsigned)blocks), dim3(kBwdThreads), qbytes, st>>>(qkv, out, dout, dqkv, stats, L, H, scale, nb);
    STGCN_LAUNCH_CHECK("vit_attention_bwd_stream_q_kernel");
    kkern<<<dim3((unsigned)blocks), dim3(kBwdThreads), kbytes, st>>>(qkv, dout, stats, dqkv, L, H, scale, nb);
    STGCN_LAUNCH_CHECK("vit_attention_bwd_stream_k_kernel");
    return STGCN_OK;
}

}  // namespace

int launch_attention_backward_stream(const float *qkv, const float *out, const float *dout, float *dqkv, float *stats, int B,
                                     int L, int H, int hd, float scale, hipStream_t st) {
    if (L < 1 || L > kMaxStreamL)
        return fail(STGCN_ERR_UNSUPPORTED, "vit attention backward (stream): L = %d (covered: 1 .. %d)", L, kMaxStreamL);
    if (hd == 32) return launch_hd<32>(qkv, out, dout, dqkv, stats, B, L, H, scale, st);
    if (hd == 64) return launch_hd<64>(qkv, out, dout, dqkv, stats, B, L, H, scale, st);
    return fail(STGCN_ERR_UNSUPPORTED, "vit attention backward (stream): head_dim = %d (covered: 32, 64)", hd);
}

}  // namespace vit
}  // namespace stgcn
